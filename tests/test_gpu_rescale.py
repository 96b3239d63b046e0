"""Guidance rescale and the zero-terminal-SNR schedule on the GPU.

1. The factor ``k_b = phi std(y_c) / std(y) + 1 - phi`` against the numpy statement (tests/rescale_ref.py: two-pass float64): at most
   1 fp32 ulp.  The kernel's one-pass double sums carry about ``n 2^-53 (1 + mean^2 / var)`` relative error, far below an fp32 ulp on
   these inputs, so only the final rounding can differ.  Bit for bit: the record alone against any position in a batch, 16-byte
   aligned pointers against pointers off by 4 bytes, any scratch contents, two calls in a row.
2. ``sampler_step(gscale=k)`` for a GIVEN ``k`` against the float32 replica, bit for bit, over both parameterisations, the history,
   the three noise sources, the dynamic threshold and the alignment; ``x0_threshold(gscale=k)`` likewise.
3. The loops of the C1-sized model (base 32, ``(1, 2)``, ``out.*`` scaled by 0.1, B = 2, 16 px, 6 steps, w = 3, phi = 0.7): fused with
   the graph == fused launch by launch == stepwise in fp32, graph == launch by launch in bf16, the handle state's toggling and errors.
4. Zero terminal SNR: the fused loops on both schedules are finite and equal the stepwise route, step 0 equals the numpy update, and
   ``train_step(prediction="v")`` at ``t = T-1`` equals the autograd route."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import rescale_ref as ref  # noqa: E402
import threshold_ref  # noqa: E402

from clip_feature_codec import _native  # noqa: E402
from clip_feature_codec.models.unet import CLIPCondUNet  # noqa: E402
from clip_feature_codec.diffusion.scheduler import NoiseScheduler  # noqa: E402
from clip_feature_codec.diffusion.ddim import DDIMSampler  # noqa: E402
from clip_feature_codec.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

PERS = [768, 969, 12288]      # 3*16*16; 3*17*19: no multiple of 4, rows off alignment; 3*64*64: several workgroups per record
WS = [3.0, 7.5, -1.0, 0.0]
PHIS = [0.7, 1.0]
KINDS = ["random", "offset", "near_constant", "large"]
COEF = (0.6, 0.8, 0.85, 0.52, 0.37)
W_G, PHI = 3.0, 0.7


def same_bits(a, b):
    """Equal as bit patterns, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def outputs(kind, B, per, rng):
    n = lambda: rng.standard_normal((B, per))
    if kind == "random":
        c, u = n(), n()
    elif kind == "offset":                                          # the mean 10 standard deviations away
        c, u = 10.0 + n(), 10.0 + n()
    elif kind == "near_constant":
        c, u = 1.0 + 1e-3 * n(), 1.0 + 1e-3 * n()
    else:
        assert kind == "large"
        c, u = 1e4 * n(), 1e4 * n()
    return c.astype(np.float32), u.astype(np.float32)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def shifted(a, off):
    """A device copy of ``a`` whose data pointer is ``4 * off`` bytes past a 16-byte boundary."""
    buf = torch.zeros(a.size + 8, device=DEV)
    t = buf[off:off + a.size].view(a.shape).copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 * off
    return t


# -------------------------------------------------------------------------------------------------------------------- 1. the factor
@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("phi", PHIS)
def test_factor_matches_the_reference_to_one_ulp(per, B, w, phi):
    rng = np.random.default_rng(per + 7 * B)
    scratch = torch.empty(_native.guidance_rescale_scratch_bytes(B, per), dtype=torch.uint8, device=DEV)
    for kind in KINDS:
        c, u = outputs(kind, B, per, rng)
        want = ref.factor(c, u, w, phi)
        got = host(_native.guidance_rescale(dev(c), dev(u), w, phi, scratch=scratch))
        d = ulps(got, want)
        print(f"{kind} per={per} B={B} w={w} phi={phi}: k {got}, reference {want}, ulps {d}")
        assert np.isfinite(want).all() and np.isfinite(got).all() and (d <= 1).all(), (kind, got, want)
        if phi == 1.0:
            # the rescaled output has the conditional output's std: to 1e-6 relative from the factor's own rounding, plus what
            # rounding k y to fp32 can move a standard deviation by -- at most the largest element error, 2^-24 max|k y|
            y = ref.rescaled(c, u, w, got).astype(np.float64)
            std_c = np.std(c.astype(np.float64), axis=1, ddof=1)
            assert np.all(np.abs(np.std(y, axis=1, ddof=1) - std_c) <= 1e-6 * std_c + 2.0 ** -24 * np.abs(y).max(axis=1))


@pytest.mark.parametrize("per", PERS)
def test_factor_is_a_function_of_the_record_alone(per):
    B = 3
    rng = np.random.default_rng(per + 1)
    c, u = outputs("random", B, per, rng)
    call = lambda cc, uu, **kw: _native.guidance_rescale(cc, uu, W_G, PHI, **kw)
    scratch = torch.empty(_native.guidance_rescale_scratch_bytes(B, per), dtype=torch.uint8, device=DEV)
    scratch.fill_(0xFF)                                             # any contents (NaNs, as doubles)
    batch = call(dev(c), dev(u), scratch=scratch)
    again = call(dev(c), dev(u), scratch=scratch)                   # the same scratch, as the first call left it
    assert torch.equal(batch, again) and bool(torch.isfinite(batch).all()) and bool((batch < 1).all())
    assert torch.equal(call(dev(c), dev(u)), batch)                 # a fresh scratch
    for b in range(B):                                              # alone, and at every position of a batch of three
        alone = call(dev(c[b:b + 1]), dev(u[b:b + 1]))
        assert torch.equal(alone[0], batch[b]), b
        for pos in range(B):
            order = [(b + pos + i) % B for i in range(B)]
            moved = call(dev(c[order]), dev(u[order]))
            assert torch.equal(moved[order.index(b)], batch[b]), (b, pos)
    # the pointers off 16-byte alignment take the 4-byte loads: the same sums in the same order
    for off_c, off_u in ((1, 1), (1, 0), (0, 3), (2, 2)):
        got = call(shifted(c, off_c), shifted(u, off_u))
        assert torch.equal(got, batch), (off_c, off_u)


@pytest.mark.parametrize("per", PERS)
def test_constant_and_non_finite_records(per):
    rng = np.random.default_rng(per + 2)
    c, u = outputs("random", 3, per, rng)
    c[1], u[1] = 0.25, 0.25                                         # std_cfg == 0: nothing to rescale
    got = host(_native.guidance_rescale(dev(c), dev(u), W_G, PHI))
    assert got[1] == 1.0 and np.isfinite(got).all() and (ulps(got, ref.factor(c, u, W_G, PHI)) <= 1).all()
    zeros = np.zeros((2, per), np.float32)                          # a zero-initialised head
    assert np.array_equal(host(_native.guidance_rescale(dev(zeros), dev(zeros), W_G, PHI)), np.ones(2, np.float32))
    for bad in (np.nan, np.inf, -np.inf):
        for which in (0, 1):
            for at in (0, per // 2, per - 1):
                cc, uu = outputs("random", 3, per, rng)
                (cc, uu)[which][1, at] = bad
                got = host(_native.guidance_rescale(dev(cc), dev(uu), W_G, PHI))
                assert np.isnan(got[1]) and np.isfinite(got[[0, 2]]).all(), (bad, which, at, got)
                assert same_bits(np.isnan(got), np.isnan(ref.factor(cc, uu, W_G, PHI)))


# ---------------------------------------------------------------------------------------------------------------------- 2. the step
@pytest.mark.parametrize("shape,offset", [((2, 768), 0), ((3, 969), 0), ((2, 768), 1), ((2, 12288), 0)])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("with_hist", [False, True])
@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("noise_kind", ["none", "noise", "seeds"])
@pytest.mark.parametrize("with_thr", [False, True])
def test_sampler_step_gscale_matches_the_replica(shape, offset, guided, with_hist, pred, noise_kind, with_thr):
    n = shape[0] * shape[1]
    g = torch.Generator().manual_seed(n + offset)
    seeds = [11, 2 ** 63 + 5, 2 ** 32 - 1][:shape[0]]
    draw, sigma = 4, 0.25 if noise_kind != "none" else 0.0
    k = torch.tensor([0.73, 1.19, 0.5][:shape[0]], device=DEV)      # GIVEN factors: the step is tested on its own

    def buf(fill=None):
        raw = torch.randn(n + 8, generator=g).mul_(2).to(DEV) if fill is None else torch.full((n + 8,), fill, device=DEV)
        return raw[offset:offset + n].view(shape)
    x0, yc, yu, h0 = buf(), buf(), buf(), buf()
    out_u, coef = (yu if guided else None), (COEF if with_hist else COEF[:4])
    thr = None
    if with_thr:
        thr = _native.x0_threshold(x0, yc, coef, pred, 0.9, out_u=out_u, w=W_G, gscale=k)
        raw = ref.raw_x0(host(x0), host(yc), coef[0], coef[1], pred, host(k), host(out_u), W_G)
        assert same_bits(host(thr), threshold_ref.threshold(raw, 0.9)) and bool((thr > 1).all())
    noise = _native.normal_fill(seeds, shape, draw, device=DEV) if noise_kind != "none" else None
    kw = dict(seeds=seeds, draw=draw) if noise_kind == "seeds" else dict(noise=noise)

    def state():
        x, hist, dup = buf(0.0).copy_(x0), buf(0.0).copy_(h0) if with_hist else None, buf(float("nan")) if guided else None
        return x, hist, dup
    x, hist, dup = state()
    _native.sampler_step(x, yc, coef, pred, out_u=out_u, w=W_G, hist=hist, sigma=sigma, x_dup=dup, thr=thr, gscale=k, **kw)
    want_x, want_x0 = ref.step(host(x0), host(yc), coef, pred, host(k), host(thr), host(out_u), W_G, host(h0) if with_hist else None, sigma,
                               host(noise))
    assert np.isfinite(want_x).all() and same_bits(host(x), want_x)
    if with_hist:
        assert same_bits(host(hist), want_x0)
    if guided:
        assert torch.equal(dup, x)
    # gscale=None is the call without it, and a factor of 1 is that call too (a multiplication by 1 is exact)
    xa, ha, da = state()
    _native.sampler_step(xa, yc, coef, pred, out_u=out_u, w=W_G, hist=ha, sigma=sigma, x_dup=da, thr=thr, gscale=None, **kw)
    xb, hb, db = state()
    _native.sampler_step(xb, yc, coef, pred, out_u=out_u, w=W_G, hist=hb, sigma=sigma, x_dup=db, thr=thr, **kw)
    xc, hc, dc = state()
    _native.sampler_step(xc, yc, coef, pred, out_u=out_u, w=W_G, hist=hc, sigma=sigma, x_dup=dc, thr=thr, gscale=torch.ones_like(k), **kw)
    assert torch.equal(xa, xb) and torch.equal(xc, xb) and not torch.equal(xa, x)
    if with_hist:
        assert torch.equal(ha, hb) and torch.equal(hc, hb)
    if guided:
        assert torch.equal(da, db) and torch.equal(dc, db)


@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("guided", [False, True])
def test_x0_threshold_gscale_matches_the_reference(per, B, pred, guided):
    rng = np.random.default_rng(per + 11 * B)
    x = (rng.standard_normal((B, per)) * 3).astype(np.float32)
    c, u = outputs("random", B, per, rng)
    k = np.array([0.73, 1.19, 0.5][:B], np.float32)
    yu = u if guided else None
    raw = ref.raw_x0(x, c, COEF[0], COEF[1], pred, k, yu, W_G)
    for p in (0.5, 0.995, 1.0):
        want = threshold_ref.threshold(raw, p)
        got = _native.x0_threshold(dev(x), dev(c), COEF, pred, p, out_u=dev(yu), w=W_G, gscale=dev(k))
        assert same_bits(host(got), want), (p, host(got), want)
        plain = _native.x0_threshold(dev(x), dev(c), COEF, pred, p, out_u=dev(yu), w=W_G)
        assert torch.equal(_native.x0_threshold(dev(x), dev(c), COEF, pred, p, out_u=dev(yu), w=W_G, gscale=None), plain)
        assert torch.equal(_native.x0_threshold(dev(x), dev(c), COEF, pred, p, out_u=dev(yu), w=W_G, gscale=torch.ones(B, device=DEV)), plain)
    got = _native.x0_threshold(shifted(x, 1), dev(c), COEF, pred, 0.995, out_u=dev(yu), w=W_G, gscale=dev(k))
    assert same_bits(host(got), threshold_ref.threshold(raw, 0.995))


# -------------------------------------------------------------------------------------------------------------------- 3. the loops
B, S, T, ETA, P = 2, 16, 6, 0.03, 0.995
SHAPE = (B, 3, S, S)
RUN_SEEDS = [7, 2 ** 63 + 8]


@pytest.fixture(scope="module")
def nets(tiny_sd):
    """The networks of tests/test_gpu_threshold.py: ``out.*`` scaled by 0.1, and ``out.bias - 2`` for the ones read as v-predictors."""
    made = {}
    for pred in ("eps", "v"):
        sd = {k: (v * np.float32(0.1) if k.startswith("out.") else v) for k, v in tiny_sd.items()}
        if pred == "v":
            sd["out.bias"] = sd["out.bias"] - np.float32(2.0)
        for d in ("fp32", "bf16"):
            net = CLIPCondUNet(z_dim=512, base=32, ch_mult=(1, 2), dtype=d).to(DEV).eval()
            net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
            made[(d, pred)] = net
    return made


@pytest.fixture(scope="module")
def z_dev(synth):
    return torch.from_numpy(synth.synth_z(B)).to(DEV)


@pytest.fixture(scope="module")
def x_T():
    return _native.normal_fill(RUN_SEEDS, SHAPE, 0, device=DEV)


def make_sampler(kind, sch, pred, **kw):
    if kind == "dpmpp2m":
        return DPMSolverSampler(sch, guided=True, prediction=pred, **kw)
    return DDIMSampler(sch, eta=ETA if kind == "ddim_eta" else 0.0, guided=True, prediction=pred, **kw)


def foreign(net):
    return lambda x, zz, t: net(x, zz, t)


@pytest.mark.parametrize("kind", ["ddim", "ddim_eta", "dpmpp2m"])
@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("thr", [None, P])
def test_rescaled_loops_fp32(nets, z_dev, x_T, kind, pred, thr):
    net, sch = nets[("fp32", pred)], NoiseScheduler(1000, "linear", DEV)
    extra = dict(seeds=RUN_SEEDS) if kind == "ddim_eta" else {}
    run = lambda s, model=net: s.sample(model, z_dev, SHAPE, steps=T, cfg_scale=W_G, x_T=x_T, **extra)
    opts = dict(dynamic_threshold=thr) if thr is not None else {}
    base_sampler = make_sampler(kind, sch, pred, **opts)
    base = run(base_sampler)                                        # the run that never had a rescale, first on this slot
    sampler = make_sampler(kind, sch, pred, guidance_rescale=PHI, **opts)
    a = run(sampler)                                                # fused, with the graph
    assert bool(torch.isfinite(a).all()) and not torch.equal(a, base)
    plain = make_sampler(kind, sch, pred, guidance_rescale=PHI, **opts)
    plain.use_graph = False
    assert torch.equal(run(plain), a)                               # launch by launch
    d = run(sampler, foreign(net))                                  # the stepwise route
    print(f"{kind} {pred} thr={thr}: rescaled vs not max-abs {float((a - base).abs().max()):.3e}, stepwise vs fused {float((a - d).abs().max()):.3e}")
    assert torch.equal(d, a), float((a - d).abs().max())
    # None, and a run after toggling it off, are the run that never had it; both graphs live on
    assert torch.equal(run(make_sampler(kind, sch, pred, guidance_rescale=None, **opts)), base)
    assert torch.equal(run(base_sampler), base)
    assert torch.equal(run(sampler), a)
    # another phi on the same slot gives that phi's result, and the first phi's graph still gives the first
    other = make_sampler(kind, sch, pred, guidance_rescale=1.0, **opts)
    o = run(other)
    assert not torch.equal(o, a) and not torch.equal(o, base) and torch.equal(o, run(other, foreign(net)))
    assert torch.equal(run(sampler), a)
    # cfg_scale == 1 takes the unguided route: the rescale is skipped, same bits as a sampler without it
    one = lambda s: s.sample(net, z_dev, SHAPE, steps=T, cfg_scale=1.0, x_T=x_T, **extra)
    assert torch.equal(one(sampler), one(base_sampler))


@pytest.mark.parametrize("kind", ["ddim", "dpmpp2m"])
@pytest.mark.parametrize("pred", ["eps", "v"])
def test_rescaled_loops_bf16(nets, z_dev, x_T, kind, pred):
    net, sch = nets[("bf16", pred)], NoiseScheduler(1000, "linear", DEV)
    run = lambda s: s.sample(net, z_dev, SHAPE, steps=T, cfg_scale=W_G, x_T=x_T)
    base = run(make_sampler(kind, sch, pred))
    a = run(make_sampler(kind, sch, pred, guidance_rescale=PHI))
    plain = make_sampler(kind, sch, pred, guidance_rescale=PHI)
    plain.use_graph = False
    assert bool(torch.isfinite(a).all()) and torch.equal(run(plain), a) and not torch.equal(a, base)
    assert torch.equal(run(make_sampler(kind, sch, pred)), base)


def test_the_loop_applies_the_factor_of_the_reference(nets, z_dev, x_T):
    """One fused step against the numpy statement fed with the device's own network outputs: the factor within 1 ulp (shown by the
    reference's own update on the device's factor being the fused state, bit for bit)."""
    net, sch = nets[("fp32", "eps")], NoiseScheduler(1000, "linear", DEV)
    ts, coef = sch.ddim_timesteps(T), sch.ddim_coefficients(T, 0.0)[:, :4]
    got = net.sample_ddim(z_dev, x_T, ts[:1], coef[:1], guidance=W_G, null_z=None, guidance_rescale=PHI, slot=5)
    t_b = torch.full((B,), int(ts[0]), device=DEV, dtype=torch.long)
    yc, yu = net(x_T, z_dev, t_b), net(x_T, torch.zeros_like(z_dev), t_b)
    k = _native.guidance_rescale(yc, yu, W_G, PHI)
    flat = lambda t: host(t).reshape(B, -1)
    assert (ulps(host(k), ref.factor(flat(yc), flat(yu), W_G, PHI)) <= 1).all()
    want, _ = ref.step(flat(x_T), flat(yc), coef[0], "eps", host(k), None, flat(yu), W_G)
    assert same_bits(flat(got), want)


def test_handle_state_errors(nets, z_dev, x_T):
    """The handle's own CCN_EINVAL cases (a handle needs a device): a bad phi, a NULL, misaligned or short scratch, a scratch too
    small for a later guided call's shape -- and an unguided call ignores the state."""
    net, sch = nets[("fp32", "eps")], NoiseScheduler(1000, "linear", DEV)
    nat = net.native(torch.device(DEV))
    lib = nat.lib
    per = 3 * S * S
    small = torch.empty(_native.guidance_rescale_scratch_bytes(1, 2) + 16, dtype=torch.uint8, device=DEV)
    assert small.numel() < _native.guidance_rescale_scratch_bytes(B, per)
    for bad in (1.5, -0.1, float("nan")):
        assert lib.ccn_set_guidance_rescale(nat.h, bad, small.data_ptr(), small.numel()) == 1
    assert lib.ccn_set_guidance_rescale(nat.h, PHI, small.data_ptr() + 4, small.numel() - 4) == 1
    assert lib.ccn_set_guidance_rescale(nat.h, PHI, None, 0) == 1
    assert lib.ccn_set_guidance_rescale(nat.h, PHI, small.data_ptr(), 16) == 1
    # accepted by the setter (it fits the smallest shape), too small for this one: the guided sampling call's CCN_EINVAL
    assert lib.ccn_set_guidance_rescale(nat.h, PHI, small.data_ptr(), small.numel()) == 0
    ts, coef = sch.ddim_timesteps(T), np.ascontiguousarray(sch.ddim_coefficients(T, 0.0)[:, :4])
    out = torch.empty_like(x_T)
    stream = _native.current_stream(x_T.device)
    ws2 = nat.workspace(2 * B, S, S, T, 3)
    eps = torch.empty((2 * B,) + SHAPE[1:], device=DEV)
    rc = lib.ccn_sample_guided(nat.h, z_dev.data_ptr(), None, x_T.data_ptr(), out.data_ptr(), B, S, S, T, ts.ctypes.data, coef.ctypes.data, None, None, W_G,
                               eps.data_ptr(), ws2.ptr, ws2.nbytes, stream, 1)
    assert rc == 1 and b"too small" in lib.ccn_last_error()
    ws1 = nat.workspace(B, S, S, T, 3)
    rc = lib.ccn_sample(nat.h, z_dev.data_ptr(), x_T.data_ptr(), out.data_ptr(), B, S, S, T, ts.ctypes.data, coef.ctypes.data, ws1.ptr, ws1.nbytes,
                        stream, 1)
    assert rc == 0                                                   # unguided: nothing to match, the state is not read
    torch.cuda.synchronize()
    want = DDIMSampler(sch).sample(net, z_dev, SHAPE, steps=T, x_T=x_T, slot=4)
    assert torch.equal(out, want)
    assert lib.ccn_set_guidance_rescale(nat.h, 0.0, None, 0) == 0
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------------- 4. zero terminal SNR
@pytest.mark.parametrize("schedule", ["linear", "cosine"])
def test_zero_snr_loops(nets, z_dev, x_T, schedule):
    net = nets[("fp32", "v")]
    sch = NoiseScheduler(1000, schedule, DEV, rescale_zero_snr=True)
    assert float(sch.alphas_cumprod[-1]) == 0.0
    samplers = [DDIMSampler(sch, prediction="v"), DPMSolverSampler(sch, spacing="logsnr", prediction="v"),
                DPMSolverSampler(sch, spacing="linspace", prediction="v")]
    for s in samplers:
        a = s.sample(net, z_dev, SHAPE, steps=T, x_T=x_T)
        assert bool(torch.isfinite(a).all())
        d = s.sample(foreign(net), z_dev, SHAPE, steps=T, x_T=x_T)
        assert torch.equal(d, a), (type(s).__name__, float((a - d).abs().max()))
    # step 0, a_t = 0: x0 = -v, e = x; the fused state against the numpy update fed with the device's own network output
    flat = lambda t: host(t).reshape(B, -1)
    for ts, coef in ((sch.ddim_timesteps(T), sch.ddim_coefficients(T, 0.0)[:, :4]), samplers[1].tables(T)):
        assert int(ts[0]) == 999 and coef[0, 0] == 1.0 and coef[0, 1] == 0.0 and np.isfinite(coef).all()
        row = np.concatenate([coef[0, :4], [0.0]]).astype(np.float32)
        fused = net.sample_ddim(z_dev, x_T, ts[:1], coef[:1, :4], prediction="v", slot=6) if coef.shape[1] == 4 else \
            net.sample_ddim(z_dev, x_T, ts[:2], coef[:2, :4], c4=coef[:2, 4], prediction="v", slot=6)
        v = net(x_T, z_dev, torch.full((B,), 999, device=DEV, dtype=torch.long))
        want, x0 = threshold_ref.step(flat(x_T), flat(v), row[:4], "v", np.ones(B, np.float32))
        assert same_bits(x0, np.clip(-flat(v), -1, 1))               # c1 = 0, c0 = 1: x0 = clamp(0 x - 1 v)
        if coef.shape[1] == 4:
            assert same_bits(flat(fused), want)
        else:                                                       # the multistep entry needs two rows: replay the second as well
            v1 = net(dev(want.reshape(SHAPE)), z_dev, torch.full((B,), int(ts[1]), device=DEV, dtype=torch.long))
            assert coef[1, 4] == 0.0
            want1, _ = threshold_ref.step(want, flat(v1), coef[1], "v", np.ones(B, np.float32), hist=x0)
            assert same_bits(flat(fused), want1)


def test_zero_snr_train_step_at_the_last_timestep(tiny_sd):
    """``train_step(prediction="v")`` with every ``t = T-1`` on the zero-SNR schedule (x_t is the noise itself, the target -x0):
    finite, and equal to ``autograd_objective_step`` on a second net at the tolerances of tests/test_gpu_vpred_train.py (5e-5
    relative on the loss, 5 % of the Adam movement + 1e-7 on the parameters)."""
    from clip_feature_codec.train.diffusion_train import FusedAdamW, autograd_objective_step, train_step
    golden = np.load(Path(__file__).resolve().parent / "golden" / "train_step.npz")
    x0, z, noise = (torch.from_numpy(golden[k]).to(DEV) for k in ("x0", "z", "noise"))
    t = torch.full((x0.shape[0],), 999, device=DEV, dtype=torch.long)
    sch = NoiseScheduler(1000, "cosine", DEV, rescale_zero_snr=True)
    assert torch.equal(sch.q_sample(x0, t, noise), noise)
    made = []
    for _ in range(2):
        net = CLIPCondUNet(z_dim=512, base=32, ch_mult=(1, 2), dtype="fp32").to(DEV)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in tiny_sd.items()}, strict=True)
        made.append((net.train(), FusedAdamW(net, lr=2e-4)))
    init = {k: p.detach().clone() for k, p in made[0][0].named_parameters()}
    fused = train_step(made[0][0], sch, made[0][1], x0, z, t, noise, recon_w=0.05, tv_w=1e-4, prediction="v").clone()
    d_v = made[0][0].train_state().static_buffers(x0, z)["d_eps"]
    assert bool(torch.isfinite(fused)) and bool(torch.isfinite(d_v).all()) and bool((d_v != 0).any())
    auto = autograd_objective_step(made[1][0], sch, made[1][1], x0, z, t, noise, recon_w=0.05, tv_w=1e-4, prediction="v")
    rel = abs(float(fused) - float(auto)) / float(auto)
    print(f"zero-SNR v step at t = T-1: loss {float(fused):.7f}, autograd {float(auto):.7f} (relative {rel:.2e})")
    assert rel < 5e-5
    worst = 0.0
    for (k, p), (_, q) in zip(made[0][0].named_parameters(), made[1][0].named_parameters()):
        assert bool(torch.isfinite(p).all()), k
        moved = float((q.detach() - init[k]).abs().max())
        dist = float((p.detach() - q.detach()).abs().max())
        worst = max(worst, dist / max(moved, 1e-30))
        assert dist <= 0.05 * moved + 1e-7, (k, dist, moved)
    print(f"worst parameter distance from the autograd route after one step: {worst:.4f} of the Adam movement (bound 0.05)")
    with pytest.raises(ValueError, match="zero_snr.*prediction"):
        train_step(made[0][0], sch, made[0][1], x0, z, t, noise)
