"""Dynamic thresholding on the GPU: the per-record quantile against the numpy reference (tests/threshold_ref.py) bit for bit on
inputs chosen to break a radix select, record independence and a reusable scratch, the thresholded step against its float32
replica, and the thresholded sampler loops (fused with the graph, launch by launch, stepwise) against each other and against the
unthresholded loops.  The C1-sized model (base 32, ``(1, 2)``) with ``out.*`` scaled by 0.1, B = 2, 16 px, 6 steps, linear table."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import threshold_ref as ref  # noqa: E402

from clip_feature_codec import _native
from clip_feature_codec.models.unet import CLIPCondUNet
from clip_feature_codec.diffusion.scheduler import NoiseScheduler
from clip_feature_codec.diffusion.ddim import DDIMSampler
from clip_feature_codec.diffusion.dpm_solver import DPMSolverSampler

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

PERS = [768, 969, 12288]      # 3*16*16; 3*17*19: no multiple of 4, rows off alignment; 3*64*64: several workgroups per record
PS = [1e-4, 0.5, 0.995, 1.0]
COEF = (0.6, 0.8, 0.85, 0.52, 0.37)
W_G = 3.0
PATTERNS = ["random", "five_levels", "all_equal", "low_bits", "zeros_denormals", "one_inf", "nan_record"]


def same_bits(a, b):
    """Equal as bit patterns, any NaN equal to any NaN (inf - inf is another NaN pattern on the host than on the device)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def pattern(kind, B, per, rng):
    """``(B, per)`` float32 raw x0 values of one kind (with identity coefficients the kernel's raw x0 is exactly these values)."""
    sign = rng.choice([-1.0, 1.0], (B, per)).astype(np.float32)
    if kind == "random":
        return (rng.standard_normal((B, per)) * 3).astype(np.float32)
    if kind == "five_levels":                                       # heavy ties straddling ranks k and k + 1
        return (rng.integers(0, 5, (B, per)) * 0.75).astype(np.float32) * sign
    if kind == "all_equal":
        return np.full((B, per), 1.7, np.float32) * sign
    if kind == "low_bits":                                          # the top 22 bits shared, the low 10 differ: two passes see one bin
        return (np.uint32(0x40490C00) | rng.integers(0, 1024, (B, per)).astype(np.uint32)).view(np.float32) * sign
    if kind == "zeros_denormals":
        bits = rng.integers(0, 1000, (B, per)).astype(np.uint32)    # +0 and denormals ...
        bits[:, ::7] = 0
        bits[:, 3::11] = np.uint32(0x3F900000)                      # ... and a few normal values
        return bits.view(np.float32) * sign                         # (-0 among them)
    v = (rng.standard_normal((B, per)) * 3).astype(np.float32)
    if kind == "one_inf":
        v[:, per // 3] = np.inf
        return v
    assert kind == "nan_record"
    v[B - 1, 5] = np.nan                                            # the last record alone
    v[B - 1, per // 2] = np.nan
    return v


def device_case(kind, B, per, pred, guided, rng):
    """Device tensors and the reference's raw x0 for one case.  ``random``: general coefficients, outputs and guidance; the designed
    patterns: c1 = 1 and zero outputs, so that raw x0 == x exactly in either parameterisation, with or without the combine."""
    x = pattern(kind, B, per, rng)
    if kind == "random":
        c0, c1 = COEF[:2]
        yc = rng.standard_normal((B, per)).astype(np.float32)
        yu = rng.standard_normal((B, per)).astype(np.float32) if guided else None
    else:
        c0, c1 = 0.6, 1.0
        yc = np.zeros((B, per), np.float32)
        yu = np.zeros((B, per), np.float32) if guided else None
    raw = ref.raw_x0(x, yc, c0, c1, pred, yu, W_G)
    if kind != "random":
        assert same_bits(np.abs(raw), np.abs(x))
    dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    return dev(x), dev(yc), dev(yu), (c0, c1), raw


# ---------------------------------------------------------------------------------------------------------------- 1. the quantile
@pytest.mark.parametrize("per", PERS)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("guided", [False, True])
def test_quantile_matches_reference_bit_for_bit(per, B, pred, guided):
    rng = np.random.default_rng(per + 7 * B)
    scratch = torch.empty(_native.x0_threshold_scratch_bytes(B, per), dtype=torch.uint8, device=DEV)
    for kind in PATTERNS:
        x, yc, yu, c, raw = device_case(kind, B, per, pred, guided, rng)
        for p in PS:
            want = ref.threshold(raw, p)
            got = _native.x0_threshold(x, yc, c, pred, p, out_u=yu, w=W_G, scratch=scratch).cpu().numpy()
            assert same_bits(got, want), (kind, p, got, want)
            if kind == "nan_record":                                # NaNs sort last: the maximum meets one, in that record alone
                assert np.isfinite(got[:B - 1]).all()
                assert bool(np.isnan(got[B - 1])) == (p == 1.0), (p, got)
            if kind == "one_inf" and p <= 0.995:
                assert np.isfinite(got).all()                       # an ordinary largest value
        # an x pointer off 16-byte alignment takes the one-element loads: the same bits
        want = ref.threshold(raw, 0.995)
        for off in (1, 2, 3):
            buf = torch.zeros(B * per + 8, device=DEV)
            xo = buf[off:off + B * per].view(B, per).copy_(x)
            assert xo.data_ptr() % 16 == 4 * off
            got = _native.x0_threshold(xo, yc, c, pred, 0.995, out_u=yu, w=W_G, scratch=scratch).cpu().numpy()
            assert same_bits(got, want), (kind, off, got, want)


@pytest.mark.parametrize("per", PERS)
def test_threshold_is_clamped_to_one_and_to_a_finite_maximum(per):
    rng = np.random.default_rng(per)
    raw = np.stack([rng.standard_normal(per) * 0.1, rng.standard_normal(per) * 5, rng.standard_normal(per) * 0.8]).astype(np.float32)
    x, y = torch.from_numpy(raw).to(DEV), torch.zeros((3, per), device=DEV)
    free = ref.threshold(raw, 0.995)
    assert free[0] == 1.0 and free[1] > 3.0 and 1.0 < free[2] < 3.0   # below 1, above the maximum, between the two
    for mx in (None, 3.0, 1.0):
        got = _native.x0_threshold(x, y, (0.6, 1.0), "eps", 0.995, mx).cpu().numpy()
        want = ref.threshold(raw, 0.995, np.inf if mx is None else mx)
        assert same_bits(got, want), (mx, got, want)
        assert got[0] == 1.0 and got[1] == (free[1] if mx is None else mx) and got[2] == (1.0 if mx == 1.0 else free[2])
        assert (got >= 1.0).all() and (mx is None or (got <= mx).all())


# ------------------------------------------------------------------------------------------------------ 2. record independence
@pytest.mark.parametrize("per", PERS)
def test_row_is_its_own_record_and_the_scratch_is_left_ready(per):
    B = 3
    rng = np.random.default_rng(per + 1)
    x, yc, yu = (torch.from_numpy((rng.standard_normal((B, per)) * 2).astype(np.float32)).to(DEV) for _ in range(3))
    scratch = torch.empty(_native.x0_threshold_scratch_bytes(B, per), dtype=torch.uint8, device=DEV)
    scratch.fill_(0xA5)                                             # any contents
    call = lambda xs, ys, us, **kw: _native.x0_threshold(xs, ys, COEF, "v", 0.995, out_u=us, w=W_G, **kw)
    batch = call(x, yc, yu, scratch=scratch)
    again = call(x, yc, yu, scratch=scratch)                        # the same scratch, as the first call left it
    assert torch.equal(batch, again)
    assert bool((batch > 1).any())
    for b in range(B):
        alone = call(x[b:b + 1].contiguous(), yc[b:b + 1].contiguous(), yu[b:b + 1].contiguous())
        assert torch.equal(alone[0], batch[b]), b
    flipped = call(x.flip(0).contiguous(), yc.flip(0).contiguous(), yu.flip(0).contiguous(), scratch=scratch)
    assert torch.equal(flipped.flip(0), batch)


# --------------------------------------------------------------------------------------------------------------------- 3. the step
@pytest.mark.parametrize("shape,offset", [((2, 768), 0), ((3, 969), 0), ((2, 768), 1), ((2, 12288), 0)])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("with_hist", [False, True])
@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("noise_kind", ["none", "noise", "seeds"])
def test_sampler_step_thr_matches_the_replica(shape, offset, guided, with_hist, pred, noise_kind):
    n = shape[0] * shape[1]
    g = torch.Generator().manual_seed(n + offset)
    seeds = [11, 2 ** 63 + 5, 2 ** 32 - 1][:shape[0]]
    draw, sigma = 4, 0.25 if noise_kind != "none" else 0.0

    def buf(fill=None):
        raw = torch.randn(n + 8, generator=g).mul_(2).to(DEV) if fill is None else torch.full((n + 8,), fill, device=DEV)
        return raw[offset:offset + n].view(shape)
    x0, yc, yu, h0 = buf(), buf(), buf(), buf()
    out_u, coef = (yu if guided else None), (COEF if with_hist else COEF[:4])
    thr = _native.x0_threshold(x0, yc, coef, pred, 0.9, out_u=out_u, w=W_G)
    assert bool((thr > 1).all())                                    # the 0.9 quantile: a tenth of every record is clamped
    noise = _native.normal_fill(seeds, shape, draw, device=DEV) if noise_kind != "none" else None
    kw = dict(seeds=seeds, draw=draw) if noise_kind == "seeds" else dict(noise=noise)

    def state():
        x, hist, dup = buf(0.0).copy_(x0), buf(0.0).copy_(h0) if with_hist else None, buf(float("nan")) if guided else None
        return x, hist, dup
    x, hist, dup = state()
    _native.sampler_step(x, yc, coef, pred, out_u=out_u, w=W_G, hist=hist, sigma=sigma, x_dup=dup, thr=thr, **kw)
    host = lambda t: None if t is None else t.cpu().numpy()
    want_x, want_x0 = ref.step(host(x0), host(yc), coef, pred, host(thr), host(out_u), W_G, host(h0) if with_hist else None, sigma, host(noise))
    assert np.isfinite(want_x).all() and same_bits(host(x), want_x)
    if with_hist:
        assert same_bits(host(hist), want_x0) and float(np.abs(want_x0).max()) <= 1.0
    if guided:
        assert torch.equal(dup, x)
    # thr = 1 is the static clamp, bit for bit: the entry without thr on the same inputs
    xa, ha, da = state()
    _native.sampler_step(xa, yc, coef, pred, out_u=out_u, w=W_G, hist=ha, sigma=sigma, x_dup=da, thr=torch.ones(shape[0], device=DEV), **kw)
    xb, hb, db = state()
    _native.sampler_step(xb, yc, coef, pred, out_u=out_u, w=W_G, hist=hb, sigma=sigma, x_dup=db, **kw)
    assert torch.equal(xa, xb) and not torch.equal(xa, x)
    if with_hist:
        assert torch.equal(ha, hb)
    if guided:
        assert torch.equal(da, db)


# -------------------------------------------------------------------------------------------------------------------- 4. the loops
B, S, T, ETA, P = 2, 16, 6, 0.03, 0.995
SHAPE = (B, 3, S, S)
RUN_SEEDS = [7, 2 ** 63 + 8]


@pytest.fixture(scope="module")
def nets(tiny_sd):
    """``out.*`` scaled by 0.1: the predicted noise is small, so the eps form's x0 ~ x / a is far outside [-1, 1] on the early steps
    of the linear table.  The v form has no division: x0 = a x - s v stays inside [-1, 1] with a small v (every threshold would be 1
    and the tests would show nothing), so the networks read as v-predictors also get ``out.bias - 2``: x0 ~ a x + 2 s."""
    assert "out.weight" in tiny_sd and "out.bias" in tiny_sd
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


def make_sampler(kind, sch, guided, pred, **thr):
    if kind == "ddim":
        return DDIMSampler(sch, eta=0.0, guided=guided, prediction=pred, **thr)
    return DPMSolverSampler(sch, guided=guided, prediction=pred, **thr)


def stepwise_by_hand(net, kind, sampler, z, x_T, guided, pred):
    """ccn_forward + x0_threshold + sampler_step(thr=) per step, the thresholds of every step kept."""
    if kind == "ddim":
        ts, coef = sampler.sch.ddim_timesteps(T), sampler.sch.ddim_coefficients(T, 0.0)[:, :4]
    else:
        ts, coef = sampler.tables(T)
    x, hist, z_u, thrs = x_T.clone(), torch.empty_like(x_T) if kind != "ddim" else None, torch.zeros_like(z), []
    for i in range(len(ts)):
        t_b = torch.full((B,), int(ts[i]), device=DEV, dtype=torch.long)
        out_c = net(x, z, t_b)
        out_u = net(x, z_u, t_b) if guided else None
        thr = _native.x0_threshold(x, out_c, coef[i], pred, P, out_u=out_u, w=W_G)
        _native.sampler_step(x, out_c, coef[i], pred, out_u=out_u, w=W_G if guided else 0.0, hist=hist, thr=thr)
        thrs.append(thr.cpu().numpy())
    return x, np.stack(thrs)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("kind", ["ddim", "dpmpp2m"])
def test_thresholded_loops(nets, z_dev, x_T, dtype, guided, pred, kind):
    net, sch = nets[(dtype, pred)], NoiseScheduler(1000, "linear", DEV)
    kw = dict(cfg_scale=W_G) if guided else {}
    run = lambda s, model=net: s.sample(model, z_dev, SHAPE, steps=T, x_T=x_T, **kw)
    base_sampler = make_sampler(kind, sch, guided, pred)
    base = run(base_sampler)                                        # the unthresholded loop, first on this slot
    sampler = make_sampler(kind, sch, guided, pred, dynamic_threshold=P)
    a = run(sampler)                                                # fused, with the graph
    assert bool(torch.isfinite(a).all()) and not torch.equal(a, base)
    plain = make_sampler(kind, sch, guided, pred, dynamic_threshold=P)
    plain.use_graph = False
    assert torch.equal(run(plain), a)                               # launch by launch
    # the stepwise route of the sampler (a foreign callable) and the same route by hand, which shows the thresholds
    d = run(sampler, lambda x, zz, t: net(x, zz, t))
    hand, thrs = stepwise_by_hand(net, kind, sampler, z_dev, x_T, guided, pred)
    assert torch.equal(d, hand)
    print(f"{dtype} guided={guided} {pred} {kind}: thresholds per step\n{thrs}\nstepwise vs fused max-abs {float((a - d).abs().max()):.3e}")
    assert (thrs >= 1).all() and bool((thrs > 1).all(axis=1).any())  # some step thresholds every record above 1
    if dtype == "fp32":
        assert torch.equal(d, a), float((a - d).abs().max())
    else:                                                           # the suite's bound for bf16 trajectories (test_gpu_rng.py)
        dist = (a - d).abs()
        assert float(dist.max()) < 0.6 and float(dist.mean()) < 0.065, (float(dist.max()), float(dist.mean()))
    # a maximum of 1 makes every threshold 1: the static clamp, through the split route
    capped = make_sampler(kind, sch, guided, pred, dynamic_threshold=P, threshold_max=1.0)
    assert torch.equal(run(capped), base)
    # both graphs live on: the unthresholded sampler on the same slot returns what it returned before, and so does the thresholded
    assert torch.equal(run(base_sampler), base)
    assert torch.equal(run(sampler), a)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("guided", [False, True])
def test_seeded_eta_thresholded_equals_materialised_draws(nets, z_dev, x_T, dtype, guided):
    net, sch = nets[(dtype, "eps")], NoiseScheduler(1000, "linear", DEV)
    kw = dict(cfg_scale=W_G) if guided else {}
    sampler = DDIMSampler(sch, eta=ETA, guided=guided, dynamic_threshold=P)
    a = sampler.sample(net, z_dev, SHAPE, steps=T, x_T=x_T, seeds=RUN_SEEDS, **kw)
    ts, coef = sch.ddim_timesteps(T), sch.ddim_coefficients(T, ETA, cap_sigma=True)
    assert np.isfinite(coef).all() and (coef[:-1, 4] > 0).all()
    noise = torch.stack([_native.normal_fill(RUN_SEEDS, SHAPE, 1 + i, device=DEV) for i in range(T)])
    guide = dict(guidance=W_G, null_z=None) if guided else {}
    want = net.sample_ddim(z_dev, x_T, ts, coef[:, :4], sigma=coef[:, 4], noise=noise, dynamic_threshold=P, **guide)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, want)
    unthresholded = DDIMSampler(sch, eta=ETA, guided=guided).sample(net, z_dev, SHAPE, steps=T, x_T=x_T, seeds=RUN_SEEDS, **kw)
    assert not torch.equal(a, unthresholded)
    # the stepwise route with seeds and thresholds: one trajectory with the fused loop in fp32
    d = sampler.sample(lambda x, zz, t: net(x, zz, t), z_dev, SHAPE, steps=T, x_T=x_T, seeds=RUN_SEEDS, **kw)
    if dtype == "fp32":
        assert torch.equal(d, a)
    else:
        dist = (a - d).abs()
        assert float(dist.max()) < 0.6 and float(dist.mean()) < 0.065, (float(dist.max()), float(dist.mean()))


def test_handle_state_errors(nets, z_dev, x_T):
    """The handle's own CCN_EINVAL cases (a handle needs a device): a short scratch for the shape, a bad quantile or maximum."""
    import ctypes
    net, sch = nets[("fp32", "eps")], NoiseScheduler(1000, "linear", DEV)
    nat = net.native(torch.device(DEV))
    lib, n = nat.lib, ctypes.c_size_t()
    assert lib.ccn_dynamic_threshold_scratch_bytes(nat.h, B, S, S, ctypes.byref(n)) == 0
    per = 3 * S * S
    assert n.value >= B * per * 4 + B * 4 + _native.x0_threshold_scratch_bytes(B, per) and n.value % 16 == 0
    assert lib.ccn_dynamic_threshold_scratch_bytes(nat.h, 65536, S, S, ctypes.byref(n)) == 1
    small = torch.empty(_native.x0_threshold_scratch_bytes(1, 1) + 64, dtype=torch.uint8, device=DEV)
    for bad in ((1.5, 2.0), (float("nan"), 2.0), (0.9, 0.5), (0.9, float("nan"))):
        assert lib.ccn_set_dynamic_threshold(nat.h, bad[0], bad[1], small.data_ptr(), small.numel()) == 1
    assert lib.ccn_set_dynamic_threshold(nat.h, 0.9, 2.0, small.data_ptr() + 4, small.numel() - 4) == 1
    assert lib.ccn_set_dynamic_threshold(nat.h, 0.9, 2.0, None, 0) == 1
    # accepted by the setter (it fits the smallest shape), too small for this one: the sampling call's CCN_EINVAL
    assert lib.ccn_set_dynamic_threshold(nat.h, 0.9, 2.0, small.data_ptr(), small.numel()) == 0
    ts, coef = sch.ddim_timesteps(T), np.ascontiguousarray(sch.ddim_coefficients(T, 0.0)[:, :4])
    ws = nat.workspace(B, S, S, T, 3)
    out = torch.empty_like(x_T)
    rc = lib.ccn_sample(nat.h, z_dev.data_ptr(), x_T.data_ptr(), out.data_ptr(), B, S, S, T, ts.ctypes.data, coef.ctypes.data, ws.ptr, ws.nbytes,
                        _native.current_stream(x_T.device), 1)
    assert rc == 1 and b"too small" in lib.ccn_last_error()
    assert lib.ccn_set_dynamic_threshold(nat.h, 0.0, 0.0, None, 0) == 0
    torch.cuda.synchronize()
