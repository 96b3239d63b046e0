"""The low-resolution guide on the GPU.

1. ``ccn_lowres_delta`` and ``ccn_block_mean`` against the numpy statement (tests/guide_ref.py), bit for bit: the block sums are int64
   sums of exactly converted values, so there is nothing to tolerate.  Shapes that put quads across blocks and rows, a width that is
   no power of two, one block per plane, 4096-element blocks driven to +-1, several strips per plane; B = 1 and 3, both
   parameterisations, guided or not, with and without ``thr`` / ``gscale``, pointers off by 4 bytes (the 4-byte loads), inputs that
   hit the clamp rarely, sometimes and mostly.  A record's ``d`` does not depend on B, its position or the call.
2. ``sampler_step(delta=)`` against the float32 replica, bit for bit; ``delta=None`` is ``ccn_sampler_step_rs``.
3. The loops of ``CLIPCondUNet(z_dim=512, base=32, ch_mult=(1, 2))`` at 16 px, N = 4, 6 steps: fused with the graph == fused launch
   by launch == stepwise in fp32; graph == launch by launch in bf16; the thumbnail of a lambda = 1 result; the handle state."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guide_ref as ref  # noqa: E402

from clip_feature_codec import _native  # noqa: E402
from clip_feature_codec.models.unet import CLIPCondUNet  # noqa: E402
from clip_feature_codec.diffusion.scheduler import NoiseScheduler  # noqa: E402
from clip_feature_codec.diffusion.ddim import DDIMSampler  # noqa: E402
from clip_feature_codec.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32

# (C, H, W, N)
SHAPES = [(3, 2, 6, 2), (3, 8, 24, 4), (3, 16, 16, 16), (1, 64, 128, 64), (3, 32, 32, 8)]
SCALES = [0.01, 0.5, 3.0]
COEF = (0.6, 0.8, 0.85, 0.52, 0.37)
W_G = 3.0
THR = np.array([1.7, 1.0, 2.5], F)
GSCALE = np.array([0.73, 1.19, 0.5], F)


def same_bits(a, b):
    """Equal as bit patterns, any NaN equal to any NaN."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def shifted(a, off):
    """A device copy of ``a`` whose data pointer is ``4 * off`` bytes past a 16-byte boundary (``off`` 0: ``dev``)."""
    if a is None:
        return None
    buf = torch.zeros(a.size + 8, device=DEV)
    t = buf[off:off + a.size].view(a.shape).copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4 * off
    return t


def inputs(C, H, W, N, B, scale, rng):
    x, yc, yu = ((rng.standard_normal((B, C, H, W)) * scale).astype(F) for _ in range(3))
    g = rng.uniform(-1, 1, (B, C, H // N, W // N)).astype(F)
    return x, yc, yu, g


# ---------------------------------------------------------------------------------------------------------------- 1. delta, block mean
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("off", [0, 1])
def test_delta_matches_the_reference(shape, B, off):
    C, H, W, N = shape
    rng = np.random.default_rng(C * H * W + N + 5 * B)
    hit = 0
    for scale in SCALES:
        x, yc, yu, g = inputs(C, H, W, N, B, scale, rng)
        for pred in ("eps", "v"):
            for guided in (False, True):
                for thr, gs in ((None, None), (THR[:B], None), (None, GSCALE[:B]), (THR[:B], GSCALE[:B])):
                    out_u = yu if guided else None
                    lam = 1.0 if thr is None else 0.6
                    want = ref.lowres_delta(x, yc, COEF, g, N, lam, pred, out_u, W_G, thr, gs)
                    got = _native.lowres_delta(shifted(x, off), shifted(yc, off), COEF, dev(g), lam, pred, out_u=shifted(out_u, off), w=W_G,
                                               thr=dev(thr), gscale=dev(gs))
                    assert np.isfinite(want).all() and same_bits(host(got), want), (scale, pred, guided, thr is not None, gs is not None)
        raw = (x - F(COEF[0]) * yc) / F(COEF[1])
        hit = max(hit, float((np.abs(raw) > 1).mean()))
    assert hit > 0.5                                                # the largest scale puts most of x0 on the clamp


def test_saturated_blocks_reach_the_largest_sum():
    """4096-element blocks with every x0 at +1 or at -1: |S| = N^2 2^30, the largest a block sum gets; d = g -+ 1 exactly."""
    C, H, W, N = 1, 64, 128, 64
    x = np.zeros((2, C, H, W), F)
    yc = np.empty_like(x)
    yc[..., :64], yc[..., 64:] = -1e6, 1e6                           # eps form: x0 = (x - c0 e) / c1 -> +1 on the left block, -1 on the right
    g = np.array([0.25, -0.5, 1.0, -1.0], F).reshape(2, 1, 1, 2)
    got = host(_native.lowres_delta(dev(x), dev(yc), COEF, dev(g), 1.0))
    assert same_bits(got, ref.lowres_delta(x, yc, COEF, g, N)) and np.array_equal(got.reshape(-1), np.array([-0.75, 0.5, 0.0, 0.0], F))
    big = np.where(yc < 0, F(7.0), F(-7.0))                         # the plain mean clamps likewise
    assert np.array_equal(host(_native.block_mean(dev(big), N)).reshape(2, 2), np.array([[1, -1], [1, -1]], F))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("off", [0, 1, 3])
def test_block_mean_matches_the_reference(shape, off):
    C, H, W, N = shape
    rng = np.random.default_rng(C * H * W + N)
    for B in (1, 3):
        for scale in SCALES:
            v = (rng.standard_normal((B, C, H, W)) * scale).astype(F)
            got = _native.block_mean(shifted(v, off), N)
            assert tuple(got.shape) == (B, C, H // N, W // N) and same_bits(host(got), ref.block_mean(v, N)), (B, scale)
    # a plane on its own is a plane of the batch; NaN counts as -1 and +-inf as +-1, as the static clamp of the update has it
    v[0, 0, 0, 0], v[0, 0, 1, 1], v[0, 0, H - 1, W - 1] = np.nan, np.inf, -np.inf
    w = np.where(np.isnan(v), F(-1), v)
    assert same_bits(host(_native.block_mean(dev(v), N)), ref.block_mean(w, N))
    assert torch.equal(_native.block_mean(dev(v[1, 0]), N), _native.block_mean(dev(v), N)[1, 0])


@pytest.mark.parametrize("shape", SHAPES)
def test_delta_is_a_function_of_the_record_alone(shape):
    C, H, W, N = shape
    B = 3
    rng = np.random.default_rng(C * H * W + 1)
    x, yc, yu, g = inputs(C, H, W, N, B, 0.5, rng)
    call = lambda sel, off=0: _native.lowres_delta(shifted(x[sel], off), shifted(yc[sel], off), COEF, dev(g[sel]), 0.6, "v", out_u=shifted(yu[sel], off),
                                                   w=W_G, thr=dev(THR[sel]), gscale=dev(GSCALE[sel]))
    batch = call([0, 1, 2])
    assert torch.equal(call([0, 1, 2]), batch)                      # a second call
    for b in range(B):
        assert torch.equal(call([b])[0], batch[b]), b              # alone
        for pos in range(B):                                        # at every position of a batch of three
            order = [(b + pos + i) % B for i in range(B)]
            assert torch.equal(call(order)[order.index(b)], batch[b]), (b, pos)
    for off in (1, 2, 3):                                           # the 4-byte loads
        assert torch.equal(call([0, 1, 2], off), batch), off


# ------------------------------------------------------------------------------------------------------------------------ 2. the step
@pytest.mark.parametrize("shape,off", [((3, 2, 6, 2), 0), ((3, 2, 6, 2), 1), ((3, 8, 24, 4), 0), ((3, 32, 32, 8), 0), ((3, 32, 32, 8), 1)])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("with_hist", [False, True])
@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("noise_kind", ["none", "noise", "seeds"])
def test_sampler_step_delta_matches_the_replica(shape, off, guided, with_hist, pred, noise_kind):
    C, H, W, N = shape
    B = 3
    rng = np.random.default_rng(C * H * W + off)
    x0, yc, yu, g = inputs(C, H, W, N, B, 1.0, rng)
    h0 = rng.standard_normal(x0.shape).astype(F)
    seeds = [11, 2 ** 63 + 5, 2 ** 32 - 1]
    draw, sigma = 4, 0.25 if noise_kind != "none" else 0.0
    coef = COEF if with_hist else COEF[:4]
    out_u = yu if guided else None
    noise = host(_native.normal_fill(seeds, x0.shape, draw, device=DEV)) if noise_kind != "none" else None
    for thr, gs in ((None, None), (THR, None), (None, GSCALE), (THR, GSCALE)):
        d = ref.lowres_delta(x0, yc, coef, g, N, 0.8, pred, out_u, W_G, thr, gs)        # (checked against the kernel's above)

        def run(delta, **more):
            x, hist = shifted(x0, off), shifted(h0, off) if with_hist else None
            dup = shifted(np.full(x0.shape, np.nan, F), off) if guided else None
            kw = dict(seeds=seeds, draw=draw) if noise_kind == "seeds" else dict(noise=shifted(noise, off))
            _native.sampler_step(x, shifted(yc, off), coef, pred, out_u=shifted(out_u, off), w=W_G, hist=hist, sigma=sigma, x_dup=dup, thr=dev(thr),
                                 gscale=dev(gs), delta=delta, **kw, **more)
            if guided:
                assert torch.equal(dup, x)
            return host(x), host(hist)
        got_x, got_h = run(dev(d), factor=N)
        want_x, want_x0 = ref.step(x0, yc, coef, pred, d, N, thr, gs, out_u, W_G, h0 if with_hist else None, sigma, noise)
        assert np.isfinite(want_x).all() and same_bits(got_x, want_x), (thr is not None, gs is not None)
        if with_hist:
            assert same_bits(got_h, want_x0)
        # delta=None is the entry without it (ccn_sampler_step_rs, _thr or the plain one), and so is a table of zeros: x0 + 0 is x0
        none_x, none_h = run(None)
        plain_x, plain_x0 = ref.step(x0, yc, coef, pred, None, N, thr, gs, out_u, W_G, h0 if with_hist else None, sigma, noise)
        assert same_bits(none_x, plain_x) and not same_bits(none_x, got_x)
        zero_x, zero_h = run(dev(np.zeros_like(d)))
        assert same_bits(zero_x, plain_x)
        if with_hist:
            assert same_bits(none_h, plain_x0) and same_bits(zero_h, plain_x0)


def test_delta_none_is_the_rs_entry():
    """``ccn_sampler_step_lr`` with a NULL table against ``ccn_sampler_step_rs`` called directly, whatever C, H, W, N say."""
    lib = _native.load_library()
    rng = np.random.default_rng(2)
    x0, yc, yu, _ = inputs(3, 8, 24, 4, 3, 1.0, rng)
    coef = (ctypes.c_float * 5)(*COEF)
    per, n = 3 * 8 * 24, x0.size
    stream = _native.current_stream(torch.device(DEV))
    outs = []
    for lr in (False, True):
        x, c, u, thr, gs = dev(x0), dev(yc), dev(yu), dev(THR), dev(GSCALE)
        args = (x.data_ptr(), None, None, c.data_ptr(), u.data_ptr(), None, None, 0, per, 1, W_G, coef, 0.0, n, thr.data_ptr(), gs.data_ptr())
        with torch.cuda.device(DEV):
            rc = lib.ccn_sampler_step_lr(*args, 0, 0, 0, 0, None, stream) if lr else lib.ccn_sampler_step_rs(*args, stream)
        assert rc == 0
        outs.append(x)
    assert torch.equal(outs[0], outs[1]) and same_bits(host(outs[0]), ref.step(x0, yc, COEF[:4], "v", None, 4, THR, GSCALE, yu, W_G)[0])


# ----------------------------------------------------------------------------------------------------------------------- 3. the loops
B, S, N_G, T, ETA, P, PHI = 2, 16, 4, 6, 0.03, 0.995, 0.7
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


@pytest.fixture(scope="module")
def guide():
    """A smooth thumbnail inside [-0.6, 0.6]: a gradient per channel and image."""
    i, j = np.meshgrid(np.arange(S // N_G), np.arange(S // N_G), indexing="ij")
    g = np.stack([np.stack([0.6 * np.cos(0.9 * i + 0.5 * c + b) * np.sin(0.7 * j - 0.3 * c) for c in range(3)]) for b in range(B)])
    return torch.from_numpy(g.astype(F)).to(DEV)


def make_sampler(kind, sch, pred, guided, **kw):
    if kind == "dpmpp2m":
        return DPMSolverSampler(sch, guided=guided, prediction=pred, **kw)
    return DDIMSampler(sch, eta=ETA if kind == "ddim_eta" else 0.0, guided=guided, prediction=pred, **kw)


def foreign(net):
    return lambda x, zz, t: net(x, zz, t)


def mid_t(sampler, kind):
    ts = sampler.tables(T)[0] if kind == "dpmpp2m" else sampler.sch.ddim_timesteps(T)
    return int(ts[len(ts) // 2])


@pytest.mark.parametrize("kind", ["ddim", "ddim_eta", "dpmpp2m"])
@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("mode", ["plain", "guided_rs_thr"])
def test_guided_loops_fp32(nets, z_dev, x_T, guide, kind, pred, mode):
    net, sch = nets[("fp32", pred)], NoiseScheduler(1000, "linear", DEV)
    guided = mode != "plain"
    opts = dict(guidance_rescale=PHI, dynamic_threshold=P) if guided else {}
    extra = dict(seeds=RUN_SEEDS) if kind == "ddim_eta" else {}
    sampler = make_sampler(kind, sch, pred, guided, **opts)
    run = lambda s, model=net, **g: s.sample(model, z_dev, SHAPE, steps=T, cfg_scale=W_G if guided else 1.0, x_T=x_T, **extra, **g)
    base = run(sampler)                                             # the run that never had a guide, first on this slot
    for g in (dict(guide=guide), dict(guide=guide, guide_strength=0.5, guide_t_min=mid_t(sampler, kind))):
        a = run(sampler, **g)                                       # fused, with the graph
        assert bool(torch.isfinite(a).all()) and not torch.equal(a, base)
        plain = make_sampler(kind, sch, pred, guided, **opts)
        plain.use_graph = False
        assert torch.equal(run(plain, **g), a)                      # launch by launch
        d = run(sampler, foreign(net), **g)                         # the stepwise route
        print(f"{kind} {pred} {mode} {sorted(g)[1:]}: guide vs none max-abs {float((a - base).abs().max()):.3e}, stepwise vs fused "
              f"{float((a - d).abs().max()):.3e}")
        assert torch.equal(d, a), float((a - d).abs().max())
        assert torch.equal(run(sampler, **g), a)                    # the replay
    # a t_min above every timestep guides no step: the run without a guide, bit for bit
    assert torch.equal(run(sampler, guide=guide, guide_t_min=1000), base)
    assert torch.equal(run(sampler), base)                          # off again


@pytest.mark.parametrize("kind", ["ddim", "dpmpp2m"])
@pytest.mark.parametrize("pred", ["eps", "v"])
def test_guided_loops_bf16(nets, z_dev, x_T, guide, kind, pred):
    net, sch = nets[("bf16", pred)], NoiseScheduler(1000, "linear", DEV)
    for guided in (False, True):
        run = lambda s, **g: s.sample(net, z_dev, SHAPE, steps=T, cfg_scale=W_G if guided else 1.0, x_T=x_T, **g)
        sampler = make_sampler(kind, sch, pred, guided)
        base = run(sampler)
        a = run(sampler, guide=guide)
        plain = make_sampler(kind, sch, pred, guided)
        plain.use_graph = False
        assert bool(torch.isfinite(a).all()) and torch.equal(run(plain, guide=guide), a) and not torch.equal(a, base)
        assert torch.equal(run(sampler), base)


@pytest.mark.parametrize("pred", ["eps", "v"])
@pytest.mark.parametrize("guided", [False, True])
def test_thumbnail_of_the_result(nets, z_dev, x_T, guide, pred, guided):
    """lambda = 1, every step guided, eta 0: the last row of the table has c2 == 1 and c3 == 0, so the result IS the last x0', and its
    block means are the guide's to 3 2^-23 (tests/test_guide_host.py derives the bound).  That row is the multistep solver's; the DDIM
    table keeps the reference's last row, c3 = sqrt(ab_s) = 1 (``NoiseScheduler.ddim_coefficients``), whose result is x0' + e.

    x0' is not clamped again and ``ccn_block_mean`` clamps to [-1, 1], so the bound can hold for ``ccn_block_mean`` only in the blocks
    whose pixels all lie in [-1, 1]; in the others it differs from the guide by the clamped excess.  Measured on an MI355X with these
    inputs, over ALL blocks: 2.2e-3 (eps) and 8.7e-3 (v) with max |result| 1.0032 and 1.0331; 93-95 % (eps) and 39 % (v) of the blocks
    lie inside -- a property of these untrained weights, not of the code, so it is printed and not asserted.  So the test holds every
    block's float64 mean of the unclamped result to the bound (measured 1.7e-8 .. 2.8e-8), and ``ccn_block_mean`` to it on the blocks
    inside (measured 1.5e-8 .. 3.0e-8)."""
    kind = "dpmpp2m"
    net, sch = nets[("fp32", pred)], NoiseScheduler(1000, "linear", DEV)
    sampler = make_sampler(kind, sch, pred, guided)
    coef = sampler.tables(T)[1]
    assert float(coef[-1, 2]) == 1.0 and float(coef[-1, 3]) == 0.0
    ddim_last = sch.ddim_coefficients(T, 0.0)[-1]
    assert float(ddim_last[2]) == 1.0 and float(ddim_last[3]) == 1.0
    out = sampler.sample(net, z_dev, SHAPE, steps=T, cfg_scale=W_G if guided else 1.0, x_T=x_T, guide=guide, guide_strength=1.0, guide_t_min=0)
    thumb = _native.block_mean(out, N_G)
    err_all, err_in, inside = ref.thumbnail_errors(host(out), host(thumb), host(guide), N_G)
    print(f"{kind} {pred} guided={guided}: max |float64 block mean of the result - guide| = {err_all:.3e}, max |ccn_block_mean - guide| over the "
          f"{inside:.0%} of blocks inside [-1, 1] = {err_in:.3e} (bound {3 * 2.0 ** -23:.3e}), over all blocks "
          f"{float((thumb.double() - guide.double()).abs().max()):.3e}, max |result| = {float(out.abs().max()):.4f}")
    assert err_all <= 3 * 2.0 ** -23 and err_in <= 3 * 2.0 ** -23
    base = sampler.sample(net, z_dev, SHAPE, steps=T, cfg_scale=W_G if guided else 1.0, x_T=x_T)
    assert float((_native.block_mean(base, N_G) - guide).abs().max()) > 1e-3          # without the guide the thumbnail is another one


def test_handle_state(nets, z_dev, x_T, guide):
    """Toggling finds each mode's graph; off again is the unguided run; new contents at the same address replay the same graph; the
    scratch size and a scratch too small for a later shape."""
    net, sch = nets[("fp32", "eps")], NoiseScheduler(1000, "linear", DEV)
    nat = net.native(torch.device(DEV))
    lib = nat.lib
    captures = lambda: lib.ccn_internal_graph_captures(nat.h)
    sampler = DDIMSampler(sch)
    run = lambda **g: sampler.sample(net, z_dev, SHAPE, steps=T, x_T=x_T, slot=3, **g)
    base = run()
    n0 = captures()
    a = run(guide=guide)
    assert captures() == n0 + 1 and not torch.equal(a, base)
    assert torch.equal(run(), base) and torch.equal(run(guide=guide), a) and captures() == n0 + 1      # each mode's graph is found again
    other = (guide * -0.5).contiguous()
    b = run(guide=other)                                            # new contents, copied to the same address: the same graph
    assert captures() == n0 + 1 and not torch.equal(b, a)
    assert torch.equal(b, sampler.sample(foreign(net), z_dev, SHAPE, steps=T, x_T=x_T, guide=other))
    half = run(guide=guide, guide_strength=0.5)                     # another strength or t_min is another key
    assert captures() == n0 + 2 and not torch.equal(half, a)
    late = run(guide=guide, guide_t_min=500)
    assert captures() == n0 + 3 and not torch.equal(late, a) and not torch.equal(late, base)
    assert torch.equal(run(), base) and captures() == n0 + 3

    # the scratch: the delta table, then the raw output of one state, each part rounded up to 16 bytes
    n = ctypes.c_size_t()

    def size(b, h, w, blk):
        assert lib.ccn_lowres_guide_scratch_bytes(nat.h, b, h, w, blk, ctypes.byref(n)) == 0
        return n.value
    r16 = lambda v: (v + 15) // 16 * 16
    assert size(B, S, S, N_G) == r16(B * 3 * 16 * 4) + B * 3 * S * S * 4
    assert size(1, 2, 6, 2) == r16(3 * 3 * 4) + r16(36 * 4) and size(3, 64, 128, 64) == r16(3 * 3 * 2 * 4) + 3 * 3 * 64 * 128 * 4
    for bad in ((0, S, S, 4), (65536, S, S, 4), (B, S, S, 3), (B, S, S, 128), (B, S, S, 0), (B, 18, S, 4), (B, S, 20, 8)):
        assert lib.ccn_lowres_guide_scratch_bytes(nat.h, *bad, ctypes.byref(n)) == 1, bad
    assert lib.ccn_lowres_guide_scratch_bytes(nat.h, B, S, S, 4, None) == 1

    # a scratch the setter accepts (it fits the smallest shape) but too small for this shape: the sampling call's CCN_EINVAL
    small = torch.empty(16 + N_G * N_G * 4, dtype=torch.uint8, device=DEV)
    gbuf = guide.clone()
    try:
        assert lib.ccn_set_lowres_guide(nat.h, gbuf.data_ptr(), N_G, 1.0, 0, small.data_ptr(), small.numel() - 1) == 1
        assert lib.ccn_set_lowres_guide(nat.h, gbuf.data_ptr(), N_G, 1.0, 0, small.data_ptr() + 4, small.numel()) == 1
        assert lib.ccn_set_lowres_guide(nat.h, gbuf.data_ptr(), N_G, 1.0, 0, small.data_ptr(), small.numel()) == 0
        ts, coef = sch.ddim_timesteps(T), np.ascontiguousarray(sch.ddim_coefficients(T, 0.0)[:, :4])
        out = torch.empty_like(x_T)
        ws = nat.workspace(B, S, S, T, 3)
        stream = _native.current_stream(x_T.device)
        with torch.cuda.device(DEV):
            rc = lib.ccn_sample(nat.h, z_dev.data_ptr(), x_T.data_ptr(), out.data_ptr(), B, S, S, T, ts.ctypes.data, coef.ctypes.data, ws.ptr,
                                ws.nbytes, stream, 1)
        assert rc == 1 and b"too small" in lib.ccn_last_error()
        # a block size that does not divide this call's image is that call's CCN_EINVAL too
        big = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
        assert lib.ccn_set_lowres_guide(nat.h, gbuf.data_ptr(), 32, 1.0, 0, big.data_ptr(), big.numel()) == 0
        with torch.cuda.device(DEV):
            rc = lib.ccn_sample(nat.h, z_dev.data_ptr(), x_T.data_ptr(), out.data_ptr(), B, S, S, T, ts.ctypes.data, coef.ctypes.data, ws.ptr,
                                ws.nbytes, stream, 1)
        assert rc == 1 and b"multiples of N" in lib.ccn_last_error()
    finally:
        assert lib.ccn_set_lowres_guide(nat.h, None, 0, 0.0, 0, None, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(run(), base)
