"""The multistep sampler (DPM-Solver++ 2M) on the GPU: the stand-alone update kernels bit for bit against the fp32 op sequence of
``multistep_ref``, the order-1 identity with the existing loop, the fused loop (``ccn_sample_ms`` / ``ccn_sample_guided_ms``) against
the CPU oracle model driven by the reference loop, its routes, graphs and error paths.  All on the C1-sized model (base 32,
``(1, 2)``), B = 2, 32 px, 6 steps unless a test says otherwise.

Tables and inputs.  The comparison with the oracle (3.) covers cosine / logsnr, linear / logsnr and cosine / linspace.  Where the
table is the test's own choice it is the well-conditioned one, decided on the CPU from the oracle alone (docs/EXPERIMENTS.md R16.3
has the figures): cosine / linspace for the guided comparison with the oracle, linear / logsnr for the bf16 bounds and the second
shape.  Six log-SNR steps of the cosine schedule start at t = 999, 998, 994, where 1 / sqrt(alpha_bar) amplifies any disagreement in
eps by up to 6e4; there the routes are compared with each other, and the bf16 figures are printed, not bounded."""
import ctypes

import numpy as np
import pytest
import torch

import multistep_ref as R
from clip_feature_codec import _native
from clip_feature_codec.models.unet import CLIPCondUNet
from clip_feature_codec.diffusion.scheduler import NoiseScheduler
from clip_feature_codec.diffusion.ddim import DDIMSampler
from clip_feature_codec.diffusion.dpm_solver import DPMSolverSampler
from oracle import ref_unet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TOL_E2E_FP32 = 1e-3       # tests/test_gpu_parity.py: BASELINE.json north_star, max-abs on the reconstructed tensor
B, S, T, W_G = 2, 32, 6, 3.0
SHAPE = (B, 3, S, S)
CASES = (("cosine", "logsnr"), ("linear", "logsnr"), ("cosine", "linspace"))


def to_dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(DEV)


def maxerr(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def make_net(sd, dtype="fp32"):
    net = CLIPCondUNet(z_dim=512, base=32, ch_mult=(1, 2), dtype=dtype).to(DEV).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net


def oracle_guided(model, w, null_row):
    def f(x, z, t):
        eu = model(x, null_row.expand(x.shape[0], -1), t)
        return R.guided_fp32(model(x, z, t), eu, w)
    return f


def oracle_sample(model, z, xT, schedule, spacing, order, steps=T):
    ts = R.timesteps(steps, spacing, schedule)
    return R.sample_fp32(model, z, xT, ts, R.coefficients64(ts, order, schedule))


@pytest.fixture(scope="module")
def tiny_net(tiny_sd):
    return make_net(tiny_sd)


@pytest.fixture(scope="module")
def cpu_model(tiny_sd):
    return ref_unet.make_model(ref_unet.as_torch_sd(tiny_sd))


@pytest.fixture(scope="module")
def inputs(synth):
    """Start noise of ``seed_base=900``: of the seeds 0, 100 ... 900 the one for which the oracle's own sample moves least when its eps
    is perturbed by +-1e-6, worst case over the loops compared with the oracle below (CPU only; docs/EXPERIMENTS.md R16.3)."""
    return torch.from_numpy(synth.synth_z(B)), torch.from_numpy(synth.start_noise(range(B), S, seed_base=900))


@pytest.fixture(scope="module")
def gpu_2m_cosine(tiny_net, inputs):
    """The fused order-2 sample (cosine, logsnr; first call: capture + replay); shared, never written to."""
    sampler = DPMSolverSampler(NoiseScheduler(1000, "cosine", DEV))
    return sampler, sampler.sample(tiny_net, to_dev(inputs[0]), SHAPE, steps=T, x_T=to_dev(inputs[1]))


# ----------------------------------------------------------------------------------------------------------------- 1. the kernels
N_STRIDE = 2048 * 256 * 4 + 3 * 256 * 4 + 3      # past the grid cap of the four-wide form: every lane strides, three-element tail
ROWS = R.coefficients64(R.timesteps(20, "logsnr", "cosine"), 2, "cosine").astype(np.float32)


def _kernel_case(n, row, c4, w=None, with_dup=False, offset=0, nan_hist=False):
    """One launch against ``multistep_ref.update_fp32`` on the CPU; ``w``: the guided kernel, on ``eu + w * (ec - eu)``.  ``offset``:
    the tensors are views that many floats into their buffers (1 and 2 take the one-element-per-lane form)."""
    coef = ROWS[row].copy()
    coef[4] = np.float32(c4)
    g = torch.Generator().manual_seed(1000 * row + n % 997)
    x, ec, eu, hist = (torch.randn(n, generator=g) for _ in range(4))
    e = ec if w is None else R.guided_fp32(ec, eu, w)
    x = float(coef[1]) * 1.2 * x + float(coef[0]) * e                      # x0 ~ 1.2 N(0, 1): both sides of the clamp
    hist = hist.clamp(-1, 1)
    ref_x, ref_x0 = R.update_fp32(x, e, hist, coef)
    assert bool((ref_x0.abs() == 1).any()) and bool((ref_x0.abs() < 1).any()) or n == 1

    def view(t):
        return torch.cat([torch.zeros(offset), t]).to(DEV)[offset:]
    xd, ecd, eud = view(x), view(ec), view(eu)
    hd = view(torch.full((n,), float("nan")) if nan_hist else hist)
    dup = view(torch.full((n,), 7.0)) if with_dup else None
    assert xd.data_ptr() % 16 == (4 * offset) % 16
    if w is None:
        _native.ms_step(xd, hd, ecd, coef)
    else:
        _native.cfg_ms_step(xd, hd, ecd, eud, w, coef, x_dup=dup)
    what = f"n={n} row={row} c4={c4} w={w} dup={with_dup} offset={offset}"
    assert np.array_equal(xd.cpu().numpy(), ref_x.numpy()), what
    assert np.array_equal(hd.cpu().numpy(), ref_x0.numpy()), what + ": the history is not the clamped x0"
    if with_dup:
        assert torch.equal(dup, xd), what + ": x_dup differs from x"
    assert torch.equal(ecd.cpu(), ec) and torch.equal(eud.cpu(), eu), what + ": an input was written"


@pytest.mark.parametrize("n", [1, 255, 2 * 3 * 17 * 19, 2 * 3 * 64 * 64])
@pytest.mark.parametrize("c4", [0.0, 0.37])
def test_ms_step_bit_exact(n, c4):
    _kernel_case(n, (n + 3) % 14, c4)
    for w in (0.0, 1.3, 3.0):
        for with_dup in (False, True):
            _kernel_case(n, int(w * 10 + n) % 14, c4, w=w, with_dup=with_dup)


@pytest.mark.parametrize("n,offset", [(255, 1), (2 * 3 * 17 * 19, 1), (2 * 3 * 17 * 19, 2), (N_STRIDE, 0), (256 * 2048 + 5, 1)])
def test_ms_step_bit_exact_other_paths(n, offset):
    """Unaligned pointers (one element per lane), and sizes past the grid cap of either form (the grid-stride loop)."""
    for c4 in (0.0, 0.37):
        _kernel_case(n, 4, c4, offset=offset)
        _kernel_case(n, 9, c4, w=3.0, with_dup=True, offset=offset)
        _kernel_case(n, 11, c4, w=1.3, offset=offset)


@pytest.mark.parametrize("n,offset", [(255, 0), (255, 1), (2 * 3 * 64 * 64, 0)])
def test_history_is_not_read_without_c4(n, offset):
    """c4 == 0 and a NaN-filled history: the result is the reference's (finite), and the history is overwritten."""
    _kernel_case(n, 5, 0.0, offset=offset, nan_hist=True)
    _kernel_case(n, 5, 0.0, w=3.0, with_dup=True, offset=offset, nan_hist=True)


# --------------------------------------------------------------------------------------------------------- 2. the order-1 identity
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "f16x3"])
def test_order_one_is_the_existing_loop(tiny_sd, inputs, dtype):
    """c4 == 0 everywhere: ccn_sample_ms equals ccn_sample on the same table bit for bit, in every mode -- the new path leaves both
    head kernels' arithmetic alone.  The order-2 call between them shares the workspace and must find its own graph."""
    net = make_net(tiny_sd, dtype)
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sch = NoiseScheduler(1000, "cosine", DEV)
    sampler = DPMSolverSampler(sch, order=1, spacing="linspace")
    ts, coef = sampler.tables(T)
    assert np.all(coef[:, 4] == 0)
    a = sampler.sample(net, z, SHAPE, steps=T, x_T=xT)
    b = net.native().sample(z, xT, ts, coef[:, :4])
    second = DPMSolverSampler(sch, order=2, spacing="linspace").sample(net, z, SHAPE, steps=T, x_T=xT)
    c = sampler.sample(net, z, SHAPE, steps=T, x_T=xT)
    d = net.native().sample(z, xT, ts, coef[:, :4])
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(b, d)
    assert not torch.equal(second, a)


# ------------------------------------------------------------------------------------------------------- 3. fused loop vs the oracle
@pytest.mark.parametrize("schedule,spacing", CASES)
def test_fused_2m_matches_oracle_and_the_order_matters(tiny_net, cpu_model, inputs, schedule, spacing):
    z, xT = inputs
    ref2 = oracle_sample(cpu_model, z, xT, schedule, spacing, 2)
    ref1 = oracle_sample(cpu_model, z, xT, schedule, spacing, 1)
    gap = maxerr(ref2, ref1)
    sampler = DPMSolverSampler(NoiseScheduler(1000, schedule, DEV), order=2, spacing=spacing)
    got = sampler.sample(tiny_net, to_dev(z), SHAPE, steps=T, x_T=to_dev(xT))
    err = maxerr(got, ref2)
    print(f"{schedule}/{spacing}: fused 2M vs oracle max-abs {err:.3e}; oracle order 2 vs order 1: {gap:.3e}")
    assert got.shape == SHAPE and got.device == torch.device(DEV)
    assert gap > 10 * TOL_E2E_FP32, gap           # (CPU only) a sampler that drops the correction term fails by more than 10x
    assert err < TOL_E2E_FP32, err


# ------------------------------------------------------------------------------------------------------------------------ 4. routes
def test_routes_agree(tiny_net, inputs, gpu_2m_cosine):
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sampler, a = gpu_2m_cosine
    b = sampler.sample(tiny_net, z, SHAPE, steps=T, x_T=xT)                                 # graph replay
    assert torch.equal(a, b)
    plain = DPMSolverSampler(sampler.sch)
    plain.use_graph = False
    c = plain.sample(tiny_net, z, SHAPE, steps=T, x_T=xT)                                   # launch by launch
    assert torch.equal(a, c)
    d = sampler.sample(lambda x, zz, t: tiny_net(x, zz, t), z, SHAPE, steps=T, x_T=xT)      # stepwise route
    print(f"stepwise vs fused 2M: max-abs {maxerr(a, d):.3e}")
    assert maxerr(a, d) < 1e-3, maxerr(a, d)


def test_ddim_and_2m_graphs_share_a_workspace(tiny_net, inputs, gpu_2m_cosine):
    """Both samplers at 6 table entries on one shape use the same plan, workspace and list of captured graphs."""
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sampler, first = gpu_2m_cosine
    assert len(sampler.tables(T)[0]) == T
    ddim = DDIMSampler(sampler.sch)
    d1 = ddim.sample(tiny_net, z, SHAPE, steps=T, x_T=xT)
    m1 = sampler.sample(tiny_net, z, SHAPE, steps=T, x_T=xT)
    d2 = ddim.sample(tiny_net, z, SHAPE, steps=T, x_T=xT)
    m2 = sampler.sample(tiny_net, z, SHAPE, steps=T, x_T=xT)
    assert torch.equal(d1, d2) and torch.equal(m1, m2) and torch.equal(m1, first)
    assert maxerr(d1, m1) > 10 * TOL_E2E_FP32


# ------------------------------------------------------------------------------------------------------------------------ 5. guided
@pytest.fixture(scope="module")
def gpu_guided_2m(tiny_net, inputs):
    sampler = DPMSolverSampler(NoiseScheduler(1000, "cosine", DEV), spacing="linspace", guided=True)
    return sampler, sampler.sample(tiny_net, to_dev(inputs[0]), SHAPE, steps=T, cfg_scale=W_G, x_T=to_dev(inputs[1]))


def test_guided_2m_matches_oracle(synth, tiny_net, cpu_model, inputs, gpu_guided_2m):
    z, xT = inputs
    ref = oracle_sample(oracle_guided(cpu_model, W_G, torch.zeros(512)), z, xT, "cosine", "linspace", 2)
    err = maxerr(gpu_guided_2m[1], ref)
    row = torch.from_numpy(synth.synth_z(1, seed=77)[0])
    ref_row = oracle_sample(oracle_guided(cpu_model, W_G, row), z, xT, "cosine", "linspace", 2)
    got_row = DPMSolverSampler(NoiseScheduler(1000, "cosine", DEV), spacing="linspace", guided=True, null_z=row).sample(
        tiny_net, to_dev(z), SHAPE, steps=T, cfg_scale=W_G, x_T=to_dev(xT))
    err_row = maxerr(got_row, ref_row)
    print(f"guided 2M vs oracle: zero null {err:.3e}, non-zero null {err_row:.3e}; the null row moves the oracle by {maxerr(ref, ref_row):.3e}")
    assert maxerr(ref, ref_row) > 10 * TOL_E2E_FP32
    assert err < TOL_E2E_FP32, err
    assert err_row < TOL_E2E_FP32, err_row


def test_guided_scale_one_is_unguided(tiny_net, inputs, gpu_2m_cosine):
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    g = DPMSolverSampler(gpu_2m_cosine[0].sch, guided=True)
    assert torch.equal(g.sample(tiny_net, z, SHAPE, steps=T, cfg_scale=1.0, x_T=xT), gpu_2m_cosine[1])
    # without the flag cfg_scale is accepted and unused, as in DDIMSampler
    assert torch.equal(gpu_2m_cosine[0].sample(tiny_net, z, SHAPE, steps=T, cfg_scale=3.0, x_T=xT), gpu_2m_cosine[1])


def test_guided_routes_and_graphs(tiny_net, inputs, gpu_guided_2m):
    """Guided 2M and guided DDIM share the workspace of batch 2B; replay, launch by launch and stepwise as in test_routes_agree."""
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sampler, first = gpu_guided_2m
    ddim = DDIMSampler(sampler.sch, guided=True)
    d1 = ddim.sample(tiny_net, z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT)
    m1 = sampler.sample(tiny_net, z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT)
    d2 = ddim.sample(tiny_net, z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT)
    m2 = sampler.sample(tiny_net, z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT)
    assert torch.equal(d1, d2) and torch.equal(m1, m2) and torch.equal(m1, first)
    assert maxerr(d1, m1) > 10 * TOL_E2E_FP32
    plain = DPMSolverSampler(sampler.sch, spacing="linspace", guided=True)
    plain.use_graph = False
    assert torch.equal(plain.sample(tiny_net, z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT), first)
    step = sampler.sample(lambda x, zz, t: tiny_net(x, zz, t), z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT)
    print(f"guided stepwise vs fused 2M: max-abs {maxerr(first, step):.3e}")
    assert maxerr(first, step) < 1e-3, maxerr(first, step)


def test_guided_routes_on_the_default_table(tiny_net, inputs):
    """cosine / logsnr, what the CLIs build: replay, launch by launch and the stepwise route against the fused guided loop.  Both
    routes round each step's eps alike, so the comparison is stable where the one with the oracle is not."""
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sampler = DPMSolverSampler(NoiseScheduler(1000, "cosine", DEV), guided=True)
    first = sampler.sample(tiny_net, z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT)
    assert torch.equal(sampler.sample(tiny_net, z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT), first)
    plain = DPMSolverSampler(sampler.sch, guided=True)
    plain.use_graph = False
    assert torch.equal(plain.sample(tiny_net, z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT), first)
    step = sampler.sample(lambda x, zz, t: tiny_net(x, zz, t), z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT)
    print(f"guided stepwise vs fused 2M, cosine / logsnr: max-abs {maxerr(first, step):.3e}")
    assert bool(torch.isfinite(first).all())
    assert maxerr(first, step) < 1e-3, maxerr(first, step)


def test_guided_batch_b_and_unguided_batch_2b_share_a_slot(tiny_sd, inputs):
    """A guided call of batch B and an unguided one of batch 2B use one workspace slot (the plan's batch is 2B for both), but
    histories of B and of 2B rows: each call must get a history of its own size, and the results are those of a fresh handle."""
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    z4, x4 = torch.cat([z, z.flip(0)]), torch.cat([xT, xT.flip(0)])
    shape4 = (2 * B, 3, S, S)
    sch = NoiseScheduler(1000, "cosine", DEV)
    guided, plain = DPMSolverSampler(sch, guided=True), DPMSolverSampler(sch)
    net = make_net(tiny_sd)
    g1 = guided.sample(net, z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT)
    u1 = plain.sample(net, z4, shape4, steps=T, x_T=x4)
    g2 = guided.sample(net, z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT)
    u2 = plain.sample(net, z4, shape4, steps=T, x_T=x4)
    ws = net.native().workspace(2 * B, S, S, T)
    assert sorted(ws.hist) == [xT.numel(), x4.numel()]
    assert all(h.numel() == n for n, h in ws.hist.items())
    fresh = make_net(tiny_sd)
    uf = plain.sample(fresh, z4, shape4, steps=T, x_T=x4)          # (unguided first here: the other order of allocation)
    gf = guided.sample(fresh, z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT)
    torch.cuda.synchronize()
    net.native().poll_errors()
    assert torch.equal(u1, uf) and torch.equal(u1, u2)
    assert torch.equal(g1, gf) and torch.equal(g1, g2)


# ---------------------------------------------------------------------------------------------------------------- 6. a second shape
def test_second_shape(synth, tiny_sd, tiny_net, cpu_model):
    """B = 3, 40 x 48 px (the width is no multiple of the bf16 head's 32-pixel tile), 4 steps, linear / logsnr (t = 999, 603, 73, 0;
    c4 = 0, 0.47, 0.48, 0; the oracle's orders differ by 0.84 here, and a +-1e-6 perturbation of eps moves it by 1.9e-4); fp32 against
    the oracle, bf16 within the bounds of test_bf16_order_two_bounded."""
    b, h, w, steps = 3, 40, 48, 4
    z = torch.from_numpy(synth.synth_z(b, seed=50))
    xT = torch.randn((b, 3, h, w), generator=torch.Generator().manual_seed(48))
    ref = oracle_sample(cpu_model, z, xT, "linear", "logsnr", 2, steps)
    sch = NoiseScheduler(1000, "linear", DEV)
    got = DPMSolverSampler(sch).sample(tiny_net, to_dev(z), (b, 3, h, w), steps=steps, x_T=to_dev(xT))
    assert maxerr(got, ref) < TOL_E2E_FP32, maxerr(got, ref)
    lo = DPMSolverSampler(sch).sample(make_net(tiny_sd, "bf16"), to_dev(z), (b, 3, h, w), steps=steps, x_T=to_dev(xT))
    d = (lo - got).abs()
    print(f"bf16 vs fp32 2M at {b} x {h} x {w}, {steps} steps: max-abs {float(d.max()):.3e} mean-abs {float(d.mean()):.3e}")
    assert bool(torch.isfinite(lo).all())
    assert float(d.max()) < 0.6 and float(d.mean()) < 0.065, (float(d.max()), float(d.mean()))


# -------------------------------------------------------------------------------------------------------------------------- 7. bf16
def test_bf16_order_two_bounded(tiny_sd, tiny_net, inputs, gpu_2m_cosine):
    """bf16 mode: finite, and within the bounds test_guided_bf16_bounded uses (0.6 max, 0.065 mean).  They catch garbage, not rounding.
    On the linear / logsnr table (see the module's docstring); the cosine / logsnr figures are printed, not bounded."""
    net = make_net(tiny_sd, dtype="bf16")
    ill = DPMSolverSampler(gpu_2m_cosine[0].sch).sample(net, to_dev(inputs[0]), SHAPE, steps=T, x_T=to_dev(inputs[1]))
    d = (ill - gpu_2m_cosine[1]).abs()
    print(f"bf16 vs fp32 2M, cosine / logsnr (not bounded): max-abs {float(d.max()):.3e} mean-abs {float(d.mean()):.3e}")
    assert bool(torch.isfinite(ill).all())
    sampler = DPMSolverSampler(NoiseScheduler(1000, "linear", DEV))
    x = sampler.sample(net, to_dev(inputs[0]), SHAPE, steps=T, x_T=to_dev(inputs[1]))
    d = (x - sampler.sample(tiny_net, to_dev(inputs[0]), SHAPE, steps=T, x_T=to_dev(inputs[1]))).abs()
    print(f"bf16 vs fp32 2M, linear / logsnr (C1 size, {T} steps): max-abs {float(d.max()):.3e} mean-abs {float(d.mean()):.3e}")
    assert bool(torch.isfinite(x).all())
    assert float(d.max()) < 0.6 and float(d.mean()) < 0.065, (float(d.max()), float(d.mean()))


# ------------------------------------------------------------------------------------------------------------------- 8. error paths
def test_error_paths(tiny_net, inputs, gpu_2m_cosine):
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sampler, first = gpu_2m_cosine
    sch = sampler.sch
    with pytest.raises(ValueError, match="shape mismatch"):
        sampler.sample(tiny_net, z[:1], SHAPE, steps=T, x_T=xT)
    with pytest.raises(ValueError, match="finite"):
        DPMSolverSampler(sch, guided=True).sample(tiny_net, z, SHAPE, steps=T, cfg_scale=float("nan"), x_T=xT)
    with pytest.raises(ValueError, match="null_z"):
        DPMSolverSampler(sch, guided=True, null_z=torch.zeros(3)).sample(tiny_net, z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT)
    with pytest.raises(ValueError):
        tiny_net.sample_ddim(z, xT, sampler.tables(T)[0], sampler.tables(T)[1][:, :4], c4=np.zeros(T - 1, np.float32))
    with pytest.raises(ValueError, match="deterministic"):
        tiny_net.sample_ddim(z, xT, sampler.tables(T)[0], sampler.tables(T)[1][:, :4], c4=np.zeros(T, np.float32), sigma=np.zeros(T, np.float32),
                             noise=torch.zeros((T,) + SHAPE, device=DEV))
    # the native wrapper's checks
    nat = tiny_net.native()
    ts, coef = sampler.tables(T)
    with pytest.raises(ValueError, match="coef"):
        nat.sample(z, xT, ts, coef[:, :4], hist=torch.empty_like(xT))
    for bad in (torch.empty(xT.numel() - 1, device=DEV), torch.empty(xT.numel(), device=DEV, dtype=torch.float64),
                torch.empty(xT.numel()), torch.empty(xT.numel() + 1, device=DEV)[1:]):
        with pytest.raises(ValueError, match="hist"):
            nat.sample(z, xT, ts, coef, hist=bad)
        with pytest.raises(ValueError, match="hist"):
            nat.sample(z, xT, ts, coef, w=W_G, hist=bad)
    with pytest.raises(ValueError, match="finite"):
        nat.sample(z, xT, ts, coef, w=float("inf"))
    with pytest.raises(ValueError, match="null_z"):
        nat.sample(z, xT, ts, coef, w=W_G, z_null=torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match="same number"):
        _native.ms_step(xT.clone(), torch.empty(5, device=DEV), xT, coef[1])
    with pytest.raises(ValueError, match="same number"):
        _native.cfg_ms_step(xT.clone(), torch.empty_like(xT), xT, xT[:1], W_G, coef[1])
    # the library's own checks, below the Python ones: CCN_EINVAL for c4 != 0 on step 0, a non-finite coefficient, a null history
    for k, (i, j, v) in enumerate(((0, 4, 0.25), (2, 4, float("nan")), (3, 1, float("inf")), (1, 0, float("nan")))):
        bad = coef.copy()
        bad[i, j] = v
        with pytest.raises(ValueError, match="c4 must be 0 on step 0" if k == 0 else "non-finite"):
            nat.sample(z, xT, ts, bad)
        with pytest.raises(ValueError, match="c4 must be 0 on step 0" if k == 0 else "non-finite"):
            nat.sample(z, xT, ts, bad, w=W_G)
    ws = nat.workspace(B, S, S, T)
    out = torch.empty_like(xT)
    tsc, cc = np.ascontiguousarray(ts, np.int32), np.ascontiguousarray(coef, np.float32)
    rc = nat.lib.ccn_sample_ms(nat.h, z.data_ptr(), xT.data_ptr(), out.data_ptr(), B, S, S, T, tsc.ctypes.data, cc.ctypes.data, None,
                               ws.ptr, ws.nbytes, _native.current_stream(xT.device), 1)
    assert rc == 1, rc                               # CCN_EINVAL
    ws2 = nat.workspace(2 * B, S, S, T)
    eps = torch.empty((2 * B, 3, S, S), device=DEV)
    rc = nat.lib.ccn_sample_guided_ms(nat.h, z.data_ptr(), None, xT.data_ptr(), out.data_ptr(), B, S, S, T, tsc.ctypes.data, cc.ctypes.data,
                                      ctypes.c_float(W_G), eps.data_ptr(), None, ws2.ptr, ws2.nbytes, _native.current_stream(xT.device), 1)
    assert rc == 1, rc                               # CCN_EINVAL
    again = sampler.sample(tiny_net, z, SHAPE, steps=T, x_T=xT)
    torch.cuda.synchronize()
    tiny_net.native().poll_errors()
    assert torch.equal(again, first)


def test_cli_refuses_eta_with_the_solver():
    from clip_feature_codec.cli import eval as cli_eval, reconstruct_diffusion as cli_rec
    with pytest.raises(SystemExit, match="eta"):
        cli_rec.main(["--store_dir", "s", "--bitstream", "b", "--weights", "w", "--sampler", "dpmpp2m", "--eta", "0.5"])
    with pytest.raises(SystemExit, match="eta"):
        cli_eval.main(["--store_dir", "s", "--weights", "w", "--sampler", "dpmpp2m", "--eta", "0.5"])
