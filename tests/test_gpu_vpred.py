"""The v-parameterisation on the GPU: ``ccn_sampler_step`` bit for bit against the fp32 op sequence of ``vpred_ref`` (and, with
``pred = eps``, against the four older step entry points), the fused loops in v mode (``ccn_set_prediction``) against the CPU oracle
model driven by ``vpred_ref``'s fp32 loop, guidance, eta > 0, routes, graph keys, the fast modes and a second shape.  All on the
C1-sized model (base 32, ``(1, 2)``), B = 2, 32 px, 6 steps unless a test says otherwise.

The oracle model's output is simply READ as v: the synthetic weights are trained for nothing, and what is under test is the update.
tests/test_vpred_host.py (item 4) shows on the CPU that the v loop moves by 2e-6 under a +-1e-6 perturbation of the model output on
all three tables, and lies more than 1.0 from the eps loop: the 1e-3 gate holds on the cosine / log-SNR table too, where the eps
form's figures are "printed, not bounded" (tests/test_gpu_multistep.py), and a build that ignores the flag misses it a thousandfold.

Measured on an MI355X (fp32 mode against the oracle, max-abs): see docs/EXPERIMENTS.md R19.
"""
import numpy as np
import pytest
import torch

import multistep_ref as M
import vpred_ref as R
from clip_feature_codec import _native
from clip_feature_codec.models.unet import CLIPCondUNet
from clip_feature_codec.diffusion.scheduler import NoiseScheduler
from clip_feature_codec.diffusion.ddim import DDIMSampler
from clip_feature_codec.diffusion.dpm_solver import DPMSolverSampler
from oracle import ref_unet, ref_diffusion

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TOL_E2E_FP32 = 1e-3       # tests/test_gpu_parity.py: BASELINE.json north_star, max-abs on the reconstructed tensor
B, S, T, W_G = 2, 32, 6, 3.0
SHAPE = (B, 3, S, S)


def to_dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(DEV)


def maxerr(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def make_net(sd, dtype="fp32"):
    net = CLIPCondUNet(z_dim=512, base=32, ch_mult=(1, 2), dtype=dtype).to(DEV).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net


class Stepwise:
    """Hides ``sample_ddim``: the samplers then take the stepwise route (one forward and one ``ccn_sampler_step`` per step)."""

    def __init__(self, net):
        self.net = net

    def __call__(self, x, z, t):
        return self.net(x, z, t)


@pytest.fixture(scope="module")
def tiny_net(tiny_sd):
    return make_net(tiny_sd)


@pytest.fixture(scope="module")
def cpu_model(tiny_sd):
    return ref_unet.make_model(ref_unet.as_torch_sd(tiny_sd))


@pytest.fixture(scope="module")
def inputs(synth):
    return torch.from_numpy(synth.synth_z(B)), torch.from_numpy(synth.start_noise(range(B), S, seed_base=900))


def solver_tables(schedule, spacing, order, steps=T):
    ts = M.timesteps(steps, spacing, schedule)
    return ts, M.coefficients64(ts, order, schedule)


# ----------------------------------------------------------------------------------------------------------------- 1. the kernel
N_STRIDE = 2048 * 256 * 4 + 3 * 256 * 4 + 3      # past the grid cap of the four-wide form: every lane strides, three-element tail
ROWS = M.coefficients64(M.timesteps(20, "logsnr", "cosine"), 2, "cosine").astype(np.float32)
PRED = {"eps": 0, "v": 1}


def _case_tensors(n, coef, w, seed, pred):
    """x, y_c, y_u, hist, noise on the CPU, scaled so that the clamped x0 of the update is ~ 1.2 N(0, 1): both sides of the clamp."""
    g = torch.Generator().manual_seed(seed)
    x0t, et, ru, rc, hist, nz = (torch.randn(n, generator=g) for _ in range(6))
    c0, c1 = float(coef[0]), float(coef[1])
    x = c1 * 1.2 * x0t + c0 * et
    y = c1 * et - c0 * 1.2 * x0t if pred == "v" else et            # v = a eps - s x0
    if w is None:
        return x, y, None, hist.clamp(-1, 1), nz
    return x, y + 0.1 * rc, y + 0.1 * ru, hist.clamp(-1, 1), nz


def _reference(pred, x, yc, yu, w, hist, coef, sigma, nz):
    y = yc if w is None else R.guided_fp32(yc, yu, w)
    if pred == "v":
        return R.update_v_fp32(x, y, hist, coef, sigma, nz)
    xn, x0 = M.update_fp32(x, y, hist, coef)
    if nz is not None:
        xn = xn + torch.tensor(float(np.float32(sigma)), dtype=torch.float32) * nz
    return xn, x0


def _kernel_case(n, row, c4, w=None, with_dup=False, with_noise=False, offset=0, nan_hist=False, no_hist=False, pred="v"):
    """One ``ccn_sampler_step`` launch against the CPU op sequence.  ``offset``: the tensors are views that many floats into their
    buffers (1 and 2 take the one-element-per-lane form).  ``no_hist``: no history pointer at all (the DDIM update)."""
    coef = ROWS[row].copy()
    coef[4] = np.float32(0.0 if no_hist else c4)
    sigma = 0.21 if with_noise else 0.0
    x, yc, yu, hist, nz = _case_tensors(n, coef, w, 1000 * row + n % 997, pred)
    ref_x, ref_x0 = _reference(pred, x, yc, yu, w, hist, coef, sigma, nz if with_noise else None)
    assert n == 1 or (bool((ref_x0.abs() == 1).any()) and bool((ref_x0.abs() < 1).any())), "x0 must land on both sides of the clamp"

    def view(t):
        return torch.cat([torch.zeros(offset), t]).to(DEV)[offset:]
    xd, ycd = view(x), view(yc)
    yud = view(yu) if w is not None else None
    hd = None if no_hist else view(torch.full((n,), float("nan")) if nan_hist else hist)
    nzd = view(nz) if with_noise else None
    dup = view(torch.full((n,), 7.0)) if with_dup else None
    assert xd.data_ptr() % 16 == (4 * offset) % 16
    _native.sampler_step(xd, ycd, coef if not no_hist else coef[:4], pred, out_u=yud, w=w or 0.0, hist=hd, sigma=sigma, noise=nzd, x_dup=dup)
    what = f"pred={pred} n={n} row={row} c4={c4} w={w} dup={with_dup} noise={with_noise} offset={offset} no_hist={no_hist}"
    assert np.array_equal(xd.cpu().numpy(), ref_x.numpy()), what
    assert bool(torch.isfinite(xd).all()), what
    if hd is not None:
        assert np.array_equal(hd.cpu().numpy(), ref_x0.numpy()), what + ": the history is not the clamped x0"
    if with_dup:
        assert torch.equal(dup, xd), what + ": x_dup differs from x"
    assert torch.equal(ycd.cpu(), yc) and (yud is None or torch.equal(yud.cpu(), yu)), what + ": an output tensor was written"
    assert nzd is None or torch.equal(nzd.cpu(), nz), what + ": the noise was written"
    return xd.cpu(), x, yc, yu, hist, nz, coef, sigma


@pytest.mark.parametrize("n", [1, 255, 2 * 3 * 17 * 19, 2 * 3 * 64 * 64])
@pytest.mark.parametrize("c4", [0.0, 0.37])
def test_sampler_step_v_bit_exact(n, c4):
    k = 0
    for w in (None, 0.0, 1.3, 3.0):
        for with_dup in (False, True):
            for with_noise in (False, True):
                _kernel_case(n, (n + 3 + k) % 14, c4, w=w, with_dup=with_dup, with_noise=with_noise)
                k += 1
    _kernel_case(n, 6, c4, no_hist=True)
    _kernel_case(n, 7, c4, w=1.3, with_noise=True, with_dup=True, no_hist=True)


@pytest.mark.parametrize("n,offset", [(255, 1), (2 * 3 * 17 * 19, 1), (2 * 3 * 17 * 19, 2), (N_STRIDE, 0), (256 * 2048 + 5, 1)])
def test_sampler_step_v_bit_exact_other_paths(n, offset):
    """Unaligned pointers (one element per lane), and sizes past the grid cap of either form (the grid-stride loop)."""
    for c4 in (0.0, 0.37):
        _kernel_case(n, 4, c4, offset=offset)
        _kernel_case(n, 9, c4, w=3.0, with_dup=True, with_noise=True, offset=offset)
        _kernel_case(n, 11, c4, w=1.3, offset=offset)


@pytest.mark.parametrize("n,offset", [(255, 0), (255, 1), (2 * 3 * 64 * 64, 0)])
def test_v_history_is_not_read_without_c4(n, offset):
    """c4 == 0 and a NaN-filled history: the result is the reference's (finite), and the history is overwritten."""
    _kernel_case(n, 5, 0.0, offset=offset, nan_hist=True)
    _kernel_case(n, 5, 0.0, w=3.0, with_dup=True, offset=offset, nan_hist=True)


@pytest.mark.parametrize("n,offset", [(1, 0), (255, 0), (2 * 3 * 17 * 19, 0), (2 * 3 * 64 * 64, 0), (2 * 3 * 17 * 19, 1), (2 * 3 * 17 * 19, 2),
                                      (N_STRIDE, 0)])
def test_sampler_step_eps_is_the_four_older_entry_points(n, offset):
    """``pred = eps``: bit for bit what ccn_ddim_step, ccn_cfg_ddim_step, ccn_ms_step and ccn_cfg_ms_step compute (and the CPU op
    sequence of the eps form, which ``_kernel_case`` checks on the way)."""
    def view(t):
        return torch.cat([torch.zeros(offset), t]).to(DEV)[offset:]
    for c4 in (0.0, 0.37):
        for with_noise in (False, True):
            got, x, yc, _, _, nz, coef, sigma = _kernel_case(n, 3, c4, with_noise=with_noise, offset=offset, no_hist=True, pred="eps")
            old = _native.ddim_step(view(x), view(yc), coef[:4], sigma, view(nz) if with_noise else None)
            assert torch.equal(old.cpu(), got), ("ddim_step", n, offset, with_noise)
            for with_dup in (False, True):
                got, x, yc, yu, _, nz, coef, sigma = _kernel_case(n, 8, c4, w=1.3, with_noise=with_noise, with_dup=with_dup, offset=offset,
                                                                  no_hist=True, pred="eps")
                dup = view(torch.zeros(n)) if with_dup else None
                old = _native.cfg_ddim_step(view(x), view(yc), view(yu), 1.3, coef[:4], sigma, view(nz) if with_noise else None, x_dup=dup)
                assert torch.equal(old.cpu(), got) and (dup is None or torch.equal(dup, old)), ("cfg_ddim_step", n, offset, with_noise, with_dup)
        got, x, yc, _, hist, _, coef, _ = _kernel_case(n, 5, c4, offset=offset, pred="eps")
        hd = view(hist)
        old = _native.ms_step(view(x), hd, view(yc), coef)
        assert torch.equal(old.cpu(), got), ("ms_step", n, offset, c4)
        for w in (0.0, 3.0):
            got, x, yc, yu, hist, _, coef, _ = _kernel_case(n, 12, c4, w=w, with_dup=True, offset=offset, pred="eps")
            old = _native.cfg_ms_step(view(x), view(hist), view(yc), view(yu), w, coef, x_dup=view(torch.zeros(n)))
            assert torch.equal(old.cpu(), got), ("cfg_ms_step", n, offset, c4, w)


def test_sampler_step_error_paths(tiny_net):
    import ctypes
    x = torch.zeros(8, device=DEV)
    with pytest.raises(ValueError, match="prediction"):
        _native.sampler_step(x, x.clone(), ROWS[1][:4], "x0")
    with pytest.raises(ValueError, match="same number"):
        _native.sampler_step(x, torch.zeros(7, device=DEV), ROWS[1][:4], "v")
    with pytest.raises(ValueError, match="coef"):
        _native.sampler_step(x, x.clone(), ROWS[1][:4], "v", hist=x.clone())
    lib = _native.load_library()
    c5 = (ctypes.c_float * 5)(*[float(v) for v in ROWS[1]])
    assert lib.ccn_sampler_step(x.data_ptr(), None, None, x.data_ptr(), None, None, 2, 0.0, c5, 0.0, 8, None) == 1     # CCN_EINVAL
    nat = tiny_net.native()
    assert lib.ccn_set_prediction(nat.h, 2) == 1 and lib.ccn_set_prediction(nat.h, -1) == 1
    with pytest.raises(ValueError, match="prediction"):
        nat.set_prediction("x0")
    with pytest.raises(ValueError, match="prediction"):
        tiny_net.sample_ddim(torch.zeros(B, 512, device=DEV), torch.zeros(SHAPE, device=DEV), [999, 0], ROWS[:2, :4], prediction="x0")


# ------------------------------------------------------------------------------------------------------- 2. fused loop vs the oracle
@pytest.fixture(scope="module")
def gpu_v_ddim(tiny_net, inputs):
    """The fused v-mode DDIM sample on cosine / linspace (first call: capture + replay); shared, never written to."""
    sampler = DDIMSampler(NoiseScheduler(1000, "cosine", DEV), prediction="v")
    return sampler, sampler.sample(tiny_net, to_dev(inputs[0]), SHAPE, steps=T, x_T=to_dev(inputs[1]))


def test_fused_ddim_v_matches_oracle(tiny_net, cpu_model, inputs, gpu_v_ddim):
    z, xT = inputs
    coef = ref_diffusion.ddim_coefficients(ref_diffusion.scheduler_tables(1000, "cosine"), T)
    ref = R.sample_v_fp32(cpu_model, z, xT, ref_diffusion.ddim_timesteps(1000, T), coef[:, :4])
    eps_result = DDIMSampler(gpu_v_ddim[0].sch).sample(tiny_net, to_dev(z), SHAPE, steps=T, x_T=to_dev(xT))
    err, gap = maxerr(gpu_v_ddim[1], ref), maxerr(gpu_v_ddim[1], eps_result)
    print(f"cosine/linspace DDIM, v mode: fused vs oracle max-abs {err:.3e}; v result vs eps result on the same inputs {gap:.3e}")
    assert gpu_v_ddim[1].shape == SHAPE and bool(torch.isfinite(gpu_v_ddim[1]).all())
    assert err < TOL_E2E_FP32, err
    assert gap > 1e-2, gap


@pytest.mark.parametrize("schedule", ["cosine", "linear"])
def test_fused_2m_v_matches_oracle(tiny_net, cpu_model, inputs, schedule):
    z, xT = inputs
    ts, coef = solver_tables(schedule, "logsnr", 2)
    ref = R.sample_v_fp32(cpu_model, z, xT, ts, coef)
    sch = NoiseScheduler(1000, schedule, DEV)
    got = DPMSolverSampler(sch, prediction="v").sample(tiny_net, to_dev(z), SHAPE, steps=T, x_T=to_dev(xT))
    eps_result = DPMSolverSampler(sch).sample(tiny_net, to_dev(z), SHAPE, steps=T, x_T=to_dev(xT))
    err, gap = maxerr(got, ref), maxerr(got, eps_result)
    print(f"{schedule}/logsnr 2M, v mode: fused vs oracle max-abs {err:.3e}; v result vs eps result on the same inputs {gap:.3e}")
    assert bool(torch.isfinite(got).all())
    assert err < TOL_E2E_FP32, err
    assert gap > 1e-2, gap


# ---------------------------------------------------------------------------------------------------------- 3. guided, and eta > 0
def test_guided_v_matches_oracle(tiny_net, cpu_model, inputs):
    z, xT = inputs
    guided = R.guided_model(cpu_model, W_G, torch.zeros(512))
    coef = ref_diffusion.ddim_coefficients(ref_diffusion.scheduler_tables(1000, "cosine"), T)
    ref_d = R.sample_v_fp32(guided, z, xT, ref_diffusion.ddim_timesteps(1000, T), coef[:, :4])
    sch = NoiseScheduler(1000, "cosine", DEV)
    got_d = DDIMSampler(sch, guided=True, prediction="v").sample(tiny_net, to_dev(z), SHAPE, steps=T, cfg_scale=W_G, x_T=to_dev(xT))
    ts, c5 = solver_tables("cosine", "logsnr", 2)
    ref_m = R.sample_v_fp32(guided, z, xT, ts, c5)
    got_m = DPMSolverSampler(sch, guided=True, prediction="v").sample(tiny_net, to_dev(z), SHAPE, steps=T, cfg_scale=W_G, x_T=to_dev(xT))
    unguided = DDIMSampler(sch, prediction="v").sample(tiny_net, to_dev(z), SHAPE, steps=T, x_T=to_dev(xT))
    print(f"guided (w = {W_G}) v mode vs oracle: DDIM cosine/linspace {maxerr(got_d, ref_d):.3e}, 2M cosine/logsnr {maxerr(got_m, ref_m):.3e}; "
          f"guidance moves the DDIM result by {maxerr(got_d, unguided):.3e}")
    assert maxerr(got_d, unguided) > 10 * TOL_E2E_FP32
    assert maxerr(got_d, ref_d) < TOL_E2E_FP32, maxerr(got_d, ref_d)
    assert maxerr(got_m, ref_m) < TOL_E2E_FP32, maxerr(got_m, ref_m)


@pytest.mark.parametrize("eta", [0.5, 0.03])
def test_eta_v_matches_oracle(tiny_net, cpu_model, inputs, eta):
    """eta > 0 on the linear schedule, the draws from a seeded generator and fed to the oracle loop as they were drawn; the gate is
    the project's 1e-3, NaN counting as equal to NaN only.
    eta = 0.5: the reference's direction coefficient sqrt(ab_s - sigma^2) (diffusion/ddim.py:42, kept on purpose) is imaginary at
    t = 999, where ab_s = 4e-5 and sigma^2 = 5e-3 -- on either schedule, for any eta above 0.045 -- so the oracle loop's result is
    NaN in every element, and so must the fused loop's be: the comparison holds, and says only that.  eta = 0.03 (the value of
    test_guided_eta_positive: every coefficient real) is the comparison in numbers."""
    z, xT = inputs
    sch = NoiseScheduler(1000, "linear", DEV)
    coef = ref_diffusion.ddim_coefficients(ref_diffusion.scheduler_tables(1000, "linear"), T, eta)
    real = bool(np.isfinite(coef).all())
    assert real == (eta < 0.045) and (coef[:-1, 4] > 0).all()
    sampler = DDIMSampler(sch, eta=eta, prediction="v")
    torch.manual_seed(1234)
    a = sampler.sample(tiny_net, to_dev(z), SHAPE, steps=T, x_T=to_dev(xT))
    draws = next(iter(sampler._noise.values())).cpu().clone()
    assert draws.shape == (T,) + SHAPE
    ref = R.sample_v_fp32(cpu_model, z, xT, ref_diffusion.ddim_timesteps(1000, T), coef[:, :4], sigma=coef[:, 4], noises=draws)
    got = a.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(ref)), "NaN in other places than the oracle loop's"
    assert bool(torch.isnan(ref).all()) == (not real)
    torch.manual_seed(1234)
    b = sampler.sample(tiny_net, to_dev(z), SHAPE, steps=T, x_T=to_dev(xT))                                           # replay
    assert torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    if real:
        plain = DDIMSampler(sch, prediction="v").sample(tiny_net, to_dev(z), SHAPE, steps=T, x_T=to_dev(xT))
        print(f"eta = {eta}, linear, v mode: fused vs oracle max-abs {maxerr(got, ref):.3e}; the noise moves the result by {maxerr(a, plain):.3e}")
        assert maxerr(a, plain) > 10 * TOL_E2E_FP32
        assert maxerr(got, ref) < TOL_E2E_FP32, maxerr(got, ref)


# ------------------------------------------------------------------------------------------------------------------------ 4. routes
def _routes(net, sampler_of, z, xT, **kw):
    """(fused graph, its replay, fused launch by launch, stepwise) of one sampler configuration in v mode."""
    s = sampler_of()
    a = s.sample(net, z, SHAPE, steps=T, x_T=xT, **kw)
    b = s.sample(net, z, SHAPE, steps=T, x_T=xT, **kw)
    plain = sampler_of()
    plain.use_graph = False
    c = plain.sample(net, z, SHAPE, steps=T, x_T=xT, **kw)
    d = s.sample(Stepwise(net), z, SHAPE, steps=T, x_T=xT, **kw)
    return a, b, c, d


@pytest.mark.parametrize("which", ["ddim", "2m", "guided-ddim", "guided-2m"])
def test_routes_are_bit_equal_in_v_mode(tiny_net, inputs, which):
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sch = NoiseScheduler(1000, "cosine", DEV)
    guided = which.startswith("guided")
    make = (lambda: DDIMSampler(sch, guided=guided, prediction="v")) if which.endswith("ddim") else \
           (lambda: DPMSolverSampler(sch, guided=guided, prediction="v"))
    a, b, c, d = _routes(tiny_net, make, z, xT, **(dict(cfg_scale=W_G) if guided else {}))
    print(f"{which}, v mode: stepwise vs fused max-abs {maxerr(a, d):.3e}")
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(a, d), maxerr(a, d)


# -------------------------------------------------------------------------------------------------------------------- 5. graph keys
def test_eps_and_v_graphs_on_one_slot(tiny_sd, tiny_net, inputs):
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sch = NoiseScheduler(1000, "cosine", DEV)
    net = make_net(tiny_sd)
    se, sv = DDIMSampler(sch), DDIMSampler(sch, prediction="v")
    e1 = se.sample(net, z, SHAPE, steps=T, x_T=xT)
    v1 = sv.sample(net, z, SHAPE, steps=T, x_T=xT)
    e2 = se.sample(net, z, SHAPE, steps=T, x_T=xT)
    v2 = sv.sample(net, z, SHAPE, steps=T, x_T=xT)
    assert torch.equal(e1, e2) and torch.equal(v1, v2)
    assert maxerr(e1, v1) > 1e-2
    fresh = make_net(tiny_sd)                                        # never sees v mode
    assert torch.equal(DDIMSampler(sch).sample(fresh, z, SHAPE, steps=T, x_T=xT), e1)
    # the multistep and the guided loops key their graphs alike
    me, mv = DPMSolverSampler(sch, guided=True), DPMSolverSampler(sch, guided=True, prediction="v")
    r = [s.sample(net, z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT) for s in (me, mv, me, mv)]
    assert torch.equal(r[0], r[2]) and torch.equal(r[1], r[3]) and maxerr(r[0], r[1]) > 1e-2
    assert torch.equal(DPMSolverSampler(sch, guided=True).sample(fresh, z, SHAPE, steps=T, cfg_scale=W_G, x_T=xT), r[0])
    torch.cuda.synchronize()
    net.native().poll_errors()


def test_every_variant_finds_its_own_graph_on_one_slot(tiny_sd, inputs):
    """The whole graph key at once: every sampler variant in turn on ONE net and ONE slot with graphs on, each result against the
    same call on a second net of the same weights that launches step by step (``use_graph = False``; that the two loops agree bit
    for bit is test_routes_are_bit_equal_in_v_mode and test_guided_routes_and_graphs).  Neighbouring calls differ in one clause of
    the key only: the sigma table (one sampler object, so one noise buffer), the c4 column (same timesteps), the history address,
    the prediction, the guidance scale; the first call comes back after the four-entry LRU has dropped it.  4 steps.
    eta = 0.5 and 0.3 give NaN in every element on both nets (the imaginary direction coefficient at t = 999, see
    test_eta_v_matches_oracle), so equality counts NaN as equal to NaN, and to nothing else; eta = 0.03 and 0.02 are the same pair
    of calls in numbers."""
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sch = NoiseScheduler(1000, "linear", DEV)
    net, ref = make_net(tiny_sd), make_net(tiny_sd)
    steps = 4

    def same(a, b):
        return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))

    def pair(make):
        graphed, plain = make(), make()
        plain.use_graph = False
        return graphed, plain

    def run(what, samplers, seed=None, **kw):
        outs = []
        for s, n in zip(samplers, (net, ref)):
            if seed is not None:
                torch.manual_seed(seed)                               # eta > 0: the same draws on both nets
            outs.append(s.sample(n, z, SHAPE, steps=steps, x_T=xT, **kw))
        assert same(*outs), what
        return outs[0]

    ddim = pair(lambda: DDIMSampler(sch))
    first = run("ddim", ddim)
    noisy = {}
    for eta in (0.5, 0.3, 0.03, 0.02):
        for s in ddim:
            s.eta = eta
        noisy[eta] = run(f"ddim, eta {eta}", ddim, seed=77)
    assert len(ddim[0]._noise) == 1 and bool(torch.isfinite(noisy[0.03]).all()) and not torch.equal(noisy[0.03], noisy[0.02])
    for s in ddim:
        s.eta = 0.0
    m2 = run("2m", pair(lambda: DPMSolverSampler(sch, order=2, spacing="linspace")))
    m1 = run("2m, order 1", pair(lambda: DPMSolverSampler(sch, order=1, spacing="linspace")))
    assert not torch.equal(m1, m2)
    ts, coef = DPMSolverSampler(sch, order=2, spacing="linspace").tables(steps)
    h1, h2, h_ref = (torch.empty_like(xT) for _ in range(3))
    for h in (h1, h2):
        got = net.native().sample(z, xT, ts, coef, hist=h)
        assert same(got, ref.native().sample(z, xT, ts, coef, use_graph=False, hist=h_ref)) and torch.equal(got, m2)
        assert torch.equal(h, h_ref)
    v = run("ddim, v", pair(lambda: DDIMSampler(sch, prediction="v")))
    assert not torch.equal(v, first)
    assert torch.equal(run("ddim again", ddim), first)
    guided = pair(lambda: DDIMSampler(sch, guided=True))
    g = [run(f"guided ddim, w = {w}", guided, cfg_scale=w) for w in (3.0, 2.0, 3.0)]
    assert torch.equal(g[0], g[2]) and not torch.equal(g[0], g[1])
    run("guided 2m", pair(lambda: DPMSolverSampler(sch, spacing="linspace", guided=True)), cfg_scale=3.0)
    torch.cuda.synchronize()
    net.native().poll_errors()
    ref.native().poll_errors()


# ----------------------------------------------------------------------------------------------------------------- 6. the fast modes
@pytest.mark.parametrize("dtype", ["bf16", "f16x3"])
def test_fast_modes_run_v_mode(tiny_sd, inputs, gpu_v_ddim, dtype):
    """bf16 (the dedicated head kernel's epilogue) and f16x3: finite, the fused routes bit-equal, the result is not the eps one; the
    distance to the fp32-mode v result is printed, not bounded (docs/EXPERIMENTS.md R19 records it).  The stepwise route is compared
    bit for bit in f16x3; in bf16 it is not the same arithmetic by design (ccn_forward always takes weight version 0 of the
    step-diffused rounding, the fused loop version i % n), so there its distance is printed."""
    net = make_net(tiny_sd, dtype)
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sch = gpu_v_ddim[0].sch
    a, b, c, d = _routes(net, lambda: DDIMSampler(sch, prediction="v"), z, xT)
    m = DPMSolverSampler(sch, prediction="v")
    m1 = m.sample(net, z, SHAPE, steps=T, x_T=xT)
    m2 = m.sample(net, z, SHAPE, steps=T, x_T=xT)
    eps_result = DDIMSampler(sch).sample(net, z, SHAPE, steps=T, x_T=xT)
    dist = (a - gpu_v_ddim[1]).abs()
    print(f"{dtype} vs fp32, v mode, DDIM cosine/linspace (not bounded): max-abs {float(dist.max()):.3e} mean-abs {float(dist.mean()):.3e}; "
          f"stepwise vs fused {maxerr(a, d):.3e}")
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(m1).all()) and bool(torch.isfinite(d).all())
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(m1, m2)
    assert maxerr(a, eps_result) > 1e-2
    if dtype == "f16x3":
        assert torch.equal(a, d), maxerr(a, d)


# ---------------------------------------------------------------------------------------------------------------- 7. a second shape
def test_second_shape_v(synth, tiny_sd, tiny_net, cpu_model):
    """B = 3, 40 x 48 px (the width is no multiple of the bf16 head's 32-pixel tile, the height none of its 8 rows), 4 steps, 2M on
    linear / logsnr: fp32 against the oracle; bf16 runs the v epilogue on the partial tiles."""
    b, h, w, steps = 3, 40, 48, 4
    z = torch.from_numpy(synth.synth_z(b, seed=50))
    xT = torch.randn((b, 3, h, w), generator=torch.Generator().manual_seed(48))
    ts, coef = solver_tables("linear", "logsnr", 2, steps)
    ref = R.sample_v_fp32(cpu_model, z, xT, ts, coef)
    sch = NoiseScheduler(1000, "linear", DEV)
    got = DPMSolverSampler(sch, prediction="v").sample(tiny_net, to_dev(z), (b, 3, h, w), steps=steps, x_T=to_dev(xT))
    print(f"second shape {b} x {h} x {w}, v mode: fused vs oracle max-abs {maxerr(got, ref):.3e}")
    assert maxerr(got, ref) < TOL_E2E_FP32, maxerr(got, ref)
    lo = DPMSolverSampler(sch, prediction="v").sample(make_net(tiny_sd, "bf16"), to_dev(z), (b, 3, h, w), steps=steps, x_T=to_dev(xT))
    d = (lo - got).abs()
    print(f"bf16 vs fp32, v mode, 2M at {b} x {h} x {w} (not bounded): max-abs {float(d.max()):.3e} mean-abs {float(d.mean()):.3e}")
    assert bool(torch.isfinite(lo).all())
