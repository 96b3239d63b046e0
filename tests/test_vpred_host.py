"""The v-parameterisation on the host: the float64 loops agree where they must, the conditioning claim that motivates it, the
scheduler's three helpers, the figures the GPU test's 1e-3 gate relies on, and the error paths.  No GPU.

Figures measured here (torch CPU, this file's own prints; docs/EXPERIMENTS.md R19 quotes them):
  1. float64 v loop vs float64 eps loop on the analytic Gaussian problem (x_T = -2.5 ... 2.5): 3.6e-8, 3.1e-7, 1.4e-7 for the three
     cases, largest |raw x0| 0.57 -- the defect is the fp32 tables' a^2 + s^2 - 1 (up to 1.2e-7), not an error
  2. t = 999, exact predictor rounded to fp32: the v form's x0 is right to 1.2e-12 (of |x0| up to 1.9e-6), the eps form returns
     exactly 0
  4. the oracle's fp32 v loop moves by 1.7e-6 ... 2.0e-6 under a +-1e-6 perturbation of the model output (the eps loop on the same
     tables: 1.5e-6 ... 6.3e-2), and lies 1.08 ... 2.0 (max-abs) from the eps-form loop on the same network
"""
import numpy as np
import pytest
import torch

import multistep_ref as M
import vpred_ref as R
from clip_feature_codec.diffusion.scheduler import NoiseScheduler
from clip_feature_codec.diffusion.ddim import DDIMSampler
from clip_feature_codec.diffusion.dpm_solver import DPMSolverSampler
from clip_feature_codec.train import diffusion_train as dt
from oracle import ref_unet, ref_diffusion

VAR = 0.05
X_T = np.linspace(-2.5, 2.5, 11)
TOL_E2E_FP32 = 1e-3
# (schedule, spacing, order) of the three tables x the two start-noise seeds of the GPU test
TABLES = (("cosine", "linspace", 1), ("cosine", "logsnr", 2), ("linear", "logsnr", 2))
SEEDS = (0, 900)


# ------------------------------------------------------------------------------------------------------------ 1. the float64 loops
@pytest.mark.parametrize("steps,spacing,order", [(10, "linspace", 1), (50, "linspace", 1), (20, "logsnr", 2)])
def test_float64_v_loop_equals_the_eps_loop_on_the_gaussian_problem(steps, spacing, order):
    ts = M.timesteps(steps, spacing, "cosine")
    coef = M.coefficients64(ts, order, "cosine")
    xe, top_e = M.sample64(M.gaussian_eps(VAR, "cosine"), None, X_T, ts, coef)
    xv, top_v = R.sample_v64(R.gaussian_v(VAR, "cosine"), None, X_T, ts, coef)
    d = float(np.abs(xe - xv).max())
    print(f"{steps}-step {spacing} order {order}: |v loop - eps loop| = {d:.3e}; largest |raw x0| {top_v:.3f} (v), {top_e:.3f} (eps)")
    assert top_v < 1.0 and top_e < 1.0, "the clamp must not be active in this comparison"
    assert d < 5e-6, d


# ---------------------------------------------------------------------------------------------------------- 2. the conditioning claim
def test_v_form_keeps_x0_at_t_999_where_the_eps_form_loses_it():
    a, s, _ = M.tables64("cosine")
    t = 999
    x = torch.tensor(X_T[X_T != 0], dtype=torch.float32)
    x64 = x.double().numpy()
    x0_true = a[t] * VAR * x64 / (a[t] ** 2 * VAR + s[t] ** 2)
    af, sf = (torch.tensor(float(np.float32(v)), dtype=torch.float32) for v in (a[t], s[t]))
    v = torch.tensor(R.gaussian_v(VAR, "cosine")(x64, None, t), dtype=torch.float32)
    e = torch.tensor(M.gaussian_eps(VAR, "cosine")(x64, None, t), dtype=torch.float32)
    x0_v = (af * x - sf * v).double().numpy()
    x0_e = ((x - sf * e) / af).double().numpy()
    x0_via_e = ((x - sf * (sf * x + af * v)) / af).double().numpy()          # e from v, then the eps form: no better
    err_v, err_e = np.abs(x0_v - x0_true), np.abs(x0_e - x0_true)
    print(f"t = 999: 1/a = {1 / a[t]:.3e}; v form max |x0 error| {err_v.max():.3e}; eps form {err_e.max():.3e} of |x0| up to {np.abs(x0_true).max():.3e}")
    assert float(sf) == 1.0
    assert err_v.max() < 1e-9
    assert np.array_equal(err_e, np.abs(x0_true)), "the eps form is expected to return exactly 0 here"
    assert np.all(np.abs(x0_via_e - x0_true) >= 0.5 * np.abs(x0_true))


# ----------------------------------------------------------------------------------------------------------------- 3. the helpers
@pytest.mark.parametrize("schedule", ["cosine", "linear"])
def test_scheduler_v_helpers(schedule):
    sch = NoiseScheduler(1000, schedule, device="cpu")
    tab = ref_diffusion.scheduler_tables(1000, schedule)
    g = torch.Generator().manual_seed(3)
    x0 = torch.rand((3, 3, 8, 8), generator=g) * 2 - 1
    noise = torch.randn((3, 3, 8, 8), generator=g)
    t = torch.tensor([0, 400, 999])
    a = tab["sqrt_alphas_cumprod"][t].view(-1, 1, 1, 1); s = tab["sqrt_one_minus_alphas_cumprod"][t].view(-1, 1, 1, 1)
    # float64 round trip with q_sample: only the fp32 tables' a^2 + s^2 - 1 is left
    x0d, nd = x0.double(), noise.double()
    x_t = a.double() * x0d + s.double() * nd
    v = sch.v_target(x0d, t, nd)
    assert v.dtype == torch.float64
    e0 = float((sch.predict_x0_from_v(x_t, t, v) - x0d).abs().max()); e1 = float((sch.predict_eps_from_v(x_t, t, v) - nd).abs().max())
    print(f"{schedule}: float64 round trip |x0 error| {e0:.2e}, |eps error| {e1:.2e}")
    assert e0 < 1e-6 and e1 < 1e-6
    # fp32: the stated op sequences, bit for bit
    xt32 = a * x0 + s * noise
    v32 = sch.v_target(x0, t, noise)
    assert v32.dtype == torch.float32
    assert torch.equal(v32, a * noise - s * x0)
    assert torch.equal(sch.predict_x0_from_v(xt32, t, v32), a * xt32 - s * v32)
    assert torch.equal(sch.predict_eps_from_v(xt32, t, v32), s * xt32 + a * v32)


# ---------------------------------------------------------------------------------------- 4. what the GPU test's 1e-3 gate relies on
@pytest.fixture(scope="module")
def cpu_model(tiny_sd):
    return ref_unet.make_model(ref_unet.as_torch_sd(tiny_sd))


@pytest.mark.parametrize("schedule,spacing,order", TABLES)
def test_the_fp32_v_loop_is_well_conditioned_and_far_from_the_eps_loop(synth, cpu_model, schedule, spacing, order):
    z = torch.from_numpy(synth.synth_z(2))
    ts = M.timesteps(6, spacing, schedule)
    coef = M.coefficients64(ts, order, schedule)
    for seed in SEEDS:
        xT = torch.from_numpy(synth.start_noise(range(2), 32, seed_base=seed))
        base = R.sample_v_fp32(cpu_model, z, xT, ts, coef)
        resp = max(float((R.sample_v_fp32(cpu_model, z, xT, ts, coef, perturb=p) - base).abs().max()) for p in (1e-6, -1e-6))
        eps_loop = R.sample_eps_fp32(cpu_model, z, xT, ts, coef)
        gap = float((eps_loop - base).abs().max())
        resp_e = max(float((R.sample_eps_fp32(cpu_model, z, xT, ts, coef, perturb=p) - eps_loop).abs().max()) for p in (1e-6, -1e-6))
        print(f"{schedule}/{spacing} order {order} seed {seed}: v loop response to +-1e-6: {resp:.2e} (eps loop: {resp_e:.2e}); "
              f"v loop vs eps loop {gap:.3f}")
        assert bool(torch.isfinite(base).all())
        assert resp < 1e-5, resp
        assert gap > 10 * TOL_E2E_FP32, gap


# ----------------------------------------------------------------------------------------------------------------- 5. error paths
def test_unknown_prediction_strings_are_value_errors():
    sch = NoiseScheduler(1000, "cosine", device="cpu")
    for bad in ("x0", "EPS", "", None, 1):
        with pytest.raises(ValueError, match="prediction"):
            DDIMSampler(sch, prediction=bad)
        with pytest.raises(ValueError, match="prediction"):
            DPMSolverSampler(sch, prediction=bad)
        with pytest.raises(ValueError, match="prediction"):
            dt.train_step(None, sch, None, torch.zeros(1, 3, 8, 8), torch.zeros(1, 512), prediction=bad)
        with pytest.raises(ValueError, match="prediction"):
            dt.train_diffusion("no-such-store", prediction=bad)
    assert DDIMSampler(sch).prediction == "eps" and DPMSolverSampler(sch).prediction == "eps"
    assert DDIMSampler(sch, prediction="v").prediction == "v" and DPMSolverSampler(sch, prediction="v").prediction == "v"


def test_resume_with_another_parameterisation_names_both():
    dt.check_resume_prediction(dict(prediction="v"), "v")
    dt.check_resume_prediction(dict(prediction="eps"), "eps")
    dt.check_resume_prediction(dict(epoch=3), "eps")                 # a state file from before the option was trained with eps
    with pytest.raises(ValueError, match=r"prediction='v'.*prediction='eps'"):
        dt.check_resume_prediction(dict(prediction="v"), "eps", "train_state.pt")
    with pytest.raises(ValueError, match=r"prediction='eps'.*prediction='v'"):
        dt.check_resume_prediction(dict(epoch=3), "v", "train_state.pt")


def test_cli_flag():
    from clip_feature_codec.cli import eval as cli_eval, reconstruct_diffusion as cli_rec
    for mod, argv in ((cli_rec, ["--store_dir", "s", "--bitstream", "b", "--weights", "w"]), (cli_eval, ["--store_dir", "s", "--weights", "w"])):
        with pytest.raises(SystemExit):
            mod.main(argv + ["--prediction", "x0"])
        # the dpmpp2m / eta check runs right after parsing: reaching it shows that --prediction v was accepted
        with pytest.raises(SystemExit, match="eta"):
            mod.main(argv + ["--prediction", "v", "--sampler", "dpmpp2m", "--eta", "0.5"])
