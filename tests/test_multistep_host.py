"""The multistep sampler (DPM-Solver++ 2M), the parts that need no GPU: the host tables against the independent float64 reference
of ``multistep_ref``, the solver's order of convergence on a model with a closed-form answer, and the error paths of the Python layer."""
import numpy as np
import pytest
import torch

import multistep_ref as R
from clip_feature_codec.diffusion.dpm_solver import DPMSolverSampler
from clip_feature_codec.diffusion.scheduler import NoiseScheduler

SCHEDULES = ("cosine", "linear")


@pytest.fixture(scope="module", params=SCHEDULES)
def sch(request):
    return NoiseScheduler(1000, request.param, "cpu")


# ------------------------------------------------------------------------------------------------------------------- table facts
@pytest.mark.parametrize("steps", [2, 6, 20, 40, 50])
def test_timestep_tables(sch, steps):
    ts = sch.solver_timesteps(steps, "logsnr")
    assert ts.dtype == np.int32 and ts[0] == 999 and ts[-1] == 0 and 2 <= len(ts) <= steps
    assert np.all(np.diff(ts.astype(np.int64)) < 0)
    assert np.array_equal(ts, R.timesteps(steps, "logsnr", sch.schedule))
    lin = sch.solver_timesteps(steps, "linspace")
    assert lin.dtype == np.int32 and np.array_equal(lin, sch.ddim_timesteps(steps))


def test_documented_table_lengths():
    cos = NoiseScheduler(1000, "cosine", "cpu")
    assert len(cos.solver_timesteps(40, "logsnr")) == 29 and len(cos.solver_timesteps(50, "logsnr")) == 35


@pytest.mark.parametrize("spacing", ["logsnr", "linspace"])
def test_coefficient_tables(sch, spacing):
    ts = sch.solver_timesteps(20, spacing)
    c2, c1 = sch.solver_coefficients(ts, 2), sch.solver_coefficients(ts, 1)
    assert c2.shape == (len(ts), 5) and c2.dtype == np.float32 and np.isfinite(c2).all()
    assert c2[0, 4] == 0 and c2[-1, 4] == 0 and c2[-1, 2] == 1 and c2[-1, 3] == 0
    assert np.all(c2[1:-1, 4] > 0)
    assert np.all(c1[:, 4] == 0) and np.array_equal(c1[:, :4], c2[:, :4])
    # the fp32 table is the float64 reference's, rounded (1e-6: the two hosts' exp / log may differ in the last bits of a double)
    assert np.allclose(c2, R.coefficients64(ts, 2, sch.schedule), rtol=1e-6, atol=0)
    # c0, c1 are the schedule's own fp32 table entries, and the state after step i is at the noise level step i + 1 is told
    assert np.array_equal(c2[:, 0], sch.host["sqrt_one_minus_alphas_cumprod"].numpy()[ts])
    assert np.array_equal(c2[:, 1], sch.host["sqrt_alphas_cumprod"].numpy()[ts])
    assert np.array_equal(c2[:-1, 2], c2[1:, 1]) and np.array_equal(c2[:-1, 3], c2[1:, 0])


def test_update_is_the_solvers_data_form(sch):
    """Without the clamp, c2*x0 + c3*e is (s_u/s_t) x + a_u (1 - e^{-h}) x0, and with the c4 term the step is the 2M step on
    D = (1 + 1/(2r)) x0 - (1/(2r)) x0_prev: float64, 1e-12."""
    ts = R.timesteps(12, "logsnr", sch.schedule)
    c = R.coefficients64(ts, 2, sch.schedule)
    a, s, lam = R.tables64(sch.schedule)
    g = np.random.default_rng(3)
    for i in range(len(ts) - 1):
        x, e, prev = g.normal(size=64) * 0.3, g.normal(size=64) * 0.3, g.normal(size=64) * 0.3
        t, u = ts[i], ts[i + 1]
        h = lam[u] - lam[t]
        x0 = (x - c[i, 0] * e) / c[i, 1]
        ours = c[i, 2] * x0 + c[i, 3] * e
        data_form = s[u] / s[t] * x + a[u] * (1 - np.exp(-h)) * x0
        assert np.abs(ours - data_form).max() < 1e-12
        if i > 0:
            r = (lam[t] - lam[ts[i - 1]]) / h
            D = (1 + 1 / (2 * r)) * x0 - 1 / (2 * r) * prev
            assert np.abs(ours + c[i, 4] * (x0 - prev) - (s[u] / s[t] * x + a[u] * (1 - np.exp(-h)) * D)).max() < 1e-12


# ---------------------------------------------------------------------------------------------------- convergence, closed-form model
V = 0.09
X_T = np.linspace(-2.5, 2.5, 11)


def gaussian_error(schedule, order, requested, spacing):
    ts = R.timesteps(requested, spacing, schedule)
    x, top = R.sample64(R.gaussian_eps(V, schedule), None, X_T, ts, R.coefficients64(ts, order, schedule))
    assert top < 1.0, f"the clamp binds (max |x0| {top}): the closed form no longer applies"
    return float(np.abs(x - R.gaussian_exact(V, X_T, schedule)).max())


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_order_of_convergence(schedule):
    """Scalar Gaussian data of variance 0.09, float64, logsnr spacing, 40 and 80 requested steps.  Measured: cosine order 1
    7.2e-2 / 3.7e-2, order 2 6.7e-3 / 1.4e-3; linear order 1 4.6e-2 / 2.3e-2, order 2 2.6e-3 / 3.8e-4."""
    e1 = [gaussian_error(schedule, 1, n, "logsnr") for n in (40, 80)]
    e2 = [gaussian_error(schedule, 2, n, "logsnr") for n in (40, 80)]
    print(f"{schedule}: order 1 {e1[0]:.2e} -> {e1[1]:.2e}, order 2 {e2[0]:.2e} -> {e2[1]:.2e}")
    assert 1.6 <= e1[0] / e1[1] <= 2.4, e1
    assert e2[0] / e2[1] >= 3.0, e2
    assert 3.0 * e2[0] <= e1[1], (e2, e1)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_order_two_wins_on_linspace_too(schedule):
    """Time-uniform steps are not what the method is designed for: only that order 2 beats order 1 at 80 steps (cosine: 8.6e-3
    against 2.1e-2)."""
    e1, e2 = gaussian_error(schedule, 1, 80, "linspace"), gaussian_error(schedule, 2, 80, "linspace")
    print(f"{schedule} linspace, 80 steps: order 1 {e1:.2e}, order 2 {e2:.2e}")
    assert e2 < e1


def test_package_tables_drive_the_same_solution():
    """The package's fp32 tables in the float64 loop: the order-2 error at 40 requested steps is the reference's to fp32 rounding."""
    sch = NoiseScheduler(1000, "cosine", "cpu")
    ts = sch.solver_timesteps(40, "logsnr")
    x, _ = R.sample64(R.gaussian_eps(V, "cosine"), None, X_T, ts, sch.solver_coefficients(ts, 2).astype(np.float64))
    err = float(np.abs(x - R.gaussian_exact(V, X_T, "cosine")).max())
    assert abs(err - gaussian_error("cosine", 2, 40, "logsnr")) < 1e-5, err


def test_fp32_update_reference_takes_no_history_without_c4():
    x, e = torch.randn(16, generator=torch.Generator().manual_seed(0)), torch.randn(16, generator=torch.Generator().manual_seed(1))
    row = np.array([0.6, 0.8, 0.9, 0.43, 0.0], np.float32)
    xn, x0 = R.update_fp32(x, e, None, row)
    from oracle import ref_diffusion
    assert torch.equal(xn, ref_diffusion.ddim_update(x, e, row))
    assert float(x0.abs().max()) <= 1.0


# ------------------------------------------------------------------------------------------------------------------- error paths
def test_python_error_paths():
    sch = NoiseScheduler(1000, "cosine", "cpu")
    for order in (0, 3, 2.5):
        with pytest.raises(ValueError, match="order"):
            DPMSolverSampler(sch, order=order)
        with pytest.raises(ValueError, match="order"):
            sch.solver_coefficients(sch.solver_timesteps(6), order)
    with pytest.raises(ValueError, match="spacing"):
        DPMSolverSampler(sch, spacing="karras")
    with pytest.raises(ValueError, match="spacing"):
        sch.solver_timesteps(6, "karras")
    with pytest.raises(ValueError, match="decreasing"):
        sch.solver_coefficients([0, 5, 9], 2)
    model, z, shape = (lambda x, zz, t: x), torch.zeros(2, 512), (2, 3, 32, 32)
    for steps in (1, 0, -3):
        with pytest.raises(ValueError, match="steps"):
            DPMSolverSampler(sch).sample(model, z, shape, steps=steps)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            DPMSolverSampler(sch, guided=True).sample(model, z, shape, steps=6, cfg_scale=bad)
    for bad in (torch.zeros(511), torch.zeros(1, 512), "zeros"):
        with pytest.raises(ValueError, match="null_z"):
            DPMSolverSampler(sch, guided=True, null_z=bad).sample(model, z, shape, steps=6, cfg_scale=3.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DPMSolverSampler(sch).sample(model, z, shape, steps=6)


def test_clis_parse_sampler_flags():
    from clip_feature_codec.cli import eval as cli_eval, reconstruct_diffusion as cli_rec
    ev, rec = ["--store_dir", "s", "--weights", "w"], ["--store_dir", "s", "--bitstream", "b", "--weights", "w"]
    for parser, base in ((cli_eval.build_parser(), ev), (cli_rec.build_parser(), rec)):
        a = parser.parse_args(base)
        assert a.sampler == "ddim" and a.spacing == "logsnr"
        a = parser.parse_args(base + ["--sampler", "dpmpp2m", "--spacing", "linspace"])
        assert a.sampler == "dpmpp2m" and a.spacing == "linspace"
        with pytest.raises(SystemExit):
            parser.parse_args(base + ["--sampler", "euler"])


def test_build_sampler_selects_the_solver():
    from clip_feature_codec.cli._common import build_sampler
    from clip_feature_codec.diffusion.ddim import DDIMSampler
    assert isinstance(build_sampler(0.0, "cpu"), DDIMSampler)
    assert isinstance(build_sampler(0.0, "cpu", sampler="ddim"), DDIMSampler)
    s = build_sampler(0.0, "cpu", guided=True, sampler="dpmpp2m", spacing="linspace")
    assert isinstance(s, DPMSolverSampler) and s.order == 2 and s.spacing == "linspace" and s.guided is True
    with pytest.raises(SystemExit, match="eta"):
        build_sampler(0.1, "cpu", sampler="dpmpp2m")
