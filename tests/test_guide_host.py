"""The low-resolution guide on the host: the numpy statement (tests/guide_ref.py) against a true float64 block mean, the consistency
it buys, the argument checks, the CLI flags with the thumbnail's derivation, and the stepwise loop on a stand-in model with the
library's calls replaced by the numpy statement.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guide_ref as ref  # noqa: E402

from clip_feature_codec import _native  # noqa: E402
from clip_feature_codec.diffusion import sampling  # noqa: E402
from clip_feature_codec.diffusion.ddim import DDIMSampler  # noqa: E402
from clip_feature_codec.diffusion.dpm_solver import DPMSolverSampler  # noqa: E402
from clip_feature_codec.diffusion.scheduler import NoiseScheduler  # noqa: E402

F = np.float32
# (C, H, W, N): the shapes of tests/test_gpu_guide.py plus one whose N is no power of two (the statement does not need one)
SHAPES = [(3, 2, 6, 2), (3, 8, 24, 4), (3, 16, 16, 16), (1, 64, 128, 64), (3, 32, 32, 8), (3, 6, 6, 3)]
SCALES = [0.01, 0.5, 3.0]
COEF = (0.6, 0.8, 0.85, 0.52, 0.37)


def true_mean(v, N):
    v = np.asarray(v, np.float64)
    H, W = v.shape[-2:]
    return v.reshape(v.shape[:-2] + (H // N, N, W // N, N)).mean(axis=(-3, -1))


def cases():
    for C, H, W, N in SHAPES:
        for B in (1, 3):
            for scale in SCALES:
                for pred in ("eps", "v"):
                    rng = np.random.default_rng(C * H * W + N + B)
                    x, yc, yu = ((rng.standard_normal((B, C, H, W)) * scale).astype(F) for _ in range(3))
                    g = rng.uniform(-1, 1, (B, C, H // N, W // N)).astype(F)
                    yield (C, H, W, N, B, scale, pred), x, yc, yu, g


def test_delta_against_a_true_float64_block_mean():
    """|d - lambda (g - mean)| <= 2^-23 + 2^-31: one fp32 rounding of |d| <= 2 (half an ulp of a value below 2 is 2^-24 -- the bound
    leaves a factor of two) plus the fixed-point grain, half of 2^-30 per element, so at most 2^-31 on the mean."""
    worst = 0.0
    for key, x, yc, yu, g in cases():
        N, pred = key[3], key[6]
        for lam in (1.0, 0.3):
            for out_u, thr in ((None, None), (yu, None), (yu, np.full(x.shape[0], 1.7, F))):
                x0, _ = ref.clamped_x0(x, yc, COEF[0], COEF[1], pred, out_u, 3.0, thr)
                assert np.abs(x0).max() <= 1.0
                d = ref.delta(x0, g, N, lam)
                want = np.float64(F(lam)) * (g.astype(np.float64) - true_mean(x0, N))
                err = float(np.abs(d.astype(np.float64) - want).max())
                worst = max(worst, err)
                assert d.dtype == F and err <= 2.0 ** -23 + 2.0 ** -31, (key, lam, err)
    print(f"largest |d - lambda (g - mean)| over the shapes: {worst:.3e} (bound {2.0 ** -23 + 2.0 ** -31:.3e})")


def test_strength_one_makes_the_block_mean_the_guide():
    """With lambda = 1 the float64 block mean of x0' = x0 + d is within 3 2^-23 of g: the bound above on d, plus the rounding of each
    x0 + d (|x0'| <= 3: at most 2^-23 per element, so at most that on their mean), with 2^-31 to spare."""
    worst = 0.0
    for key, x, yc, yu, g in cases():
        N, pred = key[3], key[6]
        x0, _ = ref.clamped_x0(x, yc, COEF[0], COEF[1], pred)
        d = ref.delta(x0, g, N, 1.0)
        xn, x0p = ref.step(x, yc, COEF, pred, d, N)
        assert np.array_equal(x0p, (x0 + ref.spread(d, N)).astype(F))
        err = float(np.abs(true_mean(x0p, N) - g.astype(np.float64)).max())
        worst = max(worst, err)
        assert err <= 3 * 2.0 ** -23, (key, err)
    print(f"largest |block mean of x0' - g| over the shapes: {worst:.3e} (bound {3 * 2.0 ** -23:.3e})")


def test_block_sums_are_exact_and_saturate_where_they_should():
    ones = np.ones((1, 1, 64, 128), F)
    assert np.array_equal(ref.block_sums(ones, 64), np.full((1, 1, 1, 2), 64 * 64 * 2 ** 30, np.int64))
    assert np.array_equal(ref.block_mean(-3 * ones, 64), -np.ones((1, 1, 1, 2), F))
    v = np.array([[0.5, -0.25], [2.0 ** -31, -(2.0 ** -31)]], F)                    # ties go to even: both halves round to 0
    assert ref.block_sums(v, 2).item() == 2 ** 29 - 2 ** 28
    # d is None: the step of tests/threshold_ref.py with a threshold of 1
    import threshold_ref
    rng = np.random.default_rng(0)
    x, y, h = (rng.standard_normal((2, 3, 4, 4)).astype(F) for _ in range(3))
    for pred in ("eps", "v"):
        a = ref.step(x, y, COEF, pred, None, 2, hist=h)
        b = threshold_ref.step(x.reshape(2, -1), y.reshape(2, -1), COEF, pred, np.ones(2, F), hist=h.reshape(2, -1))
        assert np.array_equal(a[0].reshape(2, -1), b[0]) and np.array_equal(a[1].reshape(2, -1), b[1])


# ------------------------------------------------------------------------------------------------------------------- the arguments
def test_python_argument_checks():
    g = torch.zeros(2, 3, 4, 4)
    assert _native.guide_factor(g, (2, 3, 16, 16)) == 4 and _native.guide_factor(g, (2, 3, 16, 16), 4) == 4
    assert _native.guide_args(g, (2, 3, 16, 16), 1, 0) == (4, 1.0, 0) and _native.guide_args(g, (2, 3, 8, 8), 0.25, 300) == (2, 0.25, 300)
    for shape in ((2, 3, 16, 32), (2, 3, 18, 18), (1, 3, 16, 16), (2, 1, 16, 16), (2, 3, 4, 4), (2, 3, 512, 512), (2, 3, 12, 12)):
        with pytest.raises(ValueError, match="guide|block size"):
            _native.guide_factor(g, shape)
    with pytest.raises(ValueError, match="factor"):
        _native.guide_factor(g, (2, 3, 16, 16), 2)
    with pytest.raises(ValueError):
        _native.guide_factor(torch.zeros(2, 3, 4), (2, 3, 16, 16))
    for lam in (0.0, -0.5, 1.01, float("nan")):
        with pytest.raises(ValueError, match="guide_strength"):
            _native.guide_args(g, (2, 3, 16, 16), lam, 0)
    for t in (-1, 2.5):
        with pytest.raises(ValueError, match="guide_t_min"):
            _native.guide_args(g, (2, 3, 16, 16), 1.0, t)
    assert sampling.guide_options(None, (2, 3, 16, 16), 1.0, 0, "cpu") is None
    o = sampling.guide_options(g.double().numpy(), (2, 3, 16, 16), 0.5, 7, "cpu")
    assert o["guide"].dtype == torch.float32 and o["guide_strength"] == 0.5 and o["guide_t_min"] == 7
    s = DDIMSampler(None)
    assert "guide" not in sampling.fused_kwargs(s, None, None, 0) and sampling.fused_kwargs(s, None, None, 0, o)["guide"] is o["guide"]
    # the samplers check the guide before anything runs (a CPU z is refused first, so the check is reached through guide_options)
    with pytest.raises(ValueError, match="guide"):
        sampling.guide_options(torch.zeros(2, 3, 5, 5), (2, 3, 16, 16), 1.0, 0, "cpu")


# --------------------------------------------------------------------------------------------------------------------------- the CLIs
def test_cli_flags_and_the_thumbnail(tmp_path):
    from PIL import Image
    from clip_feature_codec.cli import eval as cli_eval, reconstruct_diffusion as cli_recon, _common
    base = ["--store_dir", "s", "--weights", "w"]
    a = cli_eval.build_parser().parse_args(base)
    assert a.lowres_guide is None and a.guide_strength is None and a.guide_t_min is None and a.guide_bits == 8
    a = cli_eval.build_parser().parse_args(base + ["--lowres_guide", "8", "--guide_strength", "0.5", "--guide_t_min", "200", "--guide_bits", "6"])
    assert (a.lowres_guide, a.guide_strength, a.guide_t_min, a.guide_bits) == (8, 0.5, 200, 6)
    r = cli_recon.build_parser().parse_args(base + ["--bitstream", "b"])
    assert r.lowres_guide is None and not hasattr(r, "guide_bits")
    r = cli_recon.build_parser().parse_args(base + ["--bitstream", "b", "--lowres_guide", "t.png", "--guide_t_min", "5"])
    assert r.lowres_guide == "t.png" and r.guide_t_min == 5
    _common.check_guide_flags(None, None, None, 256, 8)
    _common.check_guide_flags(32, 0.5, 100, 256, 8)
    _common.check_guide_flags("t.png", None, None, 256)
    for bad in ((None, 0.5, None, 256, 8), (None, None, 3, 256, 8), (None, None, None, 256, 6), (3, None, None, 256, 8), (128, None, None, 256, 8),
                (1, None, None, 256, 8), (32, None, None, 48, 8), (32, 0.0, None, 256, 8), (32, 1.5, None, 256, 8), (32, None, -1, 256, 8),
                (32, None, None, 256, 0), (32, None, None, 256, 9)):
        with pytest.raises(SystemExit) as e:
            _common.check_guide_flags(*bad)
        assert e.value.code not in (0, None) and "--" in str(e.value.code), bad

    # the thumbnail: the float64 block mean, quantised to uint8 levels and mapped back to [-1, 1]
    rng = np.random.default_rng(1)
    orig = rng.uniform(-1, 1, (3, 32, 32)).astype(F)
    for n in (2, 8, 32):
        g = _common.derive_guide(orig, n)
        levels = np.rint((true_mean(orig, n) + 1.0) * 127.5)
        assert g.shape == (3, 32 // n, 32 // n) and g.dtype == F and np.array_equal(g, (levels / 127.5 - 1.0).astype(F))
        assert np.abs(g.astype(np.float64) - true_mean(orig, n)).max() <= 1.0 / 255 + 1e-7
        assert _common.guide_side_bytes(32, n) == 3 * (32 // n) ** 2
    assert _common.guide_side_bytes(32, 8, bits=4) == 24 and _common.guide_side_bytes(32, 8, bits=1) == 6
    g4 = _common.derive_guide(orig, 8, bits=4)
    assert len(np.unique(g4)) <= 16 and np.abs(g4 - true_mean(orig, 8)).max() <= 1.0 / 15 + 1e-7
    u8 = ((orig + 1.0) * 127.5).astype(np.uint8)                                    # the uint8 form of an original gives its own means
    assert np.array_equal(_common.derive_guide(u8, 8), _common.derive_guide((u8.astype(np.float64) / 127.5 - 1.0), 8))
    assert np.array_equal(_common.derive_guide(np.ones((3, 8, 8), F), 4), np.ones((3, 2, 2), F))
    assert np.array_equal(_common.derive_guide(-np.ones((3, 8, 8), F), 4), -np.ones((3, 2, 2), F))

    # the file of reconstruct_diffusion: an image or a uint8 .npy of (h, w, 3); N = size / h
    thumb = rng.integers(0, 256, (4, 4, 3), dtype=np.uint8)
    np.save(tmp_path / "t.npy", thumb)
    Image.fromarray(thumb).save(tmp_path / "t.png")
    want = (thumb.astype(F) / F(127.5) - F(1.0)).transpose(2, 0, 1)[None]
    for name in ("t.npy", "t.png"):
        got = _common.load_guide_file(str(tmp_path / name), 32)
        assert got.shape == (1, 3, 4, 4) and got.dtype == F and np.array_equal(got, want)
    np.save(tmp_path / "f.npy", thumb.astype(F))
    np.save(tmp_path / "r.npy", rng.integers(0, 256, (4, 8, 3), dtype=np.uint8))
    for name, size in (("t.npy", 30), ("t.npy", 4), ("t.npy", 512), ("t.npy", 12), ("f.npy", 32), ("r.npy", 32)):
        with pytest.raises(SystemExit) as e:
            _common.load_guide_file(str(tmp_path / name), size)
        assert "--lowres_guide" in str(e.value.code), (name, size)


# ------------------------------------------------------------------------------------------------------------------ the stepwise loop
@pytest.mark.parametrize("kind", ["ddim", "dpmpp2m"])
@pytest.mark.parametrize("guided", [False, True])
def test_stepwise_loop_on_a_stand_in_model(monkeypatch, kind, guided):
    """``sampling.stepwise`` with the library's two calls replaced by the numpy statement: the delta is asked for exactly on the steps
    with ``ts[i] >= guide_t_min``, from the step's own state and outputs, and handed to that step's update -- the result is the
    statement's loop."""
    B, C, S, N, steps, w = 2, 3, 8, 4, 6, 3.0
    sch = NoiseScheduler(1000, "linear", "cpu")
    if kind == "ddim":
        sampler = DDIMSampler(sch, guided=guided)
        ts, coef = sch.ddim_timesteps(steps), sch.ddim_coefficients(steps, 0.0)[:, :4]
    else:
        sampler = DPMSolverSampler(sch, guided=guided)
        ts, coef = sampler.tables(steps)
    t_min = int(ts[len(ts) // 2])
    calls = []

    def lowres_delta(x, out_c, c, guide, strength=1.0, prediction="eps", out_u=None, w=0.0, thr=None, gscale=None, factor=None):
        calls.append("delta")
        n = lambda t: None if t is None else t.numpy()
        return torch.from_numpy(ref.lowres_delta(n(x), n(out_c), [float(v) for v in c], n(guide), N, strength, prediction, n(out_u), w))

    def sampler_step(x, out_c, c, prediction="eps", out_u=None, w=0.0, hist=None, sigma=0.0, noise=None, thr=None, gscale=None, delta=None, **kw):
        calls.append("step+" if delta is not None else "step")
        n = lambda t: None if t is None else t.numpy()
        xn, x0 = ref.step(n(x), n(out_c), [float(v) for v in c], prediction, n(delta), N, out_u=n(out_u), w=w, hist=n(hist))
        x.copy_(torch.from_numpy(xn))
        if hist is not None:
            hist.copy_(torch.from_numpy(x0))
        return x
    monkeypatch.setattr(_native, "lowres_delta", lowres_delta)
    monkeypatch.setattr(_native, "sampler_step", sampler_step)
    monkeypatch.setattr(_native, "require_dev", lambda t, name, dtype=torch.float32: t.contiguous())

    def model(x, z, t):                                             # a stand-in: any function of the state, the embedding and t
        return 0.3 * x + 0.1 * z.mean(dim=1).view(-1, 1, 1, 1) + 1e-4 * t.view(-1, 1, 1, 1).float()
    g0 = torch.Generator().manual_seed(5)
    x_T, z = torch.randn(B, C, S, S, generator=g0), torch.randn(B, 16, generator=g0)
    guide = torch.rand(B, C, S // N, S // N, generator=g0) * 2 - 1
    opts = sampling.guide_options(guide, x_T.shape, 0.75, t_min, "cpu")
    got = sampling.stepwise(sampler, model, x_T, z, ts, coef, w if guided else None, None, multistep=kind == "dpmpp2m", guide=opts)
    n_guided = int((np.asarray(ts) >= t_min).sum())
    assert 0 < n_guided < len(ts) and calls.count("delta") == n_guided == calls.count("step+") and calls.count("step") == len(ts) - n_guided
    assert calls[:2 * n_guided] == ["delta", "step+"] * n_guided     # the guided steps come first: the table runs from T-1 down

    # the statement's own loop
    x, hist = x_T.numpy().copy(), (np.zeros_like(x_T.numpy()) if kind == "dpmpp2m" else None)
    for i in range(len(ts)):
        t_b = torch.full((B,), int(ts[i]), dtype=torch.long)
        xt = torch.from_numpy(x)
        yc = model(xt, z, t_b).numpy()
        yu = model(xt, torch.zeros_like(z), t_b).numpy() if guided else None
        d = ref.lowres_delta(x, yc, coef[i], guide.numpy(), N, 0.75, "eps", yu, w) if int(ts[i]) >= t_min else None
        x, x0 = ref.step(x, yc, coef[i], "eps", d, N, out_u=yu, w=w, hist=hist)
        if hist is not None:
            hist = x0
    assert np.array_equal(got.numpy(), x)
    # without a guide the loop never asks for a delta
    calls.clear()
    sampling.stepwise(sampler, model, x_T, z, ts, coef, w if guided else None, None, multistep=kind == "dpmpp2m")
    assert calls == ["step"] * len(ts)
