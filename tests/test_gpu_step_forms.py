"""Every form of the stand-alone sampler step, bit for bit: the whole table {no noise, noise tensor, seeds} x threshold x guidance
rescale x low-resolution guide x guided x history x {eps, v} of ``_native.sampler_step`` against the numpy statement
``tests/guide_ref.step``, ``==`` on the uint32 views of ``x``, ``x_dup`` and the history.  Each feature's own file crosses its flag
with a few others; this file walks all of them, on the smallest shapes that reach every path of the kernel:

* 3 records of (C, H, W, N) = (3, 2, 6, 2), per = 36: the four-wide body, a quad that straddles two blocks and two rows;
* the same with every tensor one float past a 16-byte boundary: the one-element path;
* 3 records of per = 37 (the forms without the guide): a record-wise form that cannot go four wide -- and, for the form with no
  per-record operand at all, one run of n = 111: the four-wide body plus an n % 4 tail.

Thresholds, rescale factors and seeds differ from record to record, so a wrong record offset shows.  The inputs put |raw x0| on both
sides of 1 and of every threshold (``census`` asserts that the reference clamps some and leaves some elements of every record), and
element 0 of record 1 is x = -0.0, y = 0: its x0 is -0.0, and the sign bit must reach the history in every form without the guide
(a guide adds d != 0 there).

The seeded draws: ``rng_ref`` states them in float64 and the kernel forms them in fp32 with the device's logf / cospif / sinpif, so
no numpy value is the device's draw bit for bit (test_gpu_rng.py: up to 1.5 ulp apart).  The draws the reference adds are therefore
``_native.normal_fill``'s -- its own kernel, the same draw_quad / draw_element -- and ``test_draws_are_the_reference_draws`` holds
them to ``rng_ref`` within test_gpu_rng's bound on exactly these shapes.

Last, the two launches that form the same x0 with all operands present at once, which the feature files leave out: the threshold and
the guide's correction with ``out_u`` and ``gscale`` (and ``thr``) at offset 1, and the rescale factor on these shapes."""
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import guide_ref  # noqa: E402
import rescale_ref  # noqa: E402
import rng_ref  # noqa: E402
import threshold_ref  # noqa: E402

from clip_feature_codec import _native  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32

COEF = (0.6, 0.8, 0.85, 0.52, 0.37)
W_G, SIGMA, DRAW, N_BLOCK = 3.0, 0.25, 4, 2
TOL_NORMAL = 4 * 3.60e-7                                            # test_gpu_rng.py's bound on |fp32 draw - float64 reference|
THR = np.array([1.25, 2.0, 1.5], F)
GSCALE = np.array([0.75, 1.125, 0.9], F)
SEEDS = [11, 2 ** 63 + 5, 2 ** 32 - 1]
SHAPES = {"chw": (3, 3, 2, 6), "flat37": (3, 37)}
NEG_ZERO = (1, 0)                                                   # (record, flat element) of the x = -0.0, y = 0 element


def inputs(key):
    """The host tensors of one shape, the same for every form: a function of the shape alone."""
    shape = SHAPES[key]
    rng = np.random.default_rng(sum(shape))
    t = {name: (scale * rng.standard_normal(shape)).astype(F) for name, scale in (("x", 1.5), ("out_c", 1.0), ("out_u", 1.0), ("hist", 1.0))}
    for name in ("x", "out_c", "out_u"):
        t[name].reshape(shape[0], -1)[NEG_ZERO] = -0.0 if name == "x" else 0.0
    if key == "chw":
        t["delta"] = (0.25 * rng.standard_normal(shape[:2] + (shape[2] // N_BLOCK, shape[3] // N_BLOCK))).astype(F)
        t["guide"] = rng.uniform(-1.0, 1.0, t["delta"].shape).astype(F)
    return t


INPUTS = {key: inputs(key) for key in SHAPES}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def census(x0, bound):
    """Per record: does the clamped x0 hold elements on the clamp (|x0| == bound) and elements inside it?"""
    flat = np.abs(x0.reshape(x0.shape[0], -1))
    return ((flat == bound).any(axis=1) & (flat < bound).any(axis=1)).all()


def reference(key, noise, thr, rs, lr, guided, hist, pred):
    """(new x, new history or None) of one form, and the check that the clamp acts and rests in every record.  ``noise``: the
    (B, ...) draws or None."""
    t = INPUTS[key]
    kw = dict(thr=THR if thr else None, gscale=GSCALE if rs else None, out_u=t["out_u"] if guided else None, w=W_G)
    x0, _ = guide_ref.clamped_x0(t["x"], t["out_c"], COEF[0], COEF[1], pred, **{k: kw[k] for k in ("out_u", "w", "thr", "gscale")})
    assert census(x0, 1.0), "the reference's clamp must act on some elements of every record and leave some alone"
    xn, h = guide_ref.step(t["x"], t["out_c"], COEF if hist else COEF[:4], pred, t["delta"] if lr else None, N_BLOCK,
                           hist=t["hist"] if hist else None, sigma=SIGMA, noise=noise, **kw)
    if not lr:
        assert bits(h).reshape(h.shape[0], -1)[NEG_ZERO] == 0x80000000, "x0 of the -0.0 element must be -0.0 in the reference"
    return xn, (h if hist else None)


def forms():
    for noise, thr, (guided, rs), lr, hist, pred in itertools.product(("none", "noise", "seeds"), (False, True),
                                                                       ((False, False), (True, False), (True, True)), (False, True),
                                                                       (False, True), ("eps", "v")):
        yield pytest.param(noise, thr, rs, lr, guided, hist, pred,
                           id=f"{noise}-{'thr' if thr else 'clamp'}-{'rs' if rs else 'guided' if guided else 'plain'}-{'lr' if lr else 'nolr'}-"
                              f"{'hist' if hist else 'nohist'}-{pred}")


def placed(a, off, fill=None):
    """(view, raw): a device tensor of ``a``'s shape ``off`` floats past a 16-byte boundary, holding ``a`` (or ``fill``), inside a
    NaN-filled buffer."""
    raw = torch.full((a.size + 8,), float("nan"), device=DEV)
    view = raw[off:off + a.size].view(a.shape)
    if fill is None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    else:
        view.fill_(fill)
    assert view.data_ptr() % 16 == 4 * off
    return view, raw


def untouched(raw, off, n):
    return bool(torch.isnan(raw[:off]).all()) and bool(torch.isnan(raw[off + n:]).all())


@pytest.fixture(scope="module")
def draws():
    """The device's draw DRAW of every record of both shapes, on the host; never written to."""
    return {key: _native.normal_fill(SEEDS, SHAPES[key], DRAW, device=DEV).cpu().numpy() for key in SHAPES}


def test_draws_are_the_reference_draws(draws):
    for key, shape in SHAPES.items():
        per = int(np.prod(shape[1:]))
        dev = float(np.abs(draws[key].reshape(3, per).astype(np.float64) - rng_ref.normal_fill(SEEDS, per, DRAW)).max())
        print(f"{key}: max |fp32 draw - float64 reference| {dev:.3e}")
        assert dev <= TOL_NORMAL, (key, dev)


@pytest.mark.parametrize("noise,thr,rs,lr,guided,hist,pred", forms())
def test_every_form_matches_the_reference_bit_for_bit(draws, noise, thr, rs, lr, guided, hist, pred):
    cases = [("chw", 0), ("chw", 1)] + ([] if lr else [("flat37", 0)])
    for key, off in cases:
        t = INPUTS[key]
        want_x, want_h = reference(key, None if noise == "none" else draws[key], thr, rs, lr, guided, hist, pred)
        n = t["x"].size
        x, x_raw = placed(t["x"], off)
        h, h_raw = placed(t["hist"], off) if hist else (None, None)
        dup, dup_raw = placed(t["x"], off, fill=float("nan")) if guided else (None, None)
        kw = {}
        if noise == "seeds":
            kw.update(seeds=SEEDS, draw=DRAW)
        elif noise == "noise":
            kw.update(noise=placed(draws[key], off)[0])
        if thr:
            kw.update(thr=placed(THR, off)[0])
        if rs:
            kw.update(gscale=placed(GSCALE, off)[0])
        if lr:
            kw.update(delta=placed(t["delta"], off)[0], factor=N_BLOCK)
        _native.sampler_step(x, placed(t["out_c"], off)[0], COEF if hist else COEF[:4], pred, out_u=placed(t["out_u"], off)[0] if guided else None,
                             w=W_G, hist=h, sigma=SIGMA, x_dup=dup, **kw)
        where = (key, off)
        assert np.array_equal(bits(x.cpu().numpy()), bits(want_x)), where
        assert untouched(x_raw, off, n), where
        if guided:
            assert np.array_equal(bits(dup.cpu().numpy()), bits(want_x)) and untouched(dup_raw, off, n), where
        if hist:
            got_h = bits(h.cpu().numpy())
            assert np.array_equal(got_h, bits(want_h)) and untouched(h_raw, off, n), where
            if not lr:
                assert got_h.reshape(3, -1)[NEG_ZERO] == 0x80000000, where       # -0.0, not +0.0


@pytest.mark.parametrize("pred", ["eps", "v"])
def test_threshold_rescale_and_delta_with_every_operand_at_offset_one(pred):
    """``x0_threshold`` and ``lowres_delta`` with ``out_u`` and ``gscale`` (the delta with ``thr`` too) both present, every tensor at
    offset 1, bit for bit; ``guidance_rescale`` on these shapes within the one ulp test_gpu_rescale.py allows against the two-pass
    float64 statement."""
    for key in SHAPES:
        t = INPUTS[key]
        flat = {name: t[name].reshape(3, -1) for name in ("x", "out_c", "out_u")}
        at = {name: placed(t[name], 1)[0] for name in ("x", "out_c", "out_u")}
        k, k_raw = placed(GSCALE, 1)
        raw = rescale_ref.raw_x0(flat["x"], flat["out_c"], COEF[0], COEF[1], pred, GSCALE, out_u=flat["out_u"], w=W_G)
        for p in (0.5, 0.9, 1.0):
            want = threshold_ref.threshold(raw, p)
            assert (want > 1).any()
            got = _native.x0_threshold(at["x"], at["out_c"], COEF, pred, p, out_u=at["out_u"], w=W_G, gscale=k)
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (key, p)
        factor = _native.guidance_rescale(at["out_c"], at["out_u"], W_G, 0.7).cpu().numpy()
        want = rescale_ref.factor(flat["out_c"], flat["out_u"], W_G, 0.7)
        assert np.isfinite(want).all() and (np.abs(bits(factor).astype(np.int64) - bits(want).astype(np.int64)) <= 1).all(), (key, factor, want)
        if key == "chw":
            for thr in (None, THR):
                want = guide_ref.lowres_delta(t["x"], t["out_c"], COEF, t["guide"], N_BLOCK, 0.75, pred, out_u=t["out_u"], w=W_G, thr=thr, gscale=GSCALE)
                got = _native.lowres_delta(at["x"], at["out_c"], COEF, placed(t["guide"], 1)[0], 0.75, pred, out_u=at["out_u"], w=W_G,
                                           thr=None if thr is None else placed(thr, 1)[0], gscale=k, factor=N_BLOCK)
                assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (key, thr is not None)
        assert untouched(k_raw, 1, 3)
