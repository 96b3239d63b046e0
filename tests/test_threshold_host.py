"""The numpy reference of dynamic thresholding (tests/threshold_ref.py) against its own definition: the interpolated quantile lies
between the two order statistics, agrees with the float64 interpolation and with ``torch.quantile`` to 2 fp32 ulps of ``v_hi``
(three roundings of half an ulp each on magnitudes <= v_hi), and its ends are the minimum and the maximum."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import threshold_ref as ref  # noqa: E402

PERS = [768, 969, 12288]
PS = [1e-4, 0.5, 0.995, 1.0]


def rows():
    rng = np.random.default_rng(5)
    for per in PERS:
        yield per, (rng.standard_normal(per) * 3).astype(np.float32)
        yield per, (rng.integers(0, 5, per) * 0.75).astype(np.float32) * rng.choice([-1, 1], per).astype(np.float32)


@pytest.mark.parametrize("p", PS)
def test_quantile_between_its_order_statistics_and_close_to_float64(p):
    for per, row in rows():
        v_lo, v_hi, frac = ref.order_statistics(row, p)
        q = ref.quantile_abs(row, p)
        assert v_lo <= q <= v_hi, (per, p, v_lo, q, v_hi)
        exact = float(v_lo) + float(frac) * (float(v_hi) - float(v_lo))
        bound = 2 * float(np.spacing(np.float32(v_hi)))
        assert abs(float(q) - exact) <= bound, (per, p, float(q), exact, bound)
        # torch.quantile on the same values held as float64: on float32 input torch also forms the POSITION p (per - 1) in float32,
        # whose rounding (up to 3e-5 of a rank at per = 768) times v_hi - v_lo is an error of torch's, outside the bound derived above
        tq = float(torch.quantile(torch.from_numpy(np.abs(row).astype(np.float64)), p))
        assert abs(float(q) - tq) <= bound, (per, p, float(q), tq, bound)


def test_ends_are_minimum_and_maximum():
    for per, row in rows():
        assert ref.quantile_abs(row, 1.0) == np.abs(row).max()
        k, k1, frac = ref.rank_and_frac(0.0, per)
        assert (k, frac) == (0, 0.0)
        assert ref.quantile_abs(row, 0.0) == np.abs(row).min()


def test_rank_and_fraction():
    assert ref.rank_and_frac(1.0, 768) == (767, 767, 0.0)
    k, k1, frac = ref.rank_and_frac(0.995, 12288)
    pos = 0.995 * 12287
    assert (k, k1) == (int(pos), int(pos) + 1) and frac == np.float32(pos - int(pos))
    assert ref.rank_and_frac(0.5, 1) == (0, 0, 0.0)


def test_threshold_clamps_to_one_and_to_the_maximum_and_keeps_nan():
    rng = np.random.default_rng(2)
    raw = np.stack([rng.standard_normal(768) * 0.1, rng.standard_normal(768) * 5, rng.standard_normal(768)]).astype(np.float32)
    raw[2, 5] = np.nan
    thr = ref.threshold(raw, 1.0, 3.0)
    assert thr[0] == 1.0 and thr[1] == 3.0 and np.isnan(thr[2])
    free = ref.threshold(raw, 0.5)
    assert free[0] == 1.0 and np.isfinite(free).all()               # one NaN sorts last: the median does not meet it


def test_step_with_threshold_one_is_the_static_clamp():
    rng = np.random.default_rng(3)
    x, y, h = (rng.standard_normal((2, 96)).astype(np.float32) * 2 for _ in range(3))
    coef = (0.6, 0.8, 0.85, 0.52, 0.37)
    for pred in ("eps", "v"):
        xn, x0 = ref.step(x, y, coef, pred, np.ones(2, np.float32), hist=h)
        raw = ref.raw_x0(x, y, coef[0], coef[1], pred)
        assert np.array_equal(x0, np.clip(raw, -1, 1))
        wide, x0w = ref.step(x, y, coef, pred, np.full(2, 2.5, np.float32), hist=h)
        assert np.abs(x0w).max() <= 1.0 and not np.array_equal(x0w, x0)
