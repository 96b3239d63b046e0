"""numpy statement of dynamic thresholding (include/ccn_hip.h, ccn_x0_threshold / ccn_sampler_step_thr): float32 ops with one rounding
each, the order statistics by ``np.sort`` on the bit patterns of ``|x0|``.  No GPU, no torch."""
import math

import numpy as np

F = np.float32


def raw_x0(x, out_c, c0, c1, pred="eps", out_u=None, w=0.0):
    """The x0 prediction before any clamp, as the sampler update forms it: the guidance combine first, then the eps or the v form."""
    x, y = np.asarray(x, F), np.asarray(out_c, F)
    with np.errstate(all="ignore"):
        if out_u is not None:
            u = np.asarray(out_u, F)
            y = u + F(w) * (y - u)
        if pred == "v":
            return F(c1) * x - F(c0) * y
        return (x - F(c0) * y) / F(c1)


def rank_and_frac(p, per):
    """(k, min(k + 1, per - 1), frac) of the interpolated quantile: the position in double, the fraction rounded to float32."""
    pos = float(p) * (per - 1)
    k = min(int(math.floor(pos)), per - 1)
    return k, min(k + 1, per - 1), F(pos - k)


def order_statistics(raw_row, p):
    """(v_lo, v_hi, frac): ranks k and k + 1 of the ascending |x0|, ordered by bit pattern (NaNs last, +inf an ordinary maximum)."""
    bits = np.ascontiguousarray(raw_row, F).reshape(-1).view(np.uint32) & np.uint32(0x7FFFFFFF)
    v = np.sort(bits).view(F)
    k, k1, frac = rank_and_frac(p, v.size)
    return v[k], v[k1], frac


def quantile_abs(raw_row, p):
    v_lo, v_hi, frac = order_statistics(raw_row, p)
    with np.errstate(all="ignore"):
        return F(v_lo + F(frac * F(v_hi - v_lo)))


def threshold(raw, p, max_value=np.inf):
    """``(B,)`` float32: min(max(Q_p(|x0_b|), 1), max_value) per row of ``raw`` ``(B, per)``; a NaN quantile stays NaN."""
    out = np.empty(raw.shape[0], F)
    for b in range(raw.shape[0]):
        q = quantile_abs(raw[b], p)
        t = F(1.0) if q < 1.0 else q
        out[b] = F(max_value) if t > F(max_value) else t
    return out


def step(x, out_c, coef, pred, thr, out_u=None, w=0.0, hist=None, sigma=0.0, noise=None):
    """The thresholded sampler update on ``(B, per)`` arrays: returns (new x, the thresholded x0 -- the next history).  ``coef`` =
    (c0, c1, c2, c3[, c4]); ``hist`` enters when c4 != 0; ``noise`` (nullable) adds sigma * noise."""
    c = [F(v) for v in coef] + [F(0.0)] * (5 - len(coef))
    x, y = np.asarray(x, F), np.asarray(out_c, F)
    with np.errstate(all="ignore"):
        if out_u is not None:
            u = np.asarray(out_u, F)
            y = u + F(w) * (y - u)
        raw = c[1] * x - c[0] * y if pred == "v" else (x - c[0] * y) / c[1]
        s = np.asarray(thr, F).reshape(-1, 1)
        x0 = np.fmin(np.fmax(raw, -s), s) / s
        e = c[0] * x + c[1] * y if pred == "v" else y
        xn = c[2] * x0 + c[3] * e
        if hist is not None and c[4] != 0:
            xn = xn + c[4] * (x0 - np.asarray(hist, F))
        if noise is not None:
            xn = xn + F(sigma) * np.asarray(noise, F)
    return xn.astype(F), x0.astype(F)
