"""numpy statement of guidance rescale (include/ccn_hip.h, ccn_guidance_rescale / ccn_sampler_step_rs): the fp32 combine with one
rounding per op, the unbiased standard deviations two-pass in float64, the factor rounded once to float32, ``y' = fl32(k y)``.
No GPU, no torch."""
import numpy as np

import threshold_ref

F = np.float32


def combine(out_c, out_u, w):
    """``y = y_u + w (y_c - y_u)`` in three float32 ops, as the step kernel forms it."""
    c, u = np.asarray(out_c, F), np.asarray(out_u, F)
    with np.errstate(all="ignore"):
        return (u + F(w) * (c - u)).astype(F)


def factor(out_c, out_u, w, phi):
    """``(B,)`` float32: ``phi std(y_c[b]) / std(y[b]) + 1 - phi`` per row of the ``(B, per)`` arrays; 1 where ``std(y[b]) == 0``,
    NaN for a row that holds a NaN or an inf."""
    c = np.asarray(out_c, F)
    y = combine(c, out_u, w)
    out = np.empty(c.shape[0], F)
    with np.errstate(all="ignore"):
        for b in range(c.shape[0]):
            std_c = np.std(c[b].astype(np.float64), ddof=1)
            std_y = np.std(y[b].astype(np.float64), ddof=1)
            if not (np.isfinite(std_c) and np.isfinite(std_y)):
                out[b] = np.nan
            elif std_y == 0.0:
                out[b] = 1.0
            else:
                out[b] = F(float(phi) * std_c / std_y + (1.0 - float(phi)))
    return out


def rescaled(out_c, out_u, w, k):
    """``y' = fl32(k_b y)``: the output every later formula reads (without ``out_u``: ``k_b out_c``)."""
    y = np.asarray(out_c, F) if out_u is None else combine(out_c, out_u, w)
    with np.errstate(all="ignore"):
        return (np.asarray(k, F).reshape(-1, 1) * y).astype(F)


def raw_x0(x, out_c, c0, c1, pred, k, out_u=None, w=0.0):
    """The x0 prediction before any clamp, formed from the rescaled output."""
    return threshold_ref.raw_x0(x, rescaled(out_c, out_u, w, k), c0, c1, pred)


def step(x, out_c, coef, pred, k, thr=None, out_u=None, w=0.0, hist=None, sigma=0.0, noise=None):
    """The rescaled sampler update on ``(B, per)`` arrays: ``threshold_ref.step`` on ``y'`` (``thr=None``: the static clamp, which is
    a threshold of 1 bit for bit).  Returns (new x, the clamped x0 -- the next history)."""
    yp = rescaled(out_c, out_u, w, k)
    s = np.ones(yp.shape[0], F) if thr is None else thr
    return threshold_ref.step(x, yp, coef, pred, s, None, 0.0, hist, sigma, noise)
