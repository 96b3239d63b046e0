"""numpy statement of the low-resolution guide (include/ccn_hip.h, ccn_block_mean / ccn_lowres_delta / ccn_sampler_step_lr): the x0 of
the sampler update in float32 ops with one rounding each, the block sums in int64 fixed point, the correction in float64 rounded once.
No GPU, no torch."""
import numpy as np

F = np.float32
D = np.float64
SCALE = 2.0 ** 30


def clamped_x0(x, out_c, c0, c1, pred="eps", out_u=None, w=0.0, thr=None, gscale=None):
    """Step 1: the x0 prediction as the update forms and clamps it, on ``(B, ...)`` arrays: the guidance combine, the multiplication by
    ``gscale[b]``, the eps or the v form, then the static clamp (``thr=None``) or ``clamp(., -thr[b], thr[b]) / thr[b]``."""
    x, y = np.asarray(x, F), np.asarray(out_c, F)
    col = (-1,) + (1,) * (x.ndim - 1)
    with np.errstate(all="ignore"):
        if out_u is not None:
            u = np.asarray(out_u, F)
            y = u + F(w) * (y - u)
        if gscale is not None:
            y = (np.asarray(gscale, F).reshape(col) * y).astype(F)
        raw = F(c1) * x - F(c0) * y if pred == "v" else (x - F(c0) * y) / F(c1)
        if thr is None:
            x0 = np.fmin(np.fmax(raw, F(-1.0)), F(1.0))
        else:
            s = np.asarray(thr, F).reshape(col)
            x0 = np.fmin(np.fmax(raw, -s), s) / s
    return x0.astype(F), y.astype(F)


def block_sums(v, N):
    """Step 2: ``S`` of every ``N x N`` block of ``v`` ``(..., H, W)``, int64: the sum of ``rint(v * 2^30)`` (ties to even)."""
    v = np.asarray(v, F)
    H, W = v.shape[-2:]
    assert H % N == 0 and W % N == 0
    q = np.rint(v.astype(D) * SCALE).astype(np.int64)
    return q.reshape(v.shape[:-2] + (H // N, N, W // N, N)).sum(axis=(-3, -1))


def block_mean(v, N):
    """ccn_block_mean: the fixed-point block mean of ``clamp(v, -1, 1)``, rounded once to float32."""
    v = np.fmin(np.fmax(np.asarray(v, F), F(-1.0)), F(1.0))
    return (block_sums(v, N).astype(D) / (N * N * SCALE)).astype(F)


def delta(x0, guide, N, strength=1.0):
    """Steps 2 and 3: ``d = (float)(lambda (g - S / (N^2 2^30)))`` for every block of the clamped ``x0`` ``(B, C, H, W)``."""
    m = block_sums(x0, N).astype(D) / (N * N * SCALE)
    return (D(F(strength)) * (np.asarray(guide, F).astype(D) - m)).astype(F)


def thumbnail_errors(out, thumb, guide, N):
    """What a result says about the thumbnail it was held to: (the largest distance of the float64 block means of ``out`` from
    ``guide``, the largest distance of ``thumb`` -- ccn_block_mean of ``out`` -- from ``guide`` over the blocks whose pixels all lie in
    [-1, 1], the fraction of such blocks).  ccn_block_mean clamps to [-1, 1] and the corrected x0 is not clamped again, so in a block
    with a pixel outside the two means differ by the clamped excess: the arithmetic promises the first figure for every block and
    the second for the blocks inside."""
    out, g = np.asarray(out, D), np.asarray(guide, D)
    H, W = out.shape[-2:]
    blocks = out.reshape(out.shape[:-2] + (H // N, N, W // N, N))
    inside = (np.abs(blocks) <= 1.0).all(axis=(-3, -1))
    err_all = float(np.abs(blocks.mean(axis=(-3, -1)) - g).max())
    err_in = float(np.abs(np.asarray(thumb, D) - g)[inside].max()) if inside.any() else 0.0
    return err_all, err_in, float(inside.mean())


def spread(d, N):
    """A+: every block value over its ``N x N`` pixels."""
    return np.repeat(np.repeat(np.asarray(d, F), N, axis=-2), N, axis=-1)


def lowres_delta(x, out_c, coef, guide, N, strength=1.0, pred="eps", out_u=None, w=0.0, thr=None, gscale=None):
    """ccn_lowres_delta on ``(B, C, H, W)`` arrays."""
    x0, _ = clamped_x0(x, out_c, coef[0], coef[1], pred, out_u, w, thr, gscale)
    return delta(x0, guide, N, strength)


def step(x, out_c, coef, pred, d, N, thr=None, gscale=None, out_u=None, w=0.0, hist=None, sigma=0.0, noise=None):
    """The step replica (ccn_sampler_step_lr) on ``(B, C, H, W)`` arrays: ``d`` (``(B, C, H/N, W/N)``; None: no guide) is added to the
    clamped x0, one float32 addition, no re-clamp.  Returns (new x, the corrected x0 -- the next history)."""
    c = [F(v) for v in coef] + [F(0.0)] * (5 - len(coef))
    x = np.asarray(x, F)
    x0, y = clamped_x0(x, out_c, c[0], c[1], pred, out_u, w, thr, gscale)
    with np.errstate(all="ignore"):
        if d is not None:
            x0 = x0 + spread(d, N)
        e = c[0] * x + c[1] * y if pred == "v" else y
        xn = c[2] * x0 + c[3] * e
        if hist is not None and c[4] != 0:
            xn = xn + c[4] * (x0 - np.asarray(hist, F))
        if noise is not None:
            xn = xn + F(sigma) * np.asarray(noise, F)
    return xn.astype(F), x0.astype(F)
