"""Reference for the v-parameterisation (the network predicts ``v = a noise - s x0``), independent of the package's host code.

TEST INFRASTRUCTURE.  Three things:

* the fp32 sampler update in v form, op by op in torch-CPU ops (every op rounds to fp32 on its own: what the kernels must match bit
  for bit), with guidance and the eta > 0 noise term, and the loop over any ``model(x, z, t)`` whose output is read as ``v``;
* the same loop in float64, and the optimal ``v`` predictor of the analytic Gaussian problem of ``multistep_ref``;
* the v objective (MSE on ``v`` + recon_w L1 + tv_w TV on the clamped x0 prediction) and its gradient in float64 closed form, with
  the rounding bound derived as ``objective_ref`` derives ``K``, ``U``, ``S``.

Notation as in ``multistep_ref``: ``a = sqrt(alpha_bar)``, ``s = sqrt(1 - alpha_bar)``; a table row is ``(c0, c1, c2, c3, c4)`` with
``c0 = s_t``, ``c1 = a_t`` -- the SAME rows the eps form uses:

    x0 = clamp(c1 x - c0 y, -1, 1);  e = c0 x + c1 y;  xn = c2 x0 + c3 e;  c4 != 0: xn += c4 (x0 - hist);  [+ sigma noise]
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np
import torch

import multistep_ref as M
import objective_ref as O

U = O.U


def _f32(v) -> torch.Tensor:
    return torch.tensor(float(np.float32(v)), dtype=torch.float32)


# ---- the sampler update -----------------------------------------------------------------------------------------------------------
def update_v_fp32(x: torch.Tensor, y: torch.Tensor, hist: Optional[torch.Tensor], row, sigma: float = 0.0,
                  noise: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One v-form update in fp32 torch-CPU ops, each rounded on its own: (new x, clamped x0 = the new history)."""
    assert x.dtype == torch.float32 and y.dtype == torch.float32
    c0, c1, c2, c3, c4 = (_f32(v) for v in row)
    x0 = (c1 * x - c0 * y).clamp(-1, 1)
    e = c0 * x + c1 * y
    xn = c2 * x0 + c3 * e
    if float(c4) != 0.0:
        xn = xn + c4 * (x0 - hist)
    if noise is not None:
        xn = xn + _f32(sigma) * noise
    return xn, x0


guided_fp32 = M.guided_fp32          # y = y_u + w (y_c - y_u): the same three ops for either parameterisation


def guided_model(model: Callable, w: float, null_row: torch.Tensor) -> Callable:
    def f(x, z, t):
        yu = model(x, null_row.expand(x.shape[0], -1), t)
        return guided_fp32(model(x, z, t), yu, w)
    return f


@torch.no_grad()
def sample_v_fp32(model: Callable, z: torch.Tensor, x_T: torch.Tensor, ts, coef, sigma=None, noises=None, perturb: float = 0.0) -> torch.Tensor:
    """The loop with the fp32 v update (``coef`` (n, 4 or 5), rounded to fp32): what the fused loop computes in v mode, on the CPU.
    ``sigma`` (n,) / ``noises`` (n, ...): the eta > 0 term on the steps with sigma > 0.  ``perturb``: added to every model output
    (the conditioning probe of tests/test_vpred_host.py)."""
    coef = np.asarray(coef).astype(np.float32)
    if coef.shape[1] == 4:
        coef = np.concatenate([coef, np.zeros((coef.shape[0], 1), np.float32)], axis=1)
    x, hist = x_T.clone(), None
    for i in range(len(ts)):
        t_b = torch.full((x.shape[0],), int(ts[i]), dtype=torch.long)
        y = model(x, z, t_b)
        if perturb:
            y = y + _f32(perturb)
        noisy = sigma is not None and float(sigma[i]) > 0
        x, hist = update_v_fp32(x, y, hist, coef[i], float(sigma[i]) if noisy else 0.0, noises[i] if noisy else None)
    return x


@torch.no_grad()
def sample_eps_fp32(model: Callable, z: torch.Tensor, x_T: torch.Tensor, ts, coef, perturb: float = 0.0) -> torch.Tensor:
    """``multistep_ref.sample_fp32`` with the same ``perturb`` probe: the eps-form loop on the same network output."""
    coef = np.asarray(coef).astype(np.float32)
    if coef.shape[1] == 4:
        coef = np.concatenate([coef, np.zeros((coef.shape[0], 1), np.float32)], axis=1)
    x, hist = x_T.clone(), None
    for i in range(len(ts)):
        t_b = torch.full((x.shape[0],), int(ts[i]), dtype=torch.long)
        y = model(x, z, t_b)
        if perturb:
            y = y + _f32(perturb)
        x, hist = M.update_fp32(x, y, hist, coef[i])
    return x


def sample_v64(model: Callable, z, x_T: np.ndarray, ts, coef: np.ndarray) -> Tuple[np.ndarray, float]:
    """The v loop in float64 on numpy arrays, ``model(x, z, t)`` with a scalar ``t``: (x_0, the largest |x0| before the clamp)."""
    x, hist, top = np.asarray(x_T, dtype=np.float64).copy(), None, 0.0
    for i in range(len(ts)):
        c0, c1, c2, c3, c4 = coef[i]
        y = model(x, z, int(ts[i]))
        raw = c1 * x - c0 * y
        top = max(top, float(np.abs(raw).max()))
        x0 = np.clip(raw, -1.0, 1.0)
        e = c0 * x + c1 * y
        x = c2 * x0 + c3 * e
        if c4 != 0.0:
            x = x + c4 * (x0 - hist)
        hist = x0
    return x, top


def gaussian_v(var: float, schedule: str, T: int = 1000) -> Callable:
    """The optimal v predictor for x_0 ~ N(0, var): with E[x0 | x] = a var x / (a^2 var + s^2) and E[eps | x] = s x / (a^2 var + s^2),
    v = a E[eps | x] - s E[x0 | x] = a s x (1 - var) / (a^2 var + s^2)."""
    a, s, _ = M.tables64(schedule, T)
    return lambda x, z, t: a[t] * s[t] * x * (1.0 - var) / (a[t] ** 2 * var + s[t] ** 2)


# ---- the objective ----------------------------------------------------------------------------------------------------------------
# Roundings on the longest path from the operands to one element of d_v, each bounded by U times the magnitude of the value it rounds.
# The auxiliary (L1 + TV) part is bounded through S = |2 (v - target) / n| + s (sum of |terms of dL/dp|): `s` stands where the eps form
# has `s / a`, because d raw / d v_hat = -s.
#   kernel:          recon_w or tv_w to fp32 (1), weight / count to fp32 (1), the two additions that join the three terms of
#                    dL/dp (2), dL/dp * (-s) (1; there is no s / a to form), the addition to the MSE part (1)                = 6
#   torch autograd:  the weight to fp32 (1), / count in mean's backward (1), up to four accumulations of the five partial gradients
#                    that meet in one element of x0_pred (4), * (-s) (1; no division), the accumulation with the MSE part (1) = 8
# K_V bounds either evaluation to first order plus one unit for the second-order terms: 9, one less than the eps form's 10.
K_V = 9
assert K_V <= O.K
# On top of that the MSE target is itself computed: a*noise (1), s*x0 (1), their difference (1) -- three roundings, each at most U
# times the value it rounds, so |target_fp32 - target| <= U (|a noise| + |s x0| + |target|) =: U T3 to first order, and it enters d_v
# through 2 (v - target) / n: an ADDITIVE term 2 U T3 / n per element, independent of K_V.  (The eps form's target is `noise`, an
# operand.)  torch's fp32 evaluation forms the target with the same three ops, so its target is the same fp32 number.


def closed_form_v(v_hat, noise, raw, x0, a, s, recon_w, tv_w, target32=None):
    """float64 evaluation on the given (fp32) operands; ``raw = a x_t - s v_hat`` is taken as an fp32 OPERAND as in ``objective_ref``.
    Returns a dict: d_v, terms (total, mse, l1, tv), mask, aux (the L1 + TV part of d_v), S and T (the target's rounding allowance
    2 U T3 / n, already multiplied by U).  The gradient uses the float64 target.  ``target32``: the fp32 target as an operand, used
    for the MSE TERM only (the kernel's sum is an exact fp64 sum over that fp32 number: the exact-operand replay)."""
    v_hat, noise, raw, x0 = (np.asarray(t, dtype=np.float64) for t in (v_hat, noise, raw, x0))
    B, C, H, W = v_hat.shape
    a = np.asarray(a, dtype=np.float64).reshape(B, 1, 1, 1); s = np.asarray(s, dtype=np.float64).reshape(B, 1, 1, 1)
    n, n_h, n_w = B * C * H * W, B * C * (H - 1) * W, B * C * H * (W - 1)
    target = a * noise - s * x0
    t3 = np.abs(a * noise) + np.abs(s * x0) + np.abs(target)
    mask = (raw >= -1.0) & (raw <= 1.0)
    p = np.clip(raw, -1.0, 1.0)
    dv = p[:, :, 1:, :] - p[:, :, :-1, :]
    dh = p[:, :, :, 1:] - p[:, :, :, :-1]
    tm = target if target32 is None else np.asarray(target32, dtype=np.float64)
    mse = np.mean((v_hat - tm) ** 2); l1 = np.mean(np.abs(p - x0)); tv = np.abs(dv).sum() / n_h + np.abs(dh).sum() / n_w
    t_l1 = recon_w * O.sgn(p - x0) / n
    sv = np.zeros_like(p); sv[:, :, 1:, :] += O.sgn(dv); sv[:, :, :-1, :] -= O.sgn(dv)
    sh = np.zeros_like(p); sh[:, :, :, 1:] += O.sgn(dh); sh[:, :, :, :-1] -= O.sgn(dh)
    t_v, t_h = tv_w * sv / n_h, tv_w * sh / n_w
    g_mse = 2.0 * (v_hat - target) / n
    aux = mask * (t_l1 + t_v + t_h) * (-s)
    S = np.abs(g_mse) + mask * (np.abs(t_l1) + np.abs(t_v) + np.abs(t_h)) * s
    return dict(d_v=g_mse + aux, terms=np.array([mse + recon_w * l1 + tv_w * tv, mse, l1, tv]), mask=mask, aux=aux, S=S,
                T=2.0 * U * t3 / n)


def worst_ratio_v(got, cf, k=K_V, ref=None):
    """max over elements of |got - d_v| / (k U S + T); ``ref``: another fp32 evaluation to compare with instead of the closed form
    (pass the doubled ``k``; both form the target with the same three fp32 ops, so it is one number in both and T drops out)."""
    want = cf["d_v"] if ref is None else np.asarray(ref, dtype=np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    bound = k * U * cf["S"] + (cf["T"] if ref is None else 0.0)
    assert np.all(err[bound == 0] == 0)
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0
