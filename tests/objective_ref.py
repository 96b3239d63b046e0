"""The closed form of the training objective (MSE + recon_w L1 + tv_w TV on the clamped x0 prediction) and of its gradient, in float64.

Shared by tests/test_objective_host.py and tests/test_gpu_objective.py.  Written from the formulas, not from the kernel:

    raw  = (x_t - s eps) / a        taken as an fp32 OPERAND (the exact-operand replay of tests/test_gpu_layer_replay.py: a float64
                                    re-run would move raw in its last bits and with it the clamp mask near |raw| = 1)
    p    = clamp(raw, -1, 1);  m = (-1 <= raw <= 1)
    mse  = mean((eps - noise)^2);  l1 = mean |p - x0|
    tv   = sum |p[y+1,x] - p[y,x]| / n_h + sum |p[y,x+1] - p[y,x]| / n_w
    dL/dp = recon_w sgn(p - x0) / n + tv_w [(sgn(p - p_up) - sgn(p_down - p)) / n_h + (sgn(p - p_left) - sgn(p_right - p)) / n_w]
    d_eps = 2 (eps - noise) / n + m dL/dp (-s / a)

with sgn(0) = 0 and neighbours outside the image absent.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)

# Roundings on the longest path from the operands to one element of d_eps, each bounded by U times the magnitude of the value it
# rounds, which never exceeds the term-by-term absolute sum S = |2 (eps - noise) / n| + (s / a) (sum of |terms of dL/dp|):
#   kernel:          recon_w or tv_w to fp32 (1), weight / count to fp32 (1), the two additions that join the three terms of
#                    dL/dp (2), s / a (1), dL/dp * (s / a) (1), the addition to the MSE part (1)                          = 7
#   torch autograd:  the weight to fp32 (1), / count in mean's backward (1), up to four accumulations of the five partial
#                    gradients that meet in one element of x0_pred (4), / a and * (-s) (2), the accumulation with the MSE
#                    part (1)                                                                                             = 9
# (the MSE path is shorter in both: eps - noise, the scale by 2 / n, the final addition).  K bounds either evaluation to first
# order plus one unit for the second-order terms.
K = 10


def sgn(v):
    return np.sign(v)


def closed_form(eps, noise, raw, x0, a, s, recon_w, tv_w):
    """float64 evaluation on the given (fp32) operands.  Returns a dict: d_eps, terms (total, mse, l1, tv), mask,
    aux (the L1 + TV part of d_eps), S (the term-by-term absolute sum that scales the rounding bound)."""
    eps, noise, raw, x0 = (np.asarray(v, dtype=np.float64) for v in (eps, noise, raw, x0))
    B, C, H, W = eps.shape
    a = np.asarray(a, dtype=np.float64).reshape(B, 1, 1, 1); s = np.asarray(s, dtype=np.float64).reshape(B, 1, 1, 1)
    n, n_h, n_w = B * C * H * W, B * C * (H - 1) * W, B * C * H * (W - 1)
    mask = (raw >= -1.0) & (raw <= 1.0)
    p = np.clip(raw, -1.0, 1.0)
    dv = p[:, :, 1:, :] - p[:, :, :-1, :]          # dv[y] = p[y+1] - p[y]
    dh = p[:, :, :, 1:] - p[:, :, :, :-1]
    mse = np.mean((eps - noise) ** 2); l1 = np.mean(np.abs(p - x0)); tv = np.abs(dv).sum() / n_h + np.abs(dh).sum() / n_w
    t_l1 = recon_w * sgn(p - x0) / n
    sv = np.zeros_like(p); sv[:, :, 1:, :] += sgn(dv); sv[:, :, :-1, :] -= sgn(dv)
    sh = np.zeros_like(p); sh[:, :, :, 1:] += sgn(dh); sh[:, :, :, :-1] -= sgn(dh)
    t_v, t_h = tv_w * sv / n_h, tv_w * sh / n_w
    g_mse = 2.0 * (eps - noise) / n
    aux = mask * (t_l1 + t_v + t_h) * (-s / a)
    S = np.abs(g_mse) + mask * (np.abs(t_l1) + np.abs(t_v) + np.abs(t_h)) * (s / a)
    return dict(d_eps=g_mse + aux, terms=np.array([mse + recon_w * l1 + tv_w * tv, mse, l1, tv]), mask=mask, aux=aux, S=S)


def worst_ratio(got, cf, k=K):
    """max over elements of |got - d_eps| / (k U S); elements with S == 0 must match exactly."""
    err = np.abs(np.asarray(got, dtype=np.float64) - cf["d_eps"])
    S = cf["S"]
    assert np.all(err[S == 0] == 0)
    return float(np.max(err[S > 0] / (k * U * S[S > 0]))) if np.any(S > 0) else 0.0
