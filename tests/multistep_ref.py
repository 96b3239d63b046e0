"""Reference for the multistep sampler (DPM-Solver++ 2M, data-prediction form), independent of the package's host code.

TEST INFRASTRUCTURE.  Two things:

* the float64 solver: timestep tables, the five coefficient columns, and the loop over any ``model(x, z, t)``;
* the fp32 update, op by op in torch-CPU ops -- every op rounds to fp32 on its own, which is what the kernels must match bit for bit.

Notation: ``a = sqrt(alpha_bar)``, ``s = sqrt(1 - alpha_bar)``, ``lambda = log(a / s)``; a step goes from ``t = ts[i]`` to
``u = ts[i+1]``, ``h_i = lambda_u - lambda_t``, ``r_i = h_(i-1) / h_i``.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np
import torch

from oracle import ref_diffusion


def tables64(schedule: str = "cosine", timesteps: int = 1000) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(a, s, lambda) per table timestep in float64, from the fp32 schedule tables (the values the samplers read)."""
    tab = ref_diffusion.scheduler_tables(timesteps, schedule)
    a = tab["sqrt_alphas_cumprod"].numpy().astype(np.float64)
    s = tab["sqrt_one_minus_alphas_cumprod"].numpy().astype(np.float64)
    return a, s, np.log(a / s)


def timesteps(steps: int, spacing: str, schedule: str = "cosine", T: int = 1000) -> np.ndarray:
    if spacing == "linspace":
        return ref_diffusion.ddim_timesteps(T, steps).astype(np.int64)
    assert spacing == "logsnr", spacing
    lam = tables64(schedule, T)[2]
    out = [T - 1]
    for k in range(1, steps):
        target = lam[T - 1] + (lam[0] - lam[T - 1]) * k / (steps - 1)
        t = 0 if k == steps - 1 else int(np.argmin(np.abs(lam - target)))
        if t < out[-1]:
            out.append(t)
    return np.asarray(out, dtype=np.int64)


def coefficients64(ts, order: int, schedule: str = "cosine", T: int = 1000) -> np.ndarray:
    """(n, 5) float64: s_t, a_t, a_u, s_u (1, 0 on the last step), and the 2M coefficient a_u (1 - e^{-h}) / (2 r) (0 on step 0, on
    the last step and for order 1)."""
    a, s, lam = tables64(schedule, T)
    n = len(ts)
    rows = np.zeros((n, 5))
    for i in range(n):
        t = int(ts[i])
        a_u, s_u = (a[int(ts[i + 1])], s[int(ts[i + 1])]) if i < n - 1 else (1.0, 0.0)
        rows[i, :4] = (s[t], a[t], a_u, s_u)
        if order == 2 and 0 < i < n - 1:
            h = lam[int(ts[i + 1])] - lam[t]
            h_prev = lam[t] - lam[int(ts[i - 1])]
            rows[i, 4] = a_u * (1.0 - np.exp(-h)) / (2.0 * (h_prev / h))
    return rows


def update_fp32(x: torch.Tensor, e: torch.Tensor, hist: Optional[torch.Tensor], row) -> Tuple[torch.Tensor, torch.Tensor]:
    """One update in fp32 torch-CPU ops, each rounded on its own: (new x, clamped x0 = the new history).  ``hist`` is not touched
    when ``c4 == 0``."""
    assert x.dtype == torch.float32 and e.dtype == torch.float32
    c0, c1, c2, c3, c4 = (torch.tensor(float(np.float32(v)), dtype=torch.float32) for v in row)
    x0 = ((x - c0 * e) / c1).clamp(-1, 1)
    xn = c2 * x0 + c3 * e
    if float(c4) != 0.0:
        xn = xn + c4 * (x0 - hist)
    return xn, x0


def guided_fp32(ec: torch.Tensor, eu: torch.Tensor, w: float) -> torch.Tensor:
    return eu + torch.tensor(float(np.float32(w)), dtype=torch.float32) * (ec - eu)


@torch.no_grad()
def sample_fp32(model: Callable, z: torch.Tensor, x_T: torch.Tensor, ts, coef) -> torch.Tensor:
    """The loop with the fp32 update (``coef`` rounded to fp32): what the fused loop computes, on the CPU."""
    coef = np.asarray(coef).astype(np.float32)
    x, hist = x_T.clone(), None
    for i in range(len(ts)):
        t_b = torch.full((x.shape[0],), int(ts[i]), dtype=torch.long)
        x, hist = update_fp32(x, model(x, z, t_b), hist, coef[i])
    return x


def sample64(model: Callable, z, x_T: np.ndarray, ts, coef: np.ndarray) -> Tuple[np.ndarray, float]:
    """The loop in float64 on numpy arrays, ``model(x, z, t)`` with a scalar ``t``: (x_0, the largest |x0| before the clamp)."""
    x, hist, top = np.asarray(x_T, dtype=np.float64).copy(), None, 0.0
    for i in range(len(ts)):
        c0, c1, c2, c3, c4 = coef[i]
        e = model(x, z, int(ts[i]))
        raw = (x - c0 * e) / c1
        top = max(top, float(np.abs(raw).max()))
        x0 = np.clip(raw, -1.0, 1.0)
        x = c2 * x0 + c3 * e
        if c4 != 0.0:
            x = x + c4 * (x0 - hist)
        hist = x0
    return x, top


# ---- the analytic problem: scalar Gaussian data of variance v -----------------------------------------------------------------
def gaussian_eps(v: float, schedule: str, T: int = 1000) -> Callable:
    """The optimal predictor for x_0 ~ N(0, v): eps(x, t) = s_t x / (a_t^2 v + s_t^2)."""
    a, s, _ = tables64(schedule, T)
    return lambda x, z, t: s[t] * x / (a[t] ** 2 * v + s[t] ** 2)


def gaussian_exact(v: float, x_T: np.ndarray, schedule: str, T: int = 1000) -> np.ndarray:
    """The probability-flow ODE's exact solution from t = T-1 to alpha_bar = 1: x_0 = x_T sqrt(v) / sqrt(a_T^2 v + s_T^2)."""
    a, s, _ = tables64(schedule, T)
    return x_T * np.sqrt(v) / np.sqrt(a[T - 1] ** 2 * v + s[T - 1] ** 2)
