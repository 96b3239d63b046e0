"""Float64 closed form of the guarded optimiser loop, and the same loop on torch's own CPU classes.

The loop of train/diffusion_train.py:137-139 with torch's semantics: ``torch.amp.GradScaler`` (scale, skipped step, update), then
``torch.nn.utils.clip_grad_norm_(norm_type=2)``, then ``torch.optim.AdamW`` whose step count advances on applied steps only.
``closed_form`` restates it elementwise in float64; ``torch_cpu_loop`` runs torch's classes in fp32.  tests/test_guard_host.py pins
the first to the second, tests/test_gpu_guard.py compares the HIP kernels with the first.

Both take the UNSCALED gradient vectors; what sits in the gradient buffer is ``fp32(g) * fp32(scale)`` (what the backward of
``scaler.scale(loss)`` leaves there), and a step is skipped when any element of THAT is non-finite.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

U = 2.0 ** -24          # fp32 unit roundoff
HYPER = dict(lr=3e-4, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)      # test_mse_loss_grad_and_adamw_kernels_against_torch's


def closed_form(p0: np.ndarray, grads: Sequence[np.ndarray], lr: float, betas, eps: float, weight_decay: float,
                init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000,
                max_grad_norm: Optional[float] = None, good_steps0: int = 0) -> dict:
    b1, b2 = betas
    p = np.asarray(p0, dtype=np.float64).copy()
    m = np.zeros_like(p); v = np.zeros_like(p)
    scale, tracker, good, skipped = float(init_scale), 0, int(good_steps0), 0
    scales: List[float] = []; applied: List[bool] = []; norms: List[float] = []
    for g in grads:
        with np.errstate(over="ignore", invalid="ignore"):
            buf = np.asarray(g, dtype=np.float32) * np.float32(scale)           # the gradient buffer
        ok = bool(np.isfinite(buf).all())
        applied.append(ok)
        if ok:
            u = buf.astype(np.float64) * (1.0 / scale)
            norm = float(np.sqrt((u * u).sum()))
            if max_grad_norm is not None and max_grad_norm > 0:
                u = u * min(1.0, max_grad_norm / (norm + 1e-6))
            good += 1
            p = p * (1.0 - lr * weight_decay)
            m = b1 * m + (1.0 - b1) * u
            v = b2 * v + (1.0 - b2) * u * u
            p = p - (lr / (1.0 - b1 ** good)) * (m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** good) + eps))
            tracker += 1
            if tracker == growth_interval:
                scale, tracker = scale * growth_factor, 0
        else:
            norm = float("nan")
            skipped += 1
            scale, tracker = scale * backoff_factor, 0
        norms.append(norm); scales.append(scale)
    return dict(p=p, m=m, v=v, scales=scales, applied=applied, norms=norms, good_steps=good, skipped_steps=skipped,
                growth_tracker=tracker)


def torch_cpu_loop(p0: np.ndarray, grads: Sequence[np.ndarray], lr: float, betas, eps: float, weight_decay: float,
                   init_scale: float = 65536.0, growth_interval: int = 2000, max_grad_norm: Optional[float] = None) -> dict:
    """scaler.unscale_(opt); clip_grad_norm_; scaler.step(opt); scaler.update() with torch's CPU GradScaler and AdamW in fp32."""
    p = torch.nn.Parameter(torch.from_numpy(np.asarray(p0, dtype=np.float32)).clone())
    opt = torch.optim.AdamW([p], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    scaler = torch.amp.GradScaler("cpu", init_scale=init_scale, growth_interval=growth_interval)
    scales = []
    for g in grads:
        scaler.scale(torch.zeros(()))                      # creates the scale tensor on the first call, as scale(loss) does
        p.grad = torch.from_numpy(np.asarray(g, dtype=np.float32)) * scaler.get_scale()
        scaler.unscale_(opt)
        if max_grad_norm is not None and max_grad_norm > 0:
            torch.nn.utils.clip_grad_norm_([p], max_grad_norm)
        scaler.step(opt)
        scaler.update()
        scales.append(float(scaler.get_scale()))
    st = opt.state[p]
    return dict(p=p.detach().numpy().copy(), scales=scales, steps=int(st["step"]) if "step" in st else 0)


def script(n: int, seed: int = 5, iters: int = 10, poison=((3, float("inf")), (7, float("nan")))):
    """The ten-iteration script: parameters randn(n), gradient g0 * it (g0 = 0.01 randn(n)), it = 1 .. iters, with one planted
    element (in the middle) at the poisoned iterations."""
    g = torch.Generator("cpu").manual_seed(seed)
    p0 = torch.randn(n, generator=g).numpy()
    g0 = (torch.randn(n, generator=g) * 0.01).numpy()
    grads = []
    for it in range(1, iters + 1):
        gi = (g0 * np.float32(it)).astype(np.float32)
        for at, val in poison:
            if at == it:
                gi[n // 2] = val
        grads.append(gi)
    return p0, grads
