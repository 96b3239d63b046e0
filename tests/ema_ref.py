"""Float64 closed form of the weight EMA, and the same loop on torch's own ``AveragedModel``.

The semantics are ``torch.optim.swa_utils.AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(decay))`` with ``update_parameters``
after every APPLIED optimiser step: the first update copies the parameters, every later one is ``ema.lerp_(p, 1 - decay)``, and
``n_averaged`` counts them.  A skipped step (the step guard's ``apply == 0``) is no update.  With warm-up the decay of update ``u``
(from 0) is ``min(decay, (1 + u) / (10 + u))``, i.e. the lerp weight is ``max(1 - decay, 9 / (10 + u))``.

``closed_form`` restates this elementwise in float64 with the fp32 weight VALUES the kernel uses (``np.float32(1 - decay)``, what
torch's ``lerp_`` receives, and ``np.float32(9) / np.float32(10 + u)``); ``torch_cpu_loop`` runs torch's class in fp32.
tests/test_ema_host.py pins the first to the second, tests/test_gpu_ema.py compares the HIP kernels with the first.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch


def ulp32(x) -> float:
    return float(np.spacing(np.float32(abs(float(x)))))


def weight(decay: float, warmup: bool, u: int) -> np.float32:
    """The fp32 lerp weight of update ``u`` (0-based; update 0 is the copy and does not use it)."""
    w = np.float32(1 - decay)
    if warmup:
        w = max(w, np.float32(9) / np.float32(10 + u))
    return np.float32(w)


def schedule(decay: float, warmup: bool, applied: Sequence[bool]):
    """Per call: the count of updates after it and the weight the state block then shows (the last applied update's; 0 before the
    first)."""
    u, w_shown = 0, np.float32(0)
    updates: List[int] = []; weights: List[np.float32] = []
    for ok in applied:
        if ok:
            w_shown = weight(decay, warmup, u)
            u += 1
        updates.append(u); weights.append(w_shown)
    return updates, weights


def closed_form(p_seq: Sequence[np.ndarray], decay: float, warmup: bool = False, applied: Optional[Sequence[bool]] = None) -> dict:
    """``p_seq[i]``: the parameters after call ``i`` (ignored where ``applied[i]`` is false).  Returns per call the average (float64,
    None before the first update), and ``schedule``'s count of updates and weight."""
    applied = [True] * len(p_seq) if applied is None else list(applied)
    updates, weights = schedule(decay, warmup, applied)
    e: Optional[np.ndarray] = None
    ema: List[Optional[np.ndarray]] = []
    for p, ok, u, w in zip(p_seq, applied, updates, weights):
        if ok:
            p64 = np.asarray(p, dtype=np.float64)
            e = p64.copy() if u == 1 else e + float(w) * (p64 - e)
        ema.append(None if e is None else e.copy())
    return dict(ema=ema, updates=updates, weights=weights)


def torch_cpu_loop(p_seq: Sequence[np.ndarray], decay: float, applied: Optional[Sequence[bool]] = None) -> dict:
    """AveragedModel(..., multi_avg_fn=get_ema_multi_avg_fn(decay)) in fp32 on the CPU, update_parameters after every applied step."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    applied = [True] * len(p_seq) if applied is None else list(applied)
    holder = torch.nn.Linear(1, 1, bias=False)
    holder.weight = torch.nn.Parameter(torch.zeros(len(np.asarray(p_seq[0]).reshape(-1))).view(1, -1))
    avg = AveragedModel(holder, multi_avg_fn=get_ema_multi_avg_fn(decay))
    ema, n_averaged = [], []
    for p, ok in zip(p_seq, applied):
        if ok:
            with torch.no_grad():
                holder.weight.copy_(torch.from_numpy(np.asarray(p, dtype=np.float32)).view(1, -1))
            avg.update_parameters(holder)
        ema.append(avg.module.weight.detach().numpy().reshape(-1).copy()); n_averaged.append(int(avg.n_averaged))
    return dict(ema=ema, n_averaged=n_averaged)


def walk(n: int, steps: int, seed: int = 11, scale: float = 0.03, move: float = 2e-4) -> List[np.ndarray]:
    """A parameter trajectory shaped like AdamW's: values around ``scale``, each step moving every element by about ``move`` (lr)."""
    g = torch.Generator("cpu").manual_seed(seed)
    p = (torch.randn(n, generator=g) * scale).numpy()
    out = []
    for _ in range(steps):
        p = (p + (torch.randn(n, generator=g) * move).numpy()).astype(np.float32)
        out.append(p.copy())
    return out
