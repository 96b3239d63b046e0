"""Classifier-free guidance as the samplers see it: what ``guided``, ``null_z`` and a call's ``cfg_scale`` amount to."""
from __future__ import annotations

import math
from typing import Optional

import torch


def resolve(guided: bool, null_z: Optional[torch.Tensor], z_clip: torch.Tensor, cfg_scale: float):
    """(scale, null row on z_clip's device) of a guided call, or (None, None): unguided, or the scale is 1.0."""
    if not guided:
        return None, None
    w = float(cfg_scale)
    if not math.isfinite(w):
        raise ValueError(f"cfg_scale must be finite, got {cfg_scale}")
    if null_z is not None:
        if not isinstance(null_z, torch.Tensor) or tuple(null_z.shape) != (z_clip.shape[-1],):
            raise ValueError(f"null_z must be a tensor of shape ({z_clip.shape[-1]},), got {tuple(getattr(null_z, 'shape', ()))}")
        null_z = null_z.to(z_clip.device, torch.float32)
    return (None, None) if w == 1.0 else (w, null_z)
