"""What ``DDIMSampler`` and ``DPMSolverSampler`` share: the constructor's checks of the parameterisation, the dynamic threshold, the
guidance rescale and the schedule's terminal SNR, the start state, the low-resolution guide's arguments, the keyword arguments of the
fused route and the stepwise loop.
What differs stays in the two classes: the tables."""
from __future__ import annotations

from typing import Optional

import torch

from .. import _native


def set_options(sampler, prediction: str, dynamic_threshold: Optional[float], threshold_max: Optional[float],
                guidance_rescale: Optional[float] = None, guided: bool = False, scheduler=None) -> None:
    """Check and keep ``prediction``, ``dynamic_threshold``, ``threshold_max`` and ``guidance_rescale`` on ``sampler``; a bad one is a
    ``ValueError``, and so are a rescale on an unguided sampler and ``prediction="eps"`` on a zero-terminal-SNR ``scheduler``."""
    _native.prediction_code(prediction)  # ValueError for an unknown parameterisation
    if prediction == "eps" and getattr(scheduler, "rescale_zero_snr", False):
        raise ValueError('prediction="eps" with a rescale_zero_snr=True scheduler: the eps form divides by sqrt(alpha_bar_t), which is 0 '
                         'at t = T-1; use prediction="v"')
    if guidance_rescale is not None:
        _native.rescale_arg(guidance_rescale)                        # ValueError for phi outside (0, 1]
        if not guided:
            raise ValueError("guidance_rescale needs guided=True: it rescales the guided combination")
    sampler.guidance_rescale = guidance_rescale
    if dynamic_threshold is not None:
        _native.threshold_args(dynamic_threshold, threshold_max)     # ValueError for p outside (0, 1] or a maximum below 1
    elif threshold_max is not None:
        raise ValueError("threshold_max needs dynamic_threshold")
    sampler.prediction = prediction
    sampler.dynamic_threshold, sampler.threshold_max = dynamic_threshold, threshold_max


def start_state(shape: tuple, device, x_T: Optional[torch.Tensor], seeds):
    """``(seeds, x)``: the seeds as the library takes them (None: unseeded) and the start state on ``device`` -- a given ``x_T`` as it
    is, else draw 0 of every record with seeds, else ``torch.randn`` from the current generator."""
    if seeds is not None:
        seeds = _native.seeds_tensor(seeds, int(shape[0]), device).to(device)
        return seeds, (_native.normal_fill(seeds, shape, 0) if x_T is None else x_T.to(device))
    return None, (torch.randn(shape, device=device) if x_T is None else x_T.to(device))


def guide_options(guide, shape: tuple, guide_strength: float, guide_t_min: int, device) -> Optional[dict]:
    """The low-resolution guide of one ``sample`` call, checked: None without a guide, else ``dict(guide=, guide_strength=,
    guide_t_min=)`` with the guide as a contiguous fp32 tensor on ``device``.  ``guide`` is ``(B, C, H/N, W/N)`` against ``shape`` =
    ``(B, C, H, W)``: N is inferred, and must be a power of two in 2..64 that divides H and W; ``guide_strength`` in (0, 1];
    ``guide_t_min >= 0``; anything else is a ``ValueError``."""
    if guide is None:
        return None
    if not isinstance(guide, torch.Tensor):
        guide = torch.as_tensor(guide)
    _, lam, t_min = _native.guide_args(guide, tuple(shape), guide_strength, guide_t_min)
    return dict(guide=guide.to(device=device, dtype=torch.float32).contiguous(), guide_strength=lam, guide_t_min=t_min)


def fused_kwargs(sampler, w: Optional[float], null_z: Optional[torch.Tensor], slot: int, guide: Optional[dict] = None) -> dict:
    """The keyword arguments of ``model.sample_ddim`` that do not depend on the tables (``guide``: ``guide_options``' result)."""
    kw = dict(use_graph=sampler.use_graph, slot=slot)
    if guide is not None:
        kw.update(guide)
    if w is not None:
        kw.update(guidance=w, null_z=null_z)
        if sampler.guidance_rescale is not None:
            kw["guidance_rescale"] = sampler.guidance_rescale
    if sampler.prediction != "eps":
        kw["prediction"] = sampler.prediction
    if sampler.dynamic_threshold is not None:
        kw.update(dynamic_threshold=sampler.dynamic_threshold, threshold_max=sampler.threshold_max)
    return kw


def stepwise(sampler, model, x: torch.Tensor, z_clip: torch.Tensor, ts, coef, w: Optional[float], null_z: Optional[torch.Tensor],
             sigma=None, seeds: Optional[torch.Tensor] = None, multistep: bool = False, guide: Optional[dict] = None) -> torch.Tensor:
    """The loop for any callable ``model(x, z, t)``.  Per step: the model call (two when guided), the guidance-rescale factors if the
    sampler has a rescale and the step is guided, the dynamic threshold if the sampler has one, the low-resolution guide's
    ``lowres_delta`` if ``guide`` (``guide_options``' result) is given and ``ts[i] >= guide_t_min``, then one ``sampler_step`` on
    ``coef[i]`` -- with ``sigma[i] > 0`` it adds draw ``1 + i`` of the seeds or, unseeded,
    one ``torch.randn_like`` (drawn on those steps only); ``multistep``: with the x0 history."""
    x = _native.require_dev(x, "x_T").clone()
    B, device = x.shape[0], z_clip.device
    hist = torch.empty_like(x) if multistep else None
    z_u = None
    if w is not None:
        z_u = (torch.zeros_like(z_clip[0]) if null_z is None else null_z).expand(B, -1).contiguous()
    for i in range(len(ts)):
        t_b = torch.full((B,), int(ts[i]), device=device, dtype=torch.long)
        out = model(x, z_clip, t_b)
        out_u = model(x, z_u, t_b) if w is not None else None
        s = float(sigma[i]) if sigma is not None else 0.0
        thr = gscale = None
        if sampler.guidance_rescale is not None and w is not None:
            gscale = _native.guidance_rescale(out, out_u, w, sampler.guidance_rescale)
        if sampler.dynamic_threshold is not None:
            thr = _native.x0_threshold(x, out, coef[i, :2], sampler.prediction, sampler.dynamic_threshold, sampler.threshold_max, out_u=out_u,
                                       w=w or 0.0, gscale=gscale)
        delta = None
        if guide is not None and int(ts[i]) >= guide["guide_t_min"]:
            delta = _native.lowres_delta(x, out, coef[i, :2], guide["guide"], guide["guide_strength"], sampler.prediction, out_u=out_u,
                                         w=w or 0.0, thr=thr, gscale=gscale)
        if s > 0 and seeds is not None:
            noise = dict(seeds=seeds, draw=1 + i)
        else:
            noise = dict(noise=torch.randn_like(x) if s > 0 else None)
        _native.sampler_step(x, out, coef[i], sampler.prediction, out_u=out_u, w=w or 0.0, hist=hist, sigma=s, thr=thr, gscale=gscale, delta=delta,
                             **noise)
    return x
