"""DPMSolverSampler: a second-order multistep sampler (DPM-Solver++ 2M, data-prediction form) on the MI355X path.

No reference counterpart: the reference ships first-order DDIM only (``diffusion/ddim.py``).  The solver integrates the same
probability-flow ODE as ``DDIMSampler(eta=0)`` and costs the same one UNet evaluation per step; it keeps the previous step's ``x0``
prediction and adds one multiply-add per element, which lives in the head kernel's epilogue next to the DDIM update.

Per step from ``t = ts[i]`` to ``u = ts[i+1]``, with ``a = sqrt(alpha_bar)``, ``s = sqrt(1 - alpha_bar)``, ``lambda = log(a/s)``,
``h_i = lambda_u - lambda_t`` and ``r_i = h_(i-1) / h_i`` (``NoiseScheduler.solver_coefficients``)::

    x0 = clamp((x - s_t e) / a_t, -1, 1)
    x  = a_u x0 + s_u e                                  # == (s_u/s_t) x + a_u (1 - exp(-h)) x0 without the clamp
    x += a_u (1 - exp(-h_i)) / (2 r_i) * (x0 - x0_prev)  # order 2, steps 0 < i < n-1

Differences from ``DDIMSampler``, on purpose: the noise level after a step is that of the NEXT table entry (``alphas_cumprod[ts[i+1]]``,
1.0 after the last step), not the reference's ``alphas_cumprod_prev[t]`` -- a multistep solver extrapolates across steps and needs the
state at the noise level the model is told; and the default timestep table is uniform in ``lambda`` (``spacing="logsnr"``), the
spacing the method is designed for.  Targets that snap to the same table timestep are merged, so the table may hold fewer than
``steps`` entries (``NoiseScheduler.solver_timesteps``).  The first step and the last one (``h`` is infinite there) are first order.
``order=1`` is the same loop without the correction term.  The sampler is deterministic: no ``eta``.

Two routes as in ``DDIMSampler``: fused (``model.sample_ddim`` -> the loop of ``ccn_sample_ms`` / ``ccn_sample_guided_ms``, one captured graph)
and stepwise for any callable ``model(x, z, t)`` (one model call per step, two when guided, then ``ccn_sampler_step``).
``guided=True`` with ``cfg_scale == 1.0`` takes the unguided route.

``prediction="v"`` (default ``"eps"``): the network output is ``v = a_t noise - s_t x0``; the first line of the step becomes
``x0 = clamp(a_t x - s_t v, -1, 1)``, ``e = s_t x + a_t v`` on the same tables, the rest is unchanged (``ccn_set_prediction`` on the
fused route, ``ccn_sampler_step`` on the stepwise one).  It must match how the weights were trained.

``sample(..., seeds=...)``: one 64-bit seed per record (ints or an int64 tensor of ``B`` entries, as for ``DDIMSampler``); ``x_T=None``
is then the records' own start noise, ``normal_fill(seeds, shape, 0)``.  The steps draw nothing, so a given ``x_T`` makes the
seeds irrelevant; a wrong length is still a ``ValueError``.

``DPMSolverSampler(..., dynamic_threshold=p, threshold_max=s_max)`` (default None: unchanged): dynamic thresholding of x0 as in
``DDIMSampler`` -- ``s = min(max(quantile(|x0|, p), 1), s_max)`` per image and step, ``x0 = clamp(x0, -s, s) / s`` -- and the x0
history holds the thresholded x0, so the second-order term differences what the solver actually used.

``DPMSolverSampler(..., guided=True, guidance_rescale=phi)`` (default None: unchanged): the guidance rescale as in ``DDIMSampler`` --
the combined output times ``phi std(y_c) / std(y) + 1 - phi`` per image and step, before x0 is formed.

A scheduler made with ``rescale_zero_snr=True`` needs ``prediction="v"`` (``"eps"`` is a ``ValueError``).  ``lambda(T-1)`` is then
``-inf``: the ``logsnr`` table places ``steps - 1`` targets between ``lambda(T-2)`` and ``lambda(0)`` and starts at ``T-1``; the step
out of ``T-1`` has an infinite ``h``, so it and the step after it are first order.

``sample(..., guide=g, guide_strength=1.0, guide_t_min=0)`` (default None: unchanged): the low-resolution guide as in ``DDIMSampler``
-- every N x N block of the clamped x0 shifted by ``guide_strength * (g - block mean)`` on the steps with ``ts[i] >= guide_t_min`` --
and the x0 history holds the shifted x0.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import guidance, sampling

_SPACINGS = ("logsnr", "linspace")


class DPMSolverSampler:
    """Deterministic DPM-Solver++ 2M (``order=2``) / its first-order form (``order=1``); ``guided=True``: classifier-free guidance."""

    def __init__(self, scheduler, order: int = 2, spacing: str = "logsnr", guided: bool = False,
                 null_z: Optional[torch.Tensor] = None, prediction: str = "eps", dynamic_threshold: Optional[float] = None,
                 threshold_max: Optional[float] = None, guidance_rescale: Optional[float] = None) -> None:
        sampling.set_options(self, prediction, dynamic_threshold, threshold_max, guidance_rescale, guided, scheduler)
        if order not in (1, 2):
            raise ValueError(f"order must be 1 or 2, got {order}")
        if spacing not in _SPACINGS:
            raise ValueError(f"Unknown spacing {spacing}")
        self.sch = scheduler
        self.order = order
        self.spacing = spacing
        self.guided = bool(guided)
        self.null_z = null_z                 # (z_dim,), the embedding of the unconditional branch; None: zeros
        self.use_graph = True

    def tables(self, steps: int):
        """(timesteps int32 (n,), coefficients fp32 (n, 5)) of a ``steps``-step run; ``n <= steps``."""
        if steps < 2:
            raise ValueError(f"a multistep sampler needs steps >= 2, got {steps}")
        ts = self.sch.solver_timesteps(steps, self.spacing)
        return ts, self.sch.solver_coefficients(ts, self.order)

    @torch.no_grad()
    def sample(self, model, z_clip: torch.Tensor, shape: tuple, steps: int = 20, cfg_scale: float = 1.0,
               x_T: Optional[torch.Tensor] = None, slot: int = 0, seeds=None, guide: Optional[torch.Tensor] = None,
               guide_strength: float = 1.0, guide_t_min: int = 0) -> torch.Tensor:
        ts, coef = self.tables(steps)
        w, null_z = guidance.resolve(self.guided, self.null_z, z_clip, cfg_scale)
        device = z_clip.device
        if device.type != "cuda":
            raise RuntimeError(f"z_clip is on {device}: DPMSolverSampler (MI355X build) needs a HIP device; no CPU fallback")
        seeds, x = sampling.start_state(shape, device, x_T, seeds)
        guide = sampling.guide_options(guide, shape, guide_strength, guide_t_min, device)
        if hasattr(model, "sample_ddim"):
            return model.sample_ddim(z_clip, x, ts, coef[:, :4], c4=coef[:, 4], **sampling.fused_kwargs(self, w, null_z, slot, guide))
        return sampling.stepwise(self, model, x, z_clip, ts, coef, w, null_z, multistep=True, guide=guide)
