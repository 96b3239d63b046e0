"""Shared pieces of the two hot-path CLIs: checkpoint loading, z decode, deterministic start noise."""
from __future__ import annotations

import os
from pathlib import Path
from typing import Sequence, Tuple

import numpy as np
import torch

from ..io.bitstream import read_bitstream, decode_embedding
from ..models.unet import CLIPCondUNet, infer_arch
from ..diffusion.scheduler import NoiseScheduler
from ..diffusion.ddim import DDIMSampler
from ..diffusion.dpm_solver import DPMSolverSampler


def pick_device(requested: str | None) -> str:
    """'cuda' (bound to LOCAL_RANK under torchrun) -- this build has no CPU path."""
    dev = requested or ("cuda" if torch.cuda.is_available() else "cpu")
    if not str(dev).startswith("cuda"):
        raise SystemExit("this MI355X build computes on a HIP device only (no CPU fallback); "
                         "run the reference package for --device cpu")
    if dev == "cuda":
        dev = f"cuda:{int(os.environ.get('LOCAL_RANK', '0')) % max(torch.cuda.device_count(), 1)}"
    torch.cuda.set_device(torch.device(dev))
    return dev


def load_codec_meta(store_dir: Path) -> Tuple[np.ndarray, np.ndarray]:
    meta = np.load(Path(store_dir) / "codec_meta.npz")
    return meta["scale"].astype("float32"), meta["zero"].astype("float32")


def load_embedding(bitstream: Path, scale: np.ndarray, zero: np.ndarray) -> np.ndarray:
    return decode_embedding(read_bitstream(Path(bitstream)), scale, zero)


def build_model(weights: str, device: str, z_dim: int, dtype: str = "fp32") -> CLIPCondUNet:
    """Architecture from the checkpoint's shapes (reference checkpoints give base=128, ch_mult=(1,2,2))."""
    sd = torch.load(weights, map_location="cpu", weights_only=True)
    arch = infer_arch(sd)
    if arch["z_dim"] != z_dim:
        raise SystemExit(f"checkpoint z_dim {arch['z_dim']} does not match the store's embedding dim {z_dim}")
    net = CLIPCondUNet(**arch, dtype=dtype).to(device)
    net.load_state_dict(sd, strict=True)
    net.eval()
    return net


def check_sampler_flags(sampler: str, eta: float) -> None:
    """``--sampler dpmpp2m`` is deterministic: ``--eta > 0`` with it is an error (both CLIs call this right after parsing)."""
    if sampler == "dpmpp2m" and eta > 0:
        raise SystemExit("--sampler dpmpp2m is deterministic: --eta must be 0")


def check_noise_flags(device_noise: bool, seed: int | None) -> None:
    """``--device_noise`` keys every draw to the record's seed, so it needs ``--seed`` (both CLIs call this right after parsing)."""
    if device_noise and seed is None:
        raise SystemExit("--device_noise needs --seed: record i draws from seed + i")


def add_threshold_flags(ap) -> None:
    """``--dynamic_threshold P [--threshold_max S]`` (both CLIs): dynamic thresholding of x0 instead of the static clamp, off by default."""
    ap.add_argument("--dynamic_threshold", type=float, default=None, metavar="P",
                    help="dynamic thresholding of x0 (Imagen): per image and step s = max(quantile(|x0|, P), 1), x0 = clamp(x0, -s, s) / s "
                         "instead of clamp(x0, -1, 1); P in (0, 1], e.g. 0.995; meant for --cfg_scale > 1; off by default")
    ap.add_argument("--threshold_max", type=float, default=None, metavar="S", help="with --dynamic_threshold: an upper bound S >= 1 on s (default: none)")


def check_threshold_flags(dynamic_threshold: float | None, threshold_max: float | None) -> None:
    """Both CLIs call this right after parsing: a quantile in (0, 1], a maximum of at least 1 and only with the quantile."""
    if dynamic_threshold is None:
        if threshold_max is not None:
            raise SystemExit("--threshold_max needs --dynamic_threshold")
        return
    if not 0.0 < dynamic_threshold <= 1.0:
        raise SystemExit("--dynamic_threshold must be a quantile in (0, 1]")
    if threshold_max is not None and not threshold_max >= 1.0:
        raise SystemExit("--threshold_max must be at least 1")


def add_rescale_flags(ap) -> None:
    """``--guidance_rescale PHI`` and ``--zero_snr`` (both CLIs), the two fixes of Lin et al. 2023; both off by default."""
    ap.add_argument("--guidance_rescale", type=float, default=None, metavar="PHI",
                    help="guidance rescale (Lin et al. 2023; diffusers' guidance_rescale): per image and step the guided output is multiplied "
                         "by PHI std(cond) / std(guided) + 1 - PHI; PHI in (0, 1], the paper suggests 0.7; needs --cfg_scale other than 1; "
                         "off by default")
    ap.add_argument("--zero_snr", action="store_true",
                    help="sample on the schedule rescaled to zero terminal SNR (same paper); needs --prediction v and must match how the "
                         "checkpoint was trained (train_diffusion(zero_snr=)): the checkpoint itself does not say")


def check_rescale_flags(guidance_rescale: float | None, cfg_scale: float, zero_snr: bool, prediction: str) -> None:
    """Both CLIs call this right after parsing: PHI in (0, 1] and only under guidance; ``--zero_snr`` only with ``--prediction v``."""
    if guidance_rescale is not None:
        if not 0.0 < guidance_rescale <= 1.0:
            raise SystemExit("--guidance_rescale must be a factor in (0, 1]")
        if cfg_scale == 1.0:
            raise SystemExit("--guidance_rescale needs guidance: --cfg_scale other than 1")
    if zero_snr and prediction != "v":
        raise SystemExit("--zero_snr needs --prediction v: the eps form divides by sqrt(alpha_bar_t), which is 0 at t = T-1")


def record_seeds(indices: Sequence[int], seed: int) -> list:
    """The 64-bit seeds of ``--device_noise``: record ``i`` of the manifest gets ``seed + i``, the rule of ``start_noise``."""
    return [int(seed) + int(i) for i in indices]


def build_sampler(eta: float, device: str, guided: bool = False, sampler: str = "ddim", spacing: str = "logsnr", prediction: str = "eps",
                  dynamic_threshold: float | None = None, threshold_max: float | None = None, guidance_rescale: float | None = None,
                  zero_snr: bool = False):
    """``guided``: the sampler gives ``cfg_scale`` its meaning (classifier-free guidance against the zero embedding).
    ``sampler="dpmpp2m"``: the second-order multistep solver on the ``spacing`` timestep table (deterministic: no ``eta``).
    ``prediction``: ``"eps"`` or ``"v"``, how the checkpoint was trained.  ``dynamic_threshold`` / ``threshold_max``: dynamic
    thresholding of x0 (None: the static clamp).  ``guidance_rescale``: the guidance rescale's phi (None: off; needs ``guided``).
    ``zero_snr``: the scheduler is built with ``rescale_zero_snr=True``, refused without ``prediction="v"``."""
    check_sampler_flags(sampler, eta)
    if zero_snr and prediction != "v":
        raise SystemExit("--zero_snr needs --prediction v: the eps form divides by sqrt(alpha_bar_t), which is 0 at t = T-1")
    thr = dict(dynamic_threshold=dynamic_threshold, threshold_max=threshold_max, guidance_rescale=guidance_rescale)
    sch = NoiseScheduler(timesteps=1000, schedule="cosine", device=device, rescale_zero_snr=zero_snr)
    if sampler == "dpmpp2m":
        return DPMSolverSampler(sch, order=2, spacing=spacing, guided=guided,
                                prediction=prediction, **thr)
    if sampler != "ddim":
        raise SystemExit(f"unknown sampler {sampler}")
    return DDIMSampler(sch, eta=eta, guided=guided, prediction=prediction, **thr)


def start_noise(indices: Sequence[int], size: int, seed: int | None, img_ch: int = 3) -> torch.Tensor | None:
    """Per-record x_T from CPU generators seeded seed+index (sharding- and batch-invariant); None = unseeded."""
    if seed is None:
        return None
    rows = [torch.randn((img_ch, size, size), generator=torch.Generator("cpu").manual_seed(int(seed) + int(i)))
            for i in indices]
    return torch.stack(rows, 0)
