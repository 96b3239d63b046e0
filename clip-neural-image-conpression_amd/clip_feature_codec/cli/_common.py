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


def add_guide_flags(ap, source: str) -> None:
    """``--lowres_guide`` with ``--guide_strength`` and ``--guide_t_min`` (both CLIs), the low-resolution guide; off by default.
    ``source="original"`` (eval): the value is the block size N and the thumbnail is derived from the record's original, with
    ``--guide_bits``; ``source="file"`` (reconstruct_diffusion): the value is the thumbnail's file."""
    if source == "original":
        ap.add_argument("--lowres_guide", type=int, default=None, metavar="N",
                        help="hold every step's x0 to a thumbnail of the original (ILVR / DDNM in x0 space): the N x N block means of the "
                             "original, quantised to --guide_bits, are what a codec would send next to the embedding "
                             "(side_bytes_per_record in --out_json); N a power of two in 2..64 that divides --size; off by default")
        ap.add_argument("--guide_bits", type=int, default=8, metavar="BITS",
                        help="with --lowres_guide: levels per thumbnail value, 2^BITS over [-1, 1]; 1..8 (default 8: uint8)")
    else:
        ap.add_argument("--lowres_guide", type=str, default=None, metavar="FILE",
                        help="hold every step's x0 to this thumbnail (ILVR / DDNM in x0 space): an image that PIL opens, or a uint8 .npy of "
                             "shape (h, w, 3); it must be square and --size / h a power of two in 2..64; off by default")
    ap.add_argument("--guide_strength", type=float, default=None, metavar="L",
                    help="with --lowres_guide: the fraction of the block-mean error removed per step, in (0, 1] (default 1)")
    ap.add_argument("--guide_t_min", type=int, default=None, metavar="T",
                    help="with --lowres_guide: only the steps at timestep T or above are guided (default 0: all)")


def check_guide_flags(lowres_guide, guide_strength: float | None, guide_t_min: int | None, size: int, guide_bits: int | None = None) -> None:
    """Both CLIs call this right after parsing: the strength in (0, 1], ``T >= 0``, ``BITS`` in 1..8, none of them without
    ``--lowres_guide``; an integer N (eval) must be a power of two in 2..64 that divides ``--size``."""
    if lowres_guide is None:
        if guide_strength is not None or guide_t_min is not None or guide_bits not in (None, 8):
            raise SystemExit("--guide_strength, --guide_t_min and --guide_bits need --lowres_guide")
        return
    if guide_strength is not None and not 0.0 < guide_strength <= 1.0:
        raise SystemExit("--guide_strength (with --lowres_guide) must be in (0, 1]")
    if guide_t_min is not None and guide_t_min < 0:
        raise SystemExit("--guide_t_min (with --lowres_guide) must not be negative")
    if guide_bits is not None and not 1 <= guide_bits <= 8:
        raise SystemExit("--guide_bits (with --lowres_guide) must be in 1..8")
    if isinstance(lowres_guide, int):
        check_guide_factor(size, lowres_guide)


def check_guide_factor(size: int, n: int) -> None:
    if n < 2 or n > 64 or n & (n - 1) or size % n:
        raise SystemExit(f"--lowres_guide: the block size must be a power of two in 2..64 that divides --size {size}, got {n}")


def derive_guide(orig: np.ndarray, n: int, bits: int = 8) -> np.ndarray:
    """The thumbnail a codec would send for ``orig`` -- ``(C, H, W)``, float in [-1, 1] or the uint8 form of it (``v / 127.5 - 1``) --
    as the decoder uses it: the float64 ``n x n`` block means, quantised to ``2^bits`` levels over [-1, 1] (8: the uint8 levels) and
    mapped back, ``(C, H/n, W/n)`` float32."""
    v = np.asarray(orig)
    v = v.astype(np.float64) / 127.5 - 1.0 if v.dtype == np.uint8 else v.astype(np.float64)
    c, h, w = v.shape
    m = v.reshape(c, h // n, n, w // n, n).mean(axis=(2, 4))
    top = float(2 ** bits - 1)
    q = np.clip(np.rint((m + 1.0) * 0.5 * top), 0.0, top)
    return (q / top * 2.0 - 1.0).astype(np.float32)


def guide_side_bytes(size: int, n: int, bits: int = 8, channels: int = 3) -> int:
    """Bytes of one record's thumbnail: ``channels (size / n)^2`` values of ``bits`` bits, rounded up."""
    return (channels * (size // n) ** 2 * bits + 7) // 8


def load_guide_file(path: str, size: int) -> np.ndarray:
    """``--lowres_guide FILE`` of reconstruct_diffusion: an image that PIL opens (read as RGB) or a uint8 ``.npy`` of shape
    ``(h, w, 3)``, as ``(1, 3, h, w)`` float32 in [-1, 1] (``v / 127.5 - 1``).  ``N = size / h``: a size that does not divide, a
    thumbnail that is not square or an N that is no power of two in 2..64 is refused."""
    if str(path).endswith(".npy"):
        a = np.load(path)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise SystemExit(f"--lowres_guide: {path} must hold a uint8 array of shape (h, w, 3), got {a.dtype} {a.shape}")
    else:
        from PIL import Image
        a = np.array(Image.open(path).convert("RGB"))
    h, w = a.shape[:2]
    if h != w or h < 1 or size % h:
        raise SystemExit(f"--lowres_guide: a {h} x {w} thumbnail does not divide --size {size} into square blocks")
    check_guide_factor(size, size // h)
    return (a.astype(np.float32) / np.float32(127.5) - np.float32(1.0)).transpose(2, 0, 1)[None].copy()


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
