"""``python -m clip_feature_codec.cli.reconstruct_diffusion`` -- .clp -> DDIM -> PNG on an MI355X.

Same flags, defaults and output as the reference CLI (cli/reconstruct_diffusion.py:26-58):
``--store_dir --bitstream --weights --out --steps --eta --size --device``; prints ``Saved to <out>``;
the PNG is written from ``((clamp(x,-1,1)+1)*127.5).astype(uint8)`` (truncation).  Additions that
default to the reference behaviour: ``--seed`` (reproducible CPU-generated start noise; the reference
never seeds), ``--dtype {fp32,bf16,f16x3}``, ``--cfg_scale`` (classifier-free guidance; 1.0 = off), ``--sampler {ddim,dpmpp2m}`` with ``--spacing {linspace,logsnr}``
(the second-order multistep solver of ``diffusion/dpm_solver.py``; default ``ddim``), ``--device_noise`` (with ``--seed``: the start
noise and the ``--eta > 0`` noise come from the device generator keyed by the seed, nothing is drawn on the host or uploaded; another
generator than ``--seed`` alone, so another image), ``--dynamic_threshold P [--threshold_max S]`` (dynamic thresholding of x0 instead
of the static clamp, for guided sampling; off by default), ``--guidance_rescale PHI`` (with ``--cfg_scale`` other than 1: the guided
output rescaled towards the conditional output's per-image standard deviation, Lin et al. 2023; off by default), ``--zero_snr`` (with
``--prediction v``: the schedule rescaled to zero terminal SNR, for a checkpoint trained on it), ``--lowres_guide FILE
[--guide_strength L] [--guide_t_min T]`` (a thumbnail that travels next to the bitstream -- an image or a uint8 ``.npy`` of shape
``(h, w, 3)``, ``N = size / h`` -- to which every step's x0 is held block mean by block mean; off by default) and the architecture is
read from the checkpoint's shapes.
"""
from __future__ import annotations

import argparse
from pathlib import Path

import numpy as np
import torch
from PIL import Image

from ._common import add_guide_flags, check_guide_flags, load_guide_file, add_rescale_flags, add_threshold_flags, check_rescale_flags, check_noise_flags, check_sampler_flags, check_threshold_flags, pick_device, record_seeds, load_codec_meta, load_embedding, build_model, build_sampler, start_noise


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Reconstruct an image from a .clp bitstream via DDIM sampling (MI355X build).")
    ap.add_argument("--store_dir", type=str, required=True)
    ap.add_argument("--bitstream", type=str, required=True)
    ap.add_argument("--weights", type=str, required=True)
    ap.add_argument("--out", type=str, default="recon.png")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--eta", type=float, default=0.0)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--seed", type=int, default=None, help="seed of the CPU-generated start noise (default: unseeded, like the reference)")
    ap.add_argument("--device_noise", action="store_true",
                    help="with --seed: every draw comes from the device generator keyed by the seed (reproducible also with --eta > 0); "
                         "another generator than --seed alone")
    ap.add_argument("--dtype", choices=["fp32", "bf16", "f16x3"], default="fp32")
    ap.add_argument("--cfg_scale", type=float, default=1.0,
                    help="classifier-free guidance scale w: eps = eps_u + w * (eps_c - eps_u), eps_u predicted from the zero embedding "
                         "(a checkpoint trained with z_drop); 1.0 (default): unguided, the reference's behaviour")
    ap.add_argument("--sampler", choices=["ddim", "dpmpp2m"], default="ddim",
                    help="ddim (default): the reference's first-order sampler; dpmpp2m: DPM-Solver++ 2M, second-order multistep, "
                         "deterministic (an error with --eta > 0), the same one UNet evaluation per step")
    ap.add_argument("--prediction", choices=["eps", "v"], default="eps",
                    help="what the network predicts: eps (default, the reference's) or v = sqrt(ab) noise - sqrt(1-ab) x0; it must match how "
                         "the checkpoint was trained (train_diffusion(prediction=)): the checkpoint itself does not say")
    ap.add_argument("--spacing", choices=["linspace", "logsnr"], default="logsnr",
                    help="timestep table of --sampler dpmpp2m (read only then): uniform in log-SNR (may merge into fewer than "
                         "--steps entries) or the reference's linspace")
    add_threshold_flags(ap)
    add_rescale_flags(ap)
    add_guide_flags(ap, "file")
    return ap


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    check_sampler_flags(args.sampler, args.eta)
    check_noise_flags(args.device_noise, args.seed)
    check_threshold_flags(args.dynamic_threshold, args.threshold_max)
    check_rescale_flags(args.guidance_rescale, args.cfg_scale, args.zero_snr, args.prediction)
    check_guide_flags(args.lowres_guide, args.guide_strength, args.guide_t_min, args.size)
    guide_kw = {}
    if args.lowres_guide is not None:                              # (read before the device is touched: a bad file exits here)
        guide_kw = dict(guide=torch.from_numpy(load_guide_file(args.lowres_guide, args.size)),
                        guide_strength=1.0 if args.guide_strength is None else args.guide_strength, guide_t_min=args.guide_t_min or 0)

    device = pick_device(args.device)
    scale, zero = load_codec_meta(Path(args.store_dir))
    z = torch.from_numpy(load_embedding(Path(args.bitstream), scale, zero)).to(device)
    net = build_model(args.weights, device, z.shape[1], args.dtype)
    sampler = build_sampler(args.eta, device, guided=args.cfg_scale != 1.0, sampler=args.sampler, spacing=args.spacing,
                            prediction=args.prediction, dynamic_threshold=args.dynamic_threshold, threshold_max=args.threshold_max,
                            guidance_rescale=args.guidance_rescale, zero_snr=args.zero_snr)
    x_T = None if args.device_noise else start_noise([0], args.size, args.seed)
    noise_kw = dict(seeds=record_seeds([0], args.seed)) if args.device_noise else {}
    with torch.no_grad():
        x = sampler.sample(net, z, shape=(1, 3, args.size, args.size), steps=args.steps, cfg_scale=args.cfg_scale,
                           x_T=None if x_T is None else x_T.to(device), **noise_kw, **guide_kw)
    img = x[0].clamp(-1, 1).cpu().numpy().transpose(1, 2, 0)
    Image.fromarray(((img + 1.0) * 127.5).astype(np.uint8)).save(args.out)
    print(f"Saved to {args.out}")


if __name__ == "__main__":
    main()
