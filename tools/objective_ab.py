#!/usr/bin/env python3
"""A/B of the training objective's routes at the bench_train.py shape (256 px, base 128, (1,2,2), batch 4, bf16), one process, one GPU.

    python tools/objective_ab.py [--rounds 5] [--steps 40] [--warmup 5] [--recon-w 0.05] [--tv-w 1e-4]

Variants, run one after the other inside every round (so that drift of the machine hits all of them alike):
  mse        train_step, eps-MSE only (what bench_train.py times by default)
  fused      train_step(recon_w, tv_w): the objective and its gradient from ccn_diffusion_loss_grad
  autograd   train_diffusion(fused_objective=False)'s loop body (autograd_objective_step): the same objective from torch ops through
             autograd, t / noise drawn with torch, the loss read back to the host every batch, opt.step() and opt.zero_grad() apart
  fused_td   train_diffusion(fused_objective=True)'s loop body: t / noise drawn with torch and handed to train_step, the running loss
             accumulated on the device
Prints ms per step of every round and the median / min / max per variant, then fused - mse in microseconds and autograd / fused.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "clip-neural-image-conpression_amd")]

from clip_feature_codec.models.unet import CLIPCondUNet  # noqa: E402
from clip_feature_codec.diffusion.scheduler import NoiseScheduler  # noqa: E402
from clip_feature_codec.train.diffusion_train import FusedAdamW, autograd_objective_step, train_step  # noqa: E402
from clip_feature_codec.utils import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16"); ap.add_argument("--batch", type=int, default=4); ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--base", type=int, default=128); ap.add_argument("--ch-mult", default="1,2,2")
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--steps", type=int, default=40); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--recon-w", type=float, default=0.05); ap.add_argument("--tv-w", type=float, default=1e-4)
    ap.add_argument("--only", default="", help="comma-separated subset of the variants (for a kernel trace of one route)")
    a = ap.parse_args()
    dev = "cuda:0"
    ch_mult = tuple(int(v) for v in a.ch_mult.split(","))
    sd = synth.synth_state_dict(synth.unet_param_spec(512, a.base, ch_mult))
    net = CLIPCondUNet(512, a.base, ch_mult, dtype=a.dtype).to(dev)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    net.train()
    sch = NoiseScheduler(1000, "cosine", device=dev)
    opt = FusedAdamW(net, lr=2e-4)
    g = torch.Generator("cpu").manual_seed(1000)
    x0 = (torch.rand((a.batch, 3, a.size, a.size), generator=g) * 2 - 1).to(dev)
    z = torch.from_numpy(synth.synth_z(a.batch)).to(dev)
    running = torch.zeros((), dtype=torch.float64, device=dev)

    def draw():
        return torch.randint(0, 1000, (a.batch,), device=dev, dtype=torch.long), torch.randn_like(x0)

    def mse():
        train_step(net, sch, opt, x0, z)

    def fused():
        train_step(net, sch, opt, x0, z, recon_w=a.recon_w, tv_w=a.tv_w)

    def autograd():
        t, noise = draw()
        return float(autograd_objective_step(net, sch, opt, x0, z, t, noise, a.recon_w, a.tv_w)) * a.batch

    def fused_td():
        t, noise = draw()
        running.add_(train_step(net, sch, opt, x0, z, t=t, noise=noise, recon_w=a.recon_w, tv_w=a.tv_w).double() * a.batch)

    variants = {"mse": mse, "fused": fused, "autograd": autograd, "fused_td": fused_td}
    if a.only:
        variants = {k: variants[k] for k in a.only.split(",")}
    for fn in variants.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for r in range(a.rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        print(f"round {r}: " + "  ".join(f"{k} {ms[k][-1]:.3f}" for k in variants), flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        print(f"{k:9s} median {med[k]:.3f} ms/step  min {min(v):.3f}  max {max(v):.3f}  ({a.batch / med[k] * 1e3:.1f} images/s)")
    if "mse" in med and "fused" in med:
        d = [f - m for f, m in zip(ms["fused"], ms["mse"])]
        print(f"fused - mse: median {statistics.median(d) * 1e3:.1f} us/step (per round: {', '.join(f'{v * 1e3:.1f}' for v in d)}), "
              f"{statistics.median(d) / med['mse'] * 100:.2f} % of the MSE-only step")
    if "autograd" in med and "fused" in med:
        print(f"autograd / fused: {med['autograd'] / med['fused']:.3f};  autograd / fused_td: {med['autograd'] / med.get('fused_td', float('nan')):.3f}")


if __name__ == "__main__":
    main()
