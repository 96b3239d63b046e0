#!/usr/bin/env python3
"""Cost of the step guard at the bench_train.py shape (256 px, base 128, (1,2,2), batch 4, bf16), one process, one GPU.

    python tools/guard_ab.py [--rounds 5] [--steps 40] [--warmup 5] [--max-grad-norm 1.0]

Arms, run one after the other inside every round (so that drift of the machine hits all of them alike), each on its own model and
optimiser (a guarded optimiser cannot go back to unguarded steps):
  plain        train_step as it was: forward, fused MSE, backward, ccn_adamw_step_zero_grad       (the yardstick)
  guard        train_step(scaler=GradScaler()): d_eps * scale, ccn_grad_guard (one extra read of the gradient buffer, two small
               launches), ccn_adamw_step_guarded
  guard_clip   the same with max_grad_norm (no further pass: the clip coefficient comes out of the same reduction)
Prints ms per step of every round, the median / min / max per arm, and guard - plain / guard_clip - plain in microseconds next to the
floor: one read of the gradient buffer at the measured 6.29 TB/s copy rate.
--trace: per-launch times of the optimiser tail of ONE step of each arm from HIP events around every launch (synchronising; the
launches of the guard are timed one by one, so the figures include the launch gaps that back-to-back launches hide).
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "clip-neural-image-conpression_amd")]

from clip_feature_codec import _native  # noqa: E402
from clip_feature_codec.models.unet import CLIPCondUNet  # noqa: E402
from clip_feature_codec.diffusion.scheduler import NoiseScheduler  # noqa: E402
from clip_feature_codec.train.diffusion_train import FusedAdamW, GradScaler, train_step  # noqa: E402
from clip_feature_codec.utils import synth  # noqa: E402

COPY_TBS = 6.29


def timed(fn, reps=20):
    """Median microseconds of one launch sequence between two HIP events, after a warm-up call."""
    fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def trace(opt, scaler):
    """The optimiser tail launch by launch on this optimiser's real buffers (zero gradients: every step is applied)."""
    fp = opt.state.fp
    blk = scaler.block(fp.flat.device)
    b1, b2 = opt.betas
    rows = [
        ("ccn_adamw_step_zero_grad (plain tail)", lambda: _native.adamw_step(fp.flat, fp.grad, opt.exp_avg, opt.exp_avg_sq, 0.0, b1, b2, opt.eps, 0.0, 1, zero_grad=True)),
        ("ccn_grad_guard (partials + finalize)", lambda: _native.grad_guard(fp.grad, blk, scaler.scratch, 0.0, b1, b2, 2.0, 0.5, 2000)),
        ("ccn_adamw_step_guarded", lambda: _native.adamw_step_guarded(fp.flat, fp.grad, opt.exp_avg, opt.exp_avg_sq, 0.0, b1, b2, opt.eps, 0.0, blk)),
        ("guard + guarded AdamW back to back", lambda: (_native.grad_guard(fp.grad, blk, scaler.scratch, 0.0, b1, b2, 2.0, 0.5, 2000),
                                                        _native.adamw_step_guarded(fp.flat, fp.grad, opt.exp_avg, opt.exp_avg_sq, 0.0, b1, b2, opt.eps, 0.0, blk))),
    ]
    n = fp.grad.numel()
    print(f"launch by launch ({n} gradients, {n * 4 / 1e6:.1f} MB per pass over one buffer; lr = 0 so the parameters stay put):")
    for name, fn in rows:
        print(f"  {name:40s} {timed(fn):8.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16"); ap.add_argument("--batch", type=int, default=4); ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--base", type=int, default=128); ap.add_argument("--ch-mult", default="1,2,2")
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--steps", type=int, default=40); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--max-grad-norm", type=float, default=1.0)
    ap.add_argument("--trace", action="store_true", help="also time the optimiser tail launch by launch")
    a = ap.parse_args()
    dev = "cuda:0"
    ch_mult = tuple(int(v) for v in a.ch_mult.split(","))
    sd = synth.synth_state_dict(synth.unet_param_spec(512, a.base, ch_mult))
    sch = NoiseScheduler(1000, "cosine", device=dev)
    g = torch.Generator("cpu").manual_seed(1000)
    x0 = (torch.rand((a.batch, 3, a.size, a.size), generator=g) * 2 - 1).to(dev)
    z = torch.from_numpy(synth.synth_z(a.batch)).to(dev)

    def arm(**kw):
        net = CLIPCondUNet(512, a.base, ch_mult, dtype=a.dtype).to(dev)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        net.train()
        opt = FusedAdamW(net, lr=2e-4)
        return (lambda: train_step(net, sch, opt, x0, z, **kw)), opt

    scalers = {"guard": GradScaler(), "guard_clip": GradScaler()}
    arms = {"plain": arm(), "guard": arm(scaler=scalers["guard"]), "guard_clip": arm(scaler=scalers["guard_clip"], max_grad_norm=a.max_grad_norm)}
    for fn, _ in arms.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for r in range(a.rounds):
        for k, (fn, _) in arms.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(a.steps):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        print(f"round {r}: " + "  ".join(f"{k} {ms[k][-1]:.3f}" for k in arms), flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, v in ms.items():
        print(f"{k:11s} median {med[k]:.3f} ms/step  min {min(v):.3f}  max {max(v):.3f}  ({a.batch / med[k] * 1e3:.1f} images/s)")
    n = arms["plain"][1].state.fp.grad.numel()
    floor = n * 4 / (COPY_TBS * 1e12) * 1e6
    for k in ("guard", "guard_clip"):
        d = [x - p for x, p in zip(ms[k], ms["plain"])]
        print(f"{k} - plain: median {statistics.median(d) * 1e3:.1f} us/step (per round: {', '.join(f'{v * 1e3:.1f}' for v in d)}), "
              f"{statistics.median(d) / med['plain'] * 100:.2f} % of the plain step; floor {floor:.1f} us (one read of {n * 4 / 1e6:.1f} MB at {COPY_TBS} TB/s)")
    for k, s in scalers.items():
        st = s.state_dict()
        print(f"{k}: scale {st['scale']:g}, applied {st['good_steps']}, skipped {st['skipped_steps']}, last grad norm {float(s.stats()['grad_norm']):.4g}")
    if a.trace:
        trace(arms["guard"][1], scalers["guard"])


if __name__ == "__main__":
    main()
