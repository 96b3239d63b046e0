#!/usr/bin/env python3
"""Cost of the weight EMA at the bench_train.py shape (256 px, base 128, (1,2,2), batch 4, bf16), one process, one GPU.

    python tools/ema_ab.py [--rounds 5] [--steps 40] [--warmup 5] [--decay 0.999]

Arms, run one after the other inside every round (so that drift of the machine hits all of them alike), each on its own model and
optimiser:
  plain        train_step as it was: forward, fused MSE, backward, ccn_adamw_step_zero_grad       (the yardstick)
  ema_fused    train_step with FusedAdamW(ema_decay=): ccn_adamw_step_ema -- the one-wave tick, then the AdamW pass that also reads
               and writes the average (two more 4-byte accesses per parameter)
  ema_torch    the plain step followed by ``ema.lerp_(flat, w)``: a separate pass that reads the parameters and the average and
               writes the average (what a host-side EMA costs when no step is ever skipped; it cannot see the guard's decision)
Prints ms per step of every round, the median / min / max per arm, and ema_fused - plain / ema_torch - plain in microseconds next to
their floors at the measured 6.29 TB/s copy rate: 2 x 4 bytes per parameter fused, 3 x 4 bytes plus a launch
for the separate pass.
--trace: the optimiser tail of ONE step from HIP events around the launches (synchronising; lr = 0 and zero gradients, so the
parameters stay put): every AdamW entry point -- plain, with the EMA, under a guard (with and without the guard's own reduction), both.
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
from clip_feature_codec.train.diffusion_train import FusedAdamW, train_step  # noqa: E402
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


def trace(opt, decay):
    """The optimiser tail on this optimiser's real buffers."""
    fp = opt.state.fp
    b1, b2 = opt.betas
    w = 1.0 - decay

    def plain():
        _native.adamw_step(fp.flat, fp.grad, opt.exp_avg, opt.exp_avg_sq, 0.0, b1, b2, opt.eps, 0.0, 1, zero_grad=True)

    def fused():
        _native.adamw_step_ema(fp.flat, fp.grad, opt.exp_avg, opt.exp_avg_sq, opt.ema, 0.0, b1, b2, opt.eps, 0.0, 1, decay, opt.ema_block,
                               zero_grad=True)

    block = torch.zeros(_native.GUARD_WORDS, dtype=torch.int32, device=fp.flat.device)
    scratch = torch.empty(_native.GUARD_SCRATCH_FLOATS, device=fp.flat.device)
    _native.step_guard_init(block, 1.0)

    def guard():
        _native.grad_guard(fp.grad, block, scratch, 1.0, b1, b2, 2.0, 0.5, 2000)

    def guarded():
        _native.adamw_step_guarded(fp.flat, fp.grad, opt.exp_avg, opt.exp_avg_sq, 0.0, b1, b2, opt.eps, 0.0, block)

    def guarded_fused():
        _native.adamw_step_ema(fp.flat, fp.grad, opt.exp_avg, opt.exp_avg_sq, opt.ema, 0.0, b1, b2, opt.eps, 0.0, 0, decay, opt.ema_block,
                               zero_grad=True, guard_block=block)

    rows = [("ccn_adamw_step (plain tail, keeps g)", lambda: _native.adamw_step(fp.flat, fp.grad, opt.exp_avg, opt.exp_avg_sq, 0.0, b1, b2, opt.eps, 0.0, 1)),
            ("ccn_adamw_step_zero_grad (plain tail)", plain), ("ccn_adamw_step_ema (tick + fused pass)", fused),
            ("ccn_grad_guard + ccn_adamw_step_guarded", lambda: (guard(), guarded())), ("ccn_adamw_step_guarded alone", guarded),
            ("ccn_grad_guard + ccn_adamw_step_ema", lambda: (guard(), guarded_fused())), ("ccn_adamw_step_ema under a guard, alone", guarded_fused),
            ("ema.lerp_(flat, w) alone", lambda: opt.ema.lerp_(fp.flat, w)),
            ("plain tail + lerp_ back to back", lambda: (plain(), opt.ema.lerp_(fp.flat, w)))]
    n = fp.grad.numel()
    print(f"launch by launch ({n} parameters, {n * 4 / 1e6:.1f} MB per pass over one buffer; lr = 0 so the parameters stay put):")
    for name, fn in rows:
        print(f"  {name:42s} {timed(fn):8.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16"); ap.add_argument("--batch", type=int, default=4); ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--base", type=int, default=128); ap.add_argument("--ch-mult", default="1,2,2")
    ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--steps", type=int, default=40); ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--decay", type=float, default=0.999)
    ap.add_argument("--trace", action="store_true", help="also time the optimiser tail launch by launch")
    a = ap.parse_args()
    dev = "cuda:0"
    ch_mult = tuple(int(v) for v in a.ch_mult.split(","))
    sd = synth.synth_state_dict(synth.unet_param_spec(512, a.base, ch_mult))
    sch = NoiseScheduler(1000, "cosine", device=dev)
    g = torch.Generator("cpu").manual_seed(1000)
    x0 = (torch.rand((a.batch, 3, a.size, a.size), generator=g) * 2 - 1).to(dev)
    z = torch.from_numpy(synth.synth_z(a.batch)).to(dev)
    w = 1.0 - a.decay

    def arm(kind):
        net = CLIPCondUNet(512, a.base, ch_mult, dtype=a.dtype).to(dev)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        net.train()
        opt = FusedAdamW(net, lr=2e-4, ema_decay=a.decay if kind == "ema_fused" else None)
        if kind != "ema_torch":
            return (lambda: train_step(net, sch, opt, x0, z)), opt
        flat = net.train_state().fp.flat
        ema = flat.clone()

        def step():
            train_step(net, sch, opt, x0, z)
            ema.lerp_(flat, w)
        return step, opt

    arms = {k: arm(k) for k in ("plain", "ema_fused", "ema_torch")}
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
    n = arms["plain"][1].state.fp.flat.numel()
    floors = {"ema_fused": (2, "one read and one write of the average"), "ema_torch": (3, "two reads and one write, plus a launch")}
    for k, (passes, what) in floors.items():
        d = [x - p for x, p in zip(ms[k], ms["plain"])]
        floor = passes * n * 4 / (COPY_TBS * 1e12) * 1e6
        print(f"{k} - plain: median {statistics.median(d) * 1e3:.1f} us/step (per round: {', '.join(f'{v * 1e3:.1f}' for v in d)}), "
              f"{statistics.median(d) / med['plain'] * 100:.2f} % of the plain step; floor {floor:.1f} us ({what}: "
              f"{passes * n * 4 / 1e6:.1f} MB at {COPY_TBS} TB/s)")
    print(f"ema_fused: {arms['ema_fused'][1].ema_updates()} EMA updates over {arms['ema_fused'][1].steps} steps")
    if a.trace:
        trace(arms["ema_fused"][1], a.decay)


if __name__ == "__main__":
    main()
