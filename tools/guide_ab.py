#!/usr/bin/env python3
"""What the low-resolution guide costs in the fused sampler loop, unguided and under classifier-free guidance, in ONE process.

    python tools/guide_ab.py [--rounds 3] [--replays 5] [--warmup 1] [--factor 32] [--strength 1.0] [--t_min 0]

The workload is C2: 256 px, base 128, ch_mult (1,2,2), batch 8, bf16, 50 steps, cosine schedule, eta = 0, key-seeded weights, one
hipGraph replay per call.  Arms: `plain`, the unguided loop as it is (the update is the head kernel's epilogue); `plain_lr`, the same
with `guide=` -- every step with `ts[i] >= t_min` the head writes the raw output instead, one launch forms the correction of every
N x N block and one sampler-step launch applies it; `cfg` / `cfg_lr`, the same pair under classifier-free guidance at w = 3 (batch
2 x 8 inside), where the split route is taken anyway and the guide adds the one delta launch.  The guide is the block mean of a
smooth synthetic image.  Each arm has its own slot, so its own workspace and graph.
Every arm is planned and captured first; then the arms alternate, `--rounds` times: `--warmup` untimed and `--replays` timed calls
per arm and round, the device synchronised on both sides of every call.  One JSON line: per arm the median ms per call over all
rounds, the spread, the per-round medians, images/s; per round plain_lr / plain and cfg_lr / cfg; the spread of the un-guided arms'
round medians, which is what those ratios have to exceed to mean anything; the added microseconds per step; the bytes of guide
scratch.  Throughput only: with key-seeded weights the reconstructions mean nothing."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
for p in (str(REPO), str(REPO / "clip-neural-image-conpression_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

ARMS = ("plain", "plain_lr", "cfg", "cfg_lr")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--factor", type=int, default=32)
    ap.add_argument("--strength", type=float, default=1.0)
    ap.add_argument("--t_min", type=int, default=0)
    ap.add_argument("--dtype", choices=["fp32", "bf16", "f16x3"], default="bf16")
    args = ap.parse_args()
    if args.rounds < 3 or args.replays < 5 or args.warmup < 1:
        ap.error("at least 3 rounds, 5 timed replays and 1 warm-up per arm")
    if not torch.cuda.is_available():
        raise SystemExit("guide_ab.py needs an MI355X; the HIP path has no CPU fallback")

    from clip_feature_codec import _native
    from clip_feature_codec.utils import synth
    from clip_feature_codec.models.unet import CLIPCondUNet
    from clip_feature_codec.diffusion.scheduler import NoiseScheduler
    from clip_feature_codec.diffusion.ddim import DDIMSampler

    dev = "cuda:0"
    S, Bn, base, ch_mult, steps, w, N = 256, 8, 128, (1, 2, 2), 50, 3.0, args.factor
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, ch_mult))
    net = CLIPCondUNet(512, base, ch_mult, dtype=args.dtype).to(dev).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    z = torch.from_numpy(synth.synth_z(Bn)).to(dev)
    x_T = torch.from_numpy(synth.start_noise(list(range(Bn)), S, seed_base=100)).to(dev)
    sch = NoiseScheduler(1000, "cosine", dev)
    shape = (Bn, 3, S, S)
    i, j = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    img = np.stack([np.stack([0.7 * np.cos(0.02 * i + c + b) * np.sin(0.03 * j - c) for c in range(3)]) for b in range(Bn)]).astype(np.float32)
    guide = _native.block_mean(torch.from_numpy(img).to(dev), N)
    lr = dict(guide=guide, guide_strength=args.strength, guide_t_min=args.t_min)
    samplers = {"plain": DDIMSampler(sch), "cfg": DDIMSampler(sch, guided=True)}
    kw = {"plain": dict(cfg_scale=1.0), "plain_lr": dict(cfg_scale=1.0, **lr), "cfg": dict(cfg_scale=w), "cfg_lr": dict(cfg_scale=w, **lr)}
    calls = {a: (lambda a=a, k=k: samplers[a.split("_")[0]].sample(net, z, shape, steps=steps, x_T=x_T, slot=k, **kw[a])) for k, a in enumerate(ARMS)}

    def replay(a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = calls[a]()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    line = {"workload": f"{S}px base={base} ch_mult={ch_mult} batch {Bn}, {args.dtype}, {steps} steps, cosine, eta 0, w {w} on the cfg arms, N {N}, "
                        f"strength {args.strength}, t_min {args.t_min}, one graph replay per call"}
    outs = {a: replay(a)[1] for a in ARMS}                          # plan + graph capture, untimed
    for a in ARMS:
        assert torch.isfinite(outs[a]).all(), a
    net.native().poll_errors()
    ms = {a: [] for a in ARMS}
    for _ in range(args.rounds):
        for a in ARMS:
            for _ in range(args.warmup):
                replay(a)
            ms[a].append([replay(a)[0] for _ in range(args.replays)])

    line.update(rounds=args.rounds, replays_per_round=args.replays, warmup_per_round=args.warmup, arms={})
    for a in ARMS:
        flat = [v for r in ms[a] for v in r]
        rm = [statistics.median(r) for r in ms[a]]
        line["arms"][a] = {"median_ms": round(statistics.median(flat), 3), "min_ms": round(min(flat), 3), "max_ms": round(max(flat), 3),
                           "round_medians_ms": [round(v, 3) for v in rm], "images_per_sec": round(Bn / statistics.median(flat) * 1e3, 3)}
    rm = {a: line["arms"][a]["round_medians_ms"] for a in ARMS}
    guided_steps = int((np.asarray(sch.ddim_timesteps(steps)) >= args.t_min).sum())
    for a in ("plain", "cfg"):
        line[f"{a}_lr_over_{a}_per_round"] = [round(t / b, 4) for t, b in zip(rm[a + "_lr"], rm[a])]
        line[f"{a}_round_spread"] = round(max(rm[a]) / min(rm[a]) - 1, 4)
        line[f"{a}_lr_added_us_per_guided_step"] = round((line["arms"][a + "_lr"]["median_ms"] - line["arms"][a]["median_ms"]) / max(guided_steps, 1) * 1e3, 2)
        line[f"{a}_lr_changes_the_result"] = not bool(torch.equal(outs[a], outs[a + "_lr"]))
        line[f"{a}_lr_replay_bit_equal"] = bool(torch.equal(replay(a + "_lr")[1], outs[a + "_lr"]))
        line[f"{a}_lr_thumbnail_max_error"] = float((_native.block_mean(outs[a + "_lr"], N) - guide).abs().max())
    line["guided_steps"] = guided_steps
    line["guide_scratch_kib"] = round(sum(s.numel() for ws in net.native()._ws.values() for _, s in ws.lr.values()) / 2 ** 10, 2)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
