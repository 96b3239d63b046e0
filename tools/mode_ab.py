#!/usr/bin/env python3
"""A/B/C of the arithmetic modes on the bench workload, in ONE process: fp32, f16x3, bf16.

    python tools/mode_ab.py [--rounds 3] [--replays 5] [--warmup 1] [--profile]

The workload is bench.py's (batch 8, 256 px, base 128, ch_mult (1,2,2), 50 DDIM steps, key-seeded weights, one hipGraph replay per
step).  Every arm is planned and captured first; then the arms alternate, `--rounds` times: `--warmup` untimed and `--replays` timed
replays per arm and round, the device synchronised on both sides of every replay.  One JSON line: per arm the median ms per replay
and images/s over all rounds, the spread (min, max), the per-round medians, and each round's f16x3 / fp32 and bf16 / fp32 ratios.
`--profile` adds the per-family table of ccn_profile_read for the f16x3 arm (one launch-by-launch pass with HIP events)."""
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

import torch

ARMS = ("fp32", "f16x3", "bf16")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--arms", type=str, default=",".join(ARMS))
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if args.rounds < 3 or args.replays < 5 or args.warmup < 1:
        ap.error("at least 3 rounds, 5 timed replays and 1 warm-up per arm")
    arms = [a for a in args.arms.split(",") if a]
    if not torch.cuda.is_available():
        raise SystemExit("mode_ab.py needs an MI355X; the HIP path has no CPU fallback")

    from clip_feature_codec.utils import synth
    from clip_feature_codec.models.unet import CLIPCondUNet
    from clip_feature_codec.diffusion.scheduler import NoiseScheduler
    from clip_feature_codec.diffusion.ddim import DDIMSampler

    dev = "cuda:0"
    B, S, T, base, ch_mult = 8, 256, 50, 128, (1, 2, 2)
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, ch_mult))
    z = torch.from_numpy(synth.synth_z(B)).to(dev)
    x_T = torch.from_numpy(synth.start_noise(list(range(B)), S, seed_base=100)).to(dev)
    sampler = DDIMSampler(NoiseScheduler(1000, "cosine", dev), eta=0.0)
    nets = {}
    for a in arms:
        net = CLIPCondUNet(512, base, ch_mult, dtype=a).to(dev).eval()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        nets[a] = net

    def replay(a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = sampler.sample(nets[a], z, (B, 3, S, S), steps=T, x_T=x_T)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    outs = {a: replay(a)[1] for a in arms}                          # plan + graph capture, untimed
    for a in arms:
        assert torch.isfinite(outs[a]).all(), a
        nets[a].native().poll_errors()
    ms = {a: [] for a in arms}
    for _ in range(args.rounds):
        for a in arms:
            for _ in range(args.warmup):
                replay(a)
            ms[a].append([replay(a)[0] for _ in range(args.replays)])

    line = {"workload": f"{S}px base={base} ch_mult={ch_mult} {T}-step DDIM, batch={B}, one graph replay per step",
            "rounds": args.rounds, "replays_per_round": args.replays, "warmup_per_round": args.warmup, "arms": {}}
    for a in arms:
        flat = [v for r in ms[a] for v in r]
        med = statistics.median(flat)
        line["arms"][a] = {"median_ms": round(med, 3), "images_per_sec": round(B / med * 1e3, 3), "min_ms": round(min(flat), 3),
                           "max_ms": round(max(flat), 3), "round_medians_ms": [round(statistics.median(r), 3) for r in ms[a]]}
    if "fp32" in arms:
        ref = line["arms"]["fp32"]["round_medians_ms"]
        for a in arms:
            if a != "fp32":
                line[f"{a}_over_fp32_per_round"] = [round(f / m, 4) for f, m in zip(ref, line["arms"][a]["round_medians_ms"])]
        if "f16x3" in arms:
            d = (outs["f16x3"] - outs["fp32"]).abs()
            line["f16x3_vs_fp32_all_rows"] = {"max_abs": float(d.max()), "mean_abs": float(d.mean())}
    if args.profile and "f16x3" in arms:
        nat = nets["f16x3"].native()
        nat.profile(True)
        sampler.sample(nets["f16x3"], z, (B, 3, S, S), steps=T, x_T=x_T)
        fams = nat.profile_read()
        nat.profile(False)
        line["f16x3_families"] = {f["name"]: {"ms": round(f["ms"], 3), "calls": f["calls"],
                                              "tflops": round(f["flops"] / (f["ms"] * 1e-3) / 1e12, 2) if f["ms"] > 0 else None,
                                              "gbs_algorithmic": round(f["bytes"] / (f["ms"] * 1e-3) / 1e9, 1) if f["ms"] > 0 else None}
                                  for f in fams}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
