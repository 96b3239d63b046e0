#!/usr/bin/env python3
"""What the v-parameterisation's epilogue costs per step on the bench workload, eps and v arms alternating in ONE process.

    python tools/pred_ab.py [--rounds 3] [--replays 5] [--warmup 1]

The workload is bench.py's (C2: 256 px, base 128, ch_mult (1,2,2), batch 8, bf16, key-seeded weights, 50-step DDIM, one hipGraph
replay per call).  Arms: `eps`, the loop as it always was; `v`, the same loop after `ccn_set_prediction(CCN_PRED_V)` -- the same
launches, the head kernel's epilogue taking the v form (two more multiplies per output element, no division).  Both arms are planned
and captured first, in slots of their own; then they alternate, `--rounds` times: `--warmup` untimed and `--replays` timed replays
per arm and round, the device synchronised on both sides of every replay.  One JSON line: per arm the median ms per replay and per
sample, the per-round medians; per round v / eps; and the eps arm's own round-to-round spread, which is what that ratio has to
exceed to mean anything ("no measurable per-step cost" may be claimed only if the v arm lies inside it).
Throughput only: with key-seeded weights the reconstructions mean nothing, and no quality figure is computed."""
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

ARMS = ("eps", "v")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--dtype", choices=["fp32", "bf16", "f16x3"], default="bf16")
    args = ap.parse_args()
    if args.rounds < 3 or args.replays < 5 or args.warmup < 1:
        ap.error("at least 3 rounds, 5 timed replays and 1 warm-up per arm")
    if not torch.cuda.is_available():
        raise SystemExit("pred_ab.py needs an MI355X; the HIP path has no CPU fallback")

    from clip_feature_codec.utils import synth
    from clip_feature_codec.models.unet import CLIPCondUNet
    from clip_feature_codec.diffusion.scheduler import NoiseScheduler
    from clip_feature_codec.diffusion.ddim import DDIMSampler

    dev = "cuda:0"
    S, Bn, base, ch_mult = 256, 8, 128, (1, 2, 2)
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, ch_mult))
    net = CLIPCondUNet(512, base, ch_mult, dtype=args.dtype).to(dev).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    z = torch.from_numpy(synth.synth_z(Bn)).to(dev)
    x_T = torch.from_numpy(synth.start_noise(list(range(Bn)), S, seed_base=100)).to(dev)
    sch = NoiseScheduler(1000, "cosine", dev)
    samplers = {"eps": DDIMSampler(sch, eta=0.0), "v": DDIMSampler(sch, eta=0.0, prediction="v")}
    shape = (Bn, 3, S, S)
    slots = {"eps": 0, "v": 1}                                     # a workspace and a captured graph per arm

    def replay(a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = samplers[a].sample(net, z, shape, steps=args.steps, x_T=x_T, slot=slots[a])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    line = {"workload": f"{S}px base={base} ch_mult={ch_mult} batch {Bn}, {args.dtype}, {args.steps}-step DDIM, one graph replay per call"}
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
                           "round_medians_ms": [round(v, 3) for v in rm], "ms_per_sample": round(statistics.median(flat) / Bn, 3),
                           "round_ms_per_sample": [round(v / Bn, 3) for v in rm]}
    rm = {a: line["arms"][a]["round_medians_ms"] for a in ARMS}
    line["v_over_eps_per_round"] = [round(v / e, 4) for v, e in zip(rm["v"], rm["eps"])]
    line["v_over_eps_median"] = round(line["arms"]["v"]["median_ms"] / line["arms"]["eps"]["median_ms"], 4)
    line["eps_round_spread"] = round(max(rm["eps"]) / min(rm["eps"]) - 1, 4)
    line["v_inside_eps_spread"] = bool(min(rm["eps"]) <= line["arms"]["v"]["median_ms"] <= max(rm["eps"]))
    # the two arms compute different things from the same network output, each the same on every replay
    line["v_vs_eps_max_abs"] = float((outs["v"] - outs["eps"]).abs().max())
    line["replay_bit_equal"] = {a: bool(torch.equal(replay(a)[1], outs[a])) for a in ARMS}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
