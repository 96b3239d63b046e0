#!/usr/bin/env python3
"""What the multistep sampler (DPM-Solver++ 2M) costs per step, and what fewer steps buy, on the bench workload, in ONE process.

    python tools/sampler_ab.py [--rounds 3] [--replays 5] [--warmup 1]

The workload is bench.py's (256 px, base 128, ch_mult (1,2,2), batch 8, bf16, key-seeded weights, one hipGraph replay per call).
Arms: `ddim_50`, the 50-step DDIM loop; `ms_50`, the 2M loop on the same 50 timesteps (`spacing="linspace"`: equal UNet evaluations,
so the difference is the history's read and write in the head's epilogue); `ms_20`, the 2M loop as shipped at 20 requested steps
(`spacing="logsnr"`, whose table merges into fewer entries: the count is reported as `evals`); `ms_20_linspace`, 20 evaluations.
Every arm is planned and captured first; then the arms alternate, `--rounds` times: `--warmup` untimed and `--replays` timed replays
per arm and round, the device synchronised on both sides of every replay.  One JSON line: per arm the UNet evaluations, the median
ms per replay over all rounds, the spread, the per-round medians and the per-round ms per evaluation; per round ms_50 / ddim_50;
the spread of the ddim_50 round medians, which is what that ratio has to exceed to mean anything; images/s per arm.
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

ARMS = ("ddim_50", "ms_50", "ms_20", "ms_20_linspace")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dtype", choices=["fp32", "bf16", "f16x3"], default="bf16")
    args = ap.parse_args()
    if args.rounds < 3 or args.replays < 5 or args.warmup < 1:
        ap.error("at least 3 rounds, 5 timed replays and 1 warm-up per arm")
    if not torch.cuda.is_available():
        raise SystemExit("sampler_ab.py needs an MI355X; the HIP path has no CPU fallback")

    from clip_feature_codec.utils import synth
    from clip_feature_codec.models.unet import CLIPCondUNet
    from clip_feature_codec.diffusion.scheduler import NoiseScheduler
    from clip_feature_codec.diffusion.ddim import DDIMSampler
    from clip_feature_codec.diffusion.dpm_solver import DPMSolverSampler

    dev = "cuda:0"
    S, Bn, base, ch_mult = 256, 8, 128, (1, 2, 2)
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, ch_mult))
    net = CLIPCondUNet(512, base, ch_mult, dtype=args.dtype).to(dev).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    z = torch.from_numpy(synth.synth_z(Bn)).to(dev)
    x_T = torch.from_numpy(synth.start_noise(list(range(Bn)), S, seed_base=100)).to(dev)
    sch = NoiseScheduler(1000, "cosine", dev)
    ddim, ms_lin, ms_log = DDIMSampler(sch, eta=0.0), DPMSolverSampler(sch, 2, "linspace"), DPMSolverSampler(sch, 2, "logsnr")
    shape = (Bn, 3, S, S)
    # slots keep the arms' workspaces and captured graphs apart (ddim_50 and ms_50 would otherwise share a plan's workspace)
    calls = {"ddim_50": lambda: ddim.sample(net, z, shape, steps=50, x_T=x_T, slot=0),
             "ms_50": lambda: ms_lin.sample(net, z, shape, steps=50, x_T=x_T, slot=1),
             "ms_20": lambda: ms_log.sample(net, z, shape, steps=20, x_T=x_T, slot=2),
             "ms_20_linspace": lambda: ms_lin.sample(net, z, shape, steps=20, x_T=x_T, slot=3)}
    evals = {"ddim_50": 50, "ms_50": len(ms_lin.tables(50)[0]), "ms_20": len(ms_log.tables(20)[0]), "ms_20_linspace": len(ms_lin.tables(20)[0])}

    def replay(a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = calls[a]()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    line = {"workload": f"{S}px base={base} ch_mult={ch_mult} batch {Bn}, {args.dtype}, one graph replay per call"}
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
        line["arms"][a] = {"evals": evals[a], "median_ms": round(statistics.median(flat), 3), "min_ms": round(min(flat), 3),
                           "max_ms": round(max(flat), 3), "round_medians_ms": [round(v, 3) for v in rm],
                           "round_ms_per_eval": [round(v / evals[a], 4) for v in rm],
                           "images_per_sec": round(Bn / statistics.median(flat) * 1e3, 3)}
    rm = {a: line["arms"][a]["round_medians_ms"] for a in ARMS}
    line["ms_50_over_ddim_50_per_round"] = [round(m / d, 4) for m, d in zip(rm["ms_50"], rm["ddim_50"])]
    line["ddim_50_round_spread"] = round(max(rm["ddim_50"]) / min(rm["ddim_50"]) - 1, 4)
    line["ms_20_over_ddim_50_images_per_sec"] = round(line["arms"]["ms_20"]["images_per_sec"] / line["arms"]["ddim_50"]["images_per_sec"], 3)
    line["history_mib"] = round(sum(t.numel() * 4 for ws in net.native()._ws.values() for t in ws.hist.values()) / 2 ** 20, 1)
    # the 2M result is not the DDIM one on the same timesteps (the correction is applied), and the same on every replay
    line["ms_50_vs_ddim_50_max_abs"] = float((outs["ms_50"] - outs["ddim_50"]).abs().max())
    line["ms_50_replay_bit_equal"] = bool(torch.equal(replay("ms_50")[1], outs["ms_50"]))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
