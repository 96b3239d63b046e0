#!/usr/bin/env python3
"""What classifier-free guidance costs on the bench workload, in ONE process: unguided batch 8, unguided batch 16, guided batch 8.

    python tools/cfg_ab.py [--rounds 3] [--replays 5] [--warmup 1] [--w 3.0] [--profile]

The workload is bench.py's (256 px, base 128, ch_mult (1,2,2), 50 DDIM steps, bf16, key-seeded weights, one hipGraph replay per
call).  A guided call of batch 8 evaluates the UNet on 16 rows per step, so its yardstick is the UNGUIDED BATCH-16 call of the same
process and round: the same two forwards per image, without the eps round trip and the combine launch.  Every arm is planned and
captured first; then the arms alternate, `--rounds` times: `--warmup` untimed and `--replays` timed replays per arm and round, the
device synchronised on both sides of every replay.  One JSON line: per arm the median ms per replay over all rounds, the spread
(min, max) and the per-round medians; per round guided-8 / unguided-16 and guided-8 / unguided-8; the spread of the unguided-16
round medians, which is what a ratio has to exceed to mean anything.  `--profile` adds the per-family table of ccn_profile_read for
one guided pass (launch by launch with HIP events: run it on its own, not next to the timed rounds)."""
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

ARMS = ("unguided_8", "unguided_16", "guided_8")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--w", type=float, default=3.0)
    ap.add_argument("--dtype", choices=["fp32", "bf16", "f16x3"], default="bf16")
    ap.add_argument("--profile", action="store_true", help="only the per-family profile of one guided pass, no timed rounds")
    args = ap.parse_args()
    if args.rounds < 3 or args.replays < 5 or args.warmup < 1:
        ap.error("at least 3 rounds, 5 timed replays and 1 warm-up per arm")
    if args.w == 1.0:
        ap.error("--w 1.0 is the unguided route")
    if not torch.cuda.is_available():
        raise SystemExit("cfg_ab.py needs an MI355X; the HIP path has no CPU fallback")

    from clip_feature_codec.utils import synth
    from clip_feature_codec.models.unet import CLIPCondUNet
    from clip_feature_codec.diffusion.scheduler import NoiseScheduler
    from clip_feature_codec.diffusion.ddim import DDIMSampler

    dev = "cuda:0"
    S, T, base, ch_mult = 256, 50, 128, (1, 2, 2)
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, ch_mult))
    net = CLIPCondUNet(512, base, ch_mult, dtype=args.dtype).to(dev).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    z = torch.from_numpy(synth.synth_z(16)).to(dev)
    x_T = torch.from_numpy(synth.start_noise(list(range(16)), S, seed_base=100)).to(dev)
    sch = NoiseScheduler(1000, "cosine", dev)
    unguided, guided = DDIMSampler(sch, eta=0.0), DDIMSampler(sch, eta=0.0, guided=True)
    # slots keep the arms' workspaces and captured graphs apart (unguided_16 and guided_8 would otherwise share a plan's workspace)
    calls = {"unguided_8": lambda: unguided.sample(net, z[:8], (8, 3, S, S), steps=T, x_T=x_T[:8], slot=0),
             "unguided_16": lambda: unguided.sample(net, z, (16, 3, S, S), steps=T, x_T=x_T, slot=1),
             "guided_8": lambda: guided.sample(net, z[:8], (8, 3, S, S), steps=T, cfg_scale=args.w, x_T=x_T[:8], slot=2)}

    def replay(a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = calls[a]()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    line = {"workload": f"{S}px base={base} ch_mult={ch_mult} {T}-step DDIM, {args.dtype}, one graph replay per call", "w": args.w}
    if args.profile:
        replay("guided_8")
        nat = net.native()
        nat.profile(True)
        calls["guided_8"]()
        fams = nat.profile_read()
        nat.profile(False)
        line["guided_8_families"] = {f["name"]: {"ms": round(f["ms"], 3), "calls": f["calls"]} for f in fams}
        print(json.dumps(line))
        return

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
        line["arms"][a] = {"median_ms": round(statistics.median(flat), 3), "min_ms": round(min(flat), 3), "max_ms": round(max(flat), 3),
                           "round_medians_ms": [round(statistics.median(r), 3) for r in ms[a]]}
    rm = {a: line["arms"][a]["round_medians_ms"] for a in ARMS}
    line["guided_8_over_unguided_16_per_round"] = [round(g / u, 4) for g, u in zip(rm["guided_8"], rm["unguided_16"])]
    line["guided_8_over_unguided_8_per_round"] = [round(g / u, 4) for g, u in zip(rm["guided_8"], rm["unguided_8"])]
    line["unguided_16_round_spread"] = round(max(rm["unguided_16"]) / min(rm["unguided_16"]) - 1, 4)
    # what each arm holds: its workspace (key: plan batch, H, W, steps, slot) and, guided, the eps of both halves
    line["workspace_mib"] = {"x".join(map(str, k)): round(ws.nbytes / 2 ** 20, 1) for k, ws in net.native()._ws.items()}
    line["eps_scratch_mib"] = round(sum(ws.eps.numel() * 4 for ws in net.native()._ws.values() if ws.eps is not None) / 2 ** 20, 1)
    line["guided_8_images_per_sec"] =round(8 / line["arms"]["guided_8"]["median_ms"] * 1e3, 3)
    # what the guided result is: not the unguided one (the scale is read), and the same on every replay
    line["guided_vs_unguided_8_max_abs"] = float((outs["guided_8"] - outs["unguided_8"]).abs().max())
    line["guided_replay_bit_equal"] = bool(torch.equal(replay("guided_8")[1], outs["guided_8"]))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
