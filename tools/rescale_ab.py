#!/usr/bin/env python3
"""What guidance rescale costs in the fused guided sampler loop, without and with dynamic thresholding, in ONE process.

    python tools/rescale_ab.py [--rounds 3] [--replays 5] [--warmup 1] [--phi 0.7] [--dynamic_threshold 0.995]

The workload is C2: 256 px, base 128, ch_mult (1,2,2), batch 8, bf16, 50 steps, cosine schedule, eta = 0, key-seeded weights,
classifier-free guidance at w = 3 (batch 2 x 8 inside), one hipGraph replay per call.  Arms: `guided`, the guided loop as it is (one
combine launch per step); `guided_rs`, the same with `guidance_rescale=phi` -- every step two small launches read both halves of the
output scratch once and leave one factor per image, which the combine launch multiplies in; `guided_thr` / `guided_thr_rs`, the same
pair with `dynamic_threshold=p` on both arms (the threshold launches then read the factors too).  Each arm has its own slot, so
its own workspace and graph.
Every arm is planned and captured first; then the arms alternate, `--rounds` times: `--warmup` untimed and `--replays` timed calls
per arm and round, the device synchronised on both sides of every call.  One JSON line: per arm the median ms per call over all
rounds, the spread, the per-round medians, images/s; per round guided_rs / guided and guided_thr_rs / guided_thr; the spread of the
un-rescaled arms' round medians, which is what those ratios have to exceed to mean anything; the bytes of rescale scratch.
Throughput only: with key-seeded weights the reconstructions mean nothing."""
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

ARMS = ("guided", "guided_rs", "guided_thr", "guided_thr_rs")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--phi", type=float, default=0.7)
    ap.add_argument("--dynamic_threshold", type=float, default=0.995)
    ap.add_argument("--dtype", choices=["fp32", "bf16", "f16x3"], default="bf16")
    args = ap.parse_args()
    if args.rounds < 3 or args.replays < 5 or args.warmup < 1:
        ap.error("at least 3 rounds, 5 timed replays and 1 warm-up per arm")
    if not torch.cuda.is_available():
        raise SystemExit("rescale_ab.py needs an MI355X; the HIP path has no CPU fallback")

    from clip_feature_codec.utils import synth
    from clip_feature_codec.models.unet import CLIPCondUNet
    from clip_feature_codec.diffusion.scheduler import NoiseScheduler
    from clip_feature_codec.diffusion.ddim import DDIMSampler

    dev = "cuda:0"
    S, Bn, base, ch_mult, steps, w = 256, 8, 128, (1, 2, 2), 50, 3.0
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, ch_mult))
    net = CLIPCondUNet(512, base, ch_mult, dtype=args.dtype).to(dev).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    z = torch.from_numpy(synth.synth_z(Bn)).to(dev)
    x_T = torch.from_numpy(synth.start_noise(list(range(Bn)), S, seed_base=100)).to(dev)
    sch = NoiseScheduler(1000, "cosine", dev)
    shape = (Bn, 3, S, S)
    thr = dict(dynamic_threshold=args.dynamic_threshold)
    samplers = {"guided": DDIMSampler(sch, guided=True), "guided_rs": DDIMSampler(sch, guided=True, guidance_rescale=args.phi),
                "guided_thr": DDIMSampler(sch, guided=True, **thr), "guided_thr_rs": DDIMSampler(sch, guided=True, guidance_rescale=args.phi, **thr)}
    calls = {a: (lambda a=a, k=k: samplers[a].sample(net, z, shape, steps=steps, x_T=x_T, slot=k, cfg_scale=w)) for k, a in enumerate(ARMS)}

    def replay(a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = calls[a]()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    line = {"workload": f"{S}px base={base} ch_mult={ch_mult} batch {Bn}, {args.dtype}, {steps} steps, cosine, eta 0, w {w}, phi {args.phi}, "
                        f"p {args.dynamic_threshold}, one graph replay per call"}
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
    for a in ("guided", "guided_thr"):
        line[f"{a}_rs_over_{a}_per_round"] = [round(t / b, 4) for t, b in zip(rm[a + "_rs"], rm[a])]
        line[f"{a}_round_spread"] = round(max(rm[a]) / min(rm[a]) - 1, 4)
        line[f"{a}_rs_added_us_per_step"] = round((line["arms"][a + "_rs"]["median_ms"] - line["arms"][a]["median_ms"]) / steps * 1e3, 2)
        line[f"{a}_rs_changes_the_result"] = not bool(torch.equal(outs[a], outs[a + "_rs"]))
        line[f"{a}_rs_replay_bit_equal"] = bool(torch.equal(replay(a + "_rs")[1], outs[a + "_rs"]))
    line["rescale_scratch_kib"] = round(sum(t.numel() for ws in net.native()._ws.values() for t in ws.rs.values()) / 2 ** 10, 2)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
