#!/usr/bin/env python3
"""What the eta > 0 sampler costs with its noise drawn up front against generated where it is consumed, in ONE process.

    python tools/noise_ab.py [--rounds 3] [--replays 5] [--warmup 1]

The workload is C2: 256 px, base 128, ch_mult (1,2,2), batch 8, bf16, 50 steps, linear schedule (every coefficient of the eta > 0
table is real there), eta = 0.03, key-seeded weights, one hipGraph replay per call.  Arms: `buffer`, today's route -- per call 49
`normal_()` fills of a (steps, B, C, H, W) buffer from the device's generator, then `ccn_sample_eta`; `seeded`, `sample(seeds=)` --
one `ccn_normal_fill` for the start noise, then `ccn_sample_seeded`, whose noisy steps end in a sampler-step launch that generates
its draws; `eta0`, the deterministic loop, for scale.  `buffer` and `eta0` start from a fixed x_T, `seeded` makes its own (that
launch is part of what it replaces: the host-drawn, uploaded start noise is outside all three arms).
Every arm is planned and captured first; then the arms alternate, `--rounds` times: `--warmup` untimed and `--replays` timed calls
per arm and round, the device synchronised on both sides of every call.  One JSON line: per arm the median ms per call over all
rounds, the spread, the per-round medians, images/s; per round seeded / buffer; the spread of the buffer arm's round medians, which
is what that ratio has to exceed to mean anything; the bytes of the noise buffer the seeded route does not allocate.
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

ARMS = ("buffer", "seeded", "eta0")


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
        raise SystemExit("noise_ab.py needs an MI355X; the HIP path has no CPU fallback")

    from clip_feature_codec.utils import synth
    from clip_feature_codec.models.unet import CLIPCondUNet
    from clip_feature_codec.diffusion.scheduler import NoiseScheduler
    from clip_feature_codec.diffusion.ddim import DDIMSampler

    dev = "cuda:0"
    S, Bn, base, ch_mult, steps, eta = 256, 8, 128, (1, 2, 2), 50, 0.03
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, ch_mult))
    net = CLIPCondUNet(512, base, ch_mult, dtype=args.dtype).to(dev).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    z = torch.from_numpy(synth.synth_z(Bn)).to(dev)
    x_T = torch.from_numpy(synth.start_noise(list(range(Bn)), S, seed_base=100)).to(dev)
    sch = NoiseScheduler(1000, "linear", dev)
    noisy, det = DDIMSampler(sch, eta=eta), DDIMSampler(sch, eta=0.0)
    seeded = DDIMSampler(sch, eta=eta)
    seeds = torch.arange(100, 100 + Bn, dtype=torch.int64, device=dev)
    shape = (Bn, 3, S, S)
    calls = {"buffer": lambda: noisy.sample(net, z, shape, steps=steps, x_T=x_T, slot=0),
             "seeded": lambda: seeded.sample(net, z, shape, steps=steps, seeds=seeds, slot=1),
             "eta0": lambda: det.sample(net, z, shape, steps=steps, x_T=x_T, slot=2)}

    def replay(a):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x = calls[a]()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, x

    line = {"workload": f"{S}px base={base} ch_mult={ch_mult} batch {Bn}, {args.dtype}, {steps} steps, linear, eta {eta}, one graph replay per call"}
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
    line["seeded_over_buffer_per_round"] = [round(s / b, 4) for s, b in zip(rm["seeded"], rm["buffer"])]
    line["buffer_round_spread"] = round(max(rm["buffer"]) / min(rm["buffer"]) - 1, 4)
    line["noise_buffer_mib_not_allocated"] = round(sum(t.numel() * 4 for t in noisy._noise.values()) / 2 ** 20, 1)
    line["seeded_noise_buffers"] = len(seeded._noise)
    line["seeded_scratch_mib"] = round(sum(ws.eps.numel() * 4 for ws in net.native()._ws.values() if ws.seeds is not None) / 2 ** 20, 1)
    line["seeded_replay_bit_equal"] = bool(torch.equal(replay("seeded")[1], outs["seeded"]))
    print(json.dumps(line))


if __name__ == "__main__":
    main()
