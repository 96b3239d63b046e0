#!/usr/bin/env python3
"""The emulation table of docs/EXPERIMENTS.md R6: the CPU oracle with its convolutions replaced by split-operand arithmetic
(tests/split_emulation.py), against the committed fixtures.  No GPU.

    python tools/split_emulation_table.py            # C1 10 steps and C2 one forward, every row (about a minute)
    python tools/split_emulation_table.py --c2-steps # + C2 50 steps for the f16x3 row (several minutes); --all-rows: for every row
"""
import argparse
import sys
import time
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / "clip-neural-image-conpression_amd"), str(REPO / "tests")]

import numpy as np
import torch

import split_emulation
from clip_feature_codec.utils import synth
from oracle import ref_unet, ref_diffusion

ROWS = [   # name, SplitFunctional arguments (None: the oracle itself)
    ("plain fp32 (the oracle itself)", None),
    ("bf16 hi+lo, 3 products, every conv", dict(T=torch.bfloat16, every_conv=True)),
    ("bf16 hi+lo, 3 products, scope", dict(T=torch.bfloat16, min_cout=0)),
    ("fp16 hi+lo, 3 products, weight scale, scope", dict(min_cout=0)),
    ("the same, only N tiles >= 64 (what the GPU runs)", dict()),
    ("fp16 hi+lo, scope, subnormal operands flushed", dict(min_cout=0, flush=True)),
]


def run(kw, fn):
    if kw is None:
        return fn()
    with split_emulation.emulated(**kw):
        return fn()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--c2-steps", action="store_true")
    ap.add_argument("--all-rows", action="store_true")
    a = ap.parse_args()
    g1 = np.load(REPO / "tests/golden/c1_sample.npz"); g2 = np.load(REPO / "tests/golden/c2_sample.npz")
    sd1 = ref_unet.as_torch_sd(synth.synth_state_dict(synth.unet_param_spec(512, 32, (1, 2))))
    sd2 = ref_unet.as_torch_sd(synth.synth_state_dict(synth.unet_param_spec(512, 128, (1, 2, 2))))
    xT = torch.from_numpy(synth.start_noise([0], 256, seed_base=100)); z = torch.from_numpy(synth.synth_z(1))
    print("| emulated arithmetic | C2 one forward, eps at t=999, max-abs | C2 50 steps, max-abs vs reference | C1 10 steps |")
    print("|---|---|---|---|")
    for name, kw in ROWS:
        t0 = time.time()
        c1 = run(kw, lambda: ref_diffusion.ddim_sample(ref_unet.make_model(sd1), torch.from_numpy(g1["z"]), torch.from_numpy(g1["x_T"]), steps=10))
        e_c1 = float(np.abs(c1.numpy() - g1["x_final"]).max())
        with torch.no_grad():
            eps = run(kw, lambda: ref_unet.unet_forward(sd2, xT, z, torch.tensor([999])))
        e_fwd = float(np.abs(eps[0, :, ::4, ::4].numpy() - g2["eps_t999.sub"]).max())
        e_50 = "-"
        if a.c2_steps and (a.all_rows or (kw is not None and kw == dict(min_cout=0)) or kw == dict()):
            x = run(kw, lambda: ref_diffusion.ddim_sample(ref_unet.make_model(sd2), z, xT, steps=50))
            e_50 = f"{float(np.abs(x[0, :, ::4, ::4].numpy() - g2['x_final.sub']).max()):.2e}"
        print(f"| {name} | {e_fwd:.1e} | {e_50} | {e_c1:.1e} |   <!-- {time.time() - t0:.0f} s -->", flush=True)


if __name__ == "__main__":
    main()
