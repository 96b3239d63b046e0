#!/usr/bin/env python3
"""Golden fixture of the optimiser tail's bits, made by RUNNING AN EARLIER COMMIT'S LIBRARY on an MI355X.

The AdamW entry points (plain, guarded, with the fused EMA) share one kernel, so they cannot check one another; what they computed
before they were merged is recorded here instead.  Build ``libccn_hip.so`` of the commit to pin, then on the GPU:

    CCN_HIP_LIB=<that libccn_hip.so> python tests/golden/make_optimizer_golden.py --commit <its hash>

The script is tests/optimizer_bits.py (inputs from numpy's generator on the host, three steps per case, every mode and case listed
there).  Stored: the commit hash as given and the device name; the case ids; a SHA-256 of p, g, m, v, ema, the guard block and the EMA
state block after every step of every case; for cases of up to 1033 elements the final arrays and blocks as well, so that a mismatch
can be located.  The file stays under 256 KB.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "clip-neural-image-conpression_amd"), str(ROOT / "tests")]

import optimizer_bits as ob  # noqa: E402
from clip_feature_codec import _native  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="hash of the commit whose library CCN_HIP_LIB names")
    ap.add_argument("--out", default=str(HERE / "optimizer_steps.npz"))
    args = ap.parse_args()
    print("library:", _native.LIB_PATH, flush=True)
    sha = np.zeros((len(ob.CASES), ob.STEPS, len(ob.BUFFERS), 32), dtype=np.uint8)
    blocks = np.zeros((len(ob.CASES), _native.GUARD_WORDS + _native.EMA_WORDS), dtype=np.int32)
    arrays = {}
    for i, (case, cid) in enumerate(zip(ob.CASES, ob.IDS)):
        sha[i], finals, blocks[i] = ob.run(*case)
        if finals is not None:
            arrays["final/" + cid] = finals
        print(cid, sha[i, -1, 0, :4].tobytes().hex(), flush=True)
    np.savez_compressed(args.out, commit=np.array(args.commit), device=np.array(torch.cuda.get_device_name(0)), ids=np.array(ob.IDS),
                        buffers=np.array(ob.BUFFERS), sha256=sha, blocks=blocks, **arrays)
    size = Path(args.out).stat().st_size
    print("wrote", args.out, size, "bytes")
    assert size < 256 * 1024, size


if __name__ == "__main__":
    main()
