#!/usr/bin/env python3
"""Golden fixture of the training step's workspace sizes and launch decisions, made by RUNNING THE PARENT COMMIT'S LIBRARY on an MI355X.

The step plan (csrc/ccn_train.hip, StepPlan) replaced three walks over the layer list with a bump allocator; what those walks gave --
``ccn_train_workspace_bytes`` and the report of ``ccn_internal_train_routes`` -- is recorded here from the last library that had them.
Build ``libccn_hip.so`` of that commit in a worktree, then on the GPU:

    python tests/golden/make_train_plan_golden.py <that libccn_hip.so> --commit <its hash>

The script refuses a library that exports ``ccn_internal_train_layout``: that one has the plan already.  Cases and the recording run are
tests/train_plan_cases.py.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("library", help="libccn_hip.so of the commit to record")
    ap.add_argument("--commit", required=True, help="hash of that commit")
    ap.add_argument("--out", default=str(HERE / "train_plan_parent.json"))
    args = ap.parse_args()
    path = Path(args.library).resolve()
    import torch                                               # before the library: both must end up on torch's HIP runtime
    if hasattr(ctypes.CDLL(str(path)), "ccn_internal_train_layout"):
        sys.exit(f"{path} exports ccn_internal_train_layout: it has the step plan; record from the commit before it")
    os.environ["CCN_HIP_LIB"] = str(path)                      # read by clip_feature_codec._native on import
    sys.path[:0] = [str(ROOT), str(ROOT / "clip-neural-image-conpression_amd"), str(ROOT / "tests")]
    import train_plan_cases as tpc
    from clip_feature_codec import _native
    assert Path(_native.LIB_PATH).resolve() == path, _native.LIB_PATH
    print("library:", _native.LIB_PATH, flush=True)
    cases = {}
    for cid in tpc.CASES:
        cases[cid] = tpc.record(cid)
        print(cid, cases[cid]["bytes"], len(cases[cid].get("routes", "").splitlines()), "lines", flush=True)
    have = tpc.bf16_coverage(v for cid, c in cases.items() if cid.startswith("bf16") for v in (c.get("routes", ""), c.get("routes_bucketed", "")))
    for k, v in have.items():
        print("coverage:", k, v)
    assert all(have.values()), "add the smallest shape that reaches the missing form"
    Path(args.out).write_text(json.dumps({"commit": args.commit, "device": torch.cuda.get_device_name(0), "cases": cases}, indent=1) + "\n")
    print("wrote", args.out, Path(args.out).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
