#!/usr/bin/env python3
"""Golden fixture of the inference plan's sizes, launch decisions and output bits, made by RUNNING THE PARENT COMMIT'S LIBRARY on an MI355X.

The shape plan (csrc/ccn_api.hip, ShapePlan) replaced a list of closures built per workspace address, and a second "measuring" walk for
``ccn_workspace_bytes`` / ``ccn_algorithmic_work``; what that code gave is recorded here from the last library that had it.  Build
``libccn_hip.so`` of that commit in a worktree, then on the GPU:

    python tests/golden/make_infer_plan_golden.py <that libccn_hip.so> --commit <its hash>

The script refuses a library that exports ``ccn_internal_plan_layout``: that one has the plan already.  Cases and the recording run are
tests/infer_plan_cases.py.  The timestep / coefficient / sigma tables are built here with the Python sampler's own table functions and
stored in the fixture, so that the test does not depend on the host's libm.  Every case is recorded twice and must give the same record.
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
    ap.add_argument("--out", default=str(HERE / "infer_plan_parent.json"))
    args = ap.parse_args()
    path = Path(args.library).resolve()
    import torch                                               # before the library: both must end up on torch's HIP runtime
    if hasattr(ctypes.CDLL(str(path)), "ccn_internal_plan_layout"):
        sys.exit(f"{path} exports ccn_internal_plan_layout: it has the shape plan; record from the commit before it")
    os.environ["CCN_HIP_LIB"] = str(path)                      # read by clip_feature_codec._native on import
    sys.path[:0] = [str(ROOT), str(ROOT / "clip-neural-image-conpression_amd"), str(ROOT / "tests")]
    import infer_plan_cases as ipc
    from clip_feature_codec import _native
    from clip_feature_codec.diffusion.scheduler import NoiseScheduler
    assert Path(_native.LIB_PATH).resolve() == path, _native.LIB_PATH
    print("library:", _native.LIB_PATH, flush=True)
    sch = NoiseScheduler(1000, "cosine", "cpu")
    cases = {}
    for cid, case in ipc.CASES.items():
        steps = case["shape"][3]
        tables = None
        if case["run"]:
            tables = {"eta0": ipc.tables_bits(sch.ddim_timesteps(steps), sch.ddim_coefficients(steps, 0.0))}
            if case.get("eta"):
                tables["eta"] = ipc.tables_bits(sch.ddim_timesteps(steps), sch.ddim_coefficients(steps, ipc.ETA))
        first = ipc.record(cid, tables, launch_for_routes=True)
        again = ipc.record(cid, tables, launch_for_routes=True)
        assert first == again, (cid, first, again)
        if tables:
            first["tables"] = tables
        cases[cid] = first
        print(cid, first["bytes"], len(first["routes"].splitlines()), "route lines", sorted(first.get("sha256", {})), flush=True)
    have = ipc.coverage(cases)
    for k, v in have.items():
        print("coverage:", k, v)
    assert all(have.values()), "add the smallest shape that reaches the missing form"
    Path(args.out).write_text(json.dumps({"commit": args.commit, "device": torch.cuda.get_device_name(0), "cases": cases}, indent=1) + "\n")
    print("wrote", args.out, Path(args.out).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
