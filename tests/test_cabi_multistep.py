"""The four entry points of the multistep sampler are declared, exported and prototyped (no GPU needed)."""
import ctypes
import re
from pathlib import Path

import pytest

from clip_feature_codec import _native

HEADER = Path(__file__).resolve().parent.parent / "include" / "ccn_hip.h"
ARGS = {"ccn_sample_ms": 15, "ccn_sample_guided_ms": 18, "ccn_ms_step": 10, "ccn_cfg_ms_step": 13}


def test_multistep_entry_points_exist():
    if not _native.LIB_PATH.exists():
        pytest.fail(f"{_native.LIB_PATH} is not built: run `python __graft_entry__.py`")
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name, nargs in ARGS.items():
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _native.SIGNATURES, f"{name} has no ctypes prototype"
        assert len(_native.SIGNATURES[name][1]) == nargs
        decl = re.search(r"\b" + name + r"\s*\(([^)]*)\)", text)
        assert decl is not None, f"{name} is not declared in ccn_hip.h"
        assert len(decl.group(1).split(",")) == nargs, name

