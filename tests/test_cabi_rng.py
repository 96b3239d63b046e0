"""The four entry points of the seeded device noise are declared, exported and prototyped, and validate before they launch
(no GPU needed)."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from clip_feature_codec import _native

HEADER = Path(__file__).resolve().parent.parent / "include" / "ccn_hip.h"
ARGS = {"ccn_normal_fill": 6, "ccn_sampler_step_seeded": 14, "ccn_sample_seeded": 17, "ccn_sample_guided_seeded": 19}


def test_rng_entry_points_exist():
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
    # the seeded entries take what their unseeded counterparts take, the noise pointer replaced
    assert len(_native.SIGNATURES["ccn_sampler_step"][1]) + 2 == ARGS["ccn_sampler_step_seeded"]
    assert len(_native.SIGNATURES["ccn_sample_eta"][1]) + 1 == ARGS["ccn_sample_seeded"]              # + the output scratch
    assert len(_native.SIGNATURES["ccn_sample_guided"][1]) == ARGS["ccn_sample_guided_seeded"]


def test_bad_arguments_are_einval_without_a_device():
    lib = _native.load_library()
    out, seeds = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)              # never dereferenced: every call below fails its checks
    assert lib.ccn_normal_fill(None, seeds, 1, 4, 0, None) == 1
    assert lib.ccn_normal_fill(out, None, 1, 4, 0, None) == 1
    assert lib.ccn_normal_fill(out, seeds, 0, 4, 0, None) == 1
    assert lib.ccn_normal_fill(out, seeds, 1, 0, 0, None) == 1
    assert lib.ccn_normal_fill(out, ctypes.c_void_p(0x2004), 1, 4, 0, None) == 1
    assert lib.ccn_normal_fill(out, seeds, 1, 1 << 34, 0, None) == 1            # C*H*W >= 2^34
    assert b"2^34" in lib.ccn_last_error()
    coef = (ctypes.c_float * 5)(1, 1, 1, 0, 0)
    x = ctypes.c_void_p(0x3000)
    assert lib.ccn_sampler_step_seeded(x, None, None, x, None, None, 1, 4, 0, 0.0, coef, 0.1, 8, None) == 1       # no seeds
    assert lib.ccn_sampler_step_seeded(x, None, None, x, None, seeds, 1, 3, 0, 0.0, coef, 0.1, 8, None) == 1      # 8 % 3
    assert lib.ccn_sampler_step_seeded(x, None, None, x, None, seeds, 1, 0, 0, 0.0, coef, 0.1, 8, None) == 1
    assert lib.ccn_sampler_step_seeded(x, None, None, x, None, seeds, 1, 4, 2, 0.0, coef, 0.1, 8, None) == 1      # unknown pred
    assert lib.ccn_sample_seeded(None, None, None, None, 1, 1, 1, 1, None, None, None, None, None, None, 0, None, 0) == 1
    assert lib.ccn_sample_guided_seeded(None, None, None, None, None, 1, 1, 1, 1, None, None, None, None, 1.0, None, None, 0, None, 0) == 1


def test_seeds_tensor():
    t = _native.seeds_tensor([0, 2 ** 32 - 1, 2 ** 63 + 5, -1], 4, "cpu")
    assert t.dtype == torch.int64 and t.tolist() == [0, 2 ** 32 - 1, -(2 ** 63) + 5, -1]
    assert _native.seeds_tensor(torch.tensor([3, -4]), 2, "cpu").tolist() == [3, -4]
    with pytest.raises(ValueError, match="one entry per record"):
        _native.seeds_tensor([1, 2, 3], 2, "cpu")
    with pytest.raises(ValueError, match="int64"):
        _native.seeds_tensor(torch.tensor([1.0, 2.0]), 2, "cpu")
