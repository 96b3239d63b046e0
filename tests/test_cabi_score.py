"""The three entry points of the device scores are declared, exported and prototyped; the host pieces beside them (no GPU needed)."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest

from clip_feature_codec import _native

HEADER = Path(__file__).resolve().parent.parent / "include" / "ccn_hip.h"
ARGS = {"ccn_score_scratch_bytes": 5, "ccn_psnr_ssim_f32": 11, "ccn_psnr_ssim_u8": 10}


def test_score_entry_points_exist():
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


def test_scratch_query_is_host_arithmetic():
    """16 bytes per workgroup of 16 x 64 window positions, at least one workgroup per plane; bad arguments are CCN_EINVAL."""
    assert _native.score_scratch_bytes(1, 1, 7, 7) == 16
    assert _native.score_scratch_bytes(3, 1, 6, 20) == 3 * 16                      # no window position: still one workgroup per plane
    assert _native.score_scratch_bytes(2, 3, 45, 141) == 2 * 3 * 3 * 3 * 16          # 39 x 135 positions: 3 x 3 tiles
    assert _native.score_scratch_bytes(8, 3, 256, 256) == 8 * 3 * 16 * 4 * 16
    lib = _native.load_library()
    n = ctypes.c_size_t(0)
    assert lib.ccn_score_scratch_bytes(0, 3, 8, 8, ctypes.byref(n)) == 1
    assert lib.ccn_score_scratch_bytes(1, 3, 8, -1, ctypes.byref(n)) == 1
    assert lib.ccn_score_scratch_bytes(1, 3, 8, 8, None) == 1


def test_psnr_from_sse():
    from clip_feature_codec.eval.metrics import psnr_from_sse, psnr_u8
    assert psnr_from_sse(0, 10) == float("inf")
    assert psnr_from_sse(65025.0 * 12, 12) == 0.0                                   # every value off by 255
    assert abs(psnr_from_sse(100, 100) - 20.0 * math.log10(255.0)) < 1e-12          # mse 1
    got = psnr_from_sse(np.array([0.0, 400.0]), 100)
    assert got.dtype == np.float64 and np.isinf(got[0]) and abs(got[1] - 20.0 * math.log10(255.0 / 2.0)) < 1e-12
    a = np.arange(48, dtype=np.uint8).reshape(3, 4, 4); b = (a + 3).astype(np.uint8)
    assert abs(psnr_from_sse(9 * 48, 48) - psnr_u8(a, b)) < 1e-4


def test_device_metrics_is_off_by_default():
    from clip_feature_codec.cli.eval import build_parser
    base = ["--store_dir", "s", "--weights", "w"]
    assert build_parser().parse_args(base).device_metrics is False
    assert build_parser().parse_args(base + ["--device_metrics"]).device_metrics is True
