"""The entry points of dynamic thresholding are declared, exported and prototyped; they validate before they launch, and the Python
layers raise ``ValueError`` for a bad quantile or maximum (no GPU needed)."""
import ctypes
import math
import re
from pathlib import Path

import pytest

from clip_feature_codec import _native
from clip_feature_codec.diffusion.ddim import DDIMSampler
from clip_feature_codec.diffusion.dpm_solver import DPMSolverSampler

HEADER = Path(__file__).resolve().parent.parent / "include" / "ccn_hip.h"
ARGS = {"ccn_x0_threshold_scratch_bytes": 3, "ccn_x0_threshold": 15, "ccn_sampler_step_thr": 16, "ccn_set_dynamic_threshold": 5,
        "ccn_dynamic_threshold_scratch_bytes": 5}
EINVAL = 1


def test_threshold_entry_points_exist():
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
    # the superset of the two step entries: both noise sources and the thresholds
    assert len(_native.SIGNATURES["ccn_sampler_step_seeded"][1]) + 2 == ARGS["ccn_sampler_step_thr"]
    assert _native.SIGNATURES["ccn_x0_threshold"][1][9] is ctypes.c_double and _native.SIGNATURES["ccn_set_dynamic_threshold"][1][1] is ctypes.c_double


def test_scratch_size_is_per_record_and_aligned():
    lib = _native.load_library()
    n1, n3 = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.ccn_x0_threshold_scratch_bytes(1, 768, ctypes.byref(n1)) == 0
    assert lib.ccn_x0_threshold_scratch_bytes(3, 12288, ctypes.byref(n3)) == 0
    assert n1.value > 0 and n1.value % 16 == 0 and n3.value == 3 * n1.value
    assert lib.ccn_x0_threshold_scratch_bytes(0, 768, ctypes.byref(n1)) == EINVAL
    assert lib.ccn_x0_threshold_scratch_bytes(65536, 768, ctypes.byref(n1)) == EINVAL
    assert lib.ccn_x0_threshold_scratch_bytes(1, 0, ctypes.byref(n1)) == EINVAL
    assert lib.ccn_x0_threshold_scratch_bytes(1, 1 << 34, ctypes.byref(n1)) == EINVAL
    assert lib.ccn_x0_threshold_scratch_bytes(1, 768, None) == EINVAL
    assert _native.x0_threshold_scratch_bytes(2, 768) == 2 * n3.value // 3


def test_bad_arguments_are_einval_without_a_device():
    lib = _native.load_library()
    x, thr, scr = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x4000)     # never dereferenced: every call fails its checks
    big = 1 << 30
    inf, nan = math.inf, math.nan

    def q(x_=x, y_=x, pred=0, B=1, per=768, p=0.5, mx=inf, thr_=thr, scr_=scr, nbytes=big):
        return lib.ccn_x0_threshold(x_, y_, None, pred, 0.0, 0.6, 0.8, B, per, p, mx, thr_, scr_, nbytes, None)
    assert q(p=-0.1) == EINVAL and q(p=1.5) == EINVAL and q(p=nan) == EINVAL
    assert b"[0, 1]" in lib.ccn_last_error()
    assert q(mx=0.5) == EINVAL and q(mx=nan) == EINVAL
    assert b"max_value" in lib.ccn_last_error()
    assert q(scr_=None) == EINVAL and q(scr_=ctypes.c_void_p(0x4004)) == EINVAL and q(nbytes=64) == EINVAL
    assert b"scratch" in lib.ccn_last_error()
    assert q(per=0) == EINVAL and q(per=1 << 34) == EINVAL
    assert b"2^34" in lib.ccn_last_error()
    assert q(B=0) == EINVAL and q(B=65536, nbytes=1 << 40) == EINVAL
    assert q(x_=None) == EINVAL and q(y_=None) == EINVAL and q(thr_=None) == EINVAL and q(pred=2) == EINVAL

    coef = (ctypes.c_float * 5)(1, 1, 1, 0, 0)
    seeds = ctypes.c_void_p(0x3000)

    def st(noise=None, seeds_=None, per=4, n=8, pred=0, x_=x):
        return lib.ccn_sampler_step_thr(x_, None, None, x, None, noise, seeds_, 1, per, pred, 0.0, coef, 0.1, n, thr, None)
    assert st(noise=x, seeds_=seeds) == EINVAL
    assert b"exclude" in lib.ccn_last_error()
    assert st(per=0) == EINVAL and st(per=1 << 34, n=1 << 35) == EINVAL and st(per=3) == EINVAL          # 8 % 3
    assert st(per=1, n=65536) == EINVAL
    assert b"65535" in lib.ccn_last_error()
    assert st(pred=2) == EINVAL and st(x_=None) == EINVAL and st(n=-4) == EINVAL

    # the handle state: the arguments are judged before the handle, and a handle cannot be made without a device
    def sd(p=0.995, mx=inf, scr_=scr, nbytes=big):
        return lib.ccn_set_dynamic_threshold(None, p, mx, scr_, nbytes)
    for bad in (dict(p=-1e-9), dict(p=1.0001), dict(p=nan)):
        assert sd(**bad) == EINVAL and b"[0, 1]" in lib.ccn_last_error()
    for bad in (dict(mx=0.999), dict(mx=nan)):
        assert sd(**bad) == EINVAL and b"max_value" in lib.ccn_last_error()
    for bad in (dict(scr_=None), dict(scr_=ctypes.c_void_p(0x4008)), dict(nbytes=16)):
        assert sd(**bad) == EINVAL and b"scratch" in lib.ccn_last_error()
    assert sd() == EINVAL and b"null handle" in lib.ccn_last_error()
    assert sd(p=0.0, scr_=None, nbytes=0) == EINVAL and b"null handle" in lib.ccn_last_error()
    n = ctypes.c_size_t()
    assert lib.ccn_dynamic_threshold_scratch_bytes(None, 1, 16, 16, ctypes.byref(n)) == EINVAL


def test_python_value_errors():
    assert _native.threshold_args(0.995) == (0.995, math.inf)
    assert _native.threshold_args(1, 1) == (1.0, 1.0)
    for p in (0.0, -0.5, 1.01, math.nan):
        with pytest.raises(ValueError, match="quantile"):
            _native.threshold_args(p)
        for cls in (DDIMSampler, DPMSolverSampler):
            with pytest.raises(ValueError, match="quantile"):
                cls(None, dynamic_threshold=p)
    for cls in (DDIMSampler, DPMSolverSampler):
        with pytest.raises(ValueError, match="at least 1"):
            cls(None, dynamic_threshold=0.9, threshold_max=0.5)
        with pytest.raises(ValueError, match="needs dynamic_threshold"):
            cls(None, threshold_max=2.0)
        s = cls(None, dynamic_threshold=0.9, threshold_max=2.0)
        assert (s.dynamic_threshold, s.threshold_max) == (0.9, 2.0)
        assert cls(None).dynamic_threshold is None


def test_cli_flags():
    from clip_feature_codec.cli import eval as cli_eval, reconstruct_diffusion as cli_recon, _common
    for cli, extra in ((cli_eval, []), (cli_recon, ["--bitstream", "b", "--out", "o"])):
        base = ["--store_dir", "s", "--weights", "w"] + extra
        a = cli.build_parser().parse_args(base)
        assert a.dynamic_threshold is None and a.threshold_max is None
        a = cli.build_parser().parse_args(base + ["--dynamic_threshold", "0.995", "--threshold_max", "4"])
        assert (a.dynamic_threshold, a.threshold_max) == (0.995, 4.0)
    _common.check_threshold_flags(None, None)
    _common.check_threshold_flags(0.995, None)
    for bad in ((0.0, None), (1.5, None), (0.9, 0.5), (None, 2.0)):
        with pytest.raises(SystemExit):
            _common.check_threshold_flags(*bad)
