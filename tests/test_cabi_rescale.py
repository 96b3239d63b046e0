"""The entry points of guidance rescale are declared, exported and prototyped; they validate before they launch (no GPU needed)."""
import ctypes
import math
import re
from pathlib import Path

import pytest

from clip_feature_codec import _native

HEADER = Path(__file__).resolve().parent.parent / "include" / "ccn_hip.h"
ARGS = {"ccn_guidance_rescale_scratch_bytes": 3, "ccn_guidance_rescale": 10, "ccn_x0_threshold_rs": 16, "ccn_sampler_step_rs": 17,
        "ccn_set_guidance_rescale": 4}
EINVAL = 1


def test_rescale_entry_points_exist():
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
    sig = _native.SIGNATURES
    # each _rs entry is its parent plus one pointer in front of the stream; the parents are untouched
    assert sig["ccn_x0_threshold_rs"][1][:-2] == sig["ccn_x0_threshold"][1][:-1] and len(sig["ccn_x0_threshold"][1]) == 15
    assert sig["ccn_sampler_step_rs"][1][:-2] == sig["ccn_sampler_step_thr"][1][:-1] and len(sig["ccn_sampler_step_thr"][1]) == 16
    assert sig["ccn_x0_threshold_rs"][1][-2:] == [ctypes.c_void_p] * 2 and sig["ccn_sampler_step_rs"][1][-3:] == [ctypes.c_void_p] * 3
    # w is a float, phi a double
    assert sig["ccn_guidance_rescale"][1][2] is ctypes.c_float and sig["ccn_guidance_rescale"][1][3] is ctypes.c_double
    assert sig["ccn_set_guidance_rescale"][1][1] is ctypes.c_double
    assert sig["ccn_x0_threshold_rs"][1][9] is ctypes.c_double and sig["ccn_x0_threshold_rs"][1][10] is ctypes.c_float
    assert sig["ccn_sampler_step_rs"][1][10] is ctypes.c_float and sig["ccn_sampler_step_rs"][1][12] is ctypes.c_float
    assert len(_native.CcnSamplerRun._fields_) == 13                 # the run record is what it was


def test_scratch_size():
    lib = _native.load_library()
    n = ctypes.c_size_t()

    def size(B, per):
        assert lib.ccn_guidance_rescale_scratch_bytes(B, per, ctypes.byref(n)) == 0
        return n.value
    # the B factors first, 16-byte aligned, then four doubles per workgroup: clamp(ceil(per / 4096), 1, 64) workgroups per record
    assert size(1, 2) == 16 + 32 and size(1, 4096) == 16 + 32 and size(1, 4097) == 16 + 64
    assert size(1, 12288) == 16 + 3 * 32 and size(3, 12288) == 16 + 3 * 3 * 32 and size(5, 768) == 32 + 5 * 32
    assert size(1, 3 * 256 * 256) == 16 + 48 * 32 and size(1, 64 * 4096 + 1) == 16 + 64 * 32 and size(1, (1 << 34) - 1) == 16 + 64 * 32
    assert all(size(B, 969) % 16 == 0 for B in range(1, 9))
    assert _native.guidance_rescale_scratch_bytes(3, 12288) == size(3, 12288)
    for bad in ((0, 768), (65536, 768), (-1, 768), (1, 1), (1, 0), (1, 1 << 34)):
        assert lib.ccn_guidance_rescale_scratch_bytes(bad[0], bad[1], ctypes.byref(n)) == EINVAL, bad
    assert lib.ccn_guidance_rescale_scratch_bytes(1, 1, ctypes.byref(n)) == EINVAL and b"[2, 2^34)" in lib.ccn_last_error()
    assert lib.ccn_guidance_rescale_scratch_bytes(1, 768, None) == EINVAL


def test_bad_arguments_are_einval_without_a_device():
    lib = _native.load_library()
    y, k, scr = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x4000)       # never dereferenced: every call fails its checks
    big = 1 << 30
    inf, nan = math.inf, math.nan

    def g(yc=y, yu=y, w=3.0, phi=0.7, B=1, per=768, k_=k, scr_=scr, nbytes=big):
        return lib.ccn_guidance_rescale(yc, yu, w, phi, B, per, k_, scr_, nbytes, None)
    assert g(yc=None) == EINVAL and g(yu=None) == EINVAL and g(k_=None) == EINVAL
    assert b"NULL" in lib.ccn_last_error()
    assert g(w=inf) == EINVAL and g(w=nan) == EINVAL
    assert b"finite" in lib.ccn_last_error()
    assert g(phi=-1e-9) == EINVAL and g(phi=1.0001) == EINVAL and g(phi=nan) == EINVAL
    assert b"[0, 1]" in lib.ccn_last_error()
    assert g(B=0) == EINVAL and g(B=65536, nbytes=1 << 40) == EINVAL
    assert b"65535" in lib.ccn_last_error()
    assert g(per=1) == EINVAL and g(per=0) == EINVAL and g(per=1 << 34) == EINVAL
    assert b"2^34" in lib.ccn_last_error()
    assert g(scr_=None) == EINVAL and g(scr_=ctypes.c_void_p(0x4004)) == EINVAL and g(nbytes=47) == EINVAL and g(per=12288, nbytes=16 + 64) == EINVAL
    assert b"scratch" in lib.ccn_last_error()

    # the handle state: the arguments are judged before the handle, and a handle cannot be made without a device
    def sd(phi=0.7, scr_=scr, nbytes=big):
        return lib.ccn_set_guidance_rescale(None, phi, scr_, nbytes)
    for bad in (dict(phi=-1e-9), dict(phi=1.0001), dict(phi=nan)):
        assert sd(**bad) == EINVAL and b"[0, 1]" in lib.ccn_last_error()
    for bad in (dict(scr_=None), dict(scr_=ctypes.c_void_p(0x4008)), dict(nbytes=16)):
        assert sd(**bad) == EINVAL and b"scratch" in lib.ccn_last_error()
    assert sd() == EINVAL and b"null handle" in lib.ccn_last_error()
    assert sd(phi=0.0, scr_=None, nbytes=0) == EINVAL and b"null handle" in lib.ccn_last_error()

    # the two _rs entries check what their parents check, with or without the factors
    thr = ctypes.c_void_p(0x3000)
    for gs in (None, k):
        def q(x_=y, per=768, p=0.5, mx=inf, scr_=scr, pred=0):
            return lib.ccn_x0_threshold_rs(x_, y, None, pred, 0.0, 0.6, 0.8, 1, per, p, mx, thr, scr_, big, gs, None)
        assert q(x_=None) == EINVAL and q(per=0) == EINVAL and q(p=1.5) == EINVAL and q(mx=0.5) == EINVAL and q(scr_=None) == EINVAL and q(pred=2) == EINVAL
        coef = (ctypes.c_float * 5)(1, 1, 1, 0, 0)

        def st(noise=None, seeds_=None, per=4, n=8, pred=0, x_=y):
            return lib.ccn_sampler_step_rs(x_, None, None, y, None, noise, seeds_, 1, per, pred, 0.0, coef, 0.1, n, thr, gs, None)
        assert st(noise=y, seeds_=thr) == EINVAL and b"exclude" in lib.ccn_last_error()
        assert st(per=0) == EINVAL and st(per=3) == EINVAL and st(per=1, n=65536) == EINVAL
        assert st(pred=2) == EINVAL and st(x_=None) == EINVAL and st(n=-4) == EINVAL
        assert st(n=0) == 0                                          # nothing to do, nothing launched


def test_python_value_errors():
    assert _native.rescale_arg(0.7) == 0.7 and _native.rescale_arg(1) == 1.0
    for phi in (0.0, -0.5, 1.01, math.nan):
        with pytest.raises(ValueError, match="guidance_rescale"):
            _native.rescale_arg(phi)
