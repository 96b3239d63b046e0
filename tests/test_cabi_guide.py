"""The entry points of the low-resolution guide are declared, exported and prototyped; they validate before they launch (no GPU
needed).  The scratch size needs a handle, and a handle needs a device: tests/test_gpu_guide.py checks its values."""
import ctypes
import math
import re
from pathlib import Path

import pytest

from clip_feature_codec import _native

HEADER = Path(__file__).resolve().parent.parent / "include" / "ccn_hip.h"
ARGS = {"ccn_block_mean": 7, "ccn_lowres_delta": 18, "ccn_sampler_step_lr": 22, "ccn_set_lowres_guide": 7, "ccn_lowres_guide_scratch_bytes": 6}
EINVAL = 1


def test_guide_entry_points_exist():
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
    # ccn_sampler_step_lr is ccn_sampler_step_rs plus C, H, W, N and the table in front of the stream; the parent is untouched
    assert sig["ccn_sampler_step_lr"][1][:-6] == sig["ccn_sampler_step_rs"][1][:-1] and len(sig["ccn_sampler_step_rs"][1]) == 17
    assert sig["ccn_sampler_step_lr"][1][-6:] == [ctypes.c_int32] * 4 + [ctypes.c_void_p] * 2
    # ccn_lowres_delta: the tensors and scalars of ccn_x0_threshold_rs first, the strength a float
    assert sig["ccn_lowres_delta"][1][:8] == sig["ccn_x0_threshold_rs"][1][:8]
    assert sig["ccn_lowres_delta"][1][13] is ctypes.c_float and sig["ccn_set_lowres_guide"][1][3] is ctypes.c_float
    assert len(_native.CcnSamplerRun._fields_) == 13                 # the run record is what it was
    assert len(sig["ccn_workspace_bytes"][1]) == 6


def test_bad_arguments_are_einval_without_a_device():
    lib = _native.load_library()
    p, q, g, d = (ctypes.c_void_p(a) for a in (0x1000, 0x2000, 0x3000, 0x4000))   # never dereferenced: every call fails its checks
    nan = math.nan

    def bm(x=p, planes=3, H=16, W=16, N=4, out=q):
        return lib.ccn_block_mean(x, planes, H, W, N, out, None)
    assert bm(x=None) == EINVAL and bm(out=None) == EINVAL and b"NULL" in lib.ccn_last_error()
    assert bm(planes=0) == EINVAL
    for n in (0, 1, 3, 6, 12, 128, -4):
        assert bm(N=n, H=384, W=384) == EINVAL and b"power of two" in lib.ccn_last_error(), n
    assert bm(H=18) == EINVAL and bm(W=18) == EINVAL and b"multiples of N" in lib.ccn_last_error()
    assert bm(H=0) == EINVAL and bm(W=-16) == EINVAL

    def ld(x=p, yc=q, yu=None, pred=0, B=2, C=3, H=16, W=16, N=4, guide=g, lam=1.0, thr=None, gs=None, out=d):
        return lib.ccn_lowres_delta(x, yc, yu, pred, 3.0, 0.6, 0.8, B, C, H, W, N, guide, lam, thr, gs, out, None)
    for bad in (dict(x=None), dict(yc=None), dict(guide=None), dict(out=None)):
        assert ld(**bad) == EINVAL and b"NULL" in lib.ccn_last_error(), bad
    assert ld(pred=2) == EINVAL and b"prediction" in lib.ccn_last_error()
    assert ld(B=0) == EINVAL and ld(B=65536) == EINVAL and b"65535" in lib.ccn_last_error()
    assert ld(C=0) == EINVAL
    for n in (0, 1, 3, 6, 128):
        assert ld(N=n, H=384, W=384) == EINVAL and b"power of two" in lib.ccn_last_error(), n
    assert ld(H=18) == EINVAL and ld(W=20, N=8) == EINVAL and b"multiples of N" in lib.ccn_last_error()
    for lam in (0.0, -0.5, 1.0001, nan):
        assert ld(lam=lam) == EINVAL and b"(0, 1]" in lib.ccn_last_error(), lam
    for yu in (None, q):                                            # (the nullable tensors change no check)
        assert ld(yu=yu, thr=p, gs=p, N=3) == EINVAL

    coef = (ctypes.c_float * 5)(1, 1, 1, 0, 0)

    def st(per=768, n=1536, C=3, H=16, W=16, N=4, delta=d, noise=None, seeds=None, pred=0, x=p):
        return lib.ccn_sampler_step_lr(x, None, None, q, None, noise, seeds, 1, per, pred, 0.0, coef, 0.1, n, None, None, C, H, W, N, delta, None)
    for n in (0, 1, 3, 128):
        assert st(N=n, H=384, W=384, per=3 * 384 * 384, n=3 * 384 * 384) == EINVAL and b"power of two" in lib.ccn_last_error(), n
    assert st(H=18, per=3 * 18 * 16, n=3 * 18 * 16) == EINVAL and b"multiples of N" in lib.ccn_last_error()
    assert st(C=1) == EINVAL and st(per=384, n=1536, C=3) == EINVAL and b"C*H*W" in lib.ccn_last_error()
    assert st(per=12, n=12 * 65536, C=3, H=2, W=2, N=2) == EINVAL and b"65535" in lib.ccn_last_error()
    assert st(noise=p, seeds=q) == EINVAL and b"exclude" in lib.ccn_last_error()
    assert st(pred=2) == EINVAL and st(x=None) == EINVAL and st(n=-4) == EINVAL and st(per=0) == EINVAL and st(per=700) == EINVAL
    assert st(n=0) == 0                                              # nothing to do, nothing launched
    # without a table the geometry is not read: ccn_sampler_step_rs's checks alone
    assert st(delta=None, N=3, H=5, n=0) == 0 and st(delta=None, per=0) == EINVAL

    # the handle state: the arguments are judged before the handle, and a handle cannot be made without a device
    big = 1 << 30

    def sg(guide=g, N=4, lam=1.0, t_min=0, scr=d, nbytes=big):
        return lib.ccn_set_lowres_guide(None, guide, N, lam, t_min, scr, nbytes)
    for n in (1, 3, 6, 128, -2):
        assert sg(N=n) == EINVAL and b"power of two" in lib.ccn_last_error(), n
    assert sg(guide=None) == EINVAL and b"NULL" in lib.ccn_last_error()
    for lam in (0.0, -0.5, 1.0001, nan):
        assert sg(lam=lam) == EINVAL and b"(0, 1]" in lib.ccn_last_error(), lam
    assert sg(t_min=-1) == EINVAL and b"t_min" in lib.ccn_last_error()
    for bad in (dict(scr=None), dict(scr=ctypes.c_void_p(0x4008)), dict(nbytes=16 + 63)):
        assert sg(**bad) == EINVAL and b"scratch" in lib.ccn_last_error(), bad
    assert sg() == EINVAL and b"null handle" in lib.ccn_last_error()
    assert sg(N=0, guide=None, scr=None, nbytes=0) == EINVAL and b"null handle" in lib.ccn_last_error()
    n = ctypes.c_size_t()
    assert lib.ccn_lowres_guide_scratch_bytes(None, 1, 16, 16, 4, ctypes.byref(n)) == EINVAL and b"null handle" in lib.ccn_last_error()
