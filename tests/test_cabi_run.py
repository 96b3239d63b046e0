"""The descriptor entry of the sampler loop, ``ccn_sample_run``, is declared, exported and prototyped; the ctypes structure is the
header's ``ccn_sampler_run_t``; and the descriptor is validated before any device is touched (no GPU needed)."""
import ctypes
import re
from pathlib import Path

import pytest

from clip_feature_codec import _native

HEADER = Path(__file__).resolve().parent.parent / "include" / "ccn_hip.h"
EINVAL = 1
C_TYPES = {"uint32_t": ctypes.c_uint32, "int32_t": ctypes.c_int32, "float": ctypes.c_float}


def test_entry_point_exists():
    if not _native.LIB_PATH.exists():
        pytest.fail(f"{_native.LIB_PATH} is not built: run `python __graft_entry__.py`")
    lib = ctypes.CDLL(str(_native.LIB_PATH))
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    assert hasattr(lib, "ccn_sample_run"), "ccn_sample_run is not exported"
    assert "ccn_sample_run" in _native.SIGNATURES, "ccn_sample_run has no ctypes prototype"
    decl = re.search(r"\bccn_sample_run\s*\(([^)]*)\)", text)
    assert decl is not None, "ccn_sample_run is not declared in ccn_hip.h"
    assert len(decl.group(1).split(",")) == len(_native.SIGNATURES["ccn_sample_run"][1]) == 12
    # the seven fixed-shape entries keep their prototypes
    for name, nargs in (("ccn_sample", 14), ("ccn_sample_eta", 16), ("ccn_sample_guided", 19), ("ccn_sample_seeded", 17),
                        ("ccn_sample_guided_seeded", 19), ("ccn_sample_ms", 15), ("ccn_sample_guided_ms", 18)):
        assert hasattr(lib, name) and len(_native.SIGNATURES[name][1]) == nargs, name


def test_structure_mirrors_the_header():
    """Field for field: the names in the header's order, pointers as pointers, the fixed-width scalars as themselves."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    body = re.search(r"typedef struct ccn_sampler_run \{(.*?)\} ccn_sampler_run_t;", text, flags=re.S)
    assert body is not None, "ccn_sampler_run_t is not declared in ccn_hip.h"
    fields = []
    for line in body.group(1).split(";"):
        if line.strip():
            assert ":" not in line, "no bit-fields"
            ctype, name = re.fullmatch(r"\s*(?:const\s+)?(\w+\s*\*?)\s*(\w+)\s*", line).groups()
            fields.append((name, ctypes.c_void_p if ctype.endswith("*") else C_TYPES[ctype.strip()]))
    assert fields == list(_native.CcnSamplerRun._fields_)
    assert fields[0] == ("size", ctypes.c_uint32)


def test_descriptor_is_checked_without_a_device():
    lib = _native.load_library()
    ts, coef = (ctypes.c_int32 * 2)(999, 0), (ctypes.c_float * 10)(*([1.0] * 10))
    tail = (None, None, None, 1, 16, 16, None, 0, None, 0)        # null tensors, no workspace: never reached

    def run(**fields):
        d = _native.CcnSamplerRun(size=ctypes.sizeof(_native.CcnSamplerRun), steps=2, ts_host=ctypes.addressof(ts),
                                  coef_host=ctypes.addressof(coef), coef_cols=4)
        for k, v in fields.items():
            setattr(d, k, v)
        return lib.ccn_sample_run(None, ctypes.byref(d), *tail), lib.ccn_last_error()

    # the library accepts sizeof of the Python structure: a well-formed run with a NULL handle fails on the handle
    rc, err = run()
    assert rc == EINVAL and b"null handle" in err and b"size" not in err
    for size in (0, ctypes.sizeof(_native.CcnSamplerRun) - 8, ctypes.sizeof(_native.CcnSamplerRun) + 8):
        rc, err = run(size=size)
        assert rc == EINVAL and b"size" in err and str(size).encode() in err
    assert lib.ccn_sample_run(None, None, *tail) == EINVAL
    assert b"descriptor" in lib.ccn_last_error()
    # what no ccn_sample* entry expresses, and what they all refuse; the device pointers are never dereferenced
    dev, odd = 0x1000, 0x1004
    for fields, word in ((dict(coef_cols=3), b"coef_cols"),
                         (dict(steps=0), b"positive"),
                         (dict(ts_host=None), b"null pointer"),
                         (dict(coef_cols=5, x0_hist_dev=dev, sigma_host=ctypes.addressof(coef), noise_dev=dev), b"no ccn_sample* entry"),
                         (dict(coef_cols=5, x0_hist_dev=dev, seeds_dev=dev), b"no ccn_sample* entry"),
                         (dict(sigma_host=ctypes.addressof(coef), noise_dev=dev, seeds_dev=dev, out_scratch_dev=dev), b"no ccn_sample* entry"),
                         (dict(sigma_host=ctypes.addressof(coef)), b"given together"),
                         (dict(noise_dev=dev), b"given together"),
                         (dict(seeds_dev=odd), b"8-byte"),
                         (dict(guided=1, w=float("inf"), out_scratch_dev=dev), b"finite"),
                         (dict(guided=1, w=2.0), b"scratch"),
                         (dict(guided=1, w=2.0, out_scratch_dev=odd), b"scratch"),
                         (dict(sigma_host=ctypes.addressof(coef), seeds_dev=dev), b"scratch"),
                         (dict(coef_cols=5), b"history"),
                         (dict(coef_cols=5, x0_hist_dev=odd), b"history")):
        rc, err = run(**fields)
        assert rc == EINVAL and word in err, (fields, err)
    coef[4] = 0.25                                                  # c4 of step 0
    rc, err = run(coef_cols=5, x0_hist_dev=dev)
    assert rc == EINVAL and b"c4 must be 0 on step 0" in err
    coef[4], coef[7] = 0.0, float("nan")
    rc, err = run(coef_cols=5, x0_hist_dev=dev)
    assert rc == EINVAL and b"non-finite" in err
    # an unused field is ignored: seeds without sigma, a scratch or a history nobody needs -- the run is well-formed, the handle is not
    rc, err = run(seeds_dev=dev, out_scratch_dev=odd, x0_hist_dev=odd, w=float("nan"), z_null_dev=dev)
    assert rc == EINVAL and b"null handle" in err


def test_the_seven_entries_still_refuse_without_a_device():
    """Every argument fails a check before any device is touched: a NULL handle, and each entry's own insistence."""
    lib = _native.load_library()
    ts, coef = (ctypes.c_int32 * 2)(999, 0), (ctypes.c_float * 10)(*([0.0] * 10))
    t, c = ctypes.addressof(ts), ctypes.addressof(coef)
    dev = 0x1000
    shape, tail = (1, 16, 16, 2, t, c), (None, 0, None, 0)
    assert lib.ccn_sample(None, None, None, None, *shape, *tail) == EINVAL
    assert lib.ccn_sample_eta(None, None, None, None, *shape, c, None, *tail) == EINVAL           # sigma without noise
    assert b"sigma" in lib.ccn_last_error()
    assert lib.ccn_sample_guided(None, None, None, None, None, *shape, None, None, 2.0, None, *tail) == EINVAL
    assert b"scratch" in lib.ccn_last_error()
    assert lib.ccn_sample_guided(None, None, None, None, None, *shape, None, dev, 2.0, dev, *tail) == EINVAL
    assert b"given together" in lib.ccn_last_error()
    assert lib.ccn_sample_seeded(None, None, None, None, *shape, None, dev, None, *tail) == EINVAL    # sigma NULL: still its scratch
    assert b"scratch" in lib.ccn_last_error()
    assert lib.ccn_sample_seeded(None, None, None, None, *shape, None, None, dev, *tail) == EINVAL    # ... and its seeds
    assert b"seeds" in lib.ccn_last_error()
    assert lib.ccn_sample_guided_seeded(None, None, None, None, None, *shape, c, None, 2.0, dev, *tail) == EINVAL
    assert b"seeds" in lib.ccn_last_error()
    assert lib.ccn_sample_ms(None, None, None, None, *shape, None, *tail) == EINVAL
    assert b"history" in lib.ccn_last_error()
    assert lib.ccn_sample_guided_ms(None, None, None, None, None, *shape, float("nan"), dev, dev, *tail) == EINVAL
    assert b"finite" in lib.ccn_last_error()
    assert lib.ccn_sample_ms(None, None, None, None, *shape, dev, *tail) == EINVAL
    assert b"null handle" in lib.ccn_last_error()
