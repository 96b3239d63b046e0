"""The three entry points of the v-parameterisation are declared, exported and prototyped (no GPU needed)."""
import ctypes
import re
from pathlib import Path

import pytest

from clip_feature_codec import _native

HEADER = Path(__file__).resolve().parent.parent / "include" / "ccn_hip.h"
ARGS = {"ccn_set_prediction": 2, "ccn_sampler_step": 12, "ccn_diffusion_loss_grad_v": 16}


def test_vpred_entry_points_exist():
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
    assert re.search(r"CCN_PRED_EPS\s*=\s*0\s*,\s*CCN_PRED_V\s*=\s*1", text)
    assert (_native.PRED_EPS, _native.PRED_V) == (0, 1)
    # the loss kernel takes what ccn_diffusion_loss_grad takes
    assert _native.SIGNATURES["ccn_diffusion_loss_grad_v"] == _native.SIGNATURES["ccn_diffusion_loss_grad"]


def test_bad_arguments_are_einval_without_a_device():
    """A handle cannot be made without a device (ccn_create asks for one), so ccn_set_prediction is only reached with a null handle
    here; ccn_sampler_step validates before it launches anything."""
    lib = _native.load_library()
    assert lib.ccn_set_prediction(None, 2) == 1                      # CCN_EINVAL
    assert lib.ccn_set_prediction(None, 0) == 1
    coef = (ctypes.c_float * 5)(1, 1, 1, 0, 0)
    assert lib.ccn_sampler_step(None, None, None, None, None, None, 0, 0.0, coef, 0.0, 4, None) == 1
    assert b"bad argument" in lib.ccn_last_error()
    with pytest.raises(ValueError, match="prediction"):
        _native.prediction_code("x0")
    assert _native.prediction_code("eps") == 0 and _native.prediction_code("v") == 1
