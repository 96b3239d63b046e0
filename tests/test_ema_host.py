"""Host-side checks of the weight EMA: the C ABI's surface, the off defaults of the new keywords, and the float64 closed form of
tests/ema_ref.py pinned to torch's own ``AveragedModel`` with ``get_ema_multi_avg_fn`` on the CPU."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np

from clip_feature_codec import _native
from clip_feature_codec.train import diffusion_train as dt

import ema_ref

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "ccn_hip.h").read_text()


def _prototype(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in ccn_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_ema_calls_and_the_ctypes_mirror_matches():
    for name in ("ccn_ema_init", "ccn_adamw_step_ema"):
        args = _prototype(name)
        res, argtypes = _native.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(argtypes) == len(args), (name, args)
        for a, ty in zip(args, argtypes):
            want = (ctypes.c_void_p if "*" in a else ctypes.c_float if a.startswith("float") else ctypes.c_double if a.startswith("double")
                    else ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_int32)
            assert ty is want, (name, a)
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    body = re.search(r"typedef struct ccn_ema_state_s \{(.*?)\} ccn_ema_state_t;", text, flags=re.S).group(1)
    names = re.findall(r"\b(weight|apply|first|updates|reserved)\b", body)
    assert names == [n for n, _ in _native.EmaStateBlock._fields_]
    assert ctypes.sizeof(_native.EmaStateBlock) == 32 and _native.EMA_WORDS == 8
    assert _native.EMA_WORD == dict(weight=0, apply=1, first=2, updates=3, reserved=4)


def test_the_new_keywords_are_off_by_default():
    sig = inspect.signature(dt.FusedAdamW.__init__).parameters
    assert sig["ema_decay"].default is None and sig["ema_warmup"].default is False
    sig = inspect.signature(dt.train_diffusion).parameters
    assert sig["ema_decay"].default is None and sig["ema_warmup"].default is False and sig["resume"].default is None
    assert inspect.signature(dt.train_step).parameters["ema_decay"].default is None


def test_constant_decay_closed_form_agrees_with_torchs_averaged_model():
    """After every update within 2 fp32 ulp of max|value| per update taken: one lerp_ is a rounding of the difference, scaled by
    w < 1, and a rounding of the sum, against the exact float64 evaluation of the same expression on the same fp32 weight."""
    for decay in (0.999, 0.5, 0.9):
        p_seq = ema_ref.walk(1000, 5)
        ref = ema_ref.closed_form(p_seq, decay)
        cpu = ema_ref.torch_cpu_loop(p_seq, decay)
        assert np.array_equal(cpu["ema"][0], p_seq[0]) and np.array_equal(ref["ema"][0], p_seq[0].astype(np.float64))     # the copy
        assert cpu["n_averaged"] == ref["updates"] == [1, 2, 3, 4, 5]
        for k in range(5):
            err = float(np.abs(cpu["ema"][k].astype(np.float64) - ref["ema"][k]).max())
            bound = 2 * ema_ref.ulp32(np.abs(ref["ema"][k]).max()) * (k + 1)
            print(f"decay {decay}, update {k}: torch CPU fp32 vs closed form {err:.3e} (bound {bound:.3e})")
            assert err <= bound, (decay, k)
        assert ref["weights"][-1] == np.float32(1 - decay)


def test_warmup_weights_are_nine_over_ten_plus_u_until_below_one_minus_decay():
    decay = 0.9
    ws = [ema_ref.weight(decay, True, u) for u in range(100)]
    for u, w in enumerate(ws):
        nine = np.float32(9) / np.float32(10 + u)
        assert w == (nine if nine > np.float32(1 - decay) else np.float32(1 - decay)), u
        # the complement of min(decay, (1 + u) / (10 + u)), to fp32 precision
        assert abs(float(w) - (1.0 - min(decay, (1 + u) / (10 + u)))) <= 2.0 ** -24, u
    assert ws[0] == np.float32(0.9) and ws[79] > np.float32(0.1) and ws[81] == np.float32(1 - decay)
    assert all(ema_ref.weight(decay, False, u) == np.float32(1 - decay) for u in range(5))
    # the closed form applies them: update 1 moves 9/11 of the way
    p_seq = ema_ref.walk(16, 3)
    ref = ema_ref.closed_form(p_seq, decay, warmup=True)
    want = p_seq[0].astype(np.float64) + float(np.float32(9) / np.float32(11)) * (p_seq[1].astype(np.float64) - p_seq[0])
    assert np.array_equal(ref["ema"][1], want) and ref["weights"] == [ws[0], ws[1], ws[2]]


def test_a_skipped_step_leaves_value_and_count_alone():
    p_seq = ema_ref.walk(64, 6)
    applied = [True, True, False, True, False, True]
    ref = ema_ref.closed_form(p_seq, 0.9, warmup=True, applied=applied)
    cpu = ema_ref.torch_cpu_loop(p_seq, 0.9, applied=applied)
    assert ref["updates"] == [1, 2, 2, 3, 3, 4] == cpu["n_averaged"]
    for k in (2, 4):
        assert np.array_equal(ref["ema"][k], ref["ema"][k - 1]) and ref["weights"][k] == ref["weights"][k - 1]
        assert np.array_equal(cpu["ema"][k], cpu["ema"][k - 1])
    # the warm-up's clock is the count of updates, not of calls: the update after a skip uses the next weight in line
    assert ref["weights"][3] == ema_ref.weight(0.9, True, 2) and ref["weights"][5] == ema_ref.weight(0.9, True, 3)
    only = ema_ref.closed_form([p for p, ok in zip(p_seq, applied) if ok], 0.9, warmup=True)
    assert np.array_equal(ref["ema"][-1], only["ema"][-1])
    # a skip before the first update: still no average
    assert ema_ref.closed_form(p_seq[:2], 0.9, applied=[False, True])["updates"] == [0, 1]
