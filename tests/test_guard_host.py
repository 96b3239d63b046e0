"""Host-side checks of the step guard (GradScaler + clip_grad_norm_ + AdamW on applied steps): the C ABI's surface, the new
keywords' off defaults, and the float64 closed form of tests/guard_ref.py pinned to torch's own CPU classes."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np

from clip_feature_codec import _native
from clip_feature_codec.train import diffusion_train as dt

import guard_ref

REPO = Path(__file__).resolve().parent.parent
HEADER = (REPO / "include" / "ccn_hip.h").read_text()
GUARD_FUNCS = ("ccn_step_guard_init", "ccn_grad_guard", "ccn_adamw_step_guarded")


def _prototype(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in ccn_hip.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_declares_the_guard_calls_and_signatures_match_in_arity():
    for name in GUARD_FUNCS:
        args = _prototype(name)
        assert name in _native.SIGNATURES, name
        res, argtypes = _native.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(argtypes) == len(args), (name, args)
        # pointers are void pointers on the Python side, floats floats, the element count 64-bit
        for a, ty in zip(args, argtypes):
            if "*" in a:
                assert ty is ctypes.c_void_p, (name, a)
            elif a.startswith("float"):
                assert ty is ctypes.c_float, (name, a)
            elif a.startswith("int64_t"):
                assert ty is ctypes.c_int64, (name, a)
            else:
                assert a.startswith("int32_t") and ty is ctypes.c_int32, (name, a)


def test_header_declares_the_control_block_and_python_views_it_word_for_word():
    m = re.search(r"typedef\s+struct\s+ccn_step_guard_s\s*\{(.*?)\}\s*ccn_step_guard_t\s*;", HEADER, flags=re.S)
    assert m, "ccn_step_guard_t is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"\b(float|int32_t)\s+([a-z_0-9]+)(?:\[(\d+)\])?\s*;", body)
    words, offset = {}, 0
    for ty, name, count in fields:
        words[name] = (offset, ty)
        offset += int(count) if count else 1
    assert offset == _native.GUARD_WORDS == 16 and ctypes.sizeof(_native.StepGuardBlock) == 64
    for name, (off, ty) in words.items():
        assert _native.GUARD_WORD[name] == off, name
        ctype = dict(_native.StepGuardBlock._fields_)[name]
        assert (ctype is ctypes.c_float) == (ty == "float"), name
    for must in ("scale", "grad_norm", "grad_mul", "bc1", "bc2_sqrt", "apply", "good_steps", "skipped_steps", "growth_tracker"):
        assert must in words
    # the fp32 words come first: GradScaler views words 0..5 as float32
    assert all(off < 6 for off, ty in words.values() if ty == "float") and all(off >= 6 for off, ty in words.values() if ty != "float")
    assert _native.GUARD_SCRATCH_FLOATS * 4 >= 2048 * 8


def test_new_keywords_exist_and_default_to_off():
    sig = inspect.signature(dt.train_step).parameters
    assert sig["scaler"].default is None and sig["max_grad_norm"].default is None
    sig = inspect.signature(dt.train_diffusion).parameters
    assert sig["grad_scaler"].default is False and sig["max_grad_norm"].default is None
    sig = inspect.signature(dt.FusedAdamW.step).parameters
    assert sig["guard"].default is None and sig["max_grad_norm"].default is None and sig["zero_grad"].default is False
    sig = inspect.signature(dt.autograd_objective_step).parameters
    assert sig["scaler"].default is None and sig["max_grad_norm"].default is None
    sig = inspect.signature(dt.GradScaler.__init__).parameters
    assert [sig[k].default for k in ("init_scale", "growth_factor", "backoff_factor", "growth_interval", "enabled")] == [65536.0, 2.0, 0.5, 2000, True]
    for name in ("scale", "step", "update", "get_scale", "state_dict", "load_state_dict", "stats"):
        assert callable(getattr(dt.GradScaler, name))
    assert "reference's" in dt.train_diffusion.__doc__ and "grad_scaler=True" in dt.train_diffusion.__doc__


def test_gradscaler_state_dict_before_any_step_and_rejects_torch_optimisers():
    import pytest
    import torch
    s = dt.GradScaler(init_scale=1024.0, growth_interval=7)
    sd = s.state_dict()
    assert sd["scale"] == 1024.0 and sd["_growth_tracker"] == 0 and sd["good_steps"] == 0 and sd["skipped_steps"] == 0 and sd["growth_interval"] == 7
    s2 = dt.GradScaler()
    s2.load_state_dict(dict(sd, scale=256.0, _growth_tracker=3, good_steps=11, skipped_steps=2))
    assert s2.get_scale() == 256.0 and s2.state_dict()["_growth_tracker"] == 3 and s2.state_dict()["good_steps"] == 11
    assert dt.GradScaler(enabled=False).get_scale() == 1.0
    with pytest.raises(TypeError, match="torch.amp.GradScaler"):
        s.step(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(3))]))
    with pytest.raises(ValueError):
        dt.GradScaler(growth_interval=0)


def test_closed_form_is_pinned_to_torch_cpu_gradscaler_clip_and_adamw():
    """GradScaler('cpu', growth_interval=3) -> unscale_ -> clip_grad_norm_(0.5) -> AdamW on a 1000-element parameter for ten
    iterations, gradient g0 * it with +inf planted at iteration 3 and NaN at iteration 7.  The scale after each iteration and the
    optimiser's step count are exact; the parameters agree within 3 U max|p| per applied step (U = 2^-24: three fp32 roundings of p
    per AdamW update -- the decay product, the update term's product and the subtraction -- are the only ones that matter at lr = 3e-4)."""
    p0, grads = guard_ref.script(1000)
    ref = guard_ref.closed_form(p0, grads, growth_interval=3, max_grad_norm=0.5, **guard_ref.HYPER)
    got = guard_ref.torch_cpu_loop(p0, grads, growth_interval=3, max_grad_norm=0.5, **guard_ref.HYPER)
    expect = [65536.0, 65536.0, 32768.0, 32768.0, 32768.0, 65536.0, 32768.0, 32768.0, 32768.0, 65536.0]
    assert ref["scales"] == expect and got["scales"] == expect
    assert ref["applied"] == [it not in (3, 7) for it in range(1, 11)]
    assert ref["good_steps"] == 8 and got["steps"] == 8 and ref["skipped_steps"] == 2
    # clipping is active from the second iteration on (|g0 * it| ~ 0.32 it), inactive in the first: both branches run
    assert ref["norms"][0] < 0.5 < ref["norms"][1]
    err = float(np.abs(got["p"].astype(np.float64) - ref["p"]).max())
    bound = 3 * guard_ref.U * float(np.abs(ref["p"]).max()) * ref["good_steps"]
    print(f"closed form vs torch CPU fp32: max abs {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_closed_form_without_scaler_or_clipping_is_plain_adamw():
    """Scale 1 that never changes and no clipping: the loop is torch.optim.AdamW itself (the oracle's adamw_update formula)."""
    import torch
    p0, grads = guard_ref.script(257, iters=4, poison=())
    ref = guard_ref.closed_form(p0, grads, init_scale=1.0, growth_factor=1.0, backoff_factor=1.0, growth_interval=2 ** 31 - 1, **guard_ref.HYPER)
    p = torch.nn.Parameter(torch.from_numpy(p0).double())
    opt = torch.optim.AdamW([p], **guard_ref.HYPER)
    for g in grads:
        p.grad = torch.from_numpy(g).double()
        opt.step()
    assert ref["scales"] == [1.0] * 4 and ref["good_steps"] == 4
    assert float(np.abs(p.detach().numpy() - ref["p"]).max()) < 1e-12
