"""Shapes, the recording run and the route helpers shared by tests/golden/make_infer_plan_golden.py, tests/test_gpu_infer_plan.py and the
tests that read ``ccn_internal_plan_routes`` (tests/test_gpu_split.py, tests/test_gpu_layer_replay.py).

Per case: ``ccn_workspace_bytes``, the text of ``ccn_internal_plan_routes`` and both doubles of ``ccn_algorithmic_work``; for the cases
that run, SHA-256 of the output bytes of ``ccn_forward``, of ``ccn_sample`` launch by launch and as a graph (twice: capture and replay)
and, where the case asks for it, of ``ccn_sample_eta`` and ``ccn_resblock_forward``.  The inference kernels are run-to-run deterministic
(DESIGN.md section 5), so the hashes of one commit's library are the hashes of the next one's unless a launch, an argument or the order
changed.  Weights and inputs are key-seeded (utils/synth); the timestep / coefficient / sigma tables come with the fixture.
"""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np
import torch

from clip_feature_codec import _native
from clip_feature_codec.utils import synth

DEV = "cuda:0"
TIME_DIM = 256
ETA = 0.5

# id -> model (dtype, base, ch_mult, weight rounding), shape (B, H, W, steps), run or sizes-and-routes only, extras
CASES = {
    # the configuration of tests/test_gpu_plan_cache.py: persistent kernel with split-K; nine steps wrap the weight version index (i % 8)
    "bf16-128-122-1x32x32-s9": dict(model=("bf16", 128, (1, 2, 2), "phases"), shape=(1, 32, 32, 9), run=True),
    "bf16-128-122-2x64x64": dict(model=("bf16", 128, (1, 2, 2), "phases"), shape=(2, 64, 64, 3), run=True, eta=True, resblock="mid1"),
    "bf16-128-122-2x40x72": dict(model=("bf16", 128, (1, 2, 2), "phases"), shape=(2, 40, 72, 2), run=True),
    "bf16-48-12-2x32x32": dict(model=("bf16", 48, (1, 2), "phases"), shape=(2, 32, 32, 3), run=True),        # no fragment operands
    "fp32-32-12-2x32x32": dict(model=("fp32", 32, (1, 2), "phases"), shape=(2, 32, 32, 3), run=True),
    "fp32-128-12-2x32x32": dict(model=("fp32", 128, (1, 2), "phases"), shape=(2, 32, 32, 2), run=True),
    "f16x3-128-12-1x32x32": dict(model=("f16x3", 128, (1, 2), "phases"), shape=(1, 32, 32, 2), run=True),
    # 8-row tiles off the persistent kernel (64-wide layers): the free-running kernel
    "fp32-64-12-2x128x256": dict(model=("fp32", 64, (1, 2), "phases"), shape=(2, 128, 256, 2), run=True),
    # sizes and routes only, never launched by the test; committed with round-to-nearest weights (routes do not depend on the rounding)
    "bf16-128-122-8x256x256-s50": dict(model=("bf16", 128, (1, 2, 2), "nearest"), shape=(8, 256, 256, 50), run=False),
    "bf16-128-16-1x16x16": dict(model=("bf16", 128, (1, 6), "nearest"), shape=(1, 16, 16, 4), run=False),   # a 768-channel level
}

_handles = {}


def library():
    lib = _native.load_library()
    for name in ("ccn_internal_plan_routes", "ccn_internal_plan_layout", "ccn_internal_plan_routes_of"):
        if hasattr(lib, name):
            getattr(lib, name).restype = ctypes.c_int
    lib.ccn_internal_plan_routes.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    shape_hook = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p, ctypes.c_size_t]
    for name in ("ccn_internal_plan_layout", "ccn_internal_plan_routes_of"):
        if hasattr(lib, name):
            getattr(lib, name).argtypes = shape_hook
    return lib


def _report(fn, *args) -> str:
    n = fn(*args, None, 0)
    assert n > 0, n
    buf = ctypes.create_string_buffer(n + 1)
    assert fn(*args, buf, n + 1) == n
    return buf.value.decode()


def route_text(nat) -> str:
    """``ccn_internal_plan_routes``: one line per conv-family launch of the plan the handle's last forward / sample used."""
    return _report(library().ccn_internal_plan_routes, nat.h)


def route_text_of(nat, B, H, W, steps) -> str:
    """The same report for a shape, from its cached plan: nothing is bound or launched."""
    return _report(library().ccn_internal_plan_routes_of, nat.h, B, H, W, steps)


def layout_text(nat, B, H, W, steps) -> str:
    """``ccn_internal_plan_layout``: ``name off=.. bytes=..`` per workspace region of the shape's plan and a final ``total=..``."""
    return _report(library().ccn_internal_plan_layout, nat.h, B, H, W, steps)


def parse_routes(text) -> dict:
    out = {}
    for line in text.splitlines():
        f = line.split()
        r = dict(name=f[0], kind=f[1], kernel=f[2], **{k: v for k, v in (x.split("=") for x in f[3:])})
        for k in ("th", "ksplit", "n_nt", "film", "res"):
            r[k] = int(r[k])
        out[r["name"]] = r
    return out


def plan_routes(nat) -> dict:
    """{activation name: route dict} of the plan the handle's last forward / sample used."""
    return parse_routes(route_text(nat))


def handle(model):
    """One committed NativeUNet per model of CASES, kept for the process (close_handles)."""
    if model not in _handles:
        dtype, base, ch_mult, rounding = model
        nat = _native.NativeUNet(512, base, ch_mult, TIME_DIM, 3, dtype=dtype, device=DEV, weight_rounding=rounding)
        nat.load_state_dict(synth.synth_state_dict(synth.unet_param_spec(512, base, ch_mult, TIME_DIM)))
        _handles[model] = nat
    return _handles[model]


def close_handles() -> None:
    for nat in _handles.values():
        nat.close()
    _handles.clear()
    torch.cuda.empty_cache()


def workspace_bytes(nat, B, H, W, steps) -> int:
    n = ctypes.c_size_t()
    _native.check(nat.lib.ccn_workspace_bytes(nat.h, B, H, W, steps, ctypes.byref(n)))
    return int(n.value)


def digest(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _noise(n, ch, H, W, seed):
    """(n, ch, H, W) from synth.start_noise (square draws, cropped)."""
    return torch.from_numpy(np.ascontiguousarray(synth.start_noise(range(n), max(H, W), seed, img_ch=ch)[:, :, :H, :W])).to(DEV)


def inputs(cid):
    B, H, W, steps = CASES[cid]["shape"]
    z = torch.from_numpy(synth.synth_z(B, seed=77)).to(DEV)
    x = _noise(B, 3, H, W, 300)
    t = torch.linspace(0, 999, B).round().long().to(DEV)
    return z, x, t


def tables_bits(ts, coef5) -> dict:
    """The sampler's tables as the fixture stores them: int32 timesteps, the fp32 bit patterns of the (steps, 5) coefficient rows."""
    return {"ts": [int(v) for v in ts], "coef_bits": np.ascontiguousarray(coef5, np.float32).view(np.uint32).ravel().tolist()}


def tables_from_bits(tab):
    ts = np.asarray(tab["ts"], np.int32)
    coef5 = np.asarray(tab["coef_bits"], np.uint32).view(np.float32).reshape(len(ts), 5)
    return ts, coef5


def record(cid, tables=None, launch_for_routes=False) -> dict:
    """What the fixture holds for one case.  ``tables``: {"eta0": .., "eta": ..} of tables_bits (cases that run).
    ``launch_for_routes``: a library without ``ccn_internal_plan_routes_of`` reports the routes of a plan only after using it, so the
    fixture's make script runs one forward for the cases that the test never launches."""
    case = CASES[cid]
    B, H, W, steps = case["shape"]
    nat = handle(case["model"])
    f, b = nat.algorithmic_work(B, H, W)
    out = {"bytes": workspace_bytes(nat, B, H, W, steps), "work": [float(f).hex(), float(b).hex()]}
    z, x, t = inputs(cid)
    if not case["run"]:
        if launch_for_routes:
            nat.forward(x, z, t)
            torch.cuda.synchronize()
            out["routes"] = route_text(nat)
        else:
            out["routes"] = route_text_of(nat, B, H, W, steps)
        return out
    ts, coef5 = tables_from_bits(tables["eta0"])
    sha = {"forward": digest(nat.forward(x, z, t))}
    sha["sample"] = digest(nat.sample(z, x, ts, coef5[:, :4], use_graph=False))
    sha["sample_graph"] = [digest(nat.sample(z, x, ts, coef5[:, :4], use_graph=True)) for _ in range(2)]
    out["routes"] = route_text(nat)
    if case.get("eta"):
        ts_e, coef_e = tables_from_bits(tables["eta"])
        noise = _noise(steps * B, 3, H, W, 900).reshape(steps, B, 3, H, W).contiguous()
        sha["sample_eta"] = digest(nat.sample(z, x, ts_e, coef_e[:, :4], use_graph=False, sigma=coef_e[:, 4], noise=noise))
        sha["sample_eta_graph"] = [digest(nat.sample(z, x, ts_e, coef_e[:, :4], use_graph=True, sigma=coef_e[:, 4], noise=noise))
                                   for _ in range(2)]
    if case.get("resblock"):
        C = dict(nat.param_spec())[case["resblock"] + ".conv1.weight"][0]
        hb, wb = H >> 2, W >> 2                                    # (any grid: the block is planned on its own)
        xb = _noise(B, C, hb, wb, 500)
        cond = torch.from_numpy(synth.synth_z(B, dim=TIME_DIM, seed=88)).to(DEV)
        sha["resblock"] = digest(nat.resblock(case["resblock"], xb, cond))
    torch.cuda.synchronize()
    nat.poll_errors()
    out["sha256"] = sha
    return out


def coverage(cases: dict) -> dict:
    """Launch forms in the union of the fixture's route texts: the forms the comparison with the parent claims to cover.

    ``gn=preact`` (the GroupNorm + SiLU pass WITHOUT its finalize folded in) is not in the table: the release library takes it only for
    an input without partial sums, and every tensor a ResBlock of an inference plan reads has them (its producer is asked for them
    whenever a ResBlock or the head follows, ccn_resblock_forward makes its own); the diagnostics build's CCN_NO_FUSED_GNACT switch is
    the only way to that record, and no test loads that build."""
    lines = [ln.split() for c in cases.values() for ln in c["routes"].splitlines()]
    have = {f"gn={g}": any(f"gn={g}" in w for w in lines) for g in ("none", "prologue", "instat", "preact_fused", "weights")}
    for word in ("ksplit=2", "res=1", "film=1", "ops=f16x3", "ops=f32"):
        have[word] = any(word in w for w in lines)
    for kernel in ("igemm", "ws", "fr", "pr", "stem2", "head2"):
        have[f"kernel {kernel}"] = any(w[2] == kernel for w in lines)
    return have
