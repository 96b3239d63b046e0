"""Shapes and the recording run shared by tests/golden/make_train_plan_golden.py and tests/test_gpu_train_plan.py.

Per case: ``ccn_train_workspace_bytes`` and the text of ``ccn_internal_train_routes`` after one forward + backward on a NativeTrainer, once
with the plain and once with the bucketed backward.  Route decisions and sizes depend on the shape alone, so the parameters and inputs are
seeded noise.
"""
from __future__ import annotations

import ctypes

import torch

from clip_feature_codec import _native

DEV = "cuda:0"
TIME_DIM = 256

# id -> (dtype, base, ch_mult, B, H, W, conv variant or None, run a step)
CASES = {
    # the six fp32 shapes of tests/test_gpu_train_routes.py::CASES
    "fp32-A": ("fp32", 128, (1, 2), 4, 128, 128, None, True),
    "fp32-B": ("fp32", 128, (1, 2), 5, 100, 136, None, True),
    "fp32-C": ("fp32", 64, (1, 2), 2, 136, 200, None, True),
    "fp32-D": ("fp32", 64, (1, 2), 2, 144, 256, None, True),
    "fp32-E": ("fp32", 64, (1, 2), 4, 128, 128, None, True),
    "fp32-F": ("fp32", 192, (1, 2), 2, 128, 128, None, True),
    "bf16-128-2x32x32": ("bf16", 128, (1, 2), 2, 32, 32, None, True),          # 4-row tiles, statistics inside the conv
    "bf16-128-4x136x200": ("bf16", 128, (1, 2), 4, 136, 200, None, True),      # stride-2 conv and ConvTranspose on the persistent kernel
    "bf16-128-4x136x200-v3": ("bf16", 128, (1, 2), 4, 136, 200, 3, True),      # the same with the persistent kernel switched off
    "bf16-48-2x32x32": ("bf16", 48, (1, 2), 2, 32, 32, None, True),            # no fragment operands anywhere
    "bf16-128-122-8x256x256": ("bf16", 128, (1, 2, 2), 8, 256, 256, None, False),
    "bf16-192-1224-2x128x128": ("bf16", 192, (1, 2, 2, 4), 2, 128, 128, None, False),
}


def library():
    lib = _native.load_library()
    lib.ccn_internal_train_routes.restype = ctypes.c_int
    lib.ccn_internal_train_routes.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    lib.ccn_internal_set_conv_variant.restype = ctypes.c_int
    lib.ccn_internal_set_conv_variant.argtypes = [ctypes.c_int]
    return lib


def routes(trainer) -> str:
    lib = library()
    n = lib.ccn_internal_train_routes(trainer.h, None, 0)
    assert n > 0
    buf = ctypes.create_string_buffer(n + 1)
    assert lib.ccn_internal_train_routes(trainer.h, buf, n + 1) == n
    return buf.value.decode()


def workspace_bytes(trainer, B, H, W) -> int:
    n = ctypes.c_size_t()
    _native.check(trainer.lib.ccn_train_workspace_bytes(trainer.h, B, H, W, ctypes.byref(n)))
    return int(n.value)


def step_inputs(trainer, B, H, W, seed=7):
    g = torch.Generator("cpu").manual_seed(seed)
    flat = (0.05 * torch.randn(trainer.total, generator=g)).to(DEV)
    x = torch.randn((B, 3, H, W), generator=g).to(DEV)
    z = torch.randn((B, 512), generator=g).to(DEV)
    t = torch.linspace(0, 999, B).round().long().to(DEV)
    d = (torch.randn((B, 3, H, W), generator=g) / (B * 3 * H * W)).to(DEV)
    return flat, x, z, t, d


def record(cid) -> dict:
    """{"bytes": .., "routes": .., "routes_bucketed": ..} of one case on a fresh trainer (the route texts only where a step is run)."""
    dtype, base, ch_mult, B, H, W, variant, step = CASES[cid]
    lib = library()
    old = lib.ccn_internal_set_conv_variant(variant) if variant is not None else None
    tr = None
    try:
        tr = _native.NativeTrainer(512, base, ch_mult, TIME_DIM, 3, dtype=dtype, device=DEV)
        out = {"bytes": workspace_bytes(tr, B, H, W)}
        if step:
            flat, x, z, t, d = step_inputs(tr, B, H, W)
            g = torch.zeros_like(flat)
            tr.forward(flat, x, z, t)
            tr.backward(flat, g, x, z, d)
            torch.cuda.synchronize()
            out["routes"] = routes(tr)
            tr.forward(flat, x, z, t)
            tr.backward(flat, g, x, z, d, bucket_cb=lambda lo, hi: None, bucket_floats=200_000)
            torch.cuda.synchronize()
            out["routes_bucketed"] = routes(tr)
            assert bool(torch.isfinite(g).all())
        return out
    finally:
        if tr is not None:
            tr.close()
        if old is not None:
            lib.ccn_internal_set_conv_variant(old)
        torch.cuda.empty_cache()


def bf16_coverage(texts) -> dict:
    """Launch forms in the union of route texts: the forms the comparison with the parent claims to cover."""
    words = [ln.split() for text in texts for ln in text.splitlines()]
    have = {f"norm {form}": any(w[:2] == ["norm", form] for w in words) for form in ("side-fused", "side-stats+act", "fused")}
    for kind in ("C3S1", "C3S2", "CT4"):
        for direction in ("fwd", "dgrad"):
            have[f"conv {direction} {kind} pr"] = any(w[:4] == ["conv", direction, kind, "pr"] for w in words)
    have["conv pr four=1"] = any(w[0] == "conv" and w[3] == "pr" and "four=1" in w for w in words)
    return have
