"""Host checks of the fused MSE + L1 + TV objective: the C ABI declares it, ``train_step`` takes the weights, and the closed form the
GPU tests use as their yardstick (tests/objective_ref.py) is pinned to the reference's own fp32 autograd run (the fixture
tests/golden/train_objective.npz, written by tests/golden/make_objective_golden.py from the reference's modules).

Measured on the fixture (worst over all elements, in units of the bound): reference gradient against the float64 closed form 0.24
of K U S with K = 10 (2.39 with K = 1); loss terms of the reference within 1.2 U relative of the float64 terms.
"""
import inspect
import re
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))
import objective_ref as R  # noqa: E402

from clip_feature_codec import _native  # noqa: E402

HEADER = HERE.parent / "include" / "ccn_hip.h"
GOLD = np.load(HERE / "golden" / "train_objective.npz")


def test_header_and_signatures_declare_the_objective_entry_point():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    m = re.search(r"int\s+ccn_diffusion_loss_grad\s*\(([^;]*)\)\s*;", text)
    assert m, "ccn_diffusion_loss_grad is not declared in include/ccn_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 16
    assert "ccn_diffusion_loss_grad" in _native.SIGNATURES
    restype, argtypes = _native.SIGNATURES["ccn_diffusion_loss_grad"]
    assert len(argtypes) == 16 and restype is _native.c_i32
    assert [argtypes[i] for i in (6, 7, 8, 9)] == [_native.c_i32] * 4 and [argtypes[i] for i in (10, 11)] == [_native.c_f32] * 2
    assert "ccn_mse_loss_grad" in _native.SIGNATURES          # the MSE-only entry point stays


def test_closed_form_reproduces_the_reference_mask_gradient_and_loss_terms():
    recon_w, tv_w = (float(v) for v in GOLD["weights"])
    assert (recon_w, tv_w) == (0.05, 1e-4)
    cf = R.closed_form(GOLD["eps_hat"], GOLD["noise"], GOLD["raw"], GOLD["x0"], GOLD["a"], GOLD["s"], recon_w, tv_w)
    # the mask of the reference's fp32 raw, exactly
    assert np.array_equal(cf["mask"], GOLD["mask"])
    share = cf["mask"].reshape(cf["mask"].shape[0], -1).mean(axis=1)
    assert (share > 0.9).sum() >= 2 and ((share > 0.1) & (share < 0.9)).sum() >= 1 and (share == 0).sum() >= 1     # not blind
    # the reference's fp32 autograd gradient, element by element within K U S (objective_ref.K: the count of roundings)
    ratio = R.worst_ratio(GOLD["d_eps"], cf)
    rel = float(np.max(np.abs(GOLD["d_eps"] - cf["d_eps"]) / np.maximum(np.abs(cf["d_eps"]), 1e-300)))
    print(f"reference fp32 autograd vs float64 closed form: worst |err| / (K U S) = {ratio:.3f} (K = {R.K}), worst relative {rel:.2e}")
    assert ratio <= 1.0, ratio
    # where the clamp cuts the gradient the auxiliary part is exactly absent in the reference too
    g_mse32 = (2.0 * (GOLD["eps_hat"].astype(np.float64) - GOLD["noise"]) / GOLD["noise"].size)
    assert np.all(np.abs(GOLD["d_eps"][~cf["mask"]] - g_mse32[~cf["mask"]]) <= 3 * R.U * np.abs(g_mse32[~cf["mask"]]))
    # loss terms: the reference sums n non-negative fp32 values, each carrying up to 3 roundings (difference, square or abs, the
    # weight), in torch's blocked pairwise order, whose depth is at most ceil(log2 n) + 1, and rounds the mean once
    n = GOLD["noise"].size
    bound = (3 + np.ceil(np.log2(n)) + 1 + 1) * R.U
    rel_terms = np.abs(GOLD["loss_terms"].astype(np.float64) - cf["terms"]) / cf["terms"]
    print(f"reference loss terms vs float64: relative error / U = {rel_terms / R.U} (bound {bound / R.U:.0f} U)")
    assert np.all(rel_terms <= bound), rel_terms / R.U


def test_train_step_accepts_the_objective_weights():
    from clip_feature_codec.train.diffusion_train import train_step, train_diffusion
    sig = inspect.signature(train_step)
    assert sig.parameters["recon_w"].default == 0.0 and sig.parameters["tv_w"].default == 0.0
    sig = inspect.signature(train_diffusion)
    assert sig.parameters["fused_objective"].default is True
    assert sig.parameters["recon_w"].default == 0.05 and sig.parameters["tv_w"].default == 1e-4 and sig.parameters["clip_w"].default == 0.1
