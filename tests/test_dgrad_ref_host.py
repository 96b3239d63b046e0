"""tests/dgrad_ref.py held from two sides, without a GPU, on the operands of the GPU matrix (tests/test_gpu_dgrad.py):

(a) correct arithmetic -- float32 accumulation (torch's float32 gradient of the same forward op) with the route's bf16 roundings -- stays
    inside the bound, and the float32 accumulation alone uses little of the accumulation term;
(b) each deliberately wrong result, the bug classes the bound exists for, exceeds the bound on at least MIN_VIOLATED = 0.5 of the
    outputs it changes (the constant and the criterion of tests/test_gpu_layer_replay.py).  The shares are printed; docs/EXPERIMENTS.md
    R20 records them.

The reference itself is torch.autograd through the forward op, so there is nothing to hold it to but that it is linear and that its
scale S dominates it.
"""
import pytest
import torch

import dgrad_ref as R

_REF = {}


def reference(cid):
    if cid not in _REF:
        w, dy, res = R.inputs(cid)
        acc, S, ref = R.dgrad_ref(R.CASES[cid]["kind"], w, dy, res)
        _REF[cid] = dict(w=w, dy=dy, res=res, acc=acc, S=S, ref=ref)
    return _REF[cid]


def bound_of(cid, d):
    c = R.CASES[cid]
    return R.dgrad_bound(c["kind"], c["kernel"], d["w"], d["acc"], d["S"], d["res"], c["dtype"] == "bf16")


def test_cases_are_the_issue_matrix():
    """every kind on every kernel it can run on, with and without the residual where the step has one, and both types"""
    seen = {(c["kind"], c["kernel"], c["th"], c["dtype"]) for c in R.CASES.values()}
    assert {("C3S1", "pr", 8, "bf16"), ("C3S1", "pr", 4, "bf16"), ("C3S1", "fr", 8, "bf16"), ("C3S1", "ws", 4, "bf16"), ("C3S1", "igemm", 4, "bf16"),
            ("C3S2", "pr", 8, "bf16"), ("C3S2", "ws", 4, "bf16"), ("C3S2", "fr", 8, "bf16"), ("C3S2", "igemm", 4, "bf16"),
            ("CT4", "pr", 8, "bf16"), ("CT4", "igemm", 4, "bf16"), ("HEAD", "stem2", 4, "bf16"), ("HEAD", "igemm", 4, "bf16"),
            ("C3S1", "igemm", 4, "fp32"), ("C3S2", "igemm", 4, "fp32")} == seen
    assert all(c["kind"] == "C3S2" for c in R.CASES.values() if c["res"])            # the step adds dskip there and nowhere else
    assert set(R.HOST_CASES) <= set(R.CASES)
    for cid in ("c3_pr8", "c3_pr4", "s2_pr8", "ct_pr8_n2"):                          # the persistent kernel's forms on tiles ragged on both edges
        c = R.CASES[cid]
        MH, MW = (c["H"] // 2, c["W"] // 2) if c["kind"] == "CT4" else (c["H"], c["W"])
        assert MH % c["th"] and MW % 32, cid


@pytest.mark.parametrize("kind", ["C3S1", "C3S2", "CT4", "HEAD"])
def test_reference_is_the_gradient_of_the_forward_op(kind):
    """<conv(x, w), dy> = <x, dgrad(dy)> for a random x; S >= |acc|"""
    gen = torch.Generator("cpu").manual_seed(7)
    r = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)
    w = r(5, 6, 4, 4) if kind == "CT4" else r(6, 5, 3, 3)
    Cin = 5
    dy = r(2, 6, 6, 10)
    acc, S, ref = R.dgrad_ref(kind, w, dy, None)
    x = r(2, Cin, *R.dx_hw(kind, 6, 10))
    lhs, rhs = float((R.forward_op(kind, x, w) * dy).sum()), float((x * acc).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    assert ref is acc and bool((S >= acc.abs() * (1 - 1e-12)).all())


@pytest.mark.parametrize("cid", R.HOST_CASES)
def test_correct_arithmetic_is_inside_the_bound(cid):
    c, d = R.CASES[cid], reference(cid)
    bf = c["dtype"] == "bf16"
    bound = bound_of(cid, d)
    assert bool((bound > 0).all())
    got = R.emulate(c["kind"], c["kernel"], d["w"], d["dy"], d["res"], bf)
    ratio = float(((got - d["ref"]).abs() / bound).max())
    acc32 = R.dgrad(c["kind"], d["w"].float(), d["dy"].float()).double()
    e_acc = R.k_summed(c["kind"], d["w"]) * R.U32 * d["S"]
    racc = float(((acc32 - d["acc"]).abs() / e_acc.clamp_min(1e-300)).max())
    print(f"dgrad host {cid} ({c['kind']} {c['kernel']} {c['dtype']}): correct arithmetic at {ratio:.3f} of the bound; float32 accumulation alone at {racc:.3f} of K 2^-24 S")
    assert ratio <= 1.0 and racc <= 1.0


@pytest.mark.parametrize("cid", R.HOST_CASES)
def test_wrong_results_are_outside_the_bound(cid):
    c, d = R.CASES[cid], reference(cid)
    bf = c["dtype"] == "bf16"
    bound = bound_of(cid, d)
    wrong = R.wrong_results(cid, d["w"], d["dy"], d["res"], d["acc"])
    expect = {"taps_transposed", "ragged_block_zero"}
    expect |= {"C3S1": {"taps_not_flipped"}, "HEAD": {"taps_not_flipped"}, "CT4": {"p4_planes_swapped_rows", "p4_planes_swapped_cols"},
               "C3S2": {"pad4_wrong_corner", "pad4_wrong_corner_rows", "parities_swapped_rows", "parities_swapped_cols"}}[c["kind"]]
    expect |= ({"res_omitted"} if c["res"] else set()) | ({"pad_channels_leak"} if c["Cin"] == 192 else set())
    assert set(wrong) == expect
    weak = {}
    for name, v in wrong.items():
        assert v.shape == d["ref"].shape
        changed = v != d["ref"]
        assert bool(changed.any()), name
        stored = R.bf16(v) if bf else v.float().double()                          # the wrong value goes through the store as well
        ratio = (stored - d["ref"]).abs()[changed] / bound[changed]
        sh, med = float((ratio > 1).double().mean()), float(ratio.median())
        print(f"dgrad host {cid} {name}: outside the bound on {sh:.4f} of {int(changed.sum())} changed outputs, median excess {med:.1f}")
        if sh < R.MIN_VIOLATED:
            weak[name] = sh
    assert not weak, weak
