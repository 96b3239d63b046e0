"""tests/train_kernel_ref.py held from three sides, without a GPU:

* each float64 reference equals torch's float64 autograd of the same operation (1e-12 relative);
* correct fp32 arithmetic on the GPU matrix's inputs (float32 accumulation in torch; the weight gradient through the reference's own
  contraction run in float32, which the first point holds to autograd, the GroupNorm backward written down a second time) stays
  below 0.1 of the bound -- the bf16 `out` tensor before its rounding (after it: at most 1, the half ulp is the bound's main part), and
  its elementwise fp32 error, which no sum averages out, below half of what is charged for it;
* each deliberately wrong result -- the bug classes the bounds exist for -- exceeds the bound on at least 90 % of the outputs it changes
  (gstat: on more than half of the groups, a group's mean can cancel), with DSILU at its cap 2^-18.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import train_kernel_ref as R

MIN_SHARE = 0.9


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def share(wrong, ref, bound, rounded=False):
    """share of the changed outputs on which the wrong result is outside the bound, and the median excess there"""
    changed = wrong != ref
    assert changed.any()
    ratio = ((R.bf16(wrong) if rounded else wrong) - ref).abs()[changed] / bound[changed]
    return float((ratio > 1).double().mean()), float(ratio.median())


# ---- the references are the operations they claim to be ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["C3S1", "C3S2", "CT4", "STEM"])
def test_wgrad_reference_is_autograd(kind):
    gen = torch.Generator("cpu").manual_seed(1)
    B, Hin, Win, Cin, Cout = 2, 6, 10, 8, 16
    Hout, Wout, _, _, _ = R.wgrad_geom(kind, B, Hin, Win)
    x = torch.randn((B, Hin, Win, Cin), generator=gen, dtype=torch.float64)
    dy = torch.randn((B, Hout, Wout, Cout), generator=gen, dtype=torch.float64)
    ref, S, flip = R.wgrad_ref(kind, x, dy)
    xn, dyn = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
    if kind == "CT4":
        w = torch.zeros((Cin, Cout, 4, 4), dtype=torch.float64, requires_grad=True)
        out = F.conv_transpose2d(xn, w, stride=2, padding=1)
    elif kind == "STEM":
        w = torch.zeros((Cout, Cin, 1, 1), dtype=torch.float64, requires_grad=True)
        out = F.conv2d(xn, w)
    else:
        w = torch.zeros((Cout, Cin, 3, 3), dtype=torch.float64, requires_grad=True)
        out = F.conv2d(xn, w, stride=2 if kind == "C3S2" else 1, padding=1)
    assert out.shape == dyn.shape
    (out * dyn).sum().backward()
    assert rel(ref.reshape(w.shape), w.grad) < 1e-12
    assert float(flip.abs().max()) == 0 and bool((S >= ref.abs() * (1 - 1e-12)).all())


def test_wgrad_reference_operand_is_the_activated_input():
    """with a table the gradient is that of conv(bf16(silu(a x + c))), the padding staying zero"""
    gen = torch.Generator("cpu").manual_seed(2)
    x = R.rand_bf16((2, 5, 7, 8), gen)
    dy = R.rand_bf16((2, 5, 7, 8), gen)
    a, c = torch.rand((2, 8), generator=gen, dtype=torch.float64) + 0.5, torch.randn((2, 8), generator=gen, dtype=torch.float64)
    for silu in (True, False):
        ref, _, flip = R.wgrad_ref("C3S1", x, dy, (a, c), silu)
        z = x * a[:, None, None] + c[:, None, None]
        A = R.bf16(F.silu(z) if silu else z)
        w = torch.zeros((8, 8, 3, 3), dtype=torch.float64, requires_grad=True)
        (F.conv2d(A.permute(0, 3, 1, 2), w, padding=1) * dy.permute(0, 3, 1, 2)).sum().backward()
        assert rel(ref, w.grad) < 1e-12 and bool((flip >= 0).all())


@pytest.mark.parametrize("silu,form", [(1, "film"), (0, "film"), (1, "addend"), (0, "plain")])
def test_gn_bwd_reference_is_autograd(silu, form):
    """F = y1 (1 + s) + shift; A = act(GroupNorm(F)); L = sum A dA (+ sum y1 addend)"""
    gen = torch.Generator("cpu").manual_seed(3)
    B, HW, C, G = 2, 15, 16, 4
    r = lambda *s: torch.randn(s, generator=gen, dtype=torch.float64)
    y1, dA, add = r(B, HW, C).requires_grad_(), r(B, HW, C), r(B, HW, C)
    gamma, beta = (1 + 0.3 * r(C)).requires_grad_(), r(C).requires_grad_()
    s, sh = (0.3 * r(B, C)).requires_grad_(), r(B, C).requires_grad_()
    Fx = y1 * (1 + s[:, None]) + sh[:, None] if form == "film" else y1 * 1.0
    Fx.retain_grad()
    gn = F.group_norm(Fx.permute(0, 2, 1), G, gamma, beta, eps=1e-5).permute(0, 2, 1)
    L = ((F.silu(gn) if silu else gn) * dA).sum()
    if form == "addend":
        L = L + (y1 * add).sum()
    L.backward()
    with torch.no_grad():
        xs = Fx.reshape(B, HW, G, C // G).permute(0, 2, 1, 3).reshape(B, G, -1)
        mu, rs = xs.mean(2), 1 / torch.sqrt(xs.var(2, unbiased=False) + 1e-5)
        a = gamma[None] * rs.repeat_interleave(C // G, 1)
        c = beta[None] - mu.repeat_interleave(C // G, 1) * a
        val, bnd, _ = R.gn_bwd_ref(Fx.detach(), dA, a, c, mu, rs, gamma.detach(), G, silu, add if form == "addend" else None,
                                   (s.detach(), sh.detach()) if form == "film" else None)
    assert rel(val["dgamma"], gamma.grad) < 1e-12 and rel(val["dbeta"], beta.grad) < 1e-12
    assert rel(val["out"], y1.grad) < 1e-12
    assert rel(val["dbias"], y1.grad.sum((0, 1))) < 1e-12             # the bias of the conv that produced y1
    if form == "film":
        assert rel(val["dfilm"], torch.cat([s.grad, sh.grad], 1)) < 1e-12
    assert all(bool((b > 0).all()) for b in bnd.values())


def test_geometry_restatement():
    assert R.gn_bwd_geom(2, 45 * 41, 128) == dict(nslb=16, pstep=16, ppb=16, nblk=116, zblocks=1, iters=1)
    assert R.gn_bwd_geom(16, 1024, 128)["iters"] == 2
    g = R.gn_bwd_geom(3, 480, 192)
    assert (g["nslb"], g["pstep"]) == (24, 10)
    assert R.gn_bwd_geom(2, 240, 384)["pstep"] == 5 and R.gn_bwd_geom(2, 400, 48)["pstep"] == 42
    assert R.gn_bwd_geom(1, 32, 3072)["zblocks"] == 2 and R.gn_bwd_geom(1, 3, 128)["nblk"] == 1
    assert R.finalize_ygrid(5 * 116) == 8 and R.finalize_ygrid(1 * 4) == 1
    assert R.DSILU <= R.DSILU_CAP == R.SILU_REL


# ---- correct fp32 arithmetic stays inside -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(R.WGRAD_CASES))
def test_wgrad_fp32_accumulation_is_inside_the_bound(cid):
    d = R.wgrad_inputs(cid)
    kind, B, Hin, Win = R.WGRAD_CASES[cid][:4]
    tiles = R.wgrad_geom(kind, B, Hin, Win)[4]
    ref, S, flip = R.wgrad_ref(d["kind"], d["x"], d["dy"], d["ab"], d["silu"], d["Civ"], d["Cov"])
    A, _ = R.wgrad_operand(d["x"], d["ab"], d["silu"])
    emu = R.wgrad_crop(kind, R.wgrad_contract(kind, A.float(), d["dy"].float()), d["Civ"], d["Cov"])
    got = (d["g0"].float() + emu).double()
    for ns in (1, tiles):
        bound = R.wgrad_bound(ref, S, flip, d["g0"], tiles, ns)
        ratio = float(((got - (d["g0"] + ref)).abs() / bound).max())
        print(f"wgrad {cid} nsplit {ns}: fp32 accumulation at {ratio:.4f} of the bound")
        assert ratio < 0.1


def gn_plain(dt, acc, x, dA, a, c, mu, rs, gamma, G, silu, addend, film, dgamma0, dbeta0, dbias0):
    """the same operation written down once more: elementwise arithmetic in dtype `dt`; the sums over a sample's pixels in `acc`, arranged
    as the kernels arrange them (a sum per pixel block, every RL-th block row added up by one lane, the lanes in double)"""
    B, HW, C = x.shape
    cpg = C // G
    geo = R.gn_bwd_geom(B, HW, C)
    t = lambda v: None if v is None else v.to(dt)

    def sum_(v, RL):
        nblk, ppb = geo["nblk"], geo["ppb"]
        K = math.ceil(nblk / RL)
        v = F.pad(v.to(acc), (0, 0, 0, nblk * ppb - HW)).reshape(B, nblk, ppb, C).sum(2)
        return F.pad(v, (0, 0, 0, K * RL - nblk)).reshape(B, K, RL, C).sum(1).double().sum(1).to(dt)
    RL1 = 256 // (64 if cpg >= 64 else (32 if cpg >= 32 else 16))
    x, dA, a, c, mu, rs, gamma, addend = map(t, (x, dA, a, c, mu, rs, gamma, addend))
    mub, rsb = mu.repeat_interleave(cpg, 1)[:, None], rs.repeat_interleave(cpg, 1)[:, None]
    da = dA
    if silu:
        y = x * a[:, None] + c[:, None]
        sg = torch.sigmoid(y)
        da = dA * (sg * (1 + y * (1 - sg)))
    xh = (x - mub) * rsb
    s1, s2 = sum_(da, RL1), sum_(da * xh, RL1)
    m1 = (gamma * s1).reshape(B, G, cpg).sum(2) / (cpg * HW)
    m2 = (gamma * s2).reshape(B, G, cpg).sum(2) / (cpg * HW)
    dx = a[:, None] * da - rsb * (m1.repeat_interleave(cpg, 1)[:, None] + xh * m2.repeat_interleave(cpg, 1)[:, None])
    out = {"dgamma": (t(dgamma0).to(acc) + s2.to(acc).sum(0)).to(dt), "dbeta": (t(dbeta0).to(acc) + s1.to(acc).sum(0)).to(dt),
           "gstat": torch.stack([m1, m2], 2)}
    if film is not None:
        sc, sft = 1 + t(film[0]), t(film[1])
        out["out"] = dx * sc[:, None]
        p1, p2 = sum_(dx, 16), sum_(dx * x, 16)
        out["dfilm"] = torch.cat([(p2 - sft * p1) / sc, p1], 1)
        out["dbias"] = (t(dbias0).to(acc) + (sc * p1).to(acc).sum(0)).to(dt)
    else:
        out["out"] = dx + addend if addend is not None else dx
        out["dbias"] = (t(dbias0).to(acc) + sum_(out["out"], 16 * R.finalize_ygrid(B * geo["nblk"])).to(acc).sum(0)).to(dt)
    return {k: v.double() for k, v in out.items()}


@pytest.mark.parametrize("cid", list(R.GN_CASES))
def test_gn_bwd_fp32_arithmetic_is_inside_the_bound(cid):
    # 0.1 everywhere but one output.  Case 7 adds 32 pixels per channel in four chains of 8 fp32 adds, each add charged a full rounding, and
    # dgamma's terms da xhat are heavy-tailed: where one term carries the sum the roundings do not average out, and the unluckiest of
    # 3072 channels reaches 0.1225 (without SiLU) with arithmetic that is correct.  Every other output of case 7 is at or below 0.052.
    limits = {(7, "dgamma"): 0.15}
    for silu, form, _, _ in R.gn_combos(cid):
        d = R.gn_inputs(cid, form)
        val, bnd, mid = R.gn_bwd_ref(silu=silu, **d)
        exact = gn_plain(torch.float64, torch.float64, silu=silu, **d)
        emu = gn_plain(torch.float64, torch.float32, silu=silu, **d)     # float32 accumulation of exact terms
        full = gn_plain(torch.float32, torch.float32, silu=silu, **d)    # every elementwise result rounded to float32 as well
        for k in val:
            assert rel(exact[k], val[k]) < 1e-11, k
            ratio = float(((emu[k] - val[k]).abs() / bnd[k]).max())
            # elementwise roundings do not average out where one term dominates a short sum (32 pixels in case 7): half the bound
            assert float(((full[k] - val[k]).abs() / (mid["e_out"] if k == "out" else bnd[k])).max()) < 0.5, k
            if k == "out":
                assert float(((R.bf16(full[k]) - val[k]).abs() / bnd[k]).max()) <= 1.0
            print(f"gn_bwd case {cid} silu {silu} {form} {k}: fp32 arithmetic at {ratio:.4f} of the bound")
            assert ratio < limits.get((cid, k), 0.1), (k, ratio)


@pytest.mark.parametrize("cid", list(R.COLSUM_CASES))
def test_colsum_fp32_accumulation_is_inside_the_bound(cid):
    dy, db0 = R.colsum_inputs(cid)
    ref, bound = R.colsum_ref(dy, db0)
    assert rel(ref, db0 + dy.sum((0, 1))) < 1e-15
    got = (db0.float() + dy.float().sum((0, 1))).double()
    assert float(((got - ref).abs() / bound).max()) < 0.1


# ---- wrong results leave ------------------------------------------------------------------------------------------------------------------
def _wgrad_b():
    d = R.wgrad_inputs("b")
    ref, S, flip = R.wgrad_ref("C3S1", d["x"], d["dy"])
    tiles = R.wgrad_geom("C3S1", 2, 10, 40)[4]
    assert tiles == 12
    return d, ref, R.wgrad_bound(ref, S, flip, d["g0"], tiles, 5)


@pytest.mark.parametrize("wrong", ["partial tile", "full tile", "halo replicated"])
def test_wrong_weight_gradients_leave_the_bound(wrong):
    d, ref, bound = _wgrad_b()
    dy = d["dy"].clone()
    if wrong == "partial tile":
        dy[1, 8:10, 32:40] = 0                                          # the 2 x 8 corner tile of the last sample
        bad = R.wgrad_contract("C3S1", d["x"], dy)
    elif wrong == "full tile":
        dy[0, 0:4, 0:32] = 0
        bad = R.wgrad_contract("C3S1", d["x"], dy)
    else:
        bad = R.wgrad_contract("C3S1", d["x"], dy, pad_mode="replicate")
    s, med = share(bad, ref, bound)
    print(f"{wrong}: outside the bound on {100 * s:.1f} % of the changed outputs, median {med:.0f} bounds")
    assert s >= MIN_SHARE


def test_halo_of_activated_zeros_leaves_the_bound():
    """case g: a border pixel that receives SiLU(GN(0)) = silu(c) instead of 0"""
    d = R.wgrad_inputs("g")
    ref, S, flip = R.wgrad_ref("C3S1", d["x"], d["dy"], d["ab"], True)
    tiles = R.wgrad_geom("C3S1", 2, 10, 40)[4]
    ns = 8
    bound = R.wgrad_bound(ref, S, flip, d["g0"], tiles, ns)
    Ap, _ = R.wgrad_operand(F.pad(d["x"], (0, 0, 1, 1, 1, 1)), d["ab"], True)
    bad = R.wgrad_contract("C3S1", Ap, d["dy"], pad_mode="given")
    s, med = share(bad, ref, bound)
    print(f"activated halo: outside the bound on {100 * s:.1f} % of the changed outputs, median {med:.0f} bounds")
    assert s >= MIN_SHARE


@pytest.mark.parametrize("axis", [1, 2])
def test_swapped_convtranspose_parities_leave_the_bound(axis):
    d = R.wgrad_inputs("h")
    ref, S, flip = R.wgrad_ref("CT4", d["x"], d["dy"])
    tiles = R.wgrad_geom("CT4", 2, 6, 40)[4]
    bound = R.wgrad_bound(ref, S, flip, d["g0"], tiles, 3)
    idx = torch.arange(d["dy"].shape[axis]) ^ 1
    bad = R.wgrad_contract("CT4", d["x"], d["dy"].index_select(axis, idx))
    s, med = share(bad, ref, bound)
    print(f"parity swapped along axis {axis}: outside on {100 * s:.1f} %, median {med:.0f} bounds")
    assert s >= MIN_SHARE


def _gn(cid, form, silu=1):
    d = R.gn_inputs(cid, form)
    val, bnd, mid = R.gn_bwd_ref(silu=silu, dsilu_rel=R.DSILU_CAP, **d)
    return d, val, bnd, mid


def _gstat(d, s1, s2):
    B, C = s1.shape
    G = d["G"]
    cnt = (C // G) * d["x"].shape[1]
    return torch.stack([(d["gamma"] * s1).reshape(B, G, -1).sum(2) / cnt, (d["gamma"] * s2).reshape(B, G, -1).sum(2) / cnt], 2)


def test_pass1_without_the_partial_last_block_leaves_the_bound():
    d, val, bnd, mid = _gn(1, "addend")
    g = mid["geom"]
    cut = (g["nblk"] - 1) * g["ppb"]
    assert d["x"].shape[1] - cut == 5
    da, xh = mid["da"][:, :cut], mid["xh"][:, :cut]
    s1, s2 = da.sum(1), (da * xh).sum(1)
    for k, bad in (("dbeta", d["dbeta0"] + s1.sum(0)), ("dgamma", d["dgamma0"] + s2.sum(0))):
        s, med = share(bad, val[k], bnd[k])
        print(f"pass 1 without the 5-pixel tail, {k}: outside on {100 * s:.1f} %, median {med:.0f} bounds")
        assert s >= MIN_SHARE
    s, med = share(_gstat(d, s1, s2), val["gstat"], bnd["gstat"])
    print(f"pass 1 without the 5-pixel tail, gstat: outside on {100 * s:.1f} %, median {med:.1f} bounds")
    assert s > 0.5


@pytest.mark.parametrize("cid", [3, 4])
def test_finalize_without_the_partial_channel_slab_leaves_the_bound(cid):
    """cpg 24 at CL 16 and cpg 48 at CL 32: channels past the first slab of every group never reach dgamma / dbeta / gstat"""
    d, val, bnd, mid = _gn(cid, "plain")
    C = d["x"].shape[2]
    cpg = C // d["G"]
    CL = 32 if cpg >= 32 else 16
    keep = (torch.arange(C) % cpg) < CL
    s1, s2 = mid["da"].sum(1) * keep, (mid["da"] * mid["xh"]).sum(1) * keep
    for k, bad in (("dbeta", d["dbeta0"] + s1.sum(0)), ("dgamma", d["dgamma0"] + s2.sum(0))):
        s, med = share(bad, val[k], bnd[k])
        assert s >= MIN_SHARE, (k, s)
    s, med = share(_gstat(d, s1, s2), val["gstat"], bnd["gstat"])
    print(f"finalize without the second slab (cpg {cpg}), gstat: outside on {100 * s:.1f} %, median {med:.1f} bounds")
    assert s > 0.5


@pytest.mark.parametrize("wrong", ["no addend", "no 1 + scale", "tail left as dA"])
def test_wrong_apply_pass_leaves_the_bound(wrong):
    d, val, bnd, mid = _gn(1, "film" if wrong == "no 1 + scale" else "addend")
    if wrong == "no addend":
        bad = val["out"] - d["addend"]
    elif wrong == "no 1 + scale":
        bad = mid["dx"]
    else:
        g = mid["geom"]
        bad = val["out"].clone()
        bad[:, (g["nblk"] - 1) * g["ppb"]:] = d["dA"][:, (g["nblk"] - 1) * g["ppb"]:]
    s, med = share(bad, val["out"], bnd["out"], rounded=True)
    print(f"{wrong}: outside on {100 * s:.1f} % of the changed outputs, median {med:.0f} bounds")
    assert s >= MIN_SHARE
