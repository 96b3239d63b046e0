"""Host-only self-check of tests/train_forward_ref.py, the harness of tests/test_gpu_train_forward.py.

The bf16 training forward is emulated on the CPU in float64 with the kernels' rounding points (test_gpu_layer_replay.ROUNDING:
round-to-nearest weights, the persistent kernel's bf16 staging before its fp32 epilogue, one pack at the store, fp32 tables from
statistics of the values BEFORE that pack), written into a synthetic workspace (train_forward_ref.pack_regions) with a synthetic route
report, and fed through the same reader, parser and checks as the GPU run.  Two emulations: T3 of the GPU file in the two-stage
pre-pass forms on the generic kernels, and a cut-down T1 (its channel counts at 36 x 40 pixels) in the in-conv forms on the persistent
kernel's rounding model with stem2 and head2.  They must pass; the three wrong references of every conv layer must be rejected on at
least MIN_VIOLATED of the outputs they change with the reference alone; and the further bug classes the GPU file exists for -- an
activated copy from statistics that count tile padding, an rstd off by 2^-10, a consistent (mean, rstd) pair off by 1e-3, a FiLM row
of the neighbouring ResBlock -- must fail.
"""
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))
import train_forward_ref as R  # noqa: E402

from oracle import ref_unet  # noqa: E402

LR = R.LR
TIME_DIM = 256
CH_MULT = (1, 2)
# id -> (base, B, H, W, style): "plain" = generic kernels (one pack), pre-pass norm forms, generic stem / head;
# "pr" = stem2, persistent kernel (bf16 staging, then the pack), in-conv norm forms, head2
EMU = {"T3": (48, 3, 40, 72, "plain"), "T1cut": (128, 2, 36, 40, "pr")}
_EMU = {}


def bf(x):
    return x.to(torch.bfloat16).double()


def f32(x):
    return x.float().double()


def tables_of(v, gamma, beta, G=8):
    """(mean, rstd, a, c) as gn_stats_kernel / gn_act_fused_kernel store them: float64 from the sums, rounded to fp32"""
    N, C = v.shape[:2]
    xs = v.reshape(N, G, -1)
    mean = xs.mean(2)
    rstd = 1.0 / torch.sqrt((xs * xs).mean(2) - mean * mean + 1e-5)
    sc = gamma[None, :] * rstd.repeat_interleave(C // G, 1)
    return f32(mean), f32(rstd), f32(sc), f32(beta[None, :] - mean.repeat_interleave(C // G, 1) * sc)


def emulate(cid):
    """{"items": [(region, tensor)], "routes": [lines], inputs ...} of one emulated forward"""
    if cid in _EMU:
        return _EMU[cid]
    from clip_feature_codec.utils import synth
    base, B, H, W, style = EMU[cid]
    pr = style == "pr"
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, CH_MULT))
    sd64 = ref_unet.as_torch_sd(sd, torch.float64)
    g = torch.Generator().manual_seed(5 + B)
    x_in = torch.randn((B, 3, H, W), generator=g)
    z = torch.from_numpy(synth.synth_z(B))
    t = torch.linspace(0, 999, B).round().long()
    lin = lambda v, k: F.linear(v, sd64[k + ".weight"], sd64[k + ".bias"])          # noqa: E731
    temb = ref_unet.timestep_embedding(t, TIME_DIM).double()
    t1 = f32(F.silu(lin(temb, "time_proj.0"))); tp = f32(lin(t1, "time_proj.2")); zpv = f32(F.silu(lin(z.double(), "z_proj.0")))
    h = f32(tp + zpv)
    layers = LR.layer_list(CH_MULT)
    blocks = [n for n, k, *_ in layers if k == "c1"]
    film = f32(torch.cat([lin(h, p + part) for p in blocks for part in (".to_scale", ".to_shift")], 1))
    items = [("temb", temb.float()), ("t1", t1.float()), ("tp", tp.float()), ("zpv", zpv.float()), ("h", h.float()), ("film", film.float())]
    routes, store, pre, foff, eps = [], {}, {}, 0, None
    kern = "pr" if pr else "igemm"

    def nhwc(v):
        return v.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)

    def conv_line(kind, kernel):
        return f"conv fwd {kind} {kernel} th={0 if kernel == 'head2' else 4} bn=128 n_nt=1 four=0"

    for i, (name, kind, inp, resn, wkey, nkey, fkey) in enumerate(layers):
        w32 = sd64[wkey + ".weight"].float().double()
        w, b = bf(w32), sd64[wkey + ".bias"][None, :, None, None]
        x = x_in.double() if kind == "stem" else store[inp]
        Hout = x.shape[2] * (2 if kind == "up" else 1) // (2 if kind == "down" else 1)
        region, _ = R.TrainSource.region_of(name)
        if nkey:
            gamma, beta = sd64[nkey + ".weight"], sd64[nkey + ".bias"]
            mean, rstd, a, c = tables_of(pre[inp], gamma, beta)
            prefix = "out_norm" if kind == "head" else region[:-2] + (".n1" if kind == "c1" else ".n2")
            a4, c4 = a[:, :, None, None], c[:, :, None, None]
        if kind == "stem":
            routes.append(conv_line("STEM", "stem2" if pr else "igemm"))
            acc = LR.conv_rows(kind, bf(x), w, 0, Hout)
            v = acc + (bf(b) if pr else b)                       # stem2: the bias is a bf16 K element; one pack of the accumulator
        elif kind in ("c1", "c2"):
            # the two-stage and the fused pre-pass compute the same copy; the in-conv forms redo the transform from fp32 statistics
            form = ("side-fused" if i % 3 else "side-stats+act") if pr else ("stats+act" if i % 3 else "fused")
            routes += [f"norm {form} slots=12", conv_line("C3S1", kern)]
            xa = bf(F.silu(x * a4 + c4))
            op = xa
            if pr:                                               # GnCoef<__bf16>::from_raw: fp32 products of fp32 statistics
                a2 = f32(gamma.float().double()[None, :] * rstd.repeat_interleave(a.shape[1] // 8, 1))
                c2 = f32(beta[None, :] - mean.repeat_interleave(a.shape[1] // 8, 1) * a2)
                op = bf(F.silu(x * a2[:, :, None, None] + c2[:, :, None, None]))
            items += [(region[:-2] + (".xa" if kind == "c1" else ".ya"), nhwc(xa))]
            acc = LR.conv_rows(kind, op, w, 0, Hout)
            if pr:
                acc = bf(acc)                                    # ROUNDING[("pr", 1)]: "acc", then "store"
            if kind == "c1":
                C = acc.shape[1]
                s, sh = film[:, foff:foff + C, None, None], film[:, foff + C:foff + 2 * C, None, None]
                foff += 2 * C
                v = (acc + b) * (1 + s) + sh
            else:
                v = acc + b + store[resn]
        elif kind in ("down", "up"):
            routes.append(conv_line("C3S2" if kind == "down" else "CT4", kern))
            acc = LR.conv_rows(kind, x, w, 0, Hout)
            if pr:
                acc = bf(acc)
            v = acc + b + (store[resn] if kind == "up" else 0.0)
        else:
            routes += ["norm prologue slots=12", conv_line("HEAD", "head2" if pr else "igemm")]
            if pr:                                               # head_prep_kernel: W' = bf16(a_b W) from the fp32 parameter, S = sum c_b W
                eps = torch.cat([LR.conv_rows(kind, x[n:n + 1], bf(a4[n][None] * w32), 0, Hout)
                                 + LR.conv_rows(kind, c4[n:n + 1] * torch.ones_like(x[n:n + 1]), w32, 0, Hout) for n in range(B)]) + b
            else:
                eps = LR.conv_rows(kind, bf(x * a4 + c4), w, 0, Hout) + b
            eps = eps.float()
        if nkey:
            items += [(prefix + ".ab", R.ab_pack(a, c)), (prefix + ".st", torch.stack([mean, rstd], 2).float())]
        if kind != "head":
            store[name], pre[name] = bf(v), f32(v)               # the statistics see the fp32 value, the next layer the stored one
            items.append((region, nhwc(store[name])))
    _EMU[cid] = dict(items=items, routes=routes, sd=sd, x=x_in, z=z, t=t, eps=eps, base=base, B=B, H=H, W=W, blocks=blocks)
    return _EMU[cid]


def regions_of(e, replace=None):
    items = [(n, (replace or {}).get(n, v)) for n, v in e["items"]]
    return R.Regions(*R.pack_regions(items))


def source_of(e, reg):
    recs = R.parse_routes(e["routes"], CH_MULT)
    samples = [0, e["B"] - 1]
    return R.TrainSource(reg, e["sd"], e["base"], CH_MULT, e["B"], e["H"], e["W"], e["x"].double()[samples], None, None, samples, recs), recs


_REPLAY = {}


def replayed(cid):
    if cid not in _REPLAY:
        e = emulate(cid)
        _REPLAY[cid] = R.replay(regions_of(e), e["routes"], e["sd"], e["base"], CH_MULT, e["B"], e["H"], e["W"], e["x"], e["z"], e["t"], e["eps"],
                                TIME_DIM, f"host emulation {cid}", rng_seed=3)
    return _REPLAY[cid]


@pytest.mark.parametrize("cid", list(EMU))
def test_emulated_forward_passes_every_check(cid):
    """Conv layers within the bound and the three wrong references rejected at MIN_VIOLATED; activated copies, tables and
    conditioning within theirs."""
    out = replayed(cid)
    assert len(out["rows"]) == 26 and len(out["acts"]) == 20 and len(out["tables"]) == 21
    LR.check_rows(out["rows"])
    assert all(r["viol"]["tap"] is not None for r in out["rows"])
    assert all(r["viol"]["shift"] is not None for r in out["rows"] if "head2" not in r["route"])   # (replay_layer's head2 branch has the tap only)
    R.check_act_rows(out["acts"])
    R.check_table_rows(out["tables"])
    R.check_cond_rows(out["cond"])
    # the checks are not vacuous: the store rounding uses most of the conv bound, the flip width is reached
    assert max(r["ratio"] for r in out["rows"]) > 0.4
    if EMU[cid][4] == "pr":
        assert any(r["viol"]["gnpad"] is not None for r in out["rows"])
    assert all(r["gnpad"] is not None for r in out["acts"])


@pytest.mark.parametrize("cid", list(EMU))
def test_activated_copy_from_padded_statistics_fails(cid):
    e = emulate(cid)
    base, H, W = e["base"], e["H"], e["W"]
    items = dict(e["items"])
    x = items["in_conv.o"].double().permute(0, 3, 1, 2)
    gamma, beta = (R.f64(e["sd"]["down.0.norm1." + k]) for k in ("weight", "bias"))
    a, c = LR.gn_affine(x, gamma, beta, 8, pad_hw=(-(-H // 4) * 4, -(-W // 32) * 32))
    bad = bf(F.silu(x * a + c)).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    src, recs = source_of(e, regions_of(e, {"down.0.xa": bad}))
    rows = R.check_acts(src, recs)
    with pytest.raises(AssertionError, match="activated copies outside"):
        R.check_act_rows(rows)
    assert [r["name"] for r in rows if r["ratio"] > 1] == ["down.0.xa"] and rows[0]["ratio_tab"] > 1


@pytest.mark.parametrize("cid", list(EMU))
def test_rstd_off_by_2_to_the_minus_10_fails(cid):
    """on a level-0 table (the most elements per group: the tightest statistics) and on out_norm"""
    e = emulate(cid)
    items = dict(e["items"])
    for name in ("down.0.n1.st", "out_norm.st"):
        st = items[name].clone()
        st[-1, 3, 1] *= 1 + 2.0 ** -10
        src, recs = source_of(e, regions_of(e, {name: st}))
        rows = R.check_tables(src, recs)
        with pytest.raises(AssertionError, match="GroupNorm tables outside"):
            R.check_table_rows(rows)
        assert [(r["name"], k) for r in rows for k, v in r["ratio"].items() if v > 1] == [(name[:-3], "rstd"), (name[:-3], "st~ab")]


@pytest.mark.parametrize("cid", list(EMU))
def test_mean_rstd_pair_off_by_1e_3_fails(cid):
    """.st and .ab of one norm both from a (mean, rstd) pair that is 1e-3 off, so the two stay consistent with each other: the bound
    of (c) alone has to see it, on every table -- behind the persistent kernel's model (T1cut: side-fused and side-stats+act tables fed
    by its FiLM, residual and bias-only epilogues) as behind the generic kernels'."""
    e = emulate(cid)
    items = dict(e["items"])
    sites = R.norm_sites(CH_MULT)
    replace = {}
    for prefix, nkey, *_ in sites:
        gamma, beta = (R.f64(e["sd"][nkey + k]) for k in (".weight", ".bias"))
        st = items[prefix + ".st"].double()
        mean, rstd = st[:, :, 0] * (1 + 1e-3), st[:, :, 1] * (1 + 1e-3)
        cpg = gamma.numel() // 8
        a = gamma[None, :] * rstd.repeat_interleave(cpg, 1)
        replace[prefix + ".st"] = torch.stack([mean, rstd], 2).float()
        replace[prefix + ".ab"] = R.ab_pack(a, beta[None, :] - mean.repeat_interleave(cpg, 1) * a)
    src, recs = source_of(e, regions_of(e, replace))
    rows = R.check_tables(src, recs)
    assert len(rows) == 21
    print("\n".join(f"  {r['name']:<10} {r['form']:<15} {r['coherence']:<7} rstd ratio {r['ratio']['rstd']:.2f}" for r in rows))
    for r in rows:
        assert r["ratio"]["st~ab"] <= 1, r
        # 1e-3 is outside the bound wherever twice the bound is below it (the emulation's own deviation is within one bound)
        if 2 * r["rstd_rel"] < 1e-3:
            assert r["ratio"]["rstd"] > 1 and r["ratio"]["a"] > 1, (r["name"], r["form"], r["coherence"], r["ratio"])
    seen = {r["name"] for r in rows if r["ratio"]["rstd"] > 1 and r["ratio"]["a"] > 1}
    # every table of the two upper levels (1440 / 2880 and 360 / 720 pixels per channel) but the one the bias-only stride-2 epilogue of
    # the persistent kernel's model feeds; at the 90 / 180 pixels of the middle 1e-3 is inside the element-wise bound itself (the GPU
    # cases have 858 pixels and more there)
    upper = {r["name"] for r in rows if r["name"][:6] in ("down.0", "down.1", "down.3", "down.4", "up.3.n", "up.4.n", "out_no") and r["coherence"] != "binade"}
    assert len(upper) >= 12
    assert upper <= seen, sorted(upper - seen)
    if EMU[cid][4] == "pr":
        assert {r["coherence"] for r in rows} == {"none", "binade", "value"}
        assert {r["form"] for r in rows if r["name"] in seen} >= {"side-fused", "side-stats+act", "prologue"}
        assert {r["coherence"] for r in rows if r["name"] in seen} == {"none", "value"}


@pytest.mark.parametrize("cid", list(EMU))
def test_film_row_of_the_neighbouring_resblock_fails(cid):
    e = emulate(cid)
    C = e["base"]
    film = dict(e["items"])["film"].clone()
    film[:, 0:2 * C] = film[:, 2 * C:4 * C]                         # down.0 reads down.1's rows
    reg = regions_of(e, {"film": film})
    out = R.check_cond(reg, e["sd"], CH_MULT, e["B"], e["z"], e["t"], TIME_DIM)
    with pytest.raises(AssertionError, match="conditioning regions outside"):
        R.check_cond_rows(out)
    assert [k for k, v in out.items() if v > 1] == ["film"]


def test_region_reader_on_a_synthetic_layout():
    g = torch.Generator().manual_seed(1)
    act = torch.randn((2, 3, 5, 8), generator=g).to(torch.bfloat16)            # NHWC
    a, c = torch.randn((2, 8), generator=g), torch.randn((2, 8), generator=g)
    st = torch.randn((2, 4, 2), generator=g)
    vec = torch.randn((2, 7), generator=g)
    text, raw = R.pack_regions([("vec", vec), ("t.o", act), ("t.n1.ab", R.ab_pack(a, c)), ("t.n1.st", st)])
    regions, total = R.parse_layout(text)
    assert [regions[k][0] % 256 for k in regions] == [0, 0, 0, 0] and regions["t.o"] == (256, 480) and total == raw.numel()
    reg = R.Regions(text, raw)
    assert torch.equal(reg.nhwc("t.o", 2, 3, 5, 8), act.double().permute(0, 3, 1, 2))
    assert torch.equal(reg.nhwc("t.o", 2, 3, 5, 8, [1]), act.double().permute(0, 3, 1, 2)[1:])
    ga, gc = reg.ab("t.n1.ab", 2, 8)
    assert torch.equal(ga, a.double()) and torch.equal(gc, c.double())
    # the table's memory order: {scale(2p), scale(2p + 1), shift(2p), shift(2p + 1)} per channel pair
    assert torch.equal(reg.f32("t.n1.ab", 2, 16)[0, :4], torch.stack([a[0, 0], a[0, 1], c[0, 0], c[0, 1]]).double())
    mean, rstd = reg.st("t.n1.st", 2, 4)
    assert torch.equal(mean, st[:, :, 0].double()) and torch.equal(rstd, st[:, :, 1].double())
    assert torch.equal(reg.f32("vec", 2, 7), vec.double())
    for call in (lambda: reg.nhwc("t.o", 2, 3, 5, 16), lambda: reg.ab("t.n1.ab", 2, 6), lambda: reg.st("t.n1.st", 2, 8),
                 lambda: reg.f32("vec", 7), lambda: R.Regions(text, raw[:300]).nhwc("t.o", 2, 3, 5, 8)):
        with pytest.raises(AssertionError):
            call()
    with pytest.raises(KeyError):
        reg.f32("missing", 1)


def test_flip_width_is_operand_plus_the_extra_term():
    g = torch.Generator().manual_seed(2)
    x = bf(torch.randn((2, 16, 6, 40), generator=g).double())
    a, c = LR.gn_affine(x, torch.rand(16, generator=g).double() + 0.5, torch.randn(16, generator=g).double(), 8)
    yb, w = LR.operand(x, a, c, True, True)
    yb0, w0 = R.flip_width(x, a, c, 0.0)
    assert torch.equal(yb, yb0) and torch.equal(w, w0)
    assert bool((R.flip_width(x, a, c, 1e-4)[1] >= w).all())


def test_route_parser_counts_lines():
    lines = []
    for name, kind, *_ in LR.layer_list(CH_MULT):
        if kind in ("c1", "c2", "head"):
            lines.append("norm fused slots=3")
        lines.append(f"conv fwd {R.KIND_OF[kind]} igemm th=4 bn=32 n_nt=2 four=0")
    recs = R.parse_routes(lines + ["conv dgrad C3S1 pr th=4 bn=128 n_nt=1 four=0", "wgrad C3S1 nsplit=2 tiles=4 cin=8 cout=8"], CH_MULT)
    assert len(recs) == 26 and list(recs)[0] == "in_conv" and list(recs)[-1] == "out" and all(r["ksplit"] == 1 for r in recs.values())
    assert recs["down.0.film"]["gn"] != "none" and recs["down.2"]["gn"] == "none" and recs["out"]["kind"] == "HEAD"
    with pytest.raises(AssertionError):
        R.parse_routes(lines + ["norm fused slots=3"], CH_MULT)
    with pytest.raises((AssertionError, StopIteration)):
        R.parse_routes(lines[:-1], CH_MULT)
    with pytest.raises(AssertionError):
        R.parse_routes(lines[1:], CH_MULT)
