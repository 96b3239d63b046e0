"""Float64 replay of the bf16 training forward from the workspace one ``ccn_train_forward`` call leaves behind.

After a forward call every activation, GroupNorm table and conditioning vector of the step sits in the caller's workspace at the
offsets ``ccn_internal_train_layout`` names, and ``ccn_internal_train_routes`` says which kernel and which forward-norm form wrote each
one.  This module reads those regions (``Regions``), turns the route report into one record per forward layer (``parse_routes``) and
checks, against float64 recomputations from the exact stored operands:

  (a) every conv layer, through the inference replay's ``replay_layer`` and its element-wise bound (tests/test_gpu_layer_replay.py;
      ``TrainSource`` is the adaptor: taps are workspace regions, weights are round-to-nearest bf16 of the fp32 parameters, which is
      what ``pack_group_kernel`` writes every step);
  (b) every activated copy ``.xa`` / ``.ya`` against ``operand()`` of the float64 GroupNorm + SiLU of the raw input region, its width
      widened by the one term a single element needs and a K-deep sum does not (``check_act``), and against the same transform with
      the device's own table;
  (c) every ``.ab`` / ``.st`` table against float64 statistics of the stored input region (``table_bounds``: ETA for the fp32 partial
      sums, plus a derived term because the epilogues sum the value before its bf16 rounding);
  (d) the conditioning regions stage by stage against oracle/ref_unet's formulas in float64 (``check_cond``).

Nothing here touches a GPU: the GPU test hands in the bytes it copied, tests/test_train_forward_host.py hands in an emulation.
"""
import math
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))
import test_gpu_layer_replay as LR  # noqa: E402  (replay_layer, Source, operand, gn_affine, conv_rows, bands, ROUNDING, ETA, ...)

from oracle import ref_unet  # noqa: E402

U32, ETA, ETA_COND, MIN_VIOLATED = LR.U32, LR.ETA, LR.ETA_COND, LR.MIN_VIOLATED
TEMB_ABS = 2e-4           # the device's timestep embedding against the CPU's (tests/test_gpu_parity.py::test_timestep_embedding)
# Hoeffding factor of the statistics' rounding term (table_bounds): a sum of n independent zero-mean errors |d_i| <= h_i exceeds
# KAPPA sqrt(sum h_i^2) with probability 2 exp(-KAPPA^2 / 2) = 2.5e-14 per table entry
KAPPA = 8.0
PRE_FORMS = ("fused", "stats+act")                       # the conv stages a plain copy of .xa / .ya
IN_CONV_FORMS = ("side-fused", "side-stats+act", "prologue")   # the conv transforms its raw input itself
KIND_OF = {"stem": "STEM", "c1": "C3S1", "c2": "C3S1", "down": "C3S2", "up": "CT4", "head": "HEAD"}


def f64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


# ---- region reader ----------------------------------------------------------------------------------------------------------------
def parse_layout(text):
    """``name off= bytes=`` lines and a last ``total=`` line -> ({name: (off, bytes)}, total)"""
    lines = text.splitlines() if isinstance(text, str) else list(text)
    assert lines and lines[-1].startswith("total="), lines[-1:]
    regions = {}
    for ln in lines[:-1]:
        name, off, size = ln.split()
        assert off.startswith("off=") and size.startswith("bytes=") and name not in regions, ln
        regions[name] = (int(off[4:]), int(size[6:]))
    return regions, int(lines[-1][6:])


class Regions:
    """The workspace bytes of one forward call (a CPU uint8 tensor that starts at the workspace base) and its layout."""

    def __init__(self, layout_text, raw):
        self.regions, self.total = parse_layout(layout_text)
        self.raw = raw
        assert raw.dtype == torch.uint8 and raw.dim() == 1

    def __contains__(self, name):
        return name in self.regions

    def _bytes(self, name, nbytes):
        off, size = self.regions[name]
        assert size == nbytes, f"region {name}: {size} bytes, the shape asked for has {nbytes}"
        assert off + size <= self.raw.numel(), f"region {name} ends at {off + size}, beyond the {self.raw.numel()} bytes copied"
        return self.raw[off:off + size].clone()

    def nhwc(self, name, B, H, W, C, samples=None):
        """a bf16 NHWC region as a float64 NCHW tensor (of `samples`, else of every sample)"""
        v = self._bytes(name, 2 * B * H * W * C).view(torch.bfloat16).view(B, H, W, C)
        if samples is not None:
            v = v[list(samples)]
        return v.double().permute(0, 3, 1, 2).contiguous()

    def ab(self, name, B, C):
        """a pair-interleaved scale / shift table (GnCoef::load: channels (2p, 2p + 1) -> {scale, scale, shift, shift}) -> (a, c), (B, C)"""
        v = self._bytes(name, 8 * B * C).view(torch.float32).view(B, C // 2, 2, 2).double()
        return v[:, :, 0].reshape(B, C), v[:, :, 1].reshape(B, C)

    def st(self, name, B, G):
        """a (mean, rstd) table -> two (B, G) tensors"""
        v = self._bytes(name, 8 * B * G).view(torch.float32).view(B, G, 2).double()
        return v[:, :, 0].contiguous(), v[:, :, 1].contiguous()

    def f32(self, name, *shape):
        return self._bytes(name, 4 * math.prod(shape)).view(torch.float32).view(*shape).double()


def pack_regions(items):
    """[(name, tensor)] -> (layout text, bytes): regions at 256-byte offsets, as Planner::take places them (the host emulation's
    counterpart of the workspace)"""
    text, chunks, off = "", [], 0
    for name, t in items:
        b = t.contiguous().view(-1).view(torch.uint8)
        pad = (-off) % 256
        chunks.append(torch.zeros(pad, dtype=torch.uint8)); off += pad
        text += f"{name} off={off} bytes={b.numel()}\n"
        chunks.append(b); off += b.numel()
    return text + f"total={off}\n", torch.cat(chunks)


def ab_pack(a, c):
    """(a, c) of shape (B, C) -> the pair-interleaved fp32 table"""
    B, C = a.shape
    return torch.stack([a.reshape(B, C // 2, 2), c.reshape(B, C // 2, 2)], 2).reshape(B, 2 * C).float()


# ---- route parser -----------------------------------------------------------------------------------------------------------------
def parse_routes(lines, ch_mult):
    """The ``conv fwd`` and ``norm`` lines of ``ccn_internal_train_routes`` -> {layer name (test_gpu_layer_replay.layer_list): record}
    in launch order (Step::forward notes a layer's norm before its conv).  Every line must be used, every layer must find its lines."""
    lines = [ln for ln in lines if ln.startswith("conv fwd ") or ln.startswith("norm ")]
    layers = LR.layer_list(ch_mult)
    it = iter(lines)
    out = {}
    for name, kind, *_ in layers:
        form, slots = "none", 0
        if kind in ("c1", "c2", "head"):
            w = next(it).split()
            assert w[0] == "norm" and w[2].startswith("slots="), (name, w)
            form, slots = w[1], int(w[2][6:])
        w = next(it).split()
        assert w[:3] == ["conv", "fwd", KIND_OF[kind]], (name, w)
        kv = {k: int(v) for k, v in (x.split("=") for x in w[4:])}
        out[name] = dict(kind=w[2], kernel=w[3], th=kv["th"], bn=kv["bn"], n_nt=kv["n_nt"], ksplit=1, gn=form, slots=slots)
    assert next(it, None) is None, "forward route lines left over"
    return out


def route_keys(recs):
    """((kind, kernel, th) of every conv, norm forms) of one report"""
    return {(r["kind"], r["kernel"], r["th"]) for r in recs.values()}, {r["gn"] for r in recs.values() if r["gn"] != "none"}


# ---- adaptor onto the inference replay ---------------------------------------------------------------------------------------------
class TrainSource(LR.Source):
    """``Source`` over the workspace of a training forward.  tap(name): ``<p>.film`` is region ``<p>.y``, an activated copy
    ``<p>.xa`` / ``<p>.ya`` (the operand of a pre-pass layer) is its own region, every other tap is ``<name>.o``.  weight(): plain
    round-to-nearest bf16 of the fp32 parameter for every kind (pack_group_kernel: ``to_elem<T>(v[t])``, no error diffusion)."""

    def __init__(self, reg, sd, base, ch_mult, B, H, W, x_in, eps, h, samples, routes):
        routes = {k: dict(v) for k, v in routes.items()}
        for r in routes.values():
            if r["kernel"] == "head2":
                r["th"] = 8      # the report carries no tile geometry for head2; ccn_head.hip works on 8 x 32 pixel tiles (10 x 34 halo)
        super().__init__(sd, ch_mult, x_in, eps, h, None, list(samples), 0, True, routes)
        self.reg, self.B = reg, B
        self.shapes = LR.tap_shapes(base, ch_mult, H, W)

    @staticmethod
    def region_of(name):
        if name.endswith((".xa", ".ya")):
            return name, name[:-3]
        if name.endswith(".film"):
            return name[:-5] + ".y", name
        return name + ".o", name

    def tap(self, name):
        if name not in self._taps:
            region, key = self.region_of(name)
            C, H, W = self.shapes[key]
            self._taps[name] = self.reg.nhwc(region, self.B, H, W, C, self.samples)
        return self._taps[name]

    def weight(self, key, kind):
        if key not in self._w:
            w = torch.from_numpy(np.ascontiguousarray(self.sd[key + ".weight"], np.float32))
            self._w[key] = w.to(torch.bfloat16).double()
        return self._w[key]


def adapt_layers(ch_mult, recs):
    """layer_list with the operand model of each route line: a pre-pass layer's operand is its activated copy exactly (no norm, no
    flip term: what separates the copy from the float64 transform is charged to the copy, check_acts); the in-conv forms keep the
    inference replay's operand(x, a, c, silu, True) with float64 statistics of the raw input"""
    out = []
    for name, kind, inp, resn, wkey, nkey, fkey in LR.layer_list(ch_mult):
        if kind in ("c1", "c2") and recs[name]["gn"] in PRE_FORMS:
            p = name[:-5] if kind == "c1" else name
            inp, nkey = p + (".xa" if kind == "c1" else ".ya"), None
        else:
            assert kind not in ("c1", "c2", "head") or recs[name]["gn"] in IN_CONV_FORMS, (name, recs[name])
        out.append((name, kind, inp, resn, wkey, nkey, fkey))
    return out


def norm_sites(ch_mult):
    """(table prefix, parameter key, raw input tap, consumer layer, activated-copy region or None) of every forward GroupNorm"""
    out = []
    for name, kind, inp, resn, wkey, nkey, fkey in LR.layer_list(ch_mult):
        if kind == "c1":
            out.append((name[:-5] + ".n1", nkey, inp, name, name[:-5] + ".xa"))
        elif kind == "c2":
            out.append((name + ".n2", nkey, inp, name, name + ".ya"))
        elif kind == "head":
            out.append(("out_norm", nkey, inp, name, None))
    return out


def producer_coherence(recs, tap):
    """How the rounding error the statistics do not see hangs together over the elements of `tap` (table_bounds' `coherence`), from
    the epilogue of the layer that wrote it.  Only a producer that rounds its accumulator to bf16 before the fp32 epilogue
    (ROUNDING's "acc": the persistent kernel) has any such structure:
      bias only (its stride-2 conv)      -> "binade": one error per (channel, binade, sign)
      FiLM (a ResBlock's first conv)     -> "value":  one error per (sample, channel, staged value), i.e. per stored value
      residual (second conv, ConvTranspose) -> None:  a second bf16 addend of its own magnitude; measured like the other kernels"""
    r = recs[tap]
    if "acc" not in LR.ROUNDING.get((r["kernel"], r["ksplit"]), ()):
        return None
    if r["kind"] == "C3S2":
        return "binade"
    return "value" if tap.endswith(".film") else None


# ---- (b) activated copies ------------------------------------------------------------------------------------------------------------
def flip_width(x, a, c, extra, eta=ETA):
    """operand(x, a, c, True, True) of the inference replay -- (bf16(y), bf16(y + d) - bf16(y - d)) -- with `extra` added to the
    uncertainty of z = x a + c before the SiLU (slope at most 1.1).  extra = 0 is operand() itself (checked on the host)."""
    z = x * a + c
    y = z * torch.sigmoid(z)
    d = 1.1 * (eta * ((x * a).abs() + c.abs()) + extra) + LR.SILU_REL * y.abs()
    return LR.bf16(y), LR.bf16(y + d) - LR.bf16(y - d)


def width_ratio(got, ref, w):
    """<= 1: inside the width, as a fraction of it; beyond: 1 + the excess in bf16 ulps of the reference"""
    diff = (got - ref).abs()
    return float(torch.where(diff <= w, diff / w.clamp_min(1e-300), 1.0 + (diff - w) / (2 * LR.hu16(ref.abs()))).max())


def check_act(x, gamma, beta, got, th, tab, G=8, coherence=None):
    """One .xa / .ya region against the float64 transform of its raw input x: every element must be a bf16 value the kernel can
    reach from its statistics, |got - bf16(y)| <= bf16(y + d) - bf16(y - d).  d is operand()'s (statistics within ETA, relative to
    |x a| + |c|) plus the term operand() has no reason to carry in front of a K-deep sum but a single element needs: the tables are
    statistics of the values BEFORE their bf16 rounding (table_bounds), so a and c are off by the rounding part of that bound (its
    eta = 0 evaluation), which is relative to |mean a| and not to the possibly cancelled |c|.
    Then against the same transform with the device's OWN table `tab` (gn_act_kernel loads it, gn_act_fused_kernel writes the pair
    it uses): what is left is the fp32 fma and the SiLU approximation, a width that is non-zero on a few elements in a thousand.
    Also the share of the elements that statistics counting the padding of partial tiles (th x 32 pixels) would change, on which
    that wrong copy is rejected."""
    a, c = LR.gn_affine(x, gamma, beta, G)
    tb = table_bounds(x, gamma, beta, G, eta=0.0, coherence=coherence)
    yb, w = flip_width(x, a, c, x.abs() * tb["a"][1][:, :, None, None] + tb["c"][1][:, :, None, None])
    ytb, wt = flip_width(x, tab[0][:, :, None, None], tab[1][:, :, None, None], 0.0, eta=4 * U32)
    H, W = x.shape[2:]
    share = None
    if W % 32 or H % th:
        a2, c2 = LR.gn_affine(x, gamma, beta, G, pad_hw=(-(-H // th) * th, -(-W // 32) * 32))
        yp = LR.operand(x, a2, c2, True, True)[0]
        ch = yp != yb
        share = float(((got - yp).abs() > w)[ch].double().mean()) if bool(ch.any()) else None
    return dict(ratio=width_ratio(got, yb, w), ratio_tab=width_ratio(got, ytb, wt), flips=float((w > 0).double().mean()),
                flips_tab=float((wt > 0).double().mean()), gnpad=share, wide=wt > 0)


def check_acts(src, recs, keep=False):
    rows = []
    for prefix, nkey, inp, consumer, region in norm_sites(src.ch_mult):
        if region is None or region not in src.reg:
            continue
        x, got = src.tap(inp), src.tap(region)
        tab = tuple(v[src.samples] for v in src.reg.ab(prefix + ".ab", src.B, x.shape[1]))
        r = check_act(x, f64(src.sd[nkey + ".weight"]), f64(src.sd[nkey + ".bias"]), got, src.routes[consumer]["th"], tab,
                      coherence=producer_coherence(recs, inp))
        r.update(name=region, form=recs[consumer]["gn"])
        if keep:
            r.update(got=got.to(torch.bfloat16), x=x.to(torch.bfloat16))
        else:
            del r["wide"]
        print(f"  {region:<14} {r['form']:<15} ratio {r['ratio']:.3f}  own table {r['ratio_tab']:.3f}  operands with a flip width {r['flips']:.4f} (own table {r['flips_tab']:.4f})  padded statistics rejected: "
              + ("-" if r["gnpad"] is None else f"{r['gnpad']:.2f}"))
        rows.append(r)
    shares = [r["gnpad"] for r in rows if r["gnpad"] is not None]
    if rows:
        print(f"  worst ratio {max(r['ratio'] for r in rows):.3f}, with the device's own table {max(r['ratio_tab'] for r in rows):.3f}, flip widths on {min(r['flips'] for r in rows):.3f} .. {max(r['flips'] for r in rows):.3f} "
              f"of the elements, padded statistics rejected on at least {min(shares) if shares else float('nan'):.2f}")
    return rows


def check_act_rows(rows):
    bad = [(r["name"], r["form"], r["ratio"], r["ratio_tab"]) for r in rows if not (r["ratio"] <= 1.0 and r["ratio_tab"] <= 1.0)]
    assert not bad, f"activated copies outside the flip width of their float64 transform (or of the transform with their own table): {bad}"
    weak = [(r["name"], r["gnpad"]) for r in rows if r["gnpad"] is not None and r["gnpad"] < MIN_VIOLATED]
    assert not weak, f"padded statistics that the flip width does not reject: {weak}"


# ---- (c) GroupNorm tables ------------------------------------------------------------------------------------------------------------
def table_bounds(x, gamma, beta, G=8, eps=1e-5, eta=ETA, coherence=None):
    """float64 (mean, rstd, a, c) of the stored tensor x (N, C, H, W) and what the kernels may be off by.

    The tables come from fp32 partial sums (s1, s2) per (tile, group) formed in the producing conv's epilogue, reduced over the slots
    in float64 (gn_stats_kernel / gn_group_stats), finished in float64 and stored as fp32.
      * fp32 partial sums of at most 4096 terms: relative ETA of sum|x| and of sum x^2 (the inference replay's ETA).
      * The epilogues sum the fp32 value v BEFORE its bf16 rounding (tile/epilogue.inc: ``pack(v)`` then ``s1[e] += v[e]``;
        ccn_conv_pr.hip: ``raw_buffer_store(pack(x))`` then ``s1[e] += x[e]``; ccn_stem.hip: ``pack_bf2(c0, c1)`` and ``t = (c0 + c1)
        + (c2 + c3)``), the reference sums the stored x = bf16(v): v_i = x_i + d_i with |d_i| <= h_i, half a bf16 ulp of x_i.  Round to
        nearest leaves d_i zero-mean and independent over elements, so by Hoeffding |sum d_i| <= KAPPA sqrt(sum h_i^2) and
        |sum (2 x_i d_i)| <= KAPPA sqrt(sum (2 x_i h_i)^2); d_i^2 is not zero-mean and is charged in full (sum h_i^2).
      * `coherence` (producer_coherence): behind the persistent kernel v is a bf16 staging value s put through an fp32 epilogue, and
        d_i is a function of what enters that epilogue.  With a bias alone, d = (s + b_c) - bf16(s + b_c) is the same number for every
        element of one channel, binade and sign (b_c mod ulp): "binade".  With FiLM, v = s (1 + f) + t with f, t per (sample, channel),
        so d is one number per (sample, channel, s), and s -> x is monotone: "value", the classes are the stored values of a channel.
        The Hoeffding terms are then taken over the classes, each class's errors fully coherent:
        |sum d_i| <= KAPPA sqrt(sum_k (sum_{i in k} h_i)^2), likewise for 2 x_i d_i.  With a residual a second bf16 tensor of the
        output's own magnitude enters and no such class exists; those tensors keep the element-wise term, and so do the fp32-
        accumulator kernels' (measured ratios per table under each choice: docs/EXPERIMENTS.md R25.3).
      * mean, var = m2 - mean^2 and rstd = (var + eps)^-1/2 propagate those; rstd by evaluating at var -+ dvar; the fp32 store adds
        one unit roundoff each.
    Returns dict name -> (ref, bound) for mean, rstd (N, g) and a, c (N, C); eta = 0: the part that is not the partial sums' own."""
    N, C, H, W = x.shape
    g = min(G, C)
    cpg, n = C // g, (C // g) * H * W
    xs = x.reshape(N, g, -1)
    mean, m2 = xs.sum(2) / n, (xs * xs).sum(2) / n
    var = m2 - mean * mean
    h = LR.hu16(xs.abs()) * (xs != 0)
    if coherence:
        xf = x.reshape(N, C, -1)
        if coherence == "binade":
            cls = (torch.floor(torch.log2(xf.abs().clamp_min(2.0 ** -60))).long() + 60).clamp(0, 127) * 2 + (xf < 0).long()
        else:
            assert coherence == "value", coherence
            cls = xf.to(torch.bfloat16).view(torch.int16).long() & 0xFFFF
        uniq, inv = torch.unique((cls + 65536 * torch.arange(N * C).view(N, C, 1)).reshape(-1), return_inverse=True)
        grp = uniq // 65536 // cpg                                # (sample, group) of each class

        def rss(wgt):
            S = torch.zeros(uniq.numel(), dtype=torch.float64).index_add_(0, inv, wgt.reshape(-1))
            return torch.sqrt(torch.zeros(N * g, dtype=torch.float64).index_add_(0, grp, S * S)).reshape(N, g)
    else:
        def rss(wgt):
            return torch.sqrt((wgt * wgt).sum(2))
    dmean = eta * xs.abs().sum(2) / n + KAPPA * rss(h) / n
    dm2 = eta * m2 + (KAPPA * rss(2 * xs.abs() * h) + (h * h).sum(2)) / n
    dvar = dm2 + 2 * mean.abs() * dmean + dmean * dmean
    rstd = 1.0 / torch.sqrt(var + eps)
    drstd = torch.maximum(rstd - 1.0 / torch.sqrt(var + dvar + eps), 1.0 / torch.sqrt((var - dvar).clamp_min(0) + eps) - rstd) + 2 * U32 * rstd
    dmean = dmean + 2 * U32 * mean.abs()
    rep = lambda v: v.repeat_interleave(cpg, 1)                                    # noqa: E731
    a = gamma[None, :] * rep(rstd)
    da = gamma[None, :].abs() * rep(drstd) + 2 * U32 * a.abs()
    c = beta[None, :] - rep(mean) * a
    dc = a.abs() * rep(dmean) + rep(mean).abs() * da + rep(dmean) * da + 2 * U32 * (beta[None, :].abs() + (rep(mean) * a).abs())
    return dict(mean=(mean, dmean), rstd=(rstd, drstd), a=(a, da), c=(c, dc))


def read_tables(reg, prefix, B, C, G=8):
    a, c = reg.ab(prefix + ".ab", B, C)
    mean, rstd = reg.st(prefix + ".st", B, min(G, C))
    return dict(mean=mean, rstd=rstd, a=a, c=c)


def tables_consistent(got, gamma, beta):
    """.ab against .st of the same norm: both are roundings of one float64 (mean, rstd) pair (gn_stats_kernel, gn_act_fused_kernel),
    so a = gamma rstd and c = beta - mean a hold between the stored numbers to a few fp32 roundoffs.  Worst ratio to 4 u."""
    cpg = got["a"].shape[1] // got["rstd"].shape[1]
    mean, rstd = got["mean"].repeat_interleave(cpg, 1), got["rstd"].repeat_interleave(cpg, 1)
    a = gamma[None, :] * rstd
    ra = (got["a"] - a).abs() / (4 * U32 * a.abs() + 1e-300)
    rc = (got["c"] - (beta[None, :] - mean * got["a"])).abs() / (4 * U32 * (beta[None, :].abs() + (mean * got["a"]).abs()) + 1e-300)
    return float(torch.maximum(ra, rc).max())


def check_tables(src, recs, keep=False):
    """every .st / .ab table (out_norm included) of the selected samples against table_bounds of the stored input region"""
    rows = []
    for prefix, nkey, inp, consumer, region in norm_sites(src.ch_mult):
        x = src.tap(inp)
        gamma, beta = f64(src.sd[nkey + ".weight"]), f64(src.sd[nkey + ".bias"])
        coh = producer_coherence(recs, inp)
        tb = table_bounds(x, gamma, beta, coherence=coh)
        got = {k: v[src.samples] for k, v in read_tables(src.reg, prefix, src.B, x.shape[1]).items()}
        r = dict(name=prefix, form=recs[consumer]["gn"], slots=recs[consumer]["slots"], coherence=coh or "none",
                 ratio={k: float(((got[k] - tb[k][0]).abs() / tb[k][1]).max()) for k in tb})
        r["ratio"]["st~ab"] = tables_consistent(got, gamma, beta)
        r["rstd_rel"] = float((tb["rstd"][1] / tb["rstd"][0]).max())
        if keep:
            r.update(got=got, ref={k: v[0] for k, v in tb.items()}, bound={k: v[1] for k, v in tb.items()})
        print(f"  {prefix:<12} {r['form']:<15} slots {r['slots']:<4} " + "  ".join(f"{k} {v:.3f}" for k, v in r["ratio"].items())
              + f"  (classes {r['coherence']}, rstd bound 2^{math.log2(r['rstd_rel']):.1f})")
        rows.append(r)
    for kind in ("mean", "rstd", "a", "c", "st~ab"):
        print(f"  worst {kind} ratio: {max(r['ratio'][kind] for r in rows):.3f}")
    return rows


def check_table_rows(rows):
    bad = [(r["name"], r["form"], k, v) for r in rows for k, v in r["ratio"].items() if not v <= 1.0]
    assert not bad, f"GroupNorm tables outside their bound: {bad}"


# ---- (d) conditioning ----------------------------------------------------------------------------------------------------------------
def check_cond(reg, sd, ch_mult, B, z, t, time_dim, temb_ref=None):
    """temb, t1, tp, zpv, h and every ResBlock's rows of film.  Each stage is recomputed in float64 from the region the device
    stage read (so an error is charged to the stage that made it), bound ETA_COND (sum |W||x| + |b|) per output; h also as
    oracle/ref_unet.cond_vector from the device's temb, with the first linear's error carried through the second (SiLU' <= 1.1).
    Returns {region: worst ratio}."""
    sd64 = ref_unet.as_torch_sd(sd, torch.float64)
    td = time_dim
    temb, t1, tp, zpv, h = (reg.f32(n, B, k) for n, k in (("temb", td), ("t1", 4 * td), ("tp", td), ("zpv", td), ("h", td)))
    z = z.double()
    out = {}
    if temb_ref is None:
        temb_ref = ref_unet.timestep_embedding(t, td).double()
    out["temb"] = float((temb - temb_ref).abs().max() / TEMB_ABS)

    def lin(x, key):
        W, b = sd64[key + ".weight"], sd64[key + ".bias"]
        return F.linear(x, W, b), x.abs() @ W.abs().T + b.abs()

    u0, s0 = lin(temb, "time_proj.0")
    out["t1"] = float(((t1 - F.silu(u0)).abs() / (1.1 * ETA_COND * s0)).max())
    r, s2 = lin(t1, "time_proj.2")
    out["tp"] = float(((tp - r).abs() / (ETA_COND * s2)).max())
    uz, sz = lin(z, "z_proj.0")
    out["zpv"] = float(((zpv - F.silu(uz)).abs() / (1.1 * ETA_COND * sz)).max())
    out["h"] = float(((h - (tp + zpv)).abs() / (ETA_COND * (tp.abs() + zpv.abs()) + 1e-300)).max())
    with torch.no_grad():
        h_ref = ref_unet.cond_vector(sd64, z, t, temb=temb)
    s2r = lin(F.silu(u0), "time_proj.2")[1]
    carried = (1.1 * ETA_COND * s0) @ sd64["time_proj.2.weight"].abs().T
    out["h (cond_vector)"] = float(((h - h_ref).abs() / (ETA_COND * (s2r + 1.1 * sz) + carried)).max())
    blocks = [name for name, kind, *_ in LR.layer_list(ch_mult) if kind == "c1"]
    F_rows = sum(2 * sd64[p + ".to_scale.weight"].shape[0] for p in blocks)
    film = reg.f32("film", B, F_rows)
    off, worst = 0, (0.0, "")
    for p in blocks:                                               # build_arch: [off, off + C) scale, [off + C, off + 2C) shift
        for part in ("to_scale", "to_shift"):
            r, s = lin(h, p + "." + part)
            C = r.shape[1]
            worst = max(worst, (float(((film[:, off:off + C] - r).abs() / (ETA_COND * s)).max()), p + "." + part))
            off += C
    out["film"] = worst[0]
    print("  conditioning: " + "  ".join(f"{k} {v:.4f}" for k, v in out.items()) + f"  (worst film rows: {worst[1]})")
    return out


def check_cond_rows(out):
    bad = {k: v for k, v in out.items() if not v <= 1.0}
    assert not bad, f"conditioning regions outside their bound: {bad}"


# ---- one case ------------------------------------------------------------------------------------------------------------------------
def replay(reg, route_lines, sd, base, ch_mult, B, H, W, x_in, z, t, eps, time_dim, label, samples=None, rng_seed=0, keep=False,
           temb_ref=None):
    """Everything of one forward call.  x_in, z, t, eps: CPU tensors of the whole batch; conv layers, activated copies and tables
    are replayed for `samples` (default: the first and the last sample)."""
    samples = sorted({0, B - 1}) if samples is None else list(samples)
    recs = parse_routes(route_lines, ch_mult)
    print(f"\n{label}: conditioning")
    cond = check_cond(reg, sd, ch_mult, B, z, t, time_dim, temb_ref)
    sd64 = ref_unet.as_torch_sd(sd, torch.float64)
    with torch.no_grad():                                           # FiLM of the conv replay: the oracle's chain on the device's temb
        h = ref_unet.cond_vector(sd64, z.double()[samples], t[samples], temb=reg.f32("temb", B, time_dim)[samples])
    src = TrainSource(reg, sd, base, ch_mult, B, H, W, x_in.double()[samples], eps.double()[samples], h, samples, recs)
    rows = LR.replay_all(src, adapt_layers(ch_mult, recs), f"{label}: conv layers (samples {samples})", rng_seed=rng_seed)
    print(f"{label}: activated copies")
    acts = check_acts(src, recs, keep)
    print(f"{label}: GroupNorm tables")
    tables = check_tables(src, recs, keep)
    src._taps.clear()
    return dict(rows=rows, acts=acts, tables=tables, cond=cond, routes=recs, samples=samples)
