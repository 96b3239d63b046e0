"""Host self-check of the f16x3 layer replay (tests/test_gpu_split_replay.py), no GPU: the two criteria of the replay are met by the
mode's arithmetic alone, and they reject the bug classes they are there for.

The chain is emulated in fp32 on the models of the GPU matrix at a reduced spatial size: fp32 taps; GroupNorm coefficients from
fp32 sums (mean / var / rstd in double, scale and shift cast to fp32 as gn_finalize_kernel does), z = fmaf(x, a, c), SiLU as
z / (1 + exp(-z)) in fp32; a split layer as three torch fp32 convolutions over ``split_emulation.split`` halves in the kernel's
order (a_lo w_hi, a_hi w_lo, a_hi w_hi), times 1 / scale; bias, FiLM and residual in fp32.  Shown per model:

  * every split layer meets (a) -- 10 RMS(got - full) <= RMS(omission reference - full) for the three omissions -- and (b), the
    element-wise bound, and the three wrong references of the bf16 / fp32 replay violate (b) on MIN_VIOLATED of what they change;
  * the emulation clears the factor 10 of (a) by at least 3x more (MARGIN), the single-slice omission included where it is asserted
    (K <= 1152);
  * an emulation that itself omits a term in one layer -- everywhere, or in the one K = 16 slice -- fails (a) on that layer.

Torch's CPU convolution and sum are not the kernels' summation orders: what this file proves is about the arithmetic (three
products of 11-bit halves, fp32 accumulation), which is all the two criteria assume.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_unet

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))
import split_emulation  # noqa: E402
import test_gpu_layer_replay as LR  # noqa: E402

MARGIN = 3.0              # the emulation clears OMIT_FACTOR by this much more
KIND = {"stem": "STEM", "c1": "C3S1", "c2": "C3S1", "down": "C3S2", "up": "CT4", "head": "HEAD"}
MODELS = [(64, (1, 2)), (128, (1, 2)), (80, (1, 2))]        # the models of test_gpu_split_replay.CASES
B, H, W = 2, 16, 40


def host_routes(sd, layers):
    """what the f16x3 plan decides, without the tile geometry: ResBlock convs and ConvTransposes with Cout >= 64 on split operands"""
    routes = {}
    for name, kind, inp, resn, wkey, nkey, fkey in layers:
        w = sd[wkey + ".weight"]
        cout = w.shape[1] if kind == "up" else w.shape[0]
        split = kind in ("c1", "c2", "up") and cout >= 64
        routes[name] = dict(kind=KIND[kind], kernel="ws" if split else "igemm", th=4, ksplit=1, gn="prologue" if nkey else "none",
                            ops="f16x3" if split else "f32")
    return routes


def conv32(kind, x, w):
    if kind == "up":
        return F.conv_transpose2d(x, w, None, stride=2, padding=1)
    return F.conv2d(x, w, None, stride=2 if kind == "down" else 1, padding=1)


def emulate_f16x3(src, layers, omit=None, G=8):
    """fill src's taps (and eps) with the emulated fp32 chain.  omit = (layer name, "alwh" | "ahwl" | "slice"): that layer's product
    without the term (LR.omissions names them)"""
    sd = src.sd
    f32 = lambda k: torch.from_numpy(np.ascontiguousarray(sd[k], np.float32))
    taps = {}
    for name, kind, inp, resn, wkey, nkey, fkey in layers:
        w, b = f32(wkey + ".weight"), f32(wkey + ".bias")
        x = src.x_in.float() if kind == "stem" else taps[inp]
        if nkey:
            N, C = x.shape[:2]
            g = min(G, C)
            xs = x.reshape(N, g, -1)
            cnt = xs.shape[2]
            mean = xs.sum(2).double() / cnt
            var = ((xs * xs).sum(2).double() / cnt - mean * mean).clamp_min(0.0)
            rstd = 1.0 / torch.sqrt(var + 1e-5)
            sc = f32(nkey + ".weight").double()[None, :] * rstd.repeat_interleave(C // g, 1)
            sh = f32(nkey + ".bias").double()[None, :] - mean.repeat_interleave(C // g, 1) * sc
            a, c = sc.float()[:, :, None, None], sh.float()[:, :, None, None]
            x = (x.double() * a.double() + c.double()).float()                    # fmaf: one rounding
            if kind != "head":
                x = x / (1.0 + torch.exp(-x))
        if src.routes[name]["ops"] == "f16x3":
            s = split_emulation.weight_scale(w)
            wh, wl = split_emulation.split(w * s)
            ah, al = split_emulation.split(x)
            what = omit[1] if omit and omit[0] == name else None
            wh1 = wh
            if what == "slice":
                c0 = 16 * ((x.shape[1] - 1) // 16)
                wh1 = wh.clone()
                if kind == "up":
                    wh1[c0:, :, 2:4, 2:4] = 0
                else:
                    wh1[:, c0:, 2, 2] = 0
            acc = torch.zeros(())
            if what != "alwh":
                acc = acc + conv32(kind, al, wh1)
            if what != "ahwl":
                acc = acc + conv32(kind, ah, wl)
            acc = (acc + conv32(kind, ah, wh)) * (1.0 / s)
        else:
            acc = conv32(kind, x, w)
        bb = b[None, :, None, None]
        if fkey:
            h = src.h
            s_, t_ = (torch.from_numpy(np.asarray(sd[fkey + k + ".weight"], np.float64)) for k in (".to_scale", ".to_shift"))
            sb, tb = (torch.from_numpy(np.asarray(sd[fkey + k + ".bias"], np.float64)) for k in (".to_scale", ".to_shift"))
            f1 = 1.0 + (h @ s_.T + sb).float()[:, :, None, None]
            f2 = bb * f1 + (h @ t_.T + tb).float()[:, :, None, None]
            v = acc * f1 + f2
        else:
            v = acc + bb
            if resn:
                v = v + taps[resn]
        if kind == "head":
            src.eps = v.double()
        else:
            taps[name] = v
            src._taps[name] = v.double()


_CACHE = {}


def chain(synth, base, ch_mult, omit=None):
    """(source with the emulated taps, layers); the correct chain of each model is computed once"""
    key = (base, ch_mult, omit)
    if key not in _CACHE:
        sd = LR.model_sd(synth, base, ch_mult)
        layers = LR.layer_list(ch_mult)
        g = torch.Generator().manual_seed(base + 5)
        x = torch.randn((B, 3, H, W), generator=g).double(); z = torch.from_numpy(synth.synth_z(B)); t = torch.tensor([900, 37])
        src = LR.Source(sd, ch_mult, x, None, LR.film_h(ref_unet.as_torch_sd(sd, torch.float64), z, t), None, [0, 1], 0, "f16x3",
                        host_routes(sd, layers))
        emulate_f16x3(src, layers, omit)
        _CACHE[key] = (src, layers)
    return _CACHE[key]


@pytest.mark.parametrize("base,ch_mult", MODELS, ids=[f"base{m[0]}" for m in MODELS])
def test_emulated_chain_meets_both_criteria_with_margin(synth, base, ch_mult):
    src, layers = chain(synth, base, ch_mult)
    rows = LR.replay_all(src, layers, f"host emulation of the f16x3 chain, base {base} {ch_mult}, {B} x {H} x {W}")
    LR.check_rows(rows)
    split = [r for r in rows if "omit" in r]
    assert len(split) == 22, [r["name"] for r in split]          # 20 ResBlock convs and the 2 ConvTransposes
    thin = [(r["name"], k, x) for r in split for k, x in r["omit"].items() if LR.slice_asserted(r, k) and x < MARGIN * LR.OMIT_FACTOR]
    assert not thin, f"the emulation does not clear {LR.OMIT_FACTOR} x by {MARGIN} x: {thin}"


@pytest.mark.parametrize("what", ["alwh", "ahwl", "slice"])
@pytest.mark.parametrize("base,ch_mult", MODELS, ids=[f"base{m[0]}" for m in MODELS])
def test_an_emulation_that_omits_a_term_fails_criterion_a(synth, base, ch_mult, what):
    """One layer of each class (first-level ResBlock conv behind a GroupNorm with FiLM, one with a residual, the ConvTranspose with
    exact operands) computed without the term: criterion (a) fails on that layer, for that omission, and check_rows says so."""
    good, layers = chain(synth, base, ch_mult)
    rng = np.random.default_rng(0)
    for lname in ("down.0.film", "down.1", "up.2"):
        layer = next(L for L in layers if L[0] == lname)
        K = good.tap(layer[2]).shape[1] * (4 if layer[1] == "up" else 9)
        if what == "slice" and K > LR.SLICE_K_MAX:
            continue
        src, _ = chain(synth, base, ch_mult, omit=(lname, what))
        # the layer's own inputs are those of the correct chain (it is the first to differ)
        r = LR.replay_layer(src, layer, rng=rng, check_wrong=False)
        print(f"base {base} {lname} computed without {what}: omissions / rms(got - full) {r['omit']}")
        assert r["omit"][what] < LR.OMIT_FACTOR, (lname, what, r["omit"])
        assert r["omit"][what] < 1.5, (lname, what, r["omit"])         # got sits ON the omission reference: ratio ~ 1
        with pytest.raises(AssertionError, match="omitted term"):      # (criterion (a) on its own: (b) may or may not notice)
            LR.check_rows([dict(r, ratio=0.0)])
