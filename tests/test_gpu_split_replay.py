"""The pin of the f16x3 arithmetic (CCN_DTYPE_F16X3): every split conv replayed against a float64 product of its own operands, on
all 16 compiled forms of the ws / fr kernels with ``T = f16x3_t`` -- {C3S1, CT4} x {ws, fr} x {4, 8 tile rows} x {BN 64, 128}.

The harness is the layer replay's (tests/test_gpu_layer_replay.py, mode "f16x3"): exact fp32 weights, the tap the kernel read,
float64 GroupNorm statistics, SiLU, conv, bias, FiLM / residual; the conditioning from the timestep embedding the device computed.
Layers that report ``ops=f32`` (stem, head, stride-2 convs, BN 32) keep the fp32 replay's bound.  A split layer (``ops=f16x3``)
must meet two criteria:

  (a) RMS discrimination, the sharp one.  The operand is built as the kernel builds it -- a32 = fp32(silu(gn(x))) (or the tap),
      (a_hi, a_lo) = split(a32), (w_hi, w_lo) = split(w scale(w)) -- and with `full` the float64 product of the fp32 operands,
          10 RMS(got - full) <= RMS(wrong - full)
      for three wrong references: a_lo w_hi omitted everywhere, a_hi w_lo omitted everywhere, and a_lo w_hi omitted in ONE K = 16
      slice, the last step of the K loop (last slice of the last tap of the last Cin chunk: where the one-term-ahead fetch of
      tile/split_steps.inc ends).  The slice reference is asserted where K <= 1152 (SLICE_K_MAX) and printed elsewhere: on wider
      layers one slice's share is too small to tell from fp32 accumulation.  The kernel's fp32 GroupNorm + SiLU differs from
      fp32(float64) by a few ulps (1e-7 relative), the omissions are 1e-4 relative: a GroupNorm in front does not blur this.
  (b) an element-wise bound, max |got - ref| / bound <= 1, from the rounding points (nothing fitted):
          3 K 2^-24 sum|a||w|                          three accumulations per product
          (2^-22 + 2^-22 + 2^-24) sum|a||w|            the two split residuals and the dropped a_lo w_lo
          2^-25 sum|w| (+ 2^-25 / scale sum|a|)        halves in fp16's subnormal range
          the GroupNorm coefficient error              derived from the summation chain (gn_chain_depth / gn_coef_err), per group
          epilogue and conditioning terms              as in the fp32 replay
      The zeroed tap, the shifted last column tile and the padded statistics must still violate it on MIN_VIOLATED of what they change.

tests/test_split_replay_host.py shows on the host that correct arithmetic meets both (clearing the factor 10 by 3x more) and that an
emulation without a term, everywhere or in the one slice, fails (a).  test_split_route_coverage asserts that the matrix reaches
every form; the range guard runs on the forms it had never run on.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))
import infer_plan_cases  # noqa: E402
import test_gpu_layer_replay as LR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = LR.DEV

B64, B128, B80 = (64, (1, 2)), (128, (1, 2)), (80, (1, 2))
# (id, (base, ch_mult), B, H, W, conv variant or None).  8-row tiles need B ceil(MH / 8) ceil(MW / 32) npar n_nt >= 256
# (conv_tile_rows): that fixes the smallest shapes.  Variant None: ws on 4 rows, fr on 8; 0: ws everywhere; 2: fr everywhere.
CASES = [
    ("b64_2x124x264", B64, 2, 124, 264, None),       # fr 8-row BN 64 on C3S1 (prologue) and CT4; ws 4-row BN 64 / 128; partial tiles
    ("b128_2x124x264", B128, 2, 124, 264, None),     # fr 8-row BN 128 on C3S1 and CT4; 256 channels: n_nt 2, preact_fused, ws 4-row
    ("b80_2x64x256", B80, 2, 64, 256, None),         # Cin 80 (partial chunk), Cout 80 / 160 (half-padded N tiles of BN 64 / 128),
                                                     # preact_fused on 8-row tiles, CT4 160 -> 80
    ("b64_1x40x72", B64, 1, 40, 72, None),           # everything on ws 4-row, ragged
    ("b128_1x40x72", B128, 1, 40, 72, None),
    ("b64_1x40x72_fr", B64, 1, 40, 72, 2),           # ... and on fr 4-row
    ("b128_1x40x72_fr", B128, 1, 40, 72, 2),
    ("b64_2x124x264_ws", B64, 2, 124, 264, 0),       # ws 8-row
    ("b128_2x124x264_ws", B128, 2, 124, 264, 0),
]
FORMS = {(kind, kernel, th, bn) for kind in ("C3S1", "CT4") for kernel in ("ws", "fr") for th in (4, 8) for bn in (64, 128)}
GN_FORMS_SPLIT = {"none", "prologue", "preact_fused"}
BAND_PX = 48 * 48         # row bands above this many output pixels (the 62 x 132 level of the large cases)


def n_tile(cout):
    return 128 if cout >= 128 else 64             # conv_bn_for, Cout >= 64


def replay(synth, case):
    big = case[2] * case[3] * case[4] > 16384
    # under a non-default variant only the split layers differ from the default run; on the large shapes one layer per route class
    return LR.replay_case(synth, case, "f16x3", only_split=case[5] is not None, one_per_class=big, band_px=BAND_PX)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_f16x3_layer_replay(synth, case):
    """Every replayed layer of one f16x3 forward: split layers meet (a) and (b), the others the fp32 bound; the wrong references of
    every layer violate the bound on most of the outputs they change."""
    rows = replay(synth, case)
    assert any("omit" in r for r in rows)
    LR.check_rows(rows)


def widths(sd):
    """{activation name: (Cin, Cout)} of the conv layers of a plan"""
    out = {}
    for name, kind, inp, resn, wkey, nkey, fkey in LR.layer_list((1, 2)):
        w = sd[wkey + ".weight"]
        out[name] = (w.shape[0], w.shape[1]) if kind == "up" else (w.shape[1], w.shape[0])
    return out


def test_split_route_coverage(synth):
    """The executed plans of CASES reach all 16 (kind, kernel, tile rows, BN) forms on split operands, the three input forms, FiLM
    and residual epilogues, a half-padded N tile and a partial Cin chunk -- as reported by the library for the plans it ran; and no
    split launch is of a route the replay has no model for."""
    seen, forms, lines = set(), set(), []
    film = res = padded = partial = False
    for case in CASES:
        run = LR.run_forward(synth, case, "f16x3")
        wd = widths(run["sd"])
        here = set()
        for name, r in run["routes"].items():
            assert r.get("ops") in ("f16x3", "f32"), (case[0], r)
            if r["ops"] != "f16x3":
                assert r["kernel"] == "igemm" and (r["kernel"], r["ksplit"]) in LR.ROUNDING, (case[0], r)
                continue
            cin, cout = wd[name]
            key = (r["kind"], r["kernel"], r["th"], n_tile(cout))
            assert key in FORMS and r["ksplit"] == 1 and r["gn"] in GN_FORMS_SPLIT, f"{case[0]}: no model for the split route {r}"
            assert r["n_nt"] == -(-cout // n_tile(cout)), (case[0], r)
            here.add(key); forms.add(r["gn"])
            film |= r["film"] == 1; res |= r["res"] == 1
            padded |= cout % n_tile(cout) != 0; partial |= cin % 32 != 0
        seen |= here
        lines.append(f"  {case[0]:<20} " + ", ".join(f"{k}/{kn}/th{th}/bn{bn}" for k, kn, th, bn in sorted(here)))
        del run
    print("\nsplit forms per case:\n" + "\n".join(lines))
    for key in sorted(FORMS):
        print(f"  {key[0]}/{key[1]}/th{key[2]}/bn{key[3]:<4} {'reached' if key in seen else 'NOT REACHED'}")
    print(f"  input forms on split layers: {sorted(forms)}; film {film}, res {res}, Cout_pad > Cout {padded}, Cin % 32 != 0 {partial}")
    assert seen == FORMS, sorted(FORMS - seen)
    assert forms == GN_FORMS_SPLIT, sorted(GN_FORMS_SPLIT - forms)
    assert film and res and padded and partial, (film, res, padded, partial)


# ---- the range guard on the forms it had never run on ---------------------------------------------------------------------------------
def _preact_overflow(sd):
    """norm1 of the first 256-channel ResBlock scaled by 1e6: the pre-pass writes activations beyond fp16's range, and the split conv
    behind it (gn=preact_fused) stages them"""
    bad = dict(sd)
    bad["mid1.norm1.weight"] = (sd["mid1.norm1.weight"] * np.float32(1e6)).astype(np.float32)
    return bad, "mid1.film", "C3S1", "preact_fused"


def _convt_overflow(sd):
    """a bias of 1e6 on conv2 of the ResBlock in front of the first ConvTranspose: its input tensor itself is beyond the range"""
    bad = dict(sd)
    bad["up.1.conv2.bias"] = (sd["up.1.conv2.bias"] + np.float32(1e6)).astype(np.float32)
    return bad, "up.2", "CT4", "none"


@pytest.mark.parametrize("variant,kernel", [(None, "ws"), (2, "fr")], ids=["ws", "fr"])
@pytest.mark.parametrize("model,spoil", [(B128, _preact_overflow), (B64, _convt_overflow)], ids=["preact_fused", "conv_transpose"])
def test_range_guard_on_the_other_forms(synth, model, spoil, variant, kernel):
    """1 x 40 x 72, an activation pushed past 65504 by one scaled parameter: the operand saturates (designed behaviour), eps stays
    finite, the handle reports it exactly once, and an unspoilt net afterwards passes its replay."""
    base, ch_mult = model
    sd = LR.model_sd(synth, base, ch_mult)
    bad, layer, kind, form = spoil(sd)
    case = (f"guard_{layer}_{kernel}", model, 1, 40, 72, variant)
    lib = LR._lib()
    old = lib.ccn_internal_set_conv_variant(variant) if variant is not None else None
    try:
        net = LR.make_net(bad, base, ch_mult, "f16x3")
        g = torch.Generator().manual_seed(1040 + 72)
        x = torch.randn((1, 3, 40, 72), generator=g); z = torch.from_numpy(synth.synth_z(1)); t = torch.tensor([500])
        eps = net(x.to(DEV), z.to(DEV), t.to(DEV))
        torch.cuda.synchronize()
        r = infer_plan_cases.plan_routes(net.native())[layer]
        assert (r["kind"], r["kernel"], r["gn"], r["ops"]) == (kind, kernel, form, "f16x3"), r
        assert torch.isfinite(eps).all()
        with pytest.raises(RuntimeError, match=r"(?s)f16x3.*fp32"):
            net.native().poll_errors()
        net.native().poll_errors()                               # reported once
    finally:
        if old is not None:
            lib.ccn_internal_set_conv_variant(old)
    rows = LR.replay_case(synth, case, "f16x3", only_split=True)
    assert any(r["name"] == layer for r in rows)
    LR.check_rows(rows)
