"""Float64 references and derived error bounds for the training step's data-gradient convolutions, route by route.

Used by tests/test_gpu_dgrad.py (one data-gradient conv alone, through the hook ccn_internal_conv_dgrad, on operands that are bf16
numbers) and by tests/test_dgrad_ref_host.py (correct fp32 arithmetic inside the bounds; deliberately wrong results outside them).  No
GPU needed.

Reference.  The gradient of the FORWARD operation with respect to its input, by torch.autograd in float64 on the CPU:

    C3S1   F.conv2d(x, w, padding=1)                        w (Cout, Cin, 3, 3)
    C3S2   F.conv2d(x, w, stride=2, padding=1)              w (Cout, Cin, 3, 3)
    CT4    F.conv_transpose2d(x, w, stride=2, padding=1)    w (Cin, Cout, 4, 4)
    HEAD   F.conv2d(x, w, padding=1)                        w (img_ch, C, 3, 3)

The library computes these as convolutions of dy with repacked weights (flipped taps, a 3x3 kernel padded to 4x4, plane passes of 2x2
taps); nothing of that is restated here, which is what makes the reference independent of the packers.  S, the same gradient of |dy|
with |w|, is the scale of the accumulation error.  Tensors are NCHW here; the tests permute to the kernels' NHWC.

Operands.  Weights are bf16 numbers written into the fp32 parameter buffer (N(0, 1) / sqrt(taps x Cout), the fan of one output), dy and
res are bf16 numbers (N(0, 1)): every conversion on the device is exact and the reference models nothing but the operation.

Bound, per element, from the route's rounding points (ROUNDING of tests/test_gpu_layer_replay.py, bias 0, no FiLM); nothing is fitted:

    e_acc = K 2^-24 S          fp32 accumulation of K exact products; K = the taps x channels the kernel sums for one output: 9 Cout
                               (3x3), 4 Cout (the stride-2 conv's gradient: the four taps of one parity of the padded 4x4 kernel),
                               16 Cout (the ConvTranspose's gradient: four plane passes of 2x2 taps), 9 img_ch (the head's)
    pr                         + half a bf16 ulp at |acc| + e_acc: the consumers round the accumulators into the bf16 staging tile
    epilogue                   + 4 x 2^-24 (|acc| + |res| + |ref|): the fp32 `+ res`
    ws / fr / igemm / stem2 / pr    + half a bf16 ulp at |ref| + the error so far: the store

In fp32 mode: e_acc plus one fp32 ulp of |ref| + e_acc.
"""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
MIN_VIOLATED = 0.5             # tests/test_gpu_layer_replay.py: share of the changed outputs on which a wrong result must exceed the bound
ROUNDING = {"pr": ("acc", "store"), "fr": ("store",), "ws": ("store",), "igemm": ("store",), "stem2": ("store",)}
TAPS = {"C3S1": 9, "C3S2": 9, "CT4": 16, "HEAD": 9}
ROUTE_KIND = {"C3S1": "C3S1", "C3S2": "CT4", "CT4": "C3S2", "HEAD": "STEM"}      # the kernel family the gradient runs on (setup_conv)


def bf16(x):
    return x.to(torch.bfloat16).to(torch.float64)


def half_ulp(m, bits):
    """half an ulp of a float with `bits` significant bits at magnitude m (>= 0)"""
    return torch.exp2(torch.floor(torch.log2(m.clamp_min(1e-30))) - bits)


def hu16(m):
    return half_ulp(m, 8)


# ---- the operation -----------------------------------------------------------------------------------------------------------------------
def forward_op(kind, x, w):
    if kind == "CT4":
        return F.conv_transpose2d(x, w, stride=2, padding=1)
    return F.conv2d(x, w, stride=2 if kind == "C3S2" else 1, padding=1)


def dx_hw(kind, Hdy, Wdy):
    if kind == "C3S2":
        return 2 * Hdy, 2 * Wdy
    if kind == "CT4":
        assert Hdy % 2 == 0 and Wdy % 2 == 0
        return Hdy // 2, Wdy // 2
    return Hdy, Wdy


def dgrad(kind, w, dy):
    """d <forward_op(x, w), dy> / dx by autograd, in the dtype of w and dy (the op is linear in x: any x does)"""
    B, Hdy, Wdy = dy.shape[0], dy.shape[2], dy.shape[3]
    Cin = w.shape[0] if kind == "CT4" else w.shape[1]
    x = torch.zeros((B, Cin) + dx_hw(kind, Hdy, Wdy), dtype=w.dtype, requires_grad=True)
    y = forward_op(kind, x, w)
    assert y.shape == dy.shape, (y.shape, dy.shape)
    return torch.autograd.grad(y, x, dy)[0]


def k_summed(kind, w):
    """taps x channels the kernel adds up for one output"""
    cout = w.shape[1] if kind == "CT4" else w.shape[0]
    return {"C3S1": 9, "C3S2": 4, "CT4": 16, "HEAD": 9}[kind] * cout


def dgrad_ref(kind, w, dy, res=None):
    """(acc, S, ref): the float64 gradient, its scale, and what the launch leaves in dx"""
    assert w.dtype == dy.dtype == torch.float64
    acc = dgrad(kind, w, dy)
    S = dgrad(kind, w.abs(), dy.abs())
    return acc, S, acc if res is None else acc + res


def dgrad_bound(kind, kernel, w, acc, S, res, bf16_mode=True):
    e_acc = k_summed(kind, w) * U32 * S
    ref = acc if res is None else acc + res
    if not bf16_mode:
        return e_acc + 2 * half_ulp(ref.abs() + e_acc, 24)
    pts = ROUNDING[kernel]
    e = e_acc
    if "acc" in pts:
        e = e + hu16(acc.abs() + e)
    e = e + 4 * U32 * (acc.abs() + (ref - acc).abs() + ref.abs())
    assert "store" in pts
    return e + hu16(ref.abs() + e)


def emulate(kind, kernel, w, dy, res, bf16_mode=True):
    """correct arithmetic: float32 accumulation (torch's float32 gradient of the same op) with the route's roundings"""
    acc = dgrad(kind, w.float(), dy.float())
    if not bf16_mode:
        return (acc if res is None else acc + res.float()).double()
    if "acc" in ROUNDING[kernel]:
        acc = acc.to(torch.bfloat16).float()
    return (acc if res is None else acc + res.float()).to(torch.bfloat16).double()


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
def _route(kind, kernel, th, bn, n_nt):
    return f"conv dgrad {ROUTE_KIND[kind]} {kernel} th={th} bn={bn} n_nt={n_nt} four={1 if kind == 'CT4' else 0}"


def _case(base, weight, kind, Cin, Cout, B, H, W, kernel, th, bn, n_nt, res=False, variant=4, dtype="bf16"):
    return dict(base=base, weight=weight, kind=kind, Cin=Cin, Cout=Cout, B=B, H=H, W=W, kernel=kernel, th=th, res=res, variant=variant,
                dtype=dtype, route=_route(kind, kernel, th, bn, n_nt))


# Forward conv (configuration: base, ch_mult (1, 2)); B x H x W of dy; the route the step's policy gives it.  The smallest shapes that
# reach each route with ragged tiles on both edges: n8 = B ceil(MH / 8) ceil(MW / 32) npar n_nt eight-row tiles; conv_tile_rows gives 8 rows
# from n8 >= 256, the training policy puts the stride-2 conv's, the ConvTranspose's gradient on the persistent kernel from n8 >= 64.
CASES = {
    # 3x3 on the persistent kernel (PK_FRAG3_DG)
    "c3_pr8": _case(128, "down.0.conv1.weight", "C3S1", 128, 128, 4, 124, 130, "pr", 8, 128, 1),      # n8 = 320; last row tile 4 rows, last column tile 2 px
    "c3_pr4": _case(128, "down.0.conv1.weight", "C3S1", 128, 128, 1, 18, 40, "pr", 4, 128, 1),        # 4-row tiles, partial in both directions
    "c3_pr4_n2": _case(128, "mid1.conv1.weight", "C3S1", 256, 256, 1, 12, 40, "pr", 4, 128, 2),       # two N tiles, four K chunks
    "c3_pr4_192": _case(192, "down.0.conv1.weight", "C3S1", 192, 192, 1, 12, 40, "pr", 4, 128, 2),    # half-padded N (192 -> 256), 3 chunks
    "c3_pr4_384": _case(192, "mid1.conv1.weight", "C3S1", 384, 384, 1, 12, 40, "pr", 4, 128, 3),      # 6 chunks
    # ... conv variant 3: the plain operand (PK_DG3S1)
    "c3_fr8": _case(128, "down.0.conv1.weight", "C3S1", 128, 128, 4, 124, 130, "fr", 8, 128, 1, variant=3),
    "c3_ws4": _case(128, "down.0.conv1.weight", "C3S1", 128, 128, 1, 18, 40, "ws", 4, 128, 1, variant=3),
    # BN 64
    "c3_fr8_bn64": _case(64, "down.0.conv1.weight", "C3S1", 64, 64, 4, 124, 130, "fr", 8, 64, 1),
    "c3_ws4_bn64": _case(64, "down.0.conv1.weight", "C3S1", 64, 64, 2, 10, 40, "ws", 4, 64, 1),
    # the generic kernel, K not a multiple of 64
    "c3_igemm_48": _case(48, "down.0.conv1.weight", "C3S1", 48, 48, 2, 10, 40, "igemm", 4, 32, 2),
    "c3_ws4_96": _case(48, "mid1.conv1.weight", "C3S1", 96, 96, 2, 10, 40, "ws", 4, 64, 2),
    # the stride-2 conv's gradient: a ConvTranspose with the 3x3 kernel padded to 4x4 (PK_FRAG_CT_DG / PK_DG3S2), with the dskip add
    "s2_pr8": _case(128, "down.5.weight", "C3S2", 128, 256, 2, 20, 72, "pr", 8, 128, 1),              # n8 = 72
    "s2_pr8_res": _case(128, "down.5.weight", "C3S2", 128, 256, 2, 20, 72, "pr", 8, 128, 1, res=True),
    "s2_ws4": _case(128, "down.5.weight", "C3S2", 128, 256, 1, 8, 40, "ws", 4, 128, 1),
    "s2_ws4_res": _case(128, "down.5.weight", "C3S2", 128, 256, 1, 8, 40, "ws", 4, 128, 1, res=True),
    "s2_fr8": _case(128, "down.5.weight", "C3S2", 128, 256, 4, 64, 64, "fr", 8, 128, 1, variant=3),
    "s2_igemm_48": _case(48, "down.5.weight", "C3S2", 48, 96, 2, 10, 40, "igemm", 4, 32, 2),
    # the ConvTranspose's gradient: a 4x4 stride-2 conv as four plane passes of 2x2 taps (PK_FRAG_P4_DG), else the generic kernel (PK_DGT)
    "ct_pr8_n2": _case(128, "up.2.weight", "CT4", 256, 128, 2, 56, 272, "pr", 8, 128, 2),             # n8 = 80; partial tiles 4 rows / 8 px
    "ct_pr8": _case(128, "up.5.weight", "CT4", 128, 128, 3, 80, 272, "pr", 8, 128, 1),                # n8 = 75
    "ct_igemm": _case(128, "up.2.weight", "CT4", 256, 128, 1, 16, 64, "igemm", 4, 128, 2),
    # the head's gradient: stem_kernel on fp32 NCHW d eps (PK_FRAG_STEM_HEAD_DG); upw 1 / 4 / 8 of stem2_blocks, then the other widths
    "head_upw1": _case(128, "out.weight", "HEAD", 128, 3, 1, 10, 40, "stem2", 4, 128, 1),
    "head_upw4": _case(128, "out.weight", "HEAD", 128, 3, 2, 72, 130, "stem2", 4, 128, 1),
    "head_upw8": _case(128, "out.weight", "HEAD", 128, 3, 1, 136, 200, "stem2", 4, 128, 1),
    "head_64": _case(64, "out.weight", "HEAD", 64, 3, 2, 10, 40, "stem2", 4, 64, 1),
    "head_192": _case(192, "out.weight", "HEAD", 192, 3, 2, 10, 40, "stem2", 4, 128, 2),
    "head_32": _case(32, "out.weight", "HEAD", 32, 3, 2, 10, 40, "stem2", 4, 32, 1),
    "head_igemm_48": _case(48, "out.weight", "HEAD", 48, 3, 2, 10, 40, "igemm", 4, 32, 2),            # PK_HEAD_DG
    # fp32 mode through the same hook: the hook's own wiring (the fp32 step is pinned on every launch form by tests/test_gpu_train_routes.py)
    "f32_c3": _case(32, "down.0.conv1.weight", "C3S1", 32, 32, 2, 10, 40, "igemm", 4, 32, 1, dtype="fp32"),
    "f32_s2_res": _case(32, "down.5.weight", "C3S2", 32, 64, 2, 10, 40, "igemm", 4, 32, 1, res=True, dtype="fp32"),
}
# the cases the host test runs the emulation and the wrong results on: every kind, both rounding accountings, the 192-channel output
HOST_CASES = ["c3_pr4", "c3_ws4_bn64", "c3_pr4_192", "c3_igemm_48", "s2_pr8_res", "s2_ws4_res", "ct_pr8_n2", "ct_igemm", "head_upw4", "head_igemm_48", "f32_s2_res"]


def operand_key(cid):
    """cases with the same key run on the same operands (another kernel, another type): one reference serves them"""
    c = CASES[cid]
    return tuple(c[k] for k in ("kind", "Cin", "Cout", "B", "H", "W", "res"))


def inputs(cid):
    """seeded operands of a case, float64 tensors whose values are bf16 numbers: w in the parameter's layout, dy and res NCHW"""
    c = CASES[cid]
    first = next(i for i, other in enumerate(CASES) if operand_key(other) == operand_key(cid))
    gen = torch.Generator("cpu").manual_seed(4000 + first)
    kind = c["kind"]
    wshape = (c["Cin"], c["Cout"], 4, 4) if kind == "CT4" else (c["Cout"], c["Cin"], 3, 3)
    w = bf16(torch.randn(wshape, generator=gen, dtype=torch.float64) / math.sqrt(TAPS[kind] * c["Cout"]))
    dy = bf16(torch.randn((c["B"], c["Cout"], c["H"], c["W"]), generator=gen, dtype=torch.float64))
    res = None
    if c["res"]:
        res = bf16(torch.randn((c["B"], c["Cin"]) + dx_hw(kind, c["H"], c["W"]), generator=gen, dtype=torch.float64))
    return w, dy, res


# ---- deliberately wrong results: the bug classes the bound exists for (host test) ------------------------------------------------------------
def wrong_results(cid, w, dy, res, acc):
    """name -> what dx would hold (float64, before the store's rounding) under one bug of the packers or kernels"""
    c = CASES[cid]
    kind, th = c["kind"], c["th"]
    r = 0.0 if res is None else res
    out = {}
    out["taps_transposed"] = dgrad(kind, w.transpose(2, 3).contiguous(), dy) + r                    # ky / kx exchanged
    if kind in ("C3S1", "HEAD"):
        out["taps_not_flipped"] = F.conv2d(dy, w.transpose(0, 1), padding=1) + r                    # the forward weights as they are
    if kind == "C3S2":
        # the gradient is a ConvTranspose of dy with the 3x3 kernel in rows / columns 0..2 of a 4x4 one; here it sits in 1..3
        right = F.conv_transpose2d(dy, F.pad(w, (0, 1, 0, 1)), stride=2, padding=1)
        assert float((right - acc).abs().max()) <= 1e-12 * float(acc.abs().max())
        out["pad4_wrong_corner"] = F.conv_transpose2d(dy, F.pad(w, (1, 0, 1, 0)), stride=2, padding=1) + r
        out["pad4_wrong_corner_rows"] = F.conv_transpose2d(dy, F.pad(w, (0, 1, 1, 0)), stride=2, padding=1) + r
        B, C, H, W = acc.shape
        out["parities_swapped_rows"] = acc.reshape(B, C, H // 2, 2, W)[:, :, :, [1, 0]].reshape(acc.shape) + r
        out["parities_swapped_cols"] = acc.reshape(B, C, H, W // 2, 2)[..., [1, 0]].reshape(acc.shape) + r
    if kind == "CT4":
        out["p4_planes_swapped_rows"] = dgrad(kind, w[:, :, [1, 0, 3, 2], :].contiguous(), dy) + r  # each tap row reads the other row plane
        out["p4_planes_swapped_cols"] = dgrad(kind, w[:, :, :, [1, 0, 3, 2]].contiguous(), dy) + r
    # the last (ragged) 32-pixel column block of the first tile row left at zero
    os_ = 2 if kind == "C3S2" else 1
    ref = acc + r
    z = ref.clone()
    z[:, :, :th * os_, 32 * ((ref.shape[3] // os_ - 1) // 32) * os_:] = 0
    out["ragged_block_zero"] = z
    if res is not None:
        out["res_omitted"] = acc
    if c["Cin"] == 192:
        # the tile's pad channels 192..255 (zeros) stored behind each pixel: they land on channels 0..63 of the next one
        z = ref.clone()
        first = z[0, :64, 0, 0].clone()
        z[:, :64] = 0
        z[0, :64, 0, 0] = first
        out["pad_channels_leak"] = z
    return out
