"""Per-layer replay of the inference forward against a float64 recomputation from the exact operands each kernel consumed.

In bf16 mode every activation between two layers is stored as bf16, so ``read_activation`` returns exactly what the next kernel
reads.  For every layer the reference recomputes, in float64 on the CPU, what the layer is meant to compute from the previous tap(s):
the version-k weights the handle committed (``ccn_internal_round_weights``, error-diffused, k = the DDIM step's weight version),
the conditioning / FiLM of the oracle (``oracle/ref_unet.py``) in float64, the input GroupNorm's statistics in float64 over the whole
tensor, ``bf16(silu(gn(x)))`` as the MFMA operand (no SiLU in front of the head), then conv + bias + FiLM / residual as the reference
writes the layer (models/blocks.py:40-44, models/unet.py:88-106).  What is left between the kernel and that reference is the kernel's
own rounding, which the bound below states element by element from the route's rounding points (ROUNDING):

    bound = gain * (K 2^-24 sum|a||w|               fp32 accumulation of K products (MFMA: exact bf16 products, fp32 sums)
                    + sum |hi - lo| |w|)            operands whose float64 value lies within the kernel's GroupNorm error (ETA) of a
                                                    bf16 rounding boundary: the kernel may round them the other way (one ulp each)
          + sum over rounding points of half an ulp of the value there (inflated by the error before it) times the gain after it
          + conditioning (ETA_COND) and fp32 epilogue terms

and each layer must meet max(|got - ref| / bound) <= 1.  Nothing is fitted to measurements.  The route of each launch (kernel, tile
rows, split-K, input-GroupNorm form) comes from the library itself (``ccn_internal_plan_routes``, decided by the same function that
launches it), and the coverage test checks that the shape matrix reaches every route of the bf16 inference plan (ROUTES_BF16).

Each replayed layer also checks three deliberately wrong references computed on the host (a zeroed weight tap of one output channel,
the input shifted by one pixel inside the last column tile, GroupNorm statistics that count the padding of partial tiles): each must
violate the bound on a clear majority of the outputs it changes, i.e. the bound tells those bug classes apart from rounding.

The fp32 and f16x3 modes (fp32 storage) run through the same harness.  Their GroupNorm term is not a constant: gn_chain_depth
states the longest chain of fp32 additions behind one partial sum from the kernel that wrote the input, and gn_coef_err turns it
into the error of scale and shift per group, from the data (the cancellation in E[x^2] - mean^2 included).  A layer on split
operands (``ops=f16x3`` in the route report) has the bound's split terms and, as its sharp criterion, the RMS comparison with
references that omit one term of the three-term product (split_terms, omissions, check_rows); tests/test_gpu_split_replay.py holds
that mode's shape matrix.
"""
import ctypes
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
from infer_plan_cases import plan_routes  # noqa: E402

DEV = "cuda:0"
U32 = 2.0 ** -24          # fp32 unit roundoff
ETA = 2.0 ** -12          # bf16 mode: relative error of the kernels' GroupNorm scale / shift (fp32 partial sums of rounded bf16 values;
                          # an operand within it of a bf16 rounding boundary may round the other way).  The fp32 and f16x3 modes do
                          # not use it: their coefficient error is derived from the summation chain (gn_chain_depth, gn_coef_err)
ETA_COND = 2.0 ** -11     # FiLM scale / shift against float64, relative to sum|W||h| + |b|: the device's timestep embedding is within
                          # 2e-4 of the CPU's on O(1) values (test_gpu_parity.test_timestep_embedding) and the linears are fp32
SILU_REL = 2.0 ** -18     # bf16 mode's SiLU (v_exp / v_rcp approximations) relative to its value
MIN_VIOLATED = 0.5        # share of the changed outputs on which a wrong reference must exceed the bound (measured: >= 0.58; the
                          # weakest is one zeroed tap of 4608 products at the 512-channel level, where K 2^-24 sum|a||w| is largest)

# Rounding points of each route, from the kernels (what the bound charges half an ulp for, in order):
ROUNDING = {
    # ccn_conv_pr.hip: the consumers round the accumulators into a bf16 staging tile; the epilogue applies bias / FiLM / residual in
    # fp32 to the staged value and rounds again at the 16-byte store.  FiLM's factor (1 + s) multiplies the first rounding.
    ("pr", 1): ("acc", "store"),
    # ... split-K (stride-2 layers, no FiLM / residual): each K half rounds its accumulator to staging; the first half stores
    # bf16(staged + bias) into `kpart`, the second adds that partial to its own staged accumulator and rounds at the store
    ("pr", 2): ("acc_half1", "kpart", "acc_half2", "store"),
    # ccn_conv_fr.hip / ccn_conv_ws.hip / generic implicit GEMM (ccn_kernels.hip): fp32 accumulator, fp32 epilogue, one pack
    ("fr", 1): ("store",), ("ws", 1): ("store",), ("igemm", 1): ("store",),
    # ccn_stem.hip: bf16(x) im2col with the bias as a bf16 K element against a constant one; one pack of the accumulator
    ("stem2", 1): ("store",),
    # ccn_head.hip: out_norm folded into per-sample weights W' = bf16(a_b W) (round to nearest at step 0, with a carry along the
    # DDIM steps), S = sum_c c_b W in fp32; eps is fp32: the only rounding is that of the weights, stated through sum|x||W'|
    ("head2", 1): ("weights",),
}
# the generic head (igemm, KIND_HEAD) writes fp32 eps: no rounding point besides its bf16 operand (covered by the flip term)

# Every route the bf16 inference plan takes in the shape matrix below: (kind, kernel, th, ksplit) and the input-GroupNorm forms.
# A threshold change that stops exercising one of them fails test_route_coverage.
ROUTES_BF16 = {
    ("STEM", "stem2", 4, 1),      # C2 (base 128)
    ("STEM", "igemm", 4, 1),      # base 48: not a stem2 width
    ("C3S1", "pr", 8, 1),         # C2 first level at batch 8
    ("C3S1", "pr", 4, 1),         # C2 deeper levels
    ("C3S1", "ws", 4, 1),         # base 48's 96-channel level (BN 64)
    ("C3S1", "igemm", 4, 1),      # base 48's 48-channel level (BN 32)
    ("C3S1", "fr", 8, 1),         # conv variant 3: the free-running kernel on 8-row tiles
    ("C3S2", "pr", 8, 1),         # stride 2 with more than 128 eight-row tiles
    ("C3S2", "pr", 8, 2),         # ... exactly 128: split-K (the conv into the 32-pixel level at the bench shape, the last two at
                                  # 16 x 128 px)
    ("C3S2", "igemm", 4, 1),      # ... fewer than 128 (batch 1 at 256 px: all three; the ragged shapes)
    ("CT4", "pr", 8, 1),          # ConvTranspose where conv_tile_rows gives 8 rows
    ("CT4", "ws", 4, 1),          # ... else
    ("CT4", "fr", 8, 1),          # ... 8 rows under conv variant 3
    ("CT4", "igemm", 4, 1),       # base 48's 96 -> 48 ConvTranspose (BN 32)
    ("HEAD", "head2", 8, 1),
    ("HEAD", "igemm", 4, 1),      # base 48
}
# (the pre-pass without its finalize folded in, "preact", needs an input without partial sums: no inference plan has one; it is the
# diagnostics build's CCN_NO_FUSED_GNACT switch, and the replay would model it like preact_fused)
GN_FORMS_BF16 = {"none", "prologue", "instat", "preact_fused", "weights"}


def _lib():
    from clip_feature_codec import _native
    lib = _native.load_library()
    lib.ccn_internal_round_weights.restype = ctypes.c_int
    lib.ccn_internal_round_weights.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                               ctypes.c_void_p]
    lib.ccn_internal_set_conv_variant.restype = ctypes.c_int
    return lib


def round_weights(w, convT, version):
    """Version `version` of the error-diffused bf16 rounding of one conv weight (ccn_commit_params: round_version)."""
    w = np.ascontiguousarray(w, np.float32)
    if convT:
        I, O, taps = w.shape[0], w.shape[1], 16
    else:
        O, I, taps = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
    out = np.empty((version + 1,) + w.shape, np.float32)
    assert _lib().ccn_internal_round_weights(w.ctypes.data, O, I, taps, 1 if convT else 0, version + 1, out.ctypes.data) == 0
    return out[version]


def bf16(x):
    return x.to(torch.bfloat16).to(torch.float64)


def half_ulp(m, bits):
    """Half an ulp of a float with `bits` significant bits at magnitude m (>= 0)."""
    return torch.exp2(torch.floor(torch.log2(m.clamp_min(1e-30))) - bits)


def hu16(m):
    return half_ulp(m, 8)


# ---- the network as a list of layers ------------------------------------------------------------------------------------------
def layer_list(ch_mult):
    """(name written, kind, input tap, residual tap, weight key, norm key, film key) in plan order (ccn_api.hip build_arch)."""
    L = [("in_conv", "stem", None, None, "in_conv", None, None)]
    prev, skips = "in_conv", []

    def res(p):
        nonlocal prev
        L.append((p + ".film", "c1", prev, None, p + ".conv1", p + ".norm1", p + ".film"))
        L.append((p, "c2", p + ".film", prev, p + ".conv2", p + ".norm2", None))
        prev = p
    n = len(ch_mult)
    for i in range(n):
        res(f"down.{3 * i}"); res(f"down.{3 * i + 1}")
        skips.append(prev)
        L.append((f"down.{3 * i + 2}", "down", prev, None, f"down.{3 * i + 2}", None, None)); prev = f"down.{3 * i + 2}"
    res("mid1"); res("mid2")
    for i in range(n):
        res(f"up.{3 * i}"); res(f"up.{3 * i + 1}")
        L.append((f"up.{3 * i + 2}", "up", prev, skips.pop(), f"up.{3 * i + 2}", None, None)); prev = f"up.{3 * i + 2}"
    L.append(("out", "head", prev, None, "out", "out_norm", None))
    return L


def tap_shapes(base, ch_mult, H, W):
    shapes, ch, h, w = {"in_conv": (base, H, W)}, base, H, W
    for name, kind, *_ in layer_list(ch_mult):
        if kind == "down":
            ch, h, w = ch * int(ch_mult[int(name.split(".")[1]) // 3]), h // 2, w // 2
        elif kind == "up":
            ch, h, w = ch // int(ch_mult[len(ch_mult) - 1 - int(name.split(".")[1]) // 3]), h * 2, w * 2
        if kind != "head":
            shapes[name] = (ch, h, w)
    return shapes


# ---- float64 pieces ---------------------------------------------------------------------------------------------------------
def rows(x, a, b):
    """rows [a, b) of x (N, C, H, W), zero rows outside [0, H)"""
    H = x.shape[2]
    y = x[:, :, max(a, 0):min(b, H)]
    return F.pad(y, (0, 0, max(0, -a), max(0, b - H)))


def conv_rows(kind, x, w, r0, r1):
    """output rows [r0, r1) of the layer's convolution (all columns) from the input x"""
    if kind == "up":                                    # ConvTranspose2d(4, stride 2, padding 1); r0, r1 even
        s0, s1 = max(r0 // 2 - 1, 0), min(r1 // 2 + 1, x.shape[2])
        return F.conv_transpose2d(x[:, :, s0:s1], w, stride=2, padding=1)[:, :, r0 - 2 * s0:r1 - 2 * s0]
    if kind == "down":
        return F.conv2d(rows(x, 2 * r0 - 1, 2 * r1), w, stride=2, padding=(0, 1))
    return F.conv2d(rows(x, r0 - 1, r1 + 1), w, padding=(0, 1))


def gn_affine(x, gamma, beta, G, pad_hw=None):
    """per (sample, channel) scale a and shift c of GroupNorm(x) in float64; pad_hw = (Hp, Wp): statistics that also count the
    zero padding of partial tiles (a deliberately wrong reference)"""
    N, C, H, W = x.shape
    g = min(G, C)
    xs = x.reshape(N, g, -1)
    cnt = xs.shape[2] if pad_hw is None else (C // g) * pad_hw[0] * pad_hw[1]
    mean = xs.sum(2) / cnt
    var = (xs * xs).sum(2) / cnt - mean * mean
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    a = (gamma[None, :].reshape(1, g, -1) * rstd[:, :, None]).reshape(N, C)
    c = beta[None, :] - (mean.repeat_interleave(C // g, 1) * a)
    return a[:, :, None, None], c[:, :, None, None]


def mode_name(m):
    """the storage / arithmetic mode of a run: "bf16", "fp32" or "f16x3" (True / False: the former bf16_mode flag)"""
    if isinstance(m, str):
        assert m in ("bf16", "fp32", "f16x3"), m
        return m
    return "bf16" if m else "fp32"


def gn_chain_depth(route, C, G=8):
    """Longest chain of fp32 additions between one stored value and the partial sum that holds it, for a tensor of C channels written
    by the launch `route` in fp32 storage (fp32 and f16x3 modes).  From the kernels:

      tile/epilogue.inc (ws / fr, 512 threads) and the epilogue of conv_igemm_kernel (ccn_kernels.hip, 256 threads): thread (o, ps)
          owns 8 channels of the pixels ps, ps + PSL, ... of each 128-pixel pass, PSL = threads / (BN / 8): it adds 128 / PSL values
          per pass, th / 4 passes (the 4-wave kernel: one), into s1 (and fmaf(v, v, s2): one rounding per term as well)
      tile/gn_part_tail.inc: xor-shuffle levels NOCT, 2 NOCT, .. 32 with NOCT = BN / 8: log2(512 / BN) additions
          the waves in index order:                                                     NWAVES additions (8; 4-wave kernel: 4)
          the channels of one group inside the N tile in index order:                   min(cpg, BN) additions
      gn_group_stats (gn_act_fused_kernel, in-kernel finalize) / gn_finalize_kernel: the slots in double (2^-53 each: nothing next
          to the above), mean, var and rstd in double; one more step is charged for them.

    A value passes through at most that many roundings, each relative 2^-24 to a partial sum that is bounded by the sum of the
    absolute values: |sum_kernel - sum| <= gamma_D sum|x|, gamma_D = D u / (1 - D u) (Higham, Accuracy and Stability, section 4.2).
    D is 20 .. 51 for the layers of the test matrices (a few dozen: 2^-19 .. 2^-18), against the 4096 u that ETA charged."""
    bn = 128 if C >= 128 else (64 if C >= 64 else 32)        # conv_bn_for
    kern = route["kernel"]
    if kern in ("ws", "fr"):
        threads, nwaves, passes = 512, 8, route["th"] // 4
    elif kern == "igemm":
        threads, nwaves, passes = 256, 4, 1
    else:
        raise AssertionError(f"no GroupNorm summation model for a tensor written by {kern!r} in fp32 storage")
    noct = bn // 8
    per_pass = 128 // (threads // noct)
    levels = int(np.log2(64 // noct))
    cpg = C // min(G, C)
    return passes * per_pass + levels + nwaves + min(cpg, bn) + 1


def gn_coef_err(x, a, c, G, D):
    """Error of the kernels' fp32 GroupNorm coefficients against the float64 (a, c) of gn_affine, from the data: (relative error of
    a, absolute error of c), per (sample, channel).  With gamma = gamma_D of gn_chain_depth and E.. the means over a group:

        |d mean|  <= gamma E|x|                              (sum of the stored values, the same fp32 values the tap returns)
        |d E[x^2]| <= gamma E[x^2]                            (all terms positive)
        |d var|   <= gamma (E[x^2] + 2 |mean| E|x|) + (d mean)^2          var = E[x^2] - mean^2 in double
        rstd      =  (var + eps)^-1/2:  relative error (1 - |d var| / (var + eps))^-1/2 - 1
                     -- this is where the cancellation factor E[x^2] / var enters
        a = fp32(gamma_c rstd):         relative error of rstd, then 2^-24
        c = fp32(beta_c - mean a):      |a| (|d mean| + |mean| rel(rstd)) (1 + rel(rstd)), then 2^-24 |c|"""
    N, C, H, W = x.shape
    g = min(G, C)
    xs = x.reshape(N, g, -1)
    gam = D * U32 / (1 - D * U32)
    m1, m2, mean = xs.abs().mean(2), (xs * xs).mean(2), xs.mean(2)
    var = m2 - mean * mean
    dmean = gam * m1
    dvar = gam * (m2 + 2 * mean.abs() * m1) + dmean * dmean
    rel = (1 - dvar / (var + 1e-5)).clamp_min(1e-30) ** -0.5 - 1
    rep = lambda v: v.repeat_interleave(C // g, 1)[:, :, None, None]
    eta_a = (1 + rep(rel)) * (1 + U32) - 1
    dc = a.abs() * (rep(dmean) + rep(mean.abs()) * rep(rel)) * (1 + rep(rel)) + U32 * c.abs()
    return eta_a, dc


def operand(x, a, c, silu, mode, coef_err=None):
    """MFMA operand of a GroupNorm input and the width of its uncertainty: bf16 mode -> (bf16(y), hi - lo) where [lo, hi] holds every
    rounding the kernel may produce from its fp32 statistics; fp32 / f16x3 mode -> (y, bound on the kernel's operand error) with the
    coefficient error of gn_coef_err: z = fmaf(x, a, c) rounds once, SiLU (slope at most 1.1) is y / (1 + expf(-y)) with a
    full-precision expf and a true division, 4 roundings' worth"""
    mode = mode_name(mode)
    z = x * a + c
    y = z * torch.sigmoid(z) if silu else z
    if mode == "bf16":
        d = (1.1 if silu else 1.0) * ETA * ((x * a).abs() + c.abs()) + (SILU_REL if silu else 4 * U32) * y.abs()
        return bf16(y), bf16(y + d) - bf16(y - d)
    eta_a, dc = coef_err
    dz = (x * a).abs() * eta_a + dc
    dz = dz + U32 * (z.abs() + dz)
    return y, (1.1 if silu else 1.0) * dz + 4 * U32 * y.abs()


def bands(Hout, T, even, rng):
    """output row bands: the first rows, a tile seam (multiple of T rows) in the middle, the last (partial) row tile with the row
    before it, and a random interior band; all columns (so every column seam and the last partial column tile)"""
    b = [(0, 3)]
    k = (Hout // T) // 2
    b.append((k * T - 2, k * T + 2))
    b.append((((Hout - 1) // T) * T - 1, Hout))
    r = int(rng.integers(4, Hout - 6))
    b.append((r, r + 3))
    if even:
        b = [(lo - lo % 2, hi + hi % 2) for lo, hi in b]
    b = sorted((max(lo, 0), min(hi, Hout)) for lo, hi in b)
    out = []
    for lo, hi in b:
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


class Source:
    """What one run of the library left behind: taps (float64, selected samples), the input image, eps, conditioning."""

    def __init__(self, sd, ch_mult, x_in, eps, h, tap_fn, samples, version, bf16_mode, routes):
        self.sd, self.ch_mult, self.x_in, self.eps, self.h = sd, ch_mult, x_in, eps, h
        self.tap_fn, self.samples, self.version, self.routes = tap_fn, samples, version, routes
        self.mode = mode_name(bf16_mode)              # "bf16", "fp32" or "f16x3" (a bool: bf16 or fp32)
        self.bf16_mode = self.mode == "bf16"
        self._taps, self._w = {}, {}

    def tap(self, name):
        if name not in self._taps:
            self._taps[name] = self.tap_fn(name)
        return self._taps[name]

    def weight(self, key, kind):
        if key not in self._w:
            w = self.sd[key + ".weight"]
            if not self.bf16_mode:
                v = w
            elif kind == "head":
                v = torch.from_numpy(np.ascontiguousarray(w, np.float32)).to(torch.bfloat16).float().numpy()   # packed round-to-nearest
            else:
                v = round_weights(w, kind == "up", self.version)
            self._w[key] = torch.from_numpy(np.asarray(v, np.float64))
        return self._w[key]


# ---- f16x3: the split operands and the omission references of criterion (a) ---------------------------------------------------------
SLICE_K_MAX = 1152        # the single-slice omission is asserted on layers with K <= 1152 (64- and 128-channel 3x3 convs, ConvTransposes
                          # with Cin <= 256); on wider layers its share is too small to tell from fp32 accumulation: printed only
OMIT_FACTOR = 10          # RMS(omission reference - full) >= 10 RMS(got - full): test_gpu_split.test_conv_transpose_exact_operand_replay


def split_terms(kind, a32, w, Cin):
    """The halves the kernel multiplies (split_emulation.split = split_pack and the commit-time weight split, test_split_host.py),
    as float64: a_hi, a_lo of the fp32 operand; w_hi / s, w_lo / s of the weights scaled by their power of two s; and the channels
    [c0, Cin) of the last K = 16 slice that holds real channels (a partial 32-channel chunk ends in a slice of padding)."""
    import split_emulation
    w32 = w.float()
    sc = split_emulation.weight_scale(w32)
    wh, wl = split_emulation.split(w32 * sc)
    ah, al = split_emulation.split(a32.float())
    return dict(scale=sc, wh=wh.double() / sc, wl=wl.double() / sc, ah=ah.double(), al=al.double(), c0=16 * ((Cin - 1) // 16))


def omissions(kind, sp, r0, r1):
    """{name: omission reference - full product, before the epilogue's gain} on output rows [r0, r1), float64:
      alwh   a_lo w_hi omitted everywhere: a_hi (w_hi + w_lo) in place of the full product
      ahwl   a_hi w_lo omitted everywhere: (a_hi + a_lo) w_hi
      slice  a_lo w_hi omitted in one K = 16 slice, the last step of the K loop (tile/split_steps.inc: last slice of the last tap of
             the last Cin chunk, where the fetch one term ahead ends): tap (2, 2) of a 3x3 conv; of a ConvTranspose the fourth tap of
             each output parity (fill_taps: kernel rows / columns 3 for even outputs, 2 for odd ones)"""
    ah, al, wh, wl, c0 = sp["ah"], sp["al"], sp["wh"], sp["wl"], sp["c0"]
    ws = torch.zeros_like(wh[:, c0:] if kind != "up" else wh[c0:])
    if kind == "up":
        ws[:, :, 2:4, 2:4] = wh[c0:, :, 2:4, 2:4]
    else:
        ws[:, :, 2, 2] = wh[:, c0:, 2, 2]
    # (the convolution is linear and float64 here: a_hi (w_hi + w_lo) - (a_hi + a_lo)(w_hi + w_lo) = -a_lo (w_hi + w_lo), and so on)
    return {"alwh": -conv_rows(kind, al, wh + wl, r0, r1), "ahwl": -conv_rows(kind, ah + al, wl, r0, r1),
            "slice": -conv_rows(kind, al[:, c0:], ws, r0, r1)}


def replay_layer(src, layer, G=8, rng=None, check_wrong=True, band_px=96 * 96):
    """max bound ratio, RMS error in output ulps and the wrong references' violated shares of one layer"""
    name, kind, inp, resn, wkey, nkey, fkey = layer
    route = src.routes[name]
    bfm = src.bf16_mode
    mode = src.mode
    split = route.get("ops") == "f16x3"
    assert (mode == "f16x3") == ("ops" in route) and route.get("ops", "f32") in ("f32", "f16x3"), (mode, route)
    if split:       # the only launches with a model for split operands: tile/split_steps.inc in ccn_conv_ws.hip / ccn_conv_fr.hip
        assert route["kernel"] in ("ws", "fr") and route["kind"] in ("C3S1", "CT4") and route["ksplit"] == 1, route
    sd = src.sd
    ks = route["ksplit"]
    kern = route["kernel"]
    w = src.weight(wkey, kind)
    b = torch.from_numpy(np.asarray(sd[wkey + ".bias"], np.float64))
    head2 = kern == "head2"
    # ---- the operand and its uncertainty
    if kind == "stem":
        x = src.x_in
        op, dop = (bf16(x) if bfm else x), torch.zeros_like(x)
        if kern == "stem2":
            b = bf16(b)
    else:
        x = src.tap(inp)
        if nkey:
            gam = torch.from_numpy(np.asarray(sd[nkey + ".weight"], np.float64)); bet = torch.from_numpy(np.asarray(sd[nkey + ".bias"], np.float64))
            ga, gc = gn_affine(x, gam, bet, G)
            # fp32 storage: the coefficient error from the summation chain of the launch that wrote the input and its partial sums
            cerr = None if bfm else gn_coef_err(x, ga, gc, G, gn_chain_depth(src.routes[inp], x.shape[1], G))
            if head2:
                op, dop = x, torch.zeros_like(x)
            else:
                op, dop = operand(x, ga, gc, kind != "head", mode, cerr)
        else:
            op, dop = x, torch.zeros_like(x)
    N, Cin, Hin, Win = x.shape
    if split:
        # the kernel's operand is an fp32 value (the tap, or fp32 GroupNorm + SiLU of it: GnCoef<float>), split by split_pack
        dop = dop + U32 * op.abs()
        op = op.float().double()
        sp = split_terms(kind, op, w, Cin)
    K = 27 if kind == "stem" else Cin * (4 if kind == "up" else 9)
    if kern == "stem2":
        K += 1
    wa = w.abs()
    if kind == "up":
        Cout, Hout, Wout = w.shape[1], 2 * Hin, 2 * Win
    elif kind == "down":
        Cout, Hout, Wout = w.shape[0], Hin // 2, Win // 2
    else:
        Cout, Hout, Wout = w.shape[0], Hin, Win
    T = route["th"] * (2 if kind == "up" else 1)
    bl = bands(Hout, T, kind == "up", rng) if Hout * Wout > band_px else [(0, Hout)]
    got = src.eps if kind == "head" else src.tap(name)
    film = None
    if fkey:
        hh = src.h
        Ws, bs = (torch.from_numpy(np.asarray(sd[fkey + ".to_scale." + k], np.float64)) for k in ("weight", "bias"))
        Wt, bt = (torch.from_numpy(np.asarray(sd[fkey + ".to_shift." + k], np.float64)) for k in ("weight", "bias"))
        s = (hh @ Ws.T + bs)[:, :, None, None]; t = (hh @ Wt.T + bt)[:, :, None, None]
        ds = ETA_COND * (hh.abs() @ Ws.abs().T + bs.abs())[:, :, None, None]
        dt = ETA_COND * (hh.abs() @ Wt.abs().T + bt.abs())[:, :, None, None]
        film = (s, t, ds, dt)
    bb = b[None, :, None, None]
    ratios, sq, sr, nel = [], 0.0, 0.0, 0
    om_sq = {}                                           # f16x3: sum of squares of (omission reference - full), per omission
    viol = {"tap": [0, 0], "shift": [0, 0], "gnpad": [0, 0]}
    # wrong references: zeroed centre tap of one output channel, shifted last column tile, padded GroupNorm statistics
    o_bad = (Cout * 2) // 3
    wz = torch.zeros_like(w)
    if kind == "up":
        wz[:, o_bad, 1, 1] = w[:, o_bad, 1, 1]
    else:
        wz[o_bad, :, 1, 1] = w[o_bad, :, 1, 1]
    c0 = 32 * ((Win - 1) // 32)
    sh = op.clone()
    sh[:, :, :, c0:Win - 1] = op[:, :, :, c0 + 1:Win]
    gp = None
    if nkey and not head2 and (Win % 32 or Hin % route["th"]):
        th = route["th"]
        ga2, gc2 = gn_affine(x, gam, bet, G, pad_hw=(-(-Hin // th) * th, -(-Win // 32) * 32))
        gp = operand(x, ga2, gc2, kind != "head", mode, cerr)[0]
    if head2:
        aw = [ga[i, :, 0, 0][None, :, None, None] * w for i in range(N)]         # per-sample W' (out, in, 3, 3), float64
        cmask = [gc[i:i + 1] * torch.ones_like(x[i:i + 1]) for i in range(N)]
    for r0, r1 in bl:
        g = got[:, :, r0:r1]
        if head2:
            acc = torch.cat([conv_rows(kind, x[i:i + 1], aw[i], r0, r1) + conv_rows(kind, cmask[i], w, r0, r1) for i in range(N)])
            e = torch.cat([conv_rows(kind, x[i:i + 1].abs(), hu16(aw[i].abs() * (1 + ETA)) + (ETA + K * U32) * aw[i].abs(), r0, r1)
                           + (ETA + K * U32) * conv_rows(kind, cmask[i].abs(), wa, r0, r1) for i in range(N)])
            ref = acc + bb
            bound = e + 32 * U32 * (ref.abs() + bb.abs())
            dref = {}
            if check_wrong:
                dref["tap"] = torch.cat([conv_rows(kind, x[i:i + 1], ga[i, :, 0, 0][None, :, None, None] * wz, r0, r1) for i in range(N)])
        else:
            acc = conv_rows(kind, op, w, r0, r1)
            if split:
                # three fp32 accumulations per product; residuals of the two splits (2^-22 each: hi to 11 bits, lo to 11 more) and the
                # dropped a_lo w_lo (2^-12 2^-12); halves in fp16's subnormal range round to 2^-25 absolute: every activation (x sum|w|),
                # and the scaled weights (split_emulation.weight_scale: 2^-25 / scale each, x sum|a|)
                e_acc = (conv_rows(kind, op.abs(), (3 * K * U32 + 2.0 ** -21 + 2.0 ** -24) * wa + 2.0 ** -25 / sp["scale"], r0, r1)
                         + conv_rows(kind, dop + 2.0 ** -25, wa, r0, r1))
            else:
                A = conv_rows(kind, torch.cat([op.abs(), dop]), wa, r0, r1)
                e_acc = K * U32 * A[:N] + A[N:]
            dref = {"tap": conv_rows(kind, op, wz, r0, r1), "shift": conv_rows(kind, sh - op, w, r0, r1)} if check_wrong else {}
            if gp is not None and check_wrong:
                dref["gnpad"] = conv_rows(kind, gp - op, w, r0, r1)
            gain = 1.0
            if film is not None:
                s, t, ds, dt = film
                gain = (1 + s).abs()
                ref = (acc + bb) * (1 + s) + t
                ecd = (acc + bb).abs() * ds + dt
            else:
                res = src.tap(resn)[:, :, r0:r1] if resn else 0.0
                ref = acc + bb + res
                ecd = 0.0
            epi = 4 * U32 * ((acc + bb).abs() * gain + (ref - acc).abs() + ref.abs())
            if split:
                for kk, d in omissions(kind, sp, r0, r1).items():
                    om_sq[kk] = om_sq.get(kk, 0.0) + float(((d * gain) ** 2).sum())
            pts = ROUNDING[(kern, ks)] if (bfm and kind != "head") else ()
            e = gain * e_acc
            if "acc" in pts:
                e = gain * (e_acc + hu16(acc.abs() + e_acc))
            if "acc_half1" in pts:                                  # split-K: the halves of the 64-channel chunks
                half = (Cin // 64 // 2) * 64
                a1 = conv_rows(kind, op[:, :half], w[:, :half], r0, r1)
                a2 = acc - a1
                e1 = e_acc + hu16(a1.abs() + e_acc)
                e = e1 + hu16((a1 + bb).abs() + e1) + hu16(a2.abs() + e_acc)
            e = e + ecd + epi
            if "store" in pts:
                e = e + hu16(ref.abs() + e)
            bound = e
        for kk, d in dref.items():
            if kk == "tap" and film is not None:
                d = d * (1 + film[0])
            wrong = ref - d
            ch = d.abs() > 0
            viol[kk][0] += int(((g - wrong).abs() > bound)[ch].sum()); viol[kk][1] += int(ch.sum())
        err = (g - ref).abs()
        ratios.append(float((err / bound).max()))
        sq += float((err * err).sum()); sr += float((ref * ref).sum()); nel += err.numel()
    # RMS error in ulps of the layer's RMS output (an ulp of each element's own value would be dominated by outputs that cancel to ~0)
    ulp = 2 * float((hu16 if bfm else (lambda m: half_ulp(m, 24)))(torch.tensor((sr / nel) ** 0.5)))
    out = dict(name=name, route=f"{route['kind']}/{kern}/th{route['th']}/k{ks}/{route['gn']}", ratio=max(ratios),
               rms_ulp=(sq / nel) ** 0.5 / ulp, viol={k: (v[0] / v[1] if v[1] else None) for k, v in viol.items()})
    if split:
        # criterion (a): RMS(got - full) against RMS(omission reference - full), over every replayed output
        out["route"] += f"/bn{128 if Cout >= 128 else 64}"
        out["K"] = K
        out["rms_got"] = (sq / nel) ** 0.5
        out["omit"] = {kk: (v / nel) ** 0.5 / max(out["rms_got"], 1e-300) for kk, v in om_sq.items()}
    return out


def replay_all(src, layers, label, skip=(), rng_seed=0, check_wrong=True, band_px=96 * 96):
    """replay every layer, print one row each, return the rows"""
    rng = np.random.default_rng(rng_seed)
    out = []
    print(f"\n{label}")
    for L in layers:
        if L[0] in skip:
            continue
        r = replay_layer(src, L, rng=rng, check_wrong=check_wrong, band_px=band_px)
        v = r["viol"]
        print(f"  {r['name']:<14} {r['route']:<34} max ratio {r['ratio']:.3f}  rms {r['rms_ulp']:.3f} ulp   wrong refs violate: "
              + " ".join(f"{k} {'-' if x is None else f'{x:.2f}'}" for k, x in v.items())
              + ("" if "omit" not in r else f"   K {r['K']} rms(got - full) {r['rms_got']:.3e}, omissions / that: "
                 + " ".join(f"{k} {x:.1f}" + ("" if slice_asserted(r, k) else " (not asserted)") for k, x in r["omit"].items())))
        out.append(r)
    return out


def slice_asserted(r, k):
    return k != "slice" or r["K"] <= SLICE_K_MAX


def check_rows(rows):
    bad = [(r["name"], r["route"], r["ratio"]) for r in rows if not r["ratio"] <= 1.0]
    assert not bad, f"layers outside their rounding bound: {bad}"
    weak = [(r["name"], k, x) for r in rows for k, x in r["viol"].items() if x is not None and x < MIN_VIOLATED]
    assert not weak, f"wrong references that the bound does not reject: {weak}"
    # f16x3 split layers, criterion (a): the kernel is at least OMIT_FACTOR times closer (RMS) to the full product than each omission
    blunt = [(r["name"], r["route"], k, x) for r in rows for k, x in r.get("omit", {}).items() if slice_asserted(r, k) and not x >= OMIT_FACTOR]
    assert not blunt, f"split layers no closer to the full product than to one with an omitted term: {blunt}"


def film_h(sd64, z, t):
    with torch.no_grad():
        return ref_unet.cond_vector(sd64, z.double(), t)


def nphase_of(sd):
    total = sum(int(np.prod(v.shape)) for v in sd.values() if np.asarray(v).ndim == 4)
    return 4 if total > 100_000_000 else 8


# ---- host-only self-check of the harness: an emulated bf16 chain must pass, the wrong references must not -------------------------
def emulate_bf16(src, layers, G=8):
    """taps of a bf16 network that rounds every stored activation once (the fr / ws rounding model), on the host"""
    for name, kind, inp, resn, wkey, nkey, fkey in layers:
        w = src.weight(wkey, kind)
        b = torch.from_numpy(np.asarray(src.sd[wkey + ".bias"], np.float64))[None, :, None, None]
        x = src.x_in if kind == "stem" else src.tap(inp)
        if kind == "stem":
            op = bf16(x)
        elif nkey:
            gam, bet = (torch.from_numpy(np.asarray(src.sd[nkey + k], np.float64)) for k in (".weight", ".bias"))
            ga, gc = gn_affine(x, gam, bet, G)
            op = operand(x, ga, gc, kind != "head", True)[0]
        else:
            op = x
        acc = conv_rows(kind, op, w, 0, x.shape[2] * (2 if kind == "up" else 1) // (2 if kind == "down" else 1))
        v = acc + b
        if fkey:
            Ws, bs = (torch.from_numpy(np.asarray(src.sd[fkey + ".to_scale." + k], np.float64)) for k in ("weight", "bias"))
            Wt, bt = (torch.from_numpy(np.asarray(src.sd[fkey + ".to_shift." + k], np.float64)) for k in ("weight", "bias"))
            v = v * (1 + (src.h @ Ws.T + bs)[:, :, None, None]) + (src.h @ Wt.T + bt)[:, :, None, None]
        if resn:
            v = v + src.tap(resn)
        if kind == "head":
            src.eps = v.float().double()
        else:
            src._taps[name] = bf16(v)


def test_replay_harness_self_check(synth):
    """Host only: the harness on a bf16 chain emulated in float64 with one rounding per stored activation (every layer within its
    bound, ratio well below 1), and the three wrong references of every layer rejected by that bound."""
    base, ch_mult, B, H, W = 32, (1, 2), 2, 24, 40
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, ch_mult))
    layers = layer_list(ch_mult)
    g = torch.Generator().manual_seed(11)
    x = torch.randn((B, 3, H, W), generator=g).double(); z = torch.from_numpy(synth.synth_z(B)); t = torch.tensor([900, 37])
    routes = {L[0]: dict(kind="", kernel="fr", th=4, ksplit=1, gn="none") for L in layers}
    routes["in_conv"]["kernel"] = "igemm"
    src = Source(sd, ch_mult, x, None, film_h(ref_unet.as_torch_sd(sd, torch.float64), z, t), None, [0, 1], 0, True, routes)
    emulate_bf16(src, layers)
    rows = replay_all(src, layers, "host self-check (emulated single-rounding bf16 chain)")
    check_rows(rows)
    # the bound is tight where the store is the only rounding: the emulated chain reaches most of its half ulp
    assert max(r["ratio"] for r in rows) > 0.5, max(r["ratio"] for r in rows)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------
C2 = (128, (1, 2, 2))
# (id, (base, ch_mult), B, H, W, conv variant or None): together they reach every route of ROUTES_BF16 (test_route_coverage)
BF16_CASES = [
    ("c2_bench", C2, 8, 256, 256, None),          # the bench shape: 8-row persistent kernel on the first level, 4-row deeper
    ("c2_b1_256", C2, 1, 256, 256, None),         # batch 1: every stride-2 conv on the generic kernel, 4-wave ConvTranspose
    ("c2_b16_128", C2, 16, 128, 128, None),       # split-K on the second and third stride-2 convs (128 eight-row tiles each)
    ("c2_3x72x104", C2, 3, 72, 104, None),        # ragged: partial row and column tiles at every level
    ("c2_5x136x200", C2, 5, 136, 200, None),
    ("c2_2x264x136", C2, 2, 264, 136, None),
    ("b192_3x200x168", (192, (1, 2)), 3, 200, 168, None),   # half-padded N tiles, generic stem / head widths
    ("b48_3x72x104", (48, (2, 1)), 3, 72, 104, None),       # BN 32 / 64: generic and 4-wave kernels only
    ("c2_fr_2x264x136", C2, 2, 264, 136, 3),      # conv variant 3: the free-running kernel in place of the persistent one
]
FP32_CASES = [("c2_3x72x104", C2, 3, 72, 104, None), ("b48_3x72x104", (48, (2, 1)), 3, 72, 104, None),
              ("c2_1x256x256", C2, 1, 256, 256, None)]
_SD = {}


def model_sd(synth, base, ch_mult):
    key = (base, tuple(ch_mult))
    if key not in _SD:
        _SD[key] = synth.synth_state_dict(synth.unet_param_spec(512, base, ch_mult))
    return _SD[key]


def make_net(sd, base, ch_mult, dtype):
    from clip_feature_codec.models.unet import CLIPCondUNet
    net = CLIPCondUNet(z_dim=512, base=base, ch_mult=ch_mult, dtype=dtype).to(DEV).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net


def run_forward(synth, case, dtype):
    """one forward through the C ABI; returns everything the replay needs"""
    _, (base, ch_mult), B, H, W, variant = case
    sd = model_sd(synth, base, ch_mult)
    lib = _lib()
    old = lib.ccn_internal_set_conv_variant(variant) if variant is not None else None
    try:
        net = make_net(sd, base, ch_mult, dtype)
        g = torch.Generator().manual_seed(B * 1000 + H + W)
        x = torch.randn((B, 3, H, W), generator=g); z = torch.from_numpy(synth.synth_z(B)); t = torch.randint(0, 1000, (B,), generator=g)
        eps = net(x.to(DEV), z.to(DEV), t.to(DEV))
        torch.cuda.synchronize()
        nat = net.native()
        nat.poll_errors()
        routes = plan_routes(nat)
    finally:
        if old is not None:
            lib.ccn_internal_set_conv_variant(old)
    return dict(sd=sd, net=net, nat=nat, x=x, z=z, t=t, eps=eps, routes=routes, base=base, ch_mult=ch_mult, B=B, H=H, W=W)


def make_source(run, samples, version, bf16_mode, t=None, device_temb=False):
    """bf16_mode: True / False or the mode's name.  device_temb: the conditioning vector in float64 from the timestep embedding the
    device computed (oracle.ref_unet.cond_vector's `temb`), so that cos / sin at up to 999 rad are not counted against the FiLM layers"""
    nat, B = run["nat"], run["B"]
    shapes = tap_shapes(run["base"], run["ch_mult"], run["H"], run["W"])
    idx = torch.tensor(samples, device=DEV)

    def tap_fn(name):
        return nat.read_activation(name, (B,) + shapes[name]).index_select(0, idx).double().cpu()
    sd64 = ref_unet.as_torch_sd(run["sd"], torch.float64)
    t = run["t"] if t is None else t
    if device_temb:
        from clip_feature_codec import _native
        temb = _native.timestep_embedding(t[samples].to(DEV), int(sd64["time_proj.0.weight"].shape[1])).cpu().double()
        with torch.no_grad():
            h = ref_unet.cond_vector(sd64, run["z"][samples].double(), t[samples], temb=temb)
    else:
        h = film_h(sd64, run["z"][samples], t[samples])
    eps = run["eps"].index_select(0, idx).double().cpu() if run["eps"] is not None else None
    return Source(run["sd"], run["ch_mult"], run["x"][samples].double(), eps, h, tap_fn, samples, version, bf16_mode, run["routes"])


def replay_case(synth, case, dtype, only_split=False, one_per_class=False, band_px=96 * 96):
    """only_split: the f16x3 layers on split operands only.  one_per_class: the first layer of every route class -- the whole route
    line but the name (kernel, tile rows, N tiles, input form, FiLM / residual, operands) and the layer's widths"""
    run = run_forward(synth, case, dtype)
    B = run["B"]
    src = make_source(run, sorted({0, B // 2, B - 1}), 0, dtype, device_temb=dtype == "f16x3")
    layers = layer_list(run["ch_mult"])
    if only_split:
        layers = [L for L in layers if run["routes"][L[0]].get("ops") == "f16x3"]
    if one_per_class:
        first = {}
        for L in layers:
            r = run["routes"][L[0]]
            first.setdefault(tuple(sorted((k, v) for k, v in r.items() if k != "name")) + tuple(run["sd"][L[4] + ".weight"].shape), L)
        layers = list(first.values())
    rows = replay_all(src, layers, f"{case[0]} {dtype}: B={B} {run['H']}x{run['W']} (samples {src.samples})", rng_seed=B + run["H"],
                      band_px=band_px)
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("case", BF16_CASES, ids=[c[0] for c in BF16_CASES])
def test_bf16_layer_replay(synth, case):
    """bf16 mode, every layer of one forward against its float64 replay within the route's rounding bound; the wrong references
    of every layer violate that bound on most of the outputs they change."""
    check_rows(replay_case(synth, case, "bf16"))


@pytest.mark.gpu
@pytest.mark.parametrize("case", FP32_CASES, ids=[c[0] for c in FP32_CASES])
def test_fp32_layer_replay(synth, case):
    """fp32 mode through the same harness (fr / ws / generic kernels, fp32 activations, exact fp32 weights): bound = fp32 accumulation
    (K 2^-24 sum|a||w|) + the operand's GroupNorm error + epilogue / conditioning terms; no bf16 rounding point."""
    check_rows(replay_case(synth, case, "fp32"))


@pytest.mark.gpu
def test_route_coverage(synth):
    """The shape matrix reaches every route of the bf16 inference plan (ROUTES_BF16) and every input-GroupNorm form, as reported by
    the library for the plans it built; and every launch of those plans is of a route the replay has a rounding model for."""
    seen, forms, lines = set(), set(), []
    for case in BF16_CASES:
        run = run_forward(synth, case, "bf16")
        for r in run["routes"].values():
            key = (r["kind"], r["kernel"], r["th"], r["ksplit"])
            seen.add(key); forms.add(r["gn"])
            assert (r["kernel"], r["ksplit"]) in ROUNDING or (r["kind"] == "HEAD" and r["kernel"] == "igemm"), (case[0], r)
        lines.append(f"  {case[0]:<18} " + ", ".join(sorted({f"{r['kind']}/{r['kernel']}/th{r['th']}/k{r['ksplit']}" for r in run["routes"].values()})))
        del run
    print("\nroutes per case:\n" + "\n".join(lines))
    for key in sorted(ROUTES_BF16):
        print(f"  {'/'.join(map(str, key)):<22} {'reached' if key in seen else 'NOT REACHED'}")
    print("  input GroupNorm forms reached:", sorted(forms))
    assert ROUTES_BF16 <= seen, sorted(ROUTES_BF16 - seen)
    assert GN_FORMS_BF16 == forms, (sorted(GN_FORMS_BF16 - forms), sorted(forms - GN_FORMS_BF16))
    assert seen <= ROUTES_BF16, f"routes not in the table (add them with a comment): {sorted(seen - ROUTES_BF16)}"


RMS_SPLIT = 0.47          # between the measured 0.41 (right weight version) and 0.53 (version 0), test_sampler_last_step_weight_version


def _rms(rows):
    return float(np.sqrt(np.mean([r["rms_ulp"] ** 2 for r in rows])))


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W", [(16, 128, 128), (8, 256, 256)])
def test_sampler_last_step_weight_version(synth, B, H, W):
    """ccn_sample with the captured graph (the product path), 4 DDIM steps: the last step runs on weight version 3 of the 8.  Every
    layer but the stem (whose input is not tapped) and the head (which updates the state in place) replayed with version 3 and the
    last step's t meets the same bounds; the same taps replayed with version 0 are clearly worse.  This is what would see the
    persistent kernel read the wrong weight version or a split-K half read a stale partial of the previous step (both shapes have
    split-K layers: the last two stride-2 convs at 16 x 128 px, the one into the 32-pixel level at the bench shape).

    Measured on an MI355X (RMS over the 34 layers, in ulps of each layer's RMS output): version 3 0.415 / 0.408, version 0 0.553 /
    0.534 (16 x 128 px / 8 x 256 px).  Version 0 puts 6 of the 34 layers outside their bound, all with exact operands: the stride-2
    convs (2.5 - 9.1 x the bound) and the ConvTranspose layers (4.8 - 25.8 x); behind a GroupNorm the operands' flip term hides one
    weight ulp.  Asserted: version 3 below RMS_SPLIT, version 0 above it, and at least 3 layers outside the bound with version 0."""
    from clip_feature_codec.diffusion.scheduler import NoiseScheduler
    sd = model_sd(synth, *C2)
    net = make_net(sd, *C2, "bf16")
    nat = net.native()
    steps = 4
    sch = NoiseScheduler(1000, "cosine", DEV)
    ts = sch.ddim_timesteps(steps); coef = sch.ddim_coefficients(steps, 0.0)[:, :4]
    g = torch.Generator().manual_seed(B + 77)
    x_T = torch.randn((B, 3, H, W), generator=g); z = torch.from_numpy(synth.synth_z(B))
    nat.sample(z.to(DEV), x_T.to(DEV), ts, coef, use_graph=True)
    torch.cuda.synchronize()
    nat.poll_errors()
    k = (steps - 1) % nphase_of(sd)
    assert k != 0
    run = dict(sd=sd, net=net, nat=nat, x=x_T, z=z, t=None, eps=None, routes=plan_routes(nat), base=C2[0], ch_mult=C2[1], B=B, H=H, W=W)
    print("\nsplit-K layers of this plan:", [n for n, r in run["routes"].items() if r["ksplit"] == 2])
    assert any(r["ksplit"] == 2 for r in run["routes"].values())
    samples = sorted({0, B // 2, B - 1})
    t_last = torch.full((B,), int(ts[-1]), dtype=torch.int64)
    src_k = make_source(run, samples, k, True, t=t_last)
    src_0 = make_source(run, samples, 0, True, t=t_last)
    src_0._taps = src_k._taps
    skip = ("in_conv", "out")
    rows_k = replay_all(src_k, layer_list(C2[1]), f"sampler B={B} {H}x{W}, last step (t={int(ts[-1])}) against weight version {k}", skip)
    rows_0 = replay_all(src_0, layer_list(C2[1]), "... the same taps against weight version 0", skip, check_wrong=False)
    rk, r0 = _rms(rows_k), _rms(rows_0)
    n_out = sum(r["ratio"] > 1 for r in rows_0)
    print(f"RMS over layers: version {k} {rk:.3f} ulp, version 0 {r0:.3f} ulp; layers outside the bound with version 0: {n_out}/{len(rows_0)}")
    check_rows(rows_k)
    assert rk < RMS_SPLIT < r0 and n_out >= 3, (rk, r0, n_out)
