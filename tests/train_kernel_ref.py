"""Float64 references and derived error bounds for the training step's backward kernels, one kernel family at a time.

Used by tests/test_gpu_train_kernels.py (the kernels alone, through the hooks ccn_internal_wgrad / ccn_internal_gn_bwd /
ccn_internal_colsum, on operands that are exactly representable in bf16) and by tests/test_train_kernel_ref_host.py (the references
against torch's float64 autograd; correct fp32 arithmetic inside the bounds; deliberately wrong results outside them).  No GPU needed.

Layouts are the kernels': activations NHWC, the GroupNorm scale / shift table per (sample, channel), (mean, rstd) per (sample, group).
All tables are the test's own fp32 values and enter the references as exact float64 numbers.

Bounds.  Nothing is fitted.  A summation tree of depth d over terms t_i is charged 1.01 d u sum|t_i|, d read from the kernels:

  weight gradient   u = 2^-23 (the MFMA's internal adds are not assumed to round to nearest); d = 128 ceil(tiles / nsplit) + nsplit:
                    a workgroup adds 128 pixels per 4 x 32 tile into its accumulator, wgrad_reduce adds the splits; the add into `grad`
                    is one more fp32 result.  Operand flips (bf16 roundings of GN(+SiLU) the kernel may decide differently) enter only with
                    a gn_ab table, as sum|hi - lo||dy| (the interval of tests/test_gpu_layer_replay.operand with ETA = 0).
  GroupNorm passes  u = 2^-24; d = iters + pstep + ceil(nblk / RL): a thread adds `iters` pixels, block_reduce16 the pstep pixel lanes, a
                    finalize lane every RL-th block row; the lanes are added in double.  Sums that reach their destination through
                    fp32 atomicAdds (dgamma, dbeta, dbias, db: one per sample or per row block, onto the value already there) count
                    those adds as further depth.
  elementwise       4 u per fp32 result; dsilu<__bf16> (v_exp / v_rcp): DSILU (1 + |y|) |dA|, DSILU measured on the device
                    (docs/EXPERIMENTS.md R13) and capped at the project's SILU_REL = 2^-18; dsilu<float>: 2^-20 (1 + |y|) |dA| (expf
                    within 2 ulp, a division and four more fp32 results, each relative to at most 1 + |y|).
  bf16 outputs      one rounding point: the error accumulated before it plus half a bf16 ulp at |v| + that error.
"""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
U_MFMA = 2.0 ** -23
SILU_REL = 2.0 ** -18          # bf16 mode's SiLU relative to its value (tests/test_gpu_layer_replay.py)
DSILU_CAP = 2.0 ** -18
DSILU = 2.0 ** -21             # measured on the MI355X: worst |got - float64| / (1 + |y|) = 8.175e-8 (at y = 0.1465) over 2048 bf16 values on
                               # [-20, 20]; x 4, rounded up to a power of two (docs/EXPERIMENTS.md R13); test_dsilu_constant re-measures it
DSILU_F32 = 2.0 ** -20
KINDS = {"C3S1": 0, "C3S2": 1, "CT4": 2, "STEM": 3}


def bf16(x):
    return x.to(torch.bfloat16).to(torch.float64)


def half_ulp_bf16(m):
    """half an ulp of a bf16 number of magnitude m (>= 0)"""
    return torch.exp2(torch.floor(torch.log2(m.clamp_min(2.0 ** -126))) - 8)


def rand_bf16(shape, gen, scale=1.0):
    return bf16(torch.randn(shape, generator=gen, dtype=torch.float64) * scale)


def f32(x):
    return x.to(torch.float32).to(torch.float64)


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------------
def wgrad_geom(kind, B, Hin, Win):
    """(Hout, Wout, MH, MW, tiles): conv_geom with 4-row tiles"""
    if kind == "C3S2":
        Hout, Wout = (Hin - 1) // 2 + 1, (Win - 1) // 2 + 1
        MH, MW = Hout, Wout
    elif kind == "CT4":
        Hout, Wout, MH, MW = 2 * Hin, 2 * Win, Hin, Win
    else:
        Hout, Wout, MH, MW = Hin, Win, Hin, Win
    return Hout, Wout, MH, MW, B * ((MH + 3) // 4) * ((MW + 31) // 32)


def wgrad_operand(x, ab, silu, bf16_mode=True):
    """(A, flip width): the kernel's A operand from x (B, H, W, C) and the table ab = (a, c), each (B, C); without a table x itself"""
    if ab is None:
        return x, None
    a, c = ab
    z = x * a[:, None, None, :] + c[:, None, None, :]
    y = z * torch.sigmoid(z) if silu else z
    d = (SILU_REL if (silu and bf16_mode) else 4 * U32) * y.abs()
    if not bf16_mode:
        return y, d
    return bf16(y), bf16(y + d) - bf16(y - d)


def wgrad_contract(kind, A, dy, pad_mode="zeros"):
    """sum over (sample, pixel) of dy x shifted A in the parameter's layout: Conv2d (O, I, kh, kw), ConvTranspose2d (I, O, 4, 4), 1x1 (O, I).
    pad_mode 'replicate' is a deliberately wrong halo, 'given' takes A with a one-pixel halo already around it (host test)."""
    B, Hin, Win, Cin = A.shape
    Cout = dy.shape[3]
    if kind == "STEM":
        return torch.einsum("byxo,byxi->oi", dy, A)
    if kind == "CT4":
        # out[2y - 1 + ky] += x[y] w[ky]
        dyp = F.pad(dy, (0, 0, 1, 1, 1, 1))
        g = A.new_zeros((Cin, Cout, 4, 4))
        for ky in range(4):
            for kx in range(4):
                g[:, :, ky, kx] = torch.einsum("byxi,byxo->io", A, dyp[:, ky:ky + 2 * Hin:2, kx:kx + 2 * Win:2])
        return g
    s = 2 if kind == "C3S2" else 1
    Hout, Wout = dy.shape[1], dy.shape[2]
    if pad_mode == "given":
        Ap = A
    elif pad_mode == "zeros":
        Ap = F.pad(A, (0, 0, 1, 1, 1, 1))
    else:
        Ap = F.pad(A.permute(0, 3, 1, 2), (1, 1, 1, 1), mode=pad_mode).permute(0, 2, 3, 1)
    g = A.new_zeros((Cout, Cin, 3, 3))
    for ky in range(3):
        for kx in range(3):
            g[:, :, ky, kx] = torch.einsum("byxo,byxi->oi", dy, Ap[:, ky:ky + s * Hout:s, kx:kx + s * Wout:s])
    return g


def wgrad_crop(kind, g, Civ, Cov):
    return g[:Civ, :Cov] if kind == "CT4" else g[:Cov, :Civ]


def wgrad_ref(kind, x, dy, ab=None, silu=True, Civ=None, Cov=None, bf16_mode=True):
    """float64 weight gradient of the kernel's operands, (ref, S, flip): S = sum|A||dy|, flip = sum|hi - lo||dy| (0 without a table)"""
    Civ = x.shape[3] if Civ is None else Civ
    Cov = dy.shape[3] if Cov is None else Cov
    A, w = wgrad_operand(x, ab, silu, bf16_mode)
    ref = wgrad_crop(kind, wgrad_contract(kind, A, dy), Civ, Cov)
    S = wgrad_crop(kind, wgrad_contract(kind, A.abs(), dy.abs()), Civ, Cov)
    flip = wgrad_crop(kind, wgrad_contract(kind, w, dy.abs()), Civ, Cov) if w is not None else torch.zeros_like(S)
    return ref, S, flip


def wgrad_bound(ref, S, flip, g0, tiles, nsplit):
    d = 128 * math.ceil(tiles / nsplit) + nsplit
    return 1.01 * d * U_MFMA * S + flip + 4 * U32 * (g0.abs() + ref.abs())


# ---- GroupNorm (+SiLU) backward, column sums ---------------------------------------------------------------------------------------------
def gn_bwd_geom(B, HW, C):
    """Python restatement of gn_bwd_geom (ccn_train_kernels.hip); asserted equal to what the hooks report"""
    nsl = C // 8
    nslb = min(nsl, 256)
    while nsl % nslb:
        nslb -= 1
    pstep = 256 // nslb
    minblk = max(512 // B, 32)
    iters = min(max(HW // (pstep * minblk), 1), 64)
    ppb = pstep * iters
    return dict(nslb=nslb, pstep=pstep, ppb=ppb, nblk=(HW + ppb - 1) // ppb, zblocks=nsl // nslb, iters=iters)


def finalize_ygrid(rows):
    return 8 if rows >= 512 else (4 if rows >= 64 else 1)


def dsilu(y):
    sg = torch.sigmoid(y)
    return sg * (1 + y * (1 - sg))


def colsum_ref(dy, db0):
    """(ref, bound) of db0 + the per-channel sum of dy (B, HW, C) as launch_colsum forms it"""
    B, HW, C = dy.shape
    g = gn_bwd_geom(B, HW, C)
    rows = B * g["nblk"]
    yg = finalize_ygrid(rows)
    d = g["iters"] + g["pstep"] + math.ceil(rows / (16 * yg)) + yg + 1
    ref = db0 + dy.sum((0, 1))
    return ref, 1.01 * d * U32 * (dy.abs().sum((0, 1)) + db0.abs())


def gn_bwd_ref(x, dA, a, c, mu, rs, gamma, G, silu, addend=None, film=None, bf16_mode=True, dsilu_rel=None,
               dgamma0=None, dbeta0=None, dbias0=None):
    """GroupNorm(+SiLU) backward exactly as the header comments of ccn_train.h state it.

    x, dA, addend (B, HW, C); a, c (B, C); mu, rs (B, G); gamma (C); film = (scale, shift), each (B, C).
      da = dA silu'(a x + c) (or dA);  xhat = (x - mean) rstd
      dgamma += sum da xhat;  dbeta += sum da;  per (sample, group): m1 = mean(gamma da), m2 = mean(gamma da xhat)
      dx = a da - rstd (m1 + xhat m2);  out = dx (1 + scale) [+ addend]
      FiLM: d shift = sum dx;  d scale = (sum dx x - shift sum dx) / (1 + scale);  dbias += sum over samples (1 + scale) sum dx
      no FiLM: dbias += sum out
    Returns values, bounds (same keys) and the per-element intermediates."""
    B, HW, C = x.shape
    cpg = C // G
    geo = gn_bwd_geom(B, HW, C)
    RL = 256 // (64 if cpg >= 64 else (32 if cpg >= 32 else 16))
    d1 = geo["iters"] + geo["pstep"] + math.ceil(geo["nblk"] / RL)
    zero = x.new_zeros(C)
    dgamma0 = zero if dgamma0 is None else dgamma0
    dbeta0 = zero if dbeta0 is None else dbeta0
    dbias0 = zero if dbias0 is None else dbias0
    ds_rel = (DSILU if bf16_mode else DSILU_F32) if dsilu_rel is None else dsilu_rel
    ab_, cb_ = a[:, None, :], c[:, None, :]
    grp = lambda t: t.repeat_interleave(cpg, 1)[:, None, :]             # (B, G) -> (B, 1, C)
    mub, rsb = grp(mu), grp(rs)

    if silu:
        y = x * ab_ + cb_
        da = dA * dsilu(y)
        e_da = dA.abs() * (ds_rel + 2 * U32) * (1 + y.abs()) + 4 * U32 * da.abs()
    else:
        da, e_da = dA, torch.zeros_like(dA)
    xh = (x - mub) * rsb
    e_xh = 4 * U32 * xh.abs()
    t2 = da * xh
    e_t2 = e_da * xh.abs() + da.abs() * e_xh
    # per (sample, channel) sums of pass 1 and their errors where finalize picks them up (double from there on)
    s1, s2 = da.sum(1), t2.sum(1)
    E1 = 1.01 * d1 * U32 * da.abs().sum(1) + e_da.sum(1)
    E2 = 1.01 * d1 * U32 * t2.abs().sum(1) + e_t2.sum(1)
    val, bnd = {}, {}
    dacc = (B + 1) * 1.01 * U32                                          # (float) of a sample's sum, then one atomicAdd per sample
    val["dbeta"] = dbeta0 + s1.sum(0)
    bnd["dbeta"] = E1.sum(0) + dacc * (s1.abs().sum(0) + dbeta0.abs())
    val["dgamma"] = dgamma0 + s2.sum(0)
    bnd["dgamma"] = E2.sum(0) + dacc * (s2.abs().sum(0) + dgamma0.abs())
    count = cpg * HW
    gsum = lambda t: t.reshape(B, G, cpg).sum(2)
    m1, m2 = gsum(gamma * s1) / count, gsum(gamma * s2) / count
    E_m1 = gsum(gamma.abs() * E1) / count + 4 * U32 * m1.abs()
    E_m2 = gsum(gamma.abs() * E2) / count + 4 * U32 * m2.abs()
    val["gstat"] = torch.stack([m1, m2], 2)
    bnd["gstat"] = torch.stack([E_m1, E_m2], 2)
    # pass 2
    m1b, m2b, E1b, E2b = grp(m1), grp(m2), grp(E_m1), grp(E_m2)
    inner = m1b + xh * m2b
    e_inner = E1b + xh.abs() * E2b + m2b.abs() * e_xh + 4 * U32 * (m1b.abs() + (xh * m2b).abs())
    dx = ab_ * da - rsb * inner
    e_dx = ab_.abs() * e_da + 4 * U32 * (ab_ * da).abs() + rsb.abs() * e_inner + 4 * U32 * (rsb * inner).abs() + 4 * U32 * dx.abs()
    fs = 1 + film[0][:, None, :] if film is not None else torch.ones_like(ab_)
    o = dx * fs + (addend if addend is not None else 0)
    e_o = fs.abs() * e_dx + 4 * U32 * (dx * fs).abs() + 4 * U32 * o.abs()
    val["out"] = o
    bnd["out"] = e_o + half_ulp_bf16(o.abs() + e_o) if bf16_mode else e_o
    d2 = geo["iters"] + geo["pstep"]
    if film is not None:
        df = d2 + math.ceil(geo["nblk"] / 16)
        sc, sft = fs[:, 0, :], film[1]
        p1, p2 = dx.sum(1), (dx * x).sum(1)
        Ep1 = 1.01 * df * U32 * dx.abs().sum(1) + e_dx.sum(1)
        Ep2 = 1.01 * df * U32 * (dx * x).abs().sum(1) + (e_dx * x.abs()).sum(1)
        dscale = (p2 - sft * p1) / sc
        val["dfilm"] = torch.cat([dscale, p1], 1)
        bnd["dfilm"] = torch.cat([(Ep2 + sft.abs() * Ep1 + 4 * U32 * (p2.abs() + (sft * p1).abs())) / sc.abs() + 4 * U32 * dscale.abs(),
                                  Ep1 + 4 * U32 * p1.abs()], 1)
        val["dbias"] = dbias0 + (sc * p1).sum(0)
        bnd["dbias"] = (sc.abs() * Ep1).sum(0) + (4 * U32 + dacc) * (sc * p1).abs().sum(0) + dacc * dbias0.abs()
    else:
        rows = B * geo["nblk"]
        yg = finalize_ygrid(rows)
        dp = d2 + math.ceil(rows / (16 * yg)) + yg + 1
        val["dbias"] = dbias0 + o.sum((0, 1))
        bnd["dbias"] = 1.01 * dp * U32 * (o.abs().sum((0, 1)) + dbias0.abs()) + e_o.sum((0, 1))
    return val, bnd, dict(da=da, xh=xh, dx=dx, fs=fs, geom=geo, e_out=e_o)


# ---- inputs of the test matrices (seeded, every operand value a bf16 number; tables fp32) ---------------------------------------------
# id -> (kind, B, Hin, Win, Cin, Civ, Cout, Cov, split choices, table form: None / "silu" / "nosilu")
WGRAD_CASES = {
    "a": ("C3S1", 1, 4, 32, 64, 64, 64, 64, (1,), None),
    "b": ("C3S1", 2, 10, 40, 64, 64, 64, 64, (5,), None),
    "c": ("C3S1", 3, 20, 72, 48, 48, 96, 96, (8,), None),
    "d": ("C3S1", 4, 64, 64, 128, 128, 128, 128, (0, -1), None),
    "e": ("C3S1", 1, 8, 32, 448, 448, 448, 448, (0,), None),
    "f": ("C3S1", 2, 12, 40, 128, 128, 8, 3, (0,), "nosilu"),
    "g": ("C3S1", 2, 10, 40, 64, 64, 64, 64, (0,), "silu"),
    "h": ("CT4", 2, 6, 40, 128, 128, 64, 64, (3,), None),
    "i": ("CT4", 1, 8, 32, 448, 448, 448, 448, (0,), None),
    "j": ("C3S2", 2, 18, 72, 64, 64, 128, 128, (0,), None),
    "k48": ("STEM", 2, 10, 40, 32, 27, 48, 48, (0,), None),
    "k128": ("STEM", 2, 10, 40, 32, 27, 128, 128, (0,), None),
}
WGRAD_FP32 = ("b", "h", "j")
# id -> (C, B, H, W); G = 8
GN_CASES = {1: (128, 2, 45, 41), 2: (128, 16, 32, 32), 3: (192, 3, 20, 24), 4: (384, 2, 12, 20), 5: (512, 2, 8, 16), 6: (768, 1, 8, 12),
            7: (3072, 1, 4, 8), 8: (48, 2, 10, 40), 9: (128, 1, 1, 3)}
GN_G = 8
# (silu, form, out aliased on dA, dbias from the pairs); every combination on cases 1, 3 and 7, two on the others
GN_COMBOS_FULL = [(1, "plain", 0, 1), (0, "plain", 1, 1), (1, "addend", 1, 0), (0, "addend", 0, 0), (1, "film", 1, 0), (0, "film", 0, 0)]
GN_COMBOS_SHORT = [(1, "addend", 1, 1), (1, "film", 0, 0)]
GN_FP32 = (1, 3)
COLSUM_CASES = {"gn1": (2, 45 * 41, 128), "gn3": (3, 20 * 24, 192), "gn7": (1, 32, 3072), "gn8": (2, 400, 48), "rows580": (5, 45 * 41, 128),
                "grid1": (1, 64, 128)}


def gn_combos(cid):
    return GN_COMBOS_FULL if cid in (1, 3, 7) else GN_COMBOS_SHORT


def wgrad_inputs(cid):
    kind, B, Hin, Win, Cin, Civ, Cout, Cov, _, form = WGRAD_CASES[cid]
    gen = torch.Generator("cpu").manual_seed(4000 + sum(map(ord, cid)))
    Hout, Wout, _, _, _ = wgrad_geom(kind, B, Hin, Win)
    x = rand_bf16((B, Hin, Win, Cin), gen)
    dy = rand_bf16((B, Hout, Wout, Cout), gen, 0.25)
    if kind == "STEM":
        x[..., Civ:] = 0                                                # im2col leaves columns 27..31 zero
    if Cov < Cout:
        dy[..., Cov:] = 0                                               # the head's d eps padded to 8 channels
    ab = None
    if form is not None:
        a = f32(1 + 0.3 * torch.randn((B, Cin), generator=gen, dtype=torch.float64))
        c = f32(0.5 * torch.randn((B, Cin), generator=gen, dtype=torch.float64))
        ab = (a, c)
    g0 = f32(0.01 * torch.randn((Civ, Cov, 4, 4) if kind == "CT4" else ((Cov, Civ) if kind == "STEM" else (Cov, Civ, 3, 3)), generator=gen,
                                dtype=torch.float64))
    return dict(kind=kind, x=x, dy=dy, ab=ab, silu=form != "nosilu", Civ=Civ, Cov=Cov, g0=g0)


def gn_inputs(cid, form):
    C, B, H, W = GN_CASES[cid]
    HW, G, cpg = H * W, GN_G, C // GN_G
    gen = torch.Generator("cpu").manual_seed(5000 + cid)
    rnd = lambda shape, s=1.0: torch.randn(shape, generator=gen, dtype=torch.float64) * s
    q = bf16                                                            # (fp32 mode takes the same bf16-valued operands)
    x = q(rnd((B, HW, C)) * (1 + 0.5 * rnd((1, 1, C)).abs()) + 0.3 * rnd((1, 1, C)))
    dA = q(rnd((B, HW, C), 0.25))
    xs = x.reshape(B, HW, G, cpg).permute(0, 2, 1, 3).reshape(B, G, -1)
    mu = f32(xs.mean(2))
    rs = f32(1 / torch.sqrt(xs.var(2, unbiased=False) + 1e-5))
    gamma = f32(1 + 0.3 * rnd((C,)))
    beta = f32(0.3 * rnd((C,)))
    a = f32(gamma[None, :] * rs.repeat_interleave(cpg, 1))
    c = f32(beta[None, :] - mu.repeat_interleave(cpg, 1) * a)
    d = dict(x=x, dA=dA, a=a, c=c, mu=mu, rs=rs, gamma=gamma, G=G, addend=None, film=None,
             dgamma0=f32(0.1 * rnd((C,))), dbeta0=f32(0.1 * rnd((C,))), dbias0=f32(0.1 * rnd((C,))))
    if form == "addend":
        d["addend"] = q(rnd((B, HW, C), 0.25))
    if form == "film":
        d["film"] = (f32(0.3 * rnd((B, C))), f32(0.3 * rnd((B, C))))
    return d


def colsum_inputs(cid):
    B, HW, C = COLSUM_CASES[cid]
    gen = torch.Generator("cpu").manual_seed(6000 + sum(map(ord, cid)))
    return rand_bf16((B, HW, C), gen, 0.25), f32(0.1 * torch.randn((C,), generator=gen, dtype=torch.float64))
