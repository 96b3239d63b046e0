"""The training step's backward kernels, one family at a time, against float64 references with derived bounds.

The whole-step bf16 tests of tests/test_gpu_train.py ask for a cosine above 0.97 per gradient tensor; a weight-gradient workgroup that drops
its last pixel tile or a GroupNorm backward that skips a partial block passes them.  Here each kernel family is launched alone, through
the hooks ccn_internal_wgrad / ccn_internal_gn_bwd / ccn_internal_colsum (thin wrappers over the launch_* functions of the step, in the
step's order), on seeded operands the test supplies, every value a bf16 number: the float64 reference has nothing to model but the
operation, every output has one rounding point, and the bound follows from the kernel's summation depth (tests/train_kernel_ref.py, which
tests/test_train_kernel_ref_host.py holds to autograd, to correct fp32 arithmetic and to the bug classes).  Every case asserts
max|got - ref| / bound <= 1 per output and prints the worst ratio.  Gradient destinations start at a non-zero pattern ("adds to"), every
scratch buffer at NaN, and every destination has a guard band behind it that must come back untouched.

The last test runs whole bf16 steps and holds every conv weight's gradient, and the biases that are column sums, to the operands the
step itself left in its workspace (regions named by ccn_internal_train_layout): the wiring between the kernels pinned above.
"""
import ctypes
import math
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "clip-neural-image-conpression_amd"), str(Path(__file__).resolve().parent)]

from clip_feature_codec import _native  # noqa: E402
import train_kernel_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
I32, SZ, VP = ctypes.c_int32, ctypes.c_size_t, ctypes.c_void_p
EINVAL = 1


def lib():
    L = _native.load_library()
    L.ccn_internal_wgrad.restype = ctypes.c_int
    L.ccn_internal_wgrad.argtypes = [I32, I32, VP, VP, I32, VP] + [I32] * 8 + [VP, SZ, VP, VP, ctypes.POINTER(I32), ctypes.POINTER(I32), ctypes.POINTER(SZ)]
    L.ccn_internal_gn_bwd.restype = ctypes.c_int
    L.ccn_internal_gn_bwd.argtypes = [I32] + [VP] * 7 + [I32] * 6 + [VP] * 7 + [SZ, VP, ctypes.POINTER(I32), ctypes.POINTER(SZ)]
    L.ccn_internal_colsum.restype = ctypes.c_int
    L.ccn_internal_colsum.argtypes = [I32, VP, I32, I32, I32, VP, SZ, VP, VP, ctypes.POINTER(SZ)]
    return L


def stream():
    return _native.current_stream(torch.device(DEV))


def elem(t, bf16_mode):
    """a float64 CPU tensor as the kernels' activation type on the device (its values are bf16 numbers: exact either way)"""
    return None if t is None else t.to(torch.bfloat16 if bf16_mode else torch.float32).to(DEV).contiguous()


def f32dev(t):
    return None if t is None else t.to(torch.float32).to(DEV).contiguous()


def ab_table(a, c):
    """the pair-interleaved scale / shift table: channels (2p, 2p + 1) -> {scale, scale, shift, shift} (GnCoef::load)"""
    B, C = a.shape
    return f32dev(torch.stack([a.reshape(B, C // 2, 2), c.reshape(B, C // 2, 2)], 2).reshape(B, 2 * C))


def nan_scratch(nbytes):
    return torch.full(((nbytes + 3) // 4 + 64,), float("nan"), dtype=torch.float32, device=DEV)


GUARD = 64


def guarded(t):
    """a device tensor with GUARD elements of a known pattern right behind it: (the tensor, the whole buffer)"""
    buf = torch.cat([t.reshape(-1), torch.full((GUARD,), 7.0, dtype=t.dtype, device=t.device)])
    return buf[:t.numel()].view(t.shape), buf


def guards_intact(*bufs):
    return all(bool((b[-GUARD:] == 7.0).all()) for b in bufs)


def worst(what, got, ref, bound):
    ratio = (got.double().cpu() - ref).abs() / bound
    assert not torch.isnan(ratio).any(), what
    r = float(ratio.max())
    print(f"{what}: worst |got - ref| / bound = {r:.4f}")
    return r


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------------
_WREF = {}


def wgrad_reference(cid, bf16_mode):
    key = (cid, bf16_mode)
    if key not in _WREF:
        d = R.wgrad_inputs(cid)
        d["ref"], d["S"], d["flip"] = R.wgrad_ref(d["kind"], d["x"], d["dy"], d["ab"], d["silu"], d["Civ"], d["Cov"], bf16_mode)
        _WREF[key] = d
    return _WREF[key]


def run_wgrad(d, cid, split, bf16_mode):
    kind, B, Hin, Win, Cin, Civ, Cout, Cov = R.WGRAD_CASES[cid][:8]
    L = lib()
    x, dy = elem(d["x"], bf16_mode), elem(d["dy"], bf16_mode)
    ab = ab_table(*d["ab"]) if d["ab"] is not None else None
    grad, grad_buf = guarded(f32dev(d["g0"]))
    ns, tiles, need = I32(), I32(), SZ()
    args = lambda scr, nbytes: (0 if not bf16_mode else 1, R.KINDS[kind], x.data_ptr(), _native.ptr(ab), 1 if d["silu"] else 0, dy.data_ptr(), B, Hin, Win, Cin,
                                Civ, Cout, Cov, split, scr, nbytes, grad.data_ptr(), stream(), ctypes.byref(ns), ctypes.byref(tiles), ctypes.byref(need))
    _native.check(L.ccn_internal_wgrad(*args(None, 0)))
    assert need.value == ns.value * (16 if kind == "CT4" else (1 if kind == "STEM" else 9)) * Cout * Cin * 4
    scr = nan_scratch(need.value)
    _native.check(L.ccn_internal_wgrad(*args(scr.data_ptr(), need.value)))
    torch.cuda.synchronize()
    assert guards_intact(grad_buf), "write past the Cov x Civ parameter"
    return grad.cpu(), ns.value, tiles.value


def check_wgrad(cid, bf16_mode):
    d = wgrad_reference(cid, bf16_mode)
    kind, B, Hin, Win = R.WGRAD_CASES[cid][:4]
    for split in R.WGRAD_CASES[cid][8]:
        got, ns, tiles = run_wgrad(d, cid, split, bf16_mode)
        assert tiles == R.wgrad_geom(kind, B, Hin, Win)[4]
        assert 1 <= ns <= tiles and (split <= 0 or ns == min(split, tiles))
        if cid == "d" and split == -1:
            assert tiles % ns != 0, "the side-stream count no longer leaves uneven tiles per split"
        bound = R.wgrad_bound(d["ref"], d["S"], d["flip"], d["g0"], tiles, ns)
        r = worst(f"wgrad {'bf16' if bf16_mode else 'fp32'} case {cid} {kind} split {split} -> nsplit {ns} of {tiles} tiles", got.reshape(d["ref"].shape),
                  d["g0"] + d["ref"], bound)
        assert r <= 1.0


@pytest.mark.parametrize("cid", list(R.WGRAD_CASES))
def test_wgrad_bf16(cid):
    check_wgrad(cid, True)


@pytest.mark.parametrize("cid", list(R.WGRAD_FP32))
def test_wgrad_fp32(cid):
    check_wgrad(cid, False)


# ---- GroupNorm (+SiLU) backward ----------------------------------------------------------------------------------------------------------
def run_gn_bwd(d, silu, alias, want_dbias, bf16_mode):
    B, HW, C = d["x"].shape
    G = d["G"]
    L = lib()
    x, addend = elem(d["x"], bf16_mode), elem(d["addend"], bf16_mode)
    dA, dA_buf = guarded(elem(d["dA"], bf16_mode))
    out, out_buf = (dA, dA_buf) if alias else guarded(torch.full_like(dA, float("nan")))
    ab = ab_table(d["a"], d["c"])
    stats = f32dev(torch.stack([d["mu"], d["rs"]], 2))
    gamma = f32dev(d["gamma"])
    gstat, gstat_buf = guarded(torch.full((B, G, 2), float("nan"), dtype=torch.float32, device=DEV))
    (dgamma, dgamma_buf), (dbeta, dbeta_buf) = guarded(f32dev(d["dgamma0"])), guarded(f32dev(d["dbeta0"]))
    bufs = [dA_buf, out_buf, gstat_buf, dgamma_buf, dbeta_buf]
    film = dfilm = None
    stride = 2 * C + 8                                                   # a row of a wider table, as in the step
    if d["film"] is not None:
        film = torch.zeros((B, stride), dtype=torch.float32, device=DEV)
        film[:, :C], film[:, C:2 * C] = f32dev(d["film"][0]), f32dev(d["film"][1])
        dfilm, dfilm_buf = guarded(torch.full((B, stride), float("nan"), dtype=torch.float32, device=DEV))
        bufs.append(dfilm_buf)
    dbias = None
    if want_dbias:
        dbias, dbias_buf = guarded(f32dev(d["dbias0"]))
        bufs.append(dbias_buf)
    geom, need = (I32 * 5)(), SZ()
    args = lambda scr, nbytes: (1 if bf16_mode else 0, x.data_ptr(), dA.data_ptr(), ab.data_ptr(), stats.data_ptr(), gamma.data_ptr(), _native.ptr(addend),
                                _native.ptr(film), stride if film is not None else 0, silu, B, HW, C, G, out.data_ptr(), gstat.data_ptr(), dgamma.data_ptr(),
                                dbeta.data_ptr(), _native.ptr(dfilm), _native.ptr(dbias), scr, nbytes, stream(), geom, ctypes.byref(need))
    _native.check(L.ccn_internal_gn_bwd(*args(None, 0)))
    scr = nan_scratch(need.value)
    _native.check(L.ccn_internal_gn_bwd(*args(scr.data_ptr(), need.value)))
    torch.cuda.synchronize()
    assert guards_intact(*bufs), "write past the end of a destination"
    got = dict(out=out, gstat=gstat, dgamma=dgamma, dbeta=dbeta)
    if dfilm is not None:
        assert bool(torch.isnan(dfilm[:, 2 * C:]).all()), "write into the spare floats of a dfilm row"
        got["dfilm"] = dfilm[:, :2 * C]
    if dbias is not None:
        got["dbias"] = dbias
    return {k: v.float().cpu() for k, v in got.items()}, dict(zip(("nslb", "pstep", "ppb", "nblk", "zblocks"), geom))


def check_gn_bwd(cid, combo, bf16_mode):
    silu, form, alias, pairs = combo
    d = R.gn_inputs(cid, form)
    val, bnd, mid = R.gn_bwd_ref(silu=silu, bf16_mode=bf16_mode, **d)
    got, geom = run_gn_bwd(d, silu, alias, pairs or form == "film", bf16_mode)
    assert geom == {k: v for k, v in mid["geom"].items() if k != "iters"}, (geom, mid["geom"])
    rs = {k: worst(f"gn_bwd {'bf16' if bf16_mode else 'fp32'} case {cid} silu {silu} {form} alias {alias} {k}", got[k], val[k], bnd[k]) for k in got}
    assert set(rs) >= {"out", "gstat", "dgamma", "dbeta"} and (form != "film" or "dfilm" in rs)
    assert all(r <= 1.0 for r in rs.values()), rs


@pytest.mark.parametrize("cid,combo", [(cid, c) for cid in R.GN_CASES for c in R.gn_combos(cid)])
def test_gn_bwd_bf16(cid, combo):
    check_gn_bwd(cid, combo, True)


@pytest.mark.parametrize("cid,combo", [(cid, c) for cid in R.GN_FP32 for c in R.gn_combos(cid)])
def test_gn_bwd_fp32(cid, combo):
    check_gn_bwd(cid, combo, False)


def pow2_ceil(v):
    return 2.0 ** math.ceil(math.log2(v))


def test_dsilu_constant():
    """dsilu<__bf16> alone: B = 1, HW = 1, dA = 1, a = 1, c = 0, so dbeta[c] = dsilu(x[c]) in fp32, undisturbed.  DSILU of the reference
    module is 4 x the worst |got - float64| / (1 + |y|), rounded up to a power of two, and at most SILU_REL."""
    C = 2048
    x = R.bf16(torch.linspace(-20, 20, C, dtype=torch.float64)).reshape(1, 1, C)
    one, zero = torch.ones((1, C), dtype=torch.float64), torch.zeros((1, C), dtype=torch.float64)
    d = dict(x=x, dA=torch.ones_like(x), a=one, c=zero, mu=torch.zeros((1, 8), dtype=torch.float64), rs=torch.ones((1, 8), dtype=torch.float64),
             gamma=one[0], G=8, addend=None, film=None, dgamma0=zero[0], dbeta0=zero[0], dbias0=zero[0])
    got, _ = run_gn_bwd(d, 1, 0, 0, True)
    y = x[0, 0]
    err = (got["dbeta"].double() - R.dsilu(y)).abs() / (1 + y.abs())
    i = int(err.argmax())
    measured = pow2_ceil(4 * float(err.max()))
    print(f"dsilu<bf16>: worst |got - float64| / (1 + |y|) = {float(err.max()):.3e} at y = {float(y[i]):.4f}; x 4, rounded up: 2^{int(math.log2(measured))}"
          f" (DSILU = 2^{int(math.log2(R.DSILU))}, cap 2^{int(math.log2(R.DSILU_CAP))})")
    assert measured <= R.DSILU_CAP, "a finding about the kernel, not a reason to raise the cap"
    assert measured == R.DSILU


# ---- column sum ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(R.COLSUM_CASES))
def test_colsum_bf16(cid):
    dy, db0 = R.colsum_inputs(cid)
    B, HW, C = dy.shape
    ref, bound = R.colsum_ref(dy, db0)
    L = lib()
    t, (db, db_buf), need = elem(dy, True), guarded(f32dev(db0)), SZ()
    _native.check(L.ccn_internal_colsum(1, t.data_ptr(), B, HW, C, None, 0, db.data_ptr(), stream(), ctypes.byref(need)))
    g = R.gn_bwd_geom(B, HW, C)
    assert need.value == B * g["nblk"] * C * 4
    if cid == "rows580":
        assert B * g["nblk"] == 580 and R.finalize_ygrid(580) == 8
    scr = nan_scratch(need.value)
    _native.check(L.ccn_internal_colsum(1, t.data_ptr(), B, HW, C, scr.data_ptr(), need.value, db.data_ptr(), stream(), ctypes.byref(need)))
    torch.cuda.synchronize()
    assert guards_intact(db_buf)
    assert worst(f"colsum case {cid} rows {B * g['nblk']}", db, ref, bound) <= 1.0


# ---- argument checks: rejected before anything is launched ----------------------------------------------------------------------------------
def test_hooks_reject_bad_arguments():
    L = lib()
    n = 1 << 14                                                          # sixteen 16 KB regions of zeros, one per argument
    buf = torch.zeros(16 * n // 4, dtype=torch.float32, device=DEV)
    q = [buf.data_ptr() + i * n for i in range(16)]
    need, ns, tl = SZ(), I32(), I32()
    out = (ctypes.byref(ns), ctypes.byref(tl), ctypes.byref(need))

    def wg(dtype=1, kind=0, x=q[0], dy=q[1], B=1, Hin=4, Win=8, Cin=8, Civ=8, Cout=8, Cov=8, split=0, scr=q[2], nbytes=n, grad=q[3]):
        return L.ccn_internal_wgrad(dtype, kind, x, None, 1, dy, B, Hin, Win, Cin, Civ, Cout, Cov, split, scr, nbytes, grad, stream(), *out)

    def gn(dtype=1, x=q[0], C=16, G=8, HW=4, B=1, film=None, dfilm=None, scr=q[9], nbytes=n, stride=0):
        return L.ccn_internal_gn_bwd(dtype, x, q[1], q[2], q[3], q[4], None, film, stride, 1, B, HW, C, G, q[5], q[6], q[7], q[8], dfilm, None, scr, nbytes, stream(),
                                     None, ctypes.byref(need))

    def cs(dy=q[0], B=1, HW=4, C=8, scr=q[1], nbytes=n, db=q[2]):
        return L.ccn_internal_colsum(1, dy, B, HW, C, scr, nbytes, db, stream(), ctypes.byref(need))

    assert wg() == 0 and gn() == 0 and cs() == 0                         # the baseline of each is accepted
    bad = {
        "wgrad null x": wg(x=None), "wgrad null grad": wg(grad=None), "wgrad B = 0": wg(B=0), "wgrad Cin % 8": wg(Cin=12, Civ=12),
        "wgrad fp32 Cout % 4": wg(dtype=0, Cout=6, Cov=6), "wgrad odd Hin on C3S2": wg(kind=1, Hin=5), "wgrad bad kind": wg(kind=4),
        "wgrad Civ > Cin": wg(Civ=9), "wgrad small scratch": wg(nbytes=64), "wgrad bad dtype": wg(dtype=2),
        "gn_bwd null x": gn(x=None), "gn_bwd C % 8": gn(C=12, G=4), "gn_bwd HW = 0": gn(HW=0), "gn_bwd C % G": gn(C=16, G=3),
        "gn_bwd small scratch": gn(nbytes=64), "gn_bwd film without dfilm": gn(film=q[10], stride=32), "gn_bwd short film row": gn(film=q[10], dfilm=q[11], stride=16),
        "colsum null db": cs(db=None), "colsum C % 8": cs(C=4), "colsum B < 0": cs(B=-1), "colsum small scratch": cs(nbytes=16),
    }
    torch.cuda.synchronize()
    wrong = {k: v for k, v in bad.items() if v != EINVAL}
    assert not wrong, wrong
    assert L.ccn_last_error()


# ---- whole-step wiring: every conv weight gradient against the operands the step itself used ------------------------------------------------
CH_MULT, TIME_DIM = (1, 2), 256
STEP_CASES = {"base64": (64, 2, 40, 72), "base128": (128, 4, 64, 64)}


def hook_text(fn, *args):
    fn.restype = ctypes.c_int
    n = fn(*args, None, 0)
    assert n > 0
    buf = ctypes.create_string_buffer(n + 1)
    assert fn(*args, buf, n + 1) == n
    return buf.value.decode().splitlines()


def layer_table(base, H, W):
    """[(name, type, Cin, Cout, Hin, Win)] in forward order (build_arch, ccn_arch.h)"""
    out, ch, h, w = [("in_conv", "stem", 3, base, H, W)], base, H, W
    for i, m in enumerate(CH_MULT):
        out += [(f"down.{3 * i}", "res", ch, ch, h, w), (f"down.{3 * i + 1}", "res", ch, ch, h, w), (f"down.{3 * i + 2}", "down", ch, ch * m, h, w)]
        ch, h, w = ch * m, h // 2, w // 2
    out += [("mid1", "res", ch, ch, h, w), ("mid2", "res", ch, ch, h, w)]
    for i, m in enumerate(reversed(CH_MULT)):
        out += [(f"up.{3 * i}", "res", ch, ch, h, w), (f"up.{3 * i + 1}", "res", ch, ch, h, w), (f"up.{3 * i + 2}", "up", ch, ch // m, h, w)]
        ch, h, w = ch // m, h * 2, w * 2
    return out + [("out", "head", ch, 3, h, w)]


@pytest.mark.parametrize("cid", list(STEP_CASES))
def test_whole_step_weight_gradients_against_the_steps_own_operands(cid):
    from clip_feature_codec.models.unet import CLIPCondUNet
    from clip_feature_codec.utils import synth
    base, B, H, W = STEP_CASES[cid]
    L = lib()
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, CH_MULT))
    net = CLIPCondUNet(z_dim=512, base=base, ch_mult=CH_MULT, time_dim=TIME_DIM, dtype="bf16").to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    st = net.train().train_state()
    tr, flat = st.trainer, st.fp.flat
    gen = torch.Generator("cpu").manual_seed(77)
    x = torch.randn((B, 3, H, W), generator=gen).to(DEV)
    target = torch.randn((B, 3, H, W), generator=gen).to(DEV)
    z, t = torch.from_numpy(synth.synth_z(B)).to(DEV), torch.linspace(0, 999, B).round().long().to(DEV)
    g = torch.zeros_like(flat)
    eps = tr.forward(flat, x, z, t)
    _, d_eps = _native.mse_loss_grad(eps, target)
    tr.backward(flat, g, x, z, d_eps)
    torch.cuda.synchronize()
    routes = hook_text(L.ccn_internal_train_routes, tr.h)
    L.ccn_internal_train_layout.argtypes = [VP, I32, I32, I32, ctypes.c_char_p, SZ]
    regions = {}
    for ln in hook_text(L.ccn_internal_train_layout, tr.h, B, H, W)[:-1]:
        name, off, size = ln.split()
        regions[name] = (int(off[4:]), int(size[6:]))
    ws = tr.workspace(B, H, W)
    raw = ws.buf.cpu()
    shift = ws.ptr - ws.buf.data_ptr()
    gc = g.cpu()
    grads = {name: gc[off:off + torch.Size(shape).numel()].view(shape).double() for name, shape, off in tr.layout}
    print(f"{cid}: forward norm forms {sorted({ln for ln in routes if ln.startswith('norm')})}")

    def act(name, *shape):
        """region `name` as a bf16 NHWC tensor of exactly that size"""
        off, size = regions[name]
        assert size == 2 * math.prod(shape), (name, size, shape)
        return raw[shift + off:shift + off + size].clone().view(torch.bfloat16).view(shape).double()

    def table(name, Bn, C):
        off, size = regions[name]
        assert size == 8 * Bn * C, (name, size)
        v = raw[shift + off:shift + off + size].clone().view(torch.float32).view(Bn, C // 2, 2, 2).double()
        return v[:, :, 0].reshape(Bn, C), v[:, :, 1].reshape(Bn, C)

    layers = layer_table(base, H, W)
    kind_of = {"stem": "STEM", "res": "C3S1", "down": "C3S2", "up": "CT4", "head": "C3S1"}
    wg_lines = [dict(kv.split("=") for kv in ln.split()[2:]) | {"kind": ln.split()[1]} for ln in routes if ln.startswith("wgrad")]
    cs_lines = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in routes if ln.startswith("colsum")]
    wg_it, cs_it = iter(wg_lines), iter(cs_lines)
    worst_w, worst_b = (0.0, ""), (0.0, "")

    def check_w(pname, kind, xin, dy, Civ, Cov, ab=None, silu=False):
        nonlocal worst_w
        r = next(wg_it)
        assert r["kind"] == kind and int(r["cin"]) == xin.shape[3] and int(r["cout"]) == dy.shape[3], (pname, r)
        ref, S, flip = R.wgrad_ref(kind, xin, dy, ab, silu, Civ, Cov)
        got = grads[pname].reshape(ref.shape)
        ratio = float(((got - ref).abs() / R.wgrad_bound(ref, S, flip, torch.zeros_like(ref), int(r["tiles"]), int(r["nsplit"]))).max())
        worst_w = max(worst_w, (ratio, pname))
        assert ratio <= 1.0, (pname, ratio)

    def check_b(pname, dy):
        nonlocal worst_b
        r = next(cs_it)
        Bn, h, w, C = dy.shape
        ref, bound = R.colsum_ref(dy.reshape(Bn, h * w, C), torch.zeros(C, dtype=torch.float64))
        if r["src"] == "pairs":
            # The apply pass of the GroupNorm backward summed its fp32 results; the region holds their bf16 roundings.  A worst case that
            # grows with the pixel count (about N 2^-9 |dy|): wide enough that a dropped block would pass HERE.  This test is about the
            # wiring -- the right region, every sample, the right destination; the kernels are pinned by the cases above.
            bound = bound + R.half_ulp_bf16(dy.abs()).sum((0, 1, 2))
        ratio = float(((grads[pname] - ref).abs() / bound).max())
        worst_b = max(worst_b, (ratio, f"{pname} ({r['src']})"))
        assert ratio <= 1.0, (pname, r, ratio)

    def grad_region(i):
        """the gradient of layer i's output: where the next layer's backward left it"""
        name, typ, Cin, _, h, w = layers[i + 1]
        return act(name + (".g2" if typ == "res" else ".g"), B, h, w, Cin)

    for i in range(len(layers) - 1, -1, -1):                              # the backward pass's order, as the route lines
        name, typ, Cin, Cout, h, w = layers[i]
        if typ == "head":
            de = act("out.de", B, h, w, 8)
            assert float(de[..., 3:].abs().max()) == 0
            check_w("out.weight", "C3S1", act(layers[i - 1][0] + ".o", B, h, w, Cin), de, Cin, 3, table("out_norm.ab", B, Cin))
        elif typ == "res":
            dy2, dy1 = grad_region(i), act(name + ".g1", B, h, w, Cin)
            # the activated copies where the pre-pass (or the side form) wrote them, else the raw tensor with its norm's table
            pre = name + ".xa" in regions
            assert pre == (name + ".ya" in regions)
            in2 = (act(name + ".ya", B, h, w, Cin), None) if pre else (act(name + ".y", B, h, w, Cin), table(name + ".n2.ab", B, Cin))
            in1 = (act(name + ".xa", B, h, w, Cin), None) if pre else (act(layers[i - 1][0] + ".o", B, h, w, Cin), table(name + ".n1.ab", B, Cin))
            check_w(name + ".conv2.weight", "C3S1", in2[0], dy2, Cin, Cin, in2[1], silu=True)
            check_b(name + ".conv2.bias", dy2)
            check_w(name + ".conv1.weight", "C3S1", in1[0], dy1, Cin, Cin, in1[1], silu=True)
        elif typ in ("down", "up"):
            Hout, Wout = (h // 2, w // 2) if typ == "down" else (2 * h, 2 * w)
            dy = grad_region(i)
            assert dy.shape == (B, Hout, Wout, Cout)
            check_w(name + ".weight", kind_of[typ], act(layers[i - 1][0] + ".o", B, h, w, Cin), dy, Cin, Cout)
            check_b(name + ".bias", dy)
        else:
            dy = grad_region(i)
            check_b("in_conv.bias", dy)
            check_w("in_conv.weight", "STEM", act("in_conv.col", B, h, w, 32), dy, 27, Cout)
    assert next(wg_it, None) is None and next(cs_it, None) is None
    print(f"{cid}: worst weight-gradient ratio {worst_w[0]:.4f} ({worst_w[1]}), worst bias ratio {worst_b[0]:.4f} ({worst_b[1]})")
    del net, st, tr
    torch.cuda.empty_cache()
