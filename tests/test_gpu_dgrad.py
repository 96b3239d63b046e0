"""The training step's data-gradient convolutions, one launch at a time, against float64 autograd with derived bounds.

The data gradients (conv_dgrad, family conv_data_grad) run on the inference kernels with swapped roles -- a 3x3 conv on flipped taps, a
ConvTranspose with the 3x3 kernel zero-padded to 4x4, a 4x4 stride-2 conv as four plane passes of 2x2 taps (the persistent kernel's P4
form, which exists for training only), stem_kernel on fp32 NCHW d eps -- on operands that eight device packers build every step.  The
whole-step bf16 tests of tests/test_gpu_train.py ask for a cosine above 0.97 per gradient tensor; a tile that drops its last ragged
column block, a plane pass that reads the wrong plane at the border or a pad channel leaking into the next pixel passes them.

Here the hook ccn_internal_conv_dgrad launches one data-gradient conv alone: the step's packer on the descriptor the route consumes,
Planner::conv_dgrad's route and arguments, Step::conv_dgrad's launch, on seeded operands that are bf16 numbers.  The reference is
torch.autograd in float64 through the forward op and the bound follows from the route's rounding points (tests/dgrad_ref.py, which
tests/test_dgrad_ref_host.py holds to correct fp32 arithmetic and to the bug classes).  Every case asserts max|got - ref| / bound <= 1
and prints the worst ratio; dx starts at NaN and has a guard band behind it that must come back untouched.  test_route_coverage asserts
that the cases still reach every route they were chosen for; the last test holds the hook to the step itself, bit for bit.
"""
import ctypes
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "clip-neural-image-conpression_amd"), str(Path(__file__).resolve().parent)]

from clip_feature_codec import _native  # noqa: E402
import dgrad_ref as R  # noqa: E402
import test_gpu_train_kernels as K  # noqa: E402  (guarded, guards_intact, worst, hook_text, layer_table: shared helpers)

pytestmark = pytest.mark.gpu
DEV = K.DEV
I32, SZ, VP = ctypes.c_int32, ctypes.c_size_t, ctypes.c_void_p
EINVAL = 1
CH_MULT, TIME_DIM = (1, 2), 256


def lib():
    L = _native.load_library()
    L.ccn_internal_conv_dgrad.restype = ctypes.c_int
    L.ccn_internal_conv_dgrad.argtypes = [VP, ctypes.c_char_p, VP, VP, VP, VP, I32, I32, I32, VP, ctypes.c_char_p, SZ]
    L.ccn_internal_set_conv_variant.restype = ctypes.c_int
    L.ccn_internal_set_conv_variant.argtypes = [ctypes.c_int]
    return L


def conv_dgrad(tr, weight, flat, dy, res, dx, B, H, W):
    """(return code, route line) of one hook call on device pointers"""
    route = ctypes.create_string_buffer(192)
    rc = lib().ccn_internal_conv_dgrad(tr.h, weight.encode() if weight is not None else None, flat, dy, res, dx, B, H, W, K.stream(), route, 192)
    return rc, route.value.decode()


# one trainer per configuration; the kernel choice is part of a trainer's plans, so it is created after the variant is switched
_TRAINERS, _REF, _RUN = {}, {}, {}


def trainer(base, dtype, variant):
    key = (base, dtype, variant)
    if key not in _TRAINERS:
        _TRAINERS[key] = _native.NativeTrainer(512, base, CH_MULT, TIME_DIM, 3, dtype=dtype, device=DEV)
    return _TRAINERS[key]


def reference(cid):
    """operands, float64 gradient and its scale: once per operand set, shared by the cases that run it on another kernel, never modified"""
    key = R.operand_key(cid)
    if key not in _REF:
        w, dy, res = R.inputs(cid)
        acc, S, ref = R.dgrad_ref(R.CASES[cid]["kind"], w, dy, res)
        _REF[key] = dict(w=w, dy=dy, res=res, acc=acc, S=S, ref=ref)
    return _REF[key]


def nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).to(dtype).to(DEV).contiguous()


def run_case(cid):
    """(route line, worst ratio) of a case; run once"""
    if cid in _RUN:
        return _RUN[cid]
    c, d = R.CASES[cid], reference(cid)
    bf = c["dtype"] == "bf16"
    et = torch.bfloat16 if bf else torch.float32
    L = lib()
    old = L.ccn_internal_set_conv_variant(c["variant"])
    try:
        tr = trainer(c["base"], c["dtype"], c["variant"])
        shape, off = next((s, o) for n, s, o in tr.layout if n == c["weight"])
        assert tuple(shape) == tuple(d["w"].shape), (shape, d["w"].shape)
        flat = torch.zeros(tr.total, dtype=torch.float32, device=DEV)             # only this conv's weight is read
        flat[off:off + d["w"].numel()] = d["w"].reshape(-1).to(torch.float32).to(DEV)
        dy = d["dy"].to(torch.float32).to(DEV).contiguous() if c["kind"] == "HEAD" else nhwc(d["dy"], et)     # the head's d eps: fp32 NCHW
        res = nhwc(d["res"], et) if d["res"] is not None else None
        Bn, Cn, Hx, Wx = d["ref"].shape
        dx, dx_buf = K.guarded(torch.full((Bn, Hx, Wx, Cn), float("nan"), dtype=et, device=DEV))
        rc, route = conv_dgrad(tr, c["weight"], flat.data_ptr(), dy.data_ptr(), _native.ptr(res), dx.data_ptr(), c["B"], c["H"], c["W"])
        _native.check(rc)
        torch.cuda.synchronize()
    finally:
        L.ccn_internal_set_conv_variant(old)
    assert K.guards_intact(dx_buf), "write past the end of dx"
    got = dx.double().cpu().permute(0, 3, 1, 2)
    assert not torch.isnan(got).any(), "an output the launch did not write"
    bound = R.dgrad_bound(c["kind"], route.split()[3], d["w"], d["acc"], d["S"], d["res"], bf)
    r = K.worst(f"dgrad {cid} [{route}]", got, d["ref"], bound)
    _RUN[cid] = (route, r)
    return _RUN[cid]


@pytest.mark.parametrize("cid", list(R.CASES))
def test_dgrad(cid):
    route, r = run_case(cid)
    assert route == R.CASES[cid]["route"], "the shape no longer reaches the route it was chosen for"
    assert r <= 1.0


def test_route_coverage():
    """the set of launches the cases made is the set they were chosen for: a threshold change that stops exercising a route fails here"""
    seen = {run_case(cid)[0] for cid in R.CASES}
    for ln in sorted(seen):
        print(ln)
    assert seen == {c["route"] for c in R.CASES.values()}
    kernels = {(ln.split()[2], ln.split()[3], ln.split()[4], ln.split()[7]) for ln in seen}
    assert kernels >= {("C3S1", "pr", "th=8", "four=0"), ("C3S1", "pr", "th=4", "four=0"), ("C3S1", "fr", "th=8", "four=0"), ("C3S1", "ws", "th=4", "four=0"),
                       ("C3S1", "igemm", "th=4", "four=0"), ("CT4", "pr", "th=8", "four=0"), ("CT4", "ws", "th=4", "four=0"), ("CT4", "fr", "th=8", "four=0"),
                       ("CT4", "igemm", "th=4", "four=0"), ("C3S2", "pr", "th=8", "four=1"), ("C3S2", "igemm", "th=4", "four=1"),
                       ("STEM", "stem2", "th=4", "four=0"), ("STEM", "igemm", "th=4", "four=0")}


def test_hook_rejects_bad_arguments():
    """CCN_EINVAL, and nothing launched: dx stays as it was"""
    tr = trainer(128, "bf16", 4)
    flat = torch.zeros(tr.total, dtype=torch.float32, device=DEV)
    dy = torch.zeros((1, 8, 40, 256), dtype=torch.bfloat16, device=DEV)            # large enough for every call below
    res0 = torch.zeros((1, 16, 80, 256), dtype=torch.bfloat16, device=DEV)
    dx = torch.full((1, 16, 80, 256), float("nan"), dtype=torch.bfloat16, device=DEV)
    call = lambda weight="down.0.conv1.weight", flat_=flat.data_ptr(), dy_=dy.data_ptr(), res=None, dx_=dx.data_ptr(), B=1, H=8, W=40: \
        conv_dgrad(tr, weight, flat_, dy_, res, dx_, B, H, W)[0]
    bad = {
        "unknown name": call(weight="down.0.conv3.weight"), "a bias": call(weight="down.0.conv1.bias"), "the stem's weight": call(weight="in_conv.weight"),
        "null name": call(weight=None), "null dx": call(dx_=None), "null dy": call(dy_=None), "null params": call(flat_=None), "B = 0": call(B=0),
        "W < 0": call(W=-8), "odd Hdy for the ConvTranspose's gradient": call(weight="up.2.weight", H=7), "odd Wdy likewise": call(weight="up.2.weight", W=39),
        "res where the step adds none": call(res=res0.data_ptr()),
    }
    torch.cuda.synchronize()
    wrong = {k: v for k, v in bad.items() if v != EINVAL}
    assert not wrong, wrong
    assert lib().ccn_last_error()
    assert bool(torch.isnan(dx).all()), "a rejected call launched something"
    assert call(weight="up.2.weight") == 0 and call(weight="down.5.weight", res=res0.data_ptr()) == 0       # the baselines are accepted


def test_hook_launches_what_the_step_launches():
    """One whole bf16 step; for the layers whose data-gradient output survives it (the stride-2 convs and the ConvTransposes: every
    3x3 and head gradient is overwritten in place by the GroupNorm backward behind it), the hook on the dy region the step left -- with
    the dskip region as res for the stride-2 convs, whose launch adds it -- gives the region the step wrote, bit for bit."""
    from clip_feature_codec.models.unet import CLIPCondUNet
    from clip_feature_codec.utils import synth
    base, B, H, W = 128, 4, 64, 64
    L = lib()
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, CH_MULT))
    net = CLIPCondUNet(z_dim=512, base=base, ch_mult=CH_MULT, time_dim=TIME_DIM, dtype="bf16").to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    st = net.train().train_state()
    tr, flat = st.trainer, st.fp.flat
    gen = torch.Generator("cpu").manual_seed(78)
    x = torch.randn((B, 3, H, W), generator=gen).to(DEV)
    target = torch.randn((B, 3, H, W), generator=gen).to(DEV)
    z, t = torch.from_numpy(synth.synth_z(B)).to(DEV), torch.linspace(0, 999, B).round().long().to(DEV)
    g = torch.zeros_like(flat)
    eps = tr.forward(flat, x, z, t)
    _, d_eps = _native.mse_loss_grad(eps, target)
    tr.backward(flat, g, x, z, d_eps)
    torch.cuda.synchronize()
    step_routes = [ln for ln in K.hook_text(L.ccn_internal_train_routes, tr.h) if ln.startswith("conv dgrad") and ln.split()[2] in ("CT4", "C3S2")]
    L.ccn_internal_train_layout.argtypes = [VP, I32, I32, I32, ctypes.c_char_p, SZ]
    regions = {}
    for ln in K.hook_text(L.ccn_internal_train_layout, tr.h, B, H, W)[:-1]:
        name, off, size = ln.split()
        regions[name] = (int(off[4:]), int(size[6:]))
    ws = tr.workspace(B, H, W)

    layers = K.layer_table(base, H, W)

    def grad_region(i):
        """the gradient of layer i's output: where the next layer's backward left it (name, pixels x channels checked against its size)"""
        name, typ, Cin, _, h, w = layers[i + 1]
        rname = name + (".g2" if typ == "res" else ".g")
        assert regions[rname][1] == 2 * B * h * w * Cin, rname
        return rname

    n_log = len(K.hook_text(L.ccn_internal_train_routes, tr.h))
    waiting, checked = [], []
    for i in range(len(layers) - 1, -1, -1):                                       # the backward pass's order, as the route lines
        name, typ, Cin, Cout, h, w = layers[i]
        if typ not in ("down", "up"):
            continue
        Hdy, Wdy = (h // 2, w // 2) if typ == "down" else (2 * h, 2 * w)
        dy = grad_region(i)
        assert regions[dy][1] == 2 * B * Hdy * Wdy * Cout
        # x = convT(xin) + skip: the gradient at an up layer's output waits for the stride-2 conv of the same level (a stack)
        if typ == "up":
            waiting.append(dy)
        res = waiting.pop() if typ == "down" else None
        off, size = regions[name + ".g"]
        assert size == 2 * B * h * w * Cin and (res is None or regions[res][1] == size)
        want = ws.buf[ws.ptr - ws.buf.data_ptr() + off:][:size].clone()
        assert bool(want.any()), name
        dx, dx_buf = K.guarded(torch.full((size // 2,), float("nan"), dtype=torch.bfloat16, device=DEV))
        rc, route = conv_dgrad(tr, name + ".weight", flat.data_ptr(), ws.ptr + regions[dy][0], ws.ptr + regions[res][0] if res else None, dx.data_ptr(),
                               B, Hdy, Wdy)
        _native.check(rc)
        torch.cuda.synchronize()
        assert K.guards_intact(dx_buf)
        assert route == step_routes[len(checked)], (name, route, step_routes)
        assert torch.equal(dx.view(torch.uint8), want), f"{name}: the hook's launch is not the step's ({route})"
        checked.append(f"{name} [{route}]")
    assert len(checked) == len(step_routes) == 4
    assert len(K.hook_text(L.ccn_internal_train_routes, tr.h)) == n_log, "the hook left lines in the handle's route log"
    print("hook == step, bit for bit: " + "; ".join(checked))
    del net, st, tr
    torch.cuda.empty_cache()
