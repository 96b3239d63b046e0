"""The fp32 training step against a float64, exact-operand oracle on every launch form it takes at realistic sizes.

The bf16 tests of tests/test_gpu_train.py at 128 px and above compare with "the fp32 mode of the same library"; the fp32 mode itself is
compared with the CPU oracle there only at toy sizes, where every weight-gradient workgroup owns a single pixel tile, every conv runs on
4-row tiles, the GroupNorm backward makes one pixel pass per workgroup and the forward norm always takes the fused route.  The shapes
below reach the other forms, and ``test_route_coverage`` reads the library's own report of what it launched
(``ccn_internal_train_routes``, written where the launches are made) so that a changed threshold fails here instead of silently shrinking
the coverage.

Oracle: oracle/ref_train.loss_and_grads(dtype=torch.float64, temb=<the device's own timestep embedding>): every leaf, input and
intermediate in float64, and the one input of the step whose fp32 rounding is not the kernels' doing -- cos / sin of up to 999 rad in
temb_kernel, which tests/test_gpu_parity.py allows 2e-4 -- handed over as the device computed it.  What is left between library and oracle
is the kernels' own fp32 arithmetic.

Gate: ``max|got - ref| / max|ref|`` per gradient tensor and for the loss, ``max|got - ref|`` for eps, all below GATE.  GATE is four times
the worst value measured on the MI355X over the whole matrix and the variants (table in docs/EXPERIMENTS.md R9), rounded up to one
significant digit: a margin of two bits, because fp32 summation error moves with data and seed.  tests/test_train_oracle_host.py holds
GATE to what one dropped 4 x 32 pixel tile does to every tensor (at least 5 x GATE; 40 x GATE for the conv weights).

Not reached here: gn_bwd_geom's cap of 64 pixel passes per workgroup (needs B >= 16 at 256 px, or 512 channels at full resolution:
beyond a CPU oracle of a few seconds) and the `prologue` norm form of C4's 3072-channel bottleneck, which stays with
test_c4_architecture_gradients_fp32.
"""
import ctypes
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "clip-neural-image-conpression_amd")]

from clip_feature_codec import _native  # noqa: E402
from clip_feature_codec.models.unet import CLIPCondUNet  # noqa: E402
from clip_feature_codec.utils import synth  # noqa: E402
from oracle import ref_unet, ref_train  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CH_MULT = (1, 2)
TIME_DIM = 256

# id -> (base, B, H, W); all fp32 mode, ch_mult (1, 2)
CASES = {
    "A": (128, 4, 128, 128),   # 8-row threshold met exactly; several tiles per weight-gradient workgroup; gnbwd iters 8 / 2
    "B": (128, 5, 100, 136),   # as A with ragged rows and columns, odd batch, a partial last gnbwd block; level 1 on 4-row ws
    "C": (64, 2, 136, 200),    # 238 partial-sum slots: the separate statistics launch; ConvTranspose on ragged 8-row tiles
    "D": (64, 2, 144, 256),    # 144 slots on 8-row tiles at BN 64
    "E": (64, 4, 128, 128),    # BN 64 at the threshold; the cheapest case, hosts the variants
    "F": (192, 2, 128, 128),   # half-padded N tile (n_nt 2); 3 x 3 channel groups in the weight gradient
}
# worst measured on the MI355X: 4.96e-6 (case B, mid2.film.to_scale.bias; docs/EXPERIMENTS.md R9); x 4, rounded up to one significant digit
GATE = 2e-5


def inputs(cid):
    """Key-seeded weights, seeded inputs, timesteps spread over 0..999 (CPU tensors; the same for the GPU step and the oracle)."""
    base, B, H, W = CASES[cid]
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, CH_MULT))
    g = torch.Generator("cpu").manual_seed(1000 + ord(cid))
    x_t = torch.randn((B, 3, H, W), generator=g)
    target = torch.randn((B, 3, H, W), generator=g)
    z = torch.from_numpy(synth.synth_z(B))
    t = torch.linspace(0, 999, B).round().long()
    return sd, x_t, z, t, target


def make_net(sd, base):
    net = CLIPCondUNet(z_dim=512, base=base, ch_mult=CH_MULT, time_dim=TIME_DIM, dtype="fp32").to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.train()


def train_routes(trainer):
    lib = _native.load_library()
    lib.ccn_internal_train_routes.restype = ctypes.c_int
    lib.ccn_internal_train_routes.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    n = lib.ccn_internal_train_routes(trainer.h, None, 0)
    assert n > 0
    buf = ctypes.create_string_buffer(n + 1)
    assert lib.ccn_internal_train_routes(trainer.h, buf, n + 1) == n
    return buf.value.decode().splitlines()


_ORACLE, _STEP = {}, {}


def oracle(cid):
    """(loss, grads, eps) of the float64 oracle on the device's own timestep embedding; computed once per shape, never modified."""
    if cid not in _ORACLE:
        sd, x_t, z, t, target = inputs(cid)
        temb = _native.timestep_embedding(t.to(DEV), TIME_DIM).cpu().double()
        loss, grads, eps = ref_train.loss_and_grads(ref_unet.as_torch_sd(sd), x_t, z, t, target, dtype=torch.float64, temb=temb)
        assert eps.dtype == torch.float64 and loss.dtype == torch.float64 and all(g.dtype == torch.float64 for g in grads.values())
        _ORACLE[cid] = (loss, grads, eps)
    return _ORACLE[cid]


def gpu_step(cid):
    """loss.backward() through CLIPCondUNet.forward in fp32 mode: (loss, grads, eps, route report); run once per shape."""
    if cid not in _STEP:
        sd, x_t, z, t, target = inputs(cid)
        net = make_net(sd, CASES[cid][0])
        net.zero_grad(set_to_none=True)
        eps = net(x_t.to(DEV), z.to(DEV), t.to(DEV))
        loss = F.mse_loss(eps, target.to(DEV))
        loss.backward()
        grads = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}
        _STEP[cid] = (loss.detach().cpu(), grads, eps.detach().cpu(), train_routes(net.train_state().trainer))
        del net
        torch.cuda.empty_cache()
    return _STEP[cid]


def trainer_step(cid, variant):
    """The trainer directly: captured hipGraphs (second call: the replay) or the bucketed backward."""
    sd, x_t, z, t, target = inputs(cid)
    net = make_net(sd, CASES[cid][0])
    st = net.train_state()
    tr, flat = st.trainer, st.fp.flat
    x, zz, tt, tg = x_t.to(DEV), z.to(DEV), t.to(DEV), target.to(DEV)
    g = torch.zeros_like(flat)
    eps = torch.empty_like(x)
    bufs = (torch.empty((), device=DEV), torch.empty_like(x), torch.empty(1024, device=DEV))
    ranges = []
    if variant == "graph":
        tr.set_graph(True)
    for _ in range(2 if variant == "graph" else 1):
        g.zero_()
        tr.forward(flat, x, zz, tt, out=eps)
        loss, d = _native.mse_loss_grad(eps, tg, bufs=bufs)
        if variant == "bucket":
            tr.backward(flat, g, x, zz, d, bucket_cb=lambda lo, hi: ranges.append((lo, hi)), bucket_floats=200_000)
        else:
            tr.backward(flat, g, x, zz, d)
    torch.cuda.synchronize()
    if variant == "bucket":
        assert len(ranges) >= 2 and ranges[0][1] == tr.total and ranges[-1][0] == 0
        assert all(hi2 == lo for (lo, _), (_, hi2) in zip(ranges, ranges[1:]))
    gc = g.cpu()
    grads = {name: gc[off:off + torch.Size(shape).numel()].view(shape) for name, shape, off in tr.layout}
    out = (loss.cpu(), grads, eps.cpu())
    del net, st, tr
    torch.cuda.empty_cache()
    return out


def errors(got, ref):
    """name -> error in the gate's measure: relative to the tensor's max for the loss and the gradients, absolute for eps."""
    (loss, grads, eps), (rloss, rgrads, reps) = got, ref
    assert set(grads) == set(rgrads)
    e = {"loss": abs(float(loss) - float(rloss)) / abs(float(rloss)), "eps": float((eps.double() - reps).abs().max())}
    for k, r in rgrads.items():
        e[k] = float((grads[k].double() - r).abs().max() / max(float(r.abs().max()), 1e-300))
    return e


def check(what, got, ref):
    e = errors(got, ref)
    worst = max((k for k in e if k not in ("loss", "eps")), key=e.get)
    print(f"{what}: loss {e['loss']:.2e} eps {e['eps']:.2e} worst gradient {worst} {e[worst]:.2e} (gate {GATE:.0e})")
    bad = {k: v for k, v in e.items() if not v < GATE}
    assert not bad, f"{what}: above the gate {GATE:.0e}: " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(bad.items(), key=lambda kv: -kv[1])[:8])


def fields(line):
    w = line.split()
    return w, {k: int(v) for k, v in (x.split("=") for x in w if "=" in x) if v.lstrip("-").isdigit()}


def test_route_coverage():
    """The union of the route reports over the shape matrix contains every launch form this file exists for."""
    lines = sorted({ln for cid in CASES for ln in gpu_step(cid)[3]})
    parsed = [fields(ln) for ln in lines]

    def conv(direction, kind, kernel, **kv):
        return any(w[:4] == ["conv", direction, kind, kernel] and all(f.get(k) == v for k, v in kv.items()) for w, f in parsed)

    def wgrad_uneven(kind):
        return any(w[:2] == ["wgrad", kind] and f["nsplit"] < f["tiles"] and f["tiles"] % f["nsplit"] != 0 for w, f in parsed)

    want = {
        "C3S1 forward on 8-row fr, BN 128": conv("fwd", "C3S1", "fr", th=8, bn=128),
        "C3S1 data gradient on 8-row fr, BN 128": conv("dgrad", "C3S1", "fr", th=8, bn=128),
        "C3S1 forward on 8-row fr, BN 64": conv("fwd", "C3S1", "fr", th=8, bn=64),
        "C3S1 data gradient on 8-row fr, BN 64": conv("dgrad", "C3S1", "fr", th=8, bn=64),
        "C3S1 on 8-row fr with two N tiles": conv("fwd", "C3S1", "fr", th=8, n_nt=2) and conv("dgrad", "C3S1", "fr", th=8, n_nt=2),
        "ConvTranspose forward on 8-row fr": conv("fwd", "CT4", "fr", th=8),
        "ConvTranspose as the stride-2 conv's data gradient on 8-row fr": conv("dgrad", "CT4", "fr", th=8),
        "C3S1 on 4-row ws": conv("fwd", "C3S1", "ws", th=4) and conv("dgrad", "C3S1", "ws", th=4),
        "stride-2 conv on igemm": conv("fwd", "C3S2", "igemm", four=0),
        "4x4 stride-2 conv (the ConvTranspose's data gradient) on igemm": conv("dgrad", "C3S2", "igemm", four=1),
        "stem on igemm": conv("fwd", "STEM", "igemm"),
        "head on igemm": conv("fwd", "HEAD", "igemm"),
        "fused forward norm": any(w[:2] == ["norm", "fused"] for w, _ in parsed),
        "forward norm as statistics + activation launches": any(w[:2] == ["norm", "stats+act"] and f["slots"] > 128 for w, f in parsed),
        "GroupNorm backward with several pixel passes per workgroup": any(w[0] == "gnbwd" and f["iters"] > 1 for w, f in parsed),
        "GroupNorm backward with a partial last pixel block": any(w[0] == "gnbwd" and f["tail"] != 0 for w, f in parsed),
        "colsum finalize with 8 row blocks": any(w[:2] == ["colsum", "src=dy"] and f["ygrid"] == 8 for w, f in parsed),
    }
    for kind in ("C3S1", "C3S2", "CT4", "STEM"):
        want[f"{kind} weight gradient with an uneven number of tiles per workgroup"] = wgrad_uneven(kind)
    for ln in lines:
        print(ln)
    missing = [k for k, ok in want.items() if not ok]
    assert not missing, f"launch forms the shape matrix no longer reaches: {missing}"


@pytest.mark.parametrize("cid", list(CASES))
def test_fp32_step_against_float64_oracle(cid):
    """Loss, eps and every gradient tensor of loss.backward() through CLIPCondUNet.forward, per shape of the matrix."""
    base, B, H, W = CASES[cid]
    check(f"case {cid} base {base} {B}x{H}x{W}", gpu_step(cid)[:3], oracle(cid))


@pytest.mark.parametrize("variant", ["graph", "bucket"])
@pytest.mark.parametrize("cid", ["E", "B"])
def test_fp32_trainer_variants_against_float64_oracle(cid, variant):
    """NativeTrainer directly with set_graph(True) (capture, then a replay) and with the bucketed backward: the same cached oracle, the
    same gate."""
    base, B, H, W = CASES[cid]
    check(f"case {cid} base {base} {B}x{H}x{W} {variant}", trainer_step(cid, variant), oracle(cid))
