"""GPU parity of the f16x3 mode (CCN_DTYPE_F16X3: fp32 storage, ResBlock convs and ConvTransposes on split fp16 hi + lo operands,
three v_mfma_f32_32x32x16_f16 per product).  It is held to the fp32 parity mode's own tolerances (tests/test_gpu_parity.py): the CPU
emulation of the arithmetic (tests/split_emulation.py) meets each of them with >= 6x headroom -- C1 taps worst 2.9e-6, eps 1.6e-7 at C2,
C2 50 steps 3.2e-5 -- and the GPU's own fp32 summation order is what those constants already carry for the fp32 mode.  The route and
exact-operand tests at the end are what an alias of the fp32 mode, or a kernel that dropped a cross term, cannot pass.

These are end-to-end gates: the measured errors sit 10x to 60x below them (docs/EXPERIMENTS.md R6.4).  The pin of the arithmetic
itself is tests/test_gpu_split_replay.py: every split conv, on all 16 compiled forms of the ws / fr kernels, against a float64
product of its own operands (with tests/test_split_replay_host.py as its proof on the host)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clip_feature_codec import _native
from clip_feature_codec.models.unet import CLIPCondUNet
from clip_feature_codec.models.blocks import ResBlock
from clip_feature_codec.diffusion.scheduler import NoiseScheduler
from clip_feature_codec.diffusion.ddim import DDIMSampler
from oracle import ref_unet

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))
import infer_plan_cases  # noqa: E402
import split_emulation  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TOL_EPS_FP32 = 2e-5       # the fp32 mode's constants (tests/test_gpu_parity.py)
TOL_ACT_FP32 = 1e-4
TOL_E2E_FP32 = 1e-3


def to_dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(DEV)


def make_net(sd, base, ch_mult, dtype="f16x3"):
    net = CLIPCondUNet(z_dim=512, base=base, ch_mult=ch_mult, dtype=dtype).to(DEV).eval()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return net


def maxerr(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def check_packed(name, got, g, tol):
    got = got[0].detach().cpu()
    err = float(np.abs(got[:, ::4, ::4].numpy() - g[f"{name}.sub"]).max())
    mean_err = float(np.abs(got.double().mean((1, 2)).numpy() - g[f"{name}.mean"]).max())
    abssum = float(got.double().abs().sum())
    print(f"{name}: max-abs {err:.3e}, mean err {mean_err:.3e}")
    assert err < tol, (name, err)
    assert mean_err < tol and abs(abssum / float(g[f"{name}.abssum"]) - 1) < 1e-3, (name, mean_err, abssum)
    return err


def route_lines(nat):
    return infer_plan_cases.route_text(nat).splitlines()


@pytest.fixture(scope="module")
def tiny_net(tiny_sd):
    return make_net(tiny_sd, 32, (1, 2))


@pytest.fixture(scope="module")
def c2_sd(synth):
    return synth.synth_state_dict(synth.unet_param_spec(512, 128, (1, 2, 2)))


@pytest.fixture(scope="module")
def c2_net(c2_sd):
    return make_net(c2_sd, 128, (1, 2, 2))


# ---------------------------------------------------------------- C1 and the odd shapes
def test_c1_taps_and_eps(golden, tiny_net):
    g = golden("unet_tiny_taps.npz")
    eps = tiny_net(to_dev(g["x"]), to_dev(g["z"]), to_dev(g["t"]))
    report = []
    for name in ["in_conv", "down.0", "down.1", "down.2", "down.3", "down.5", "mid1", "mid2", "up.0", "up.1"]:
        ref = g[f"tap.{name}"]
        report.append((name, maxerr(tiny_net.read_activation(name, ref.shape), torch.from_numpy(ref))))
    err_eps = maxerr(eps, torch.from_numpy(g["eps"]))
    msg = "; ".join(f"{n}: {e:.2e}" for n, e in report) + f"; eps {err_eps:.2e}"
    print("f16x3 C1 taps:", msg)
    for n, e in report:
        assert e < TOL_ACT_FP32, msg
    assert err_eps < TOL_EPS_FP32, msg
    lines = route_lines(tiny_net.native())
    assert any("ops=f16x3" in ln for ln in lines) and any("ops=f32" in ln for ln in lines), lines    # 64-wide layers split, 32-wide not
    tiny_net.native().poll_errors()


@pytest.mark.parametrize("base,ch_mult,B,H,W", [
    (32, (1, 2), 3, 24, 40),
    (48, (2, 1), 2, 16, 16),
    (64, (1, 2, 2), 1, 32, 64),
    (16, (1,), 2, 8, 8),
])
def test_forward_shapes_vs_oracle(synth, base, ch_mult, B, H, W):
    """The four odd shapes of test_forward_shapes_vs_oracle_fp32 (same weights, inputs and bound)."""
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, ch_mult), seed=1)
    net = make_net(sd, base, ch_mult)
    g = torch.Generator().manual_seed(base + H)
    x = torch.randn((B, 3, H, W), generator=g); z = torch.from_numpy(synth.synth_z(B, seed=9))
    t = torch.randint(0, 1000, (B,), generator=g)
    with torch.no_grad():
        ref = ref_unet.unet_forward(ref_unet.as_torch_sd(sd), x, z, t)
    eps = net(x.to(DEV), z.to(DEV), t.to(DEV))
    err = maxerr(eps, ref)
    print(f"f16x3 base {base} {ch_mult} {B}x{H}x{W}: eps max-abs vs oracle {err:.2e}")
    assert eps.shape == x.shape and err < TOL_EPS_FP32, err
    net.native().poll_errors()


def test_other_width_base192_two_levels(synth):
    sd = synth.synth_state_dict(synth.unet_param_spec(512, 192, (1, 2)))
    B, S = 4, 128
    g = torch.Generator("cpu").manual_seed(7)
    x = torch.randn((B, 3, S, S), generator=g); z = torch.from_numpy(synth.synth_z(B)); t = torch.tensor([999, 600, 300, 10])
    net = make_net(sd, 192, (1, 2))
    e = net(to_dev(x), to_dev(z), to_dev(t))
    with torch.no_grad():
        ref = ref_unet.unet_forward(ref_unet.as_torch_sd(sd), x[1:2], z[1:2], t[1:2])
    err = maxerr(e[1:2], ref)
    print(f"f16x3 base 192 @128px: eps max-abs vs oracle {err:.2e}")
    assert err < TOL_EPS_FP32, err
    net.native().poll_errors()


def test_c1_ten_steps_and_determinism(golden, tiny_net):
    g = golden("c1_sample.npz")
    z, xT = to_dev(g["z"]), to_dev(g["x_T"])
    sampler = DDIMSampler(NoiseScheduler(1000, "cosine", DEV), eta=0.0)
    a = sampler.sample(tiny_net, z, (1, 3, 64, 64), steps=10, x_T=xT)
    err = maxerr(a, torch.from_numpy(g["x_final"]))
    print(f"f16x3 C1 10 steps max-abs vs reference: {err:.3e}")
    assert err < TOL_E2E_FP32, err
    b = sampler.sample(tiny_net, z, (1, 3, 64, 64), steps=10, x_T=xT)          # graph replay
    sampler.use_graph = False
    c = sampler.sample(tiny_net, z, (1, 3, 64, 64), steps=10, x_T=xT)          # launch by launch
    d = sampler.sample(lambda x, zz, t: tiny_net(x, zz, t), z, (1, 3, 64, 64), steps=10, x_T=xT)   # generic callable route
    assert torch.equal(a, b) and torch.equal(a, c)
    assert maxerr(a, d) < 1e-5, maxerr(a, d)
    tiny_net.native().poll_errors()


def test_batch_rows_are_independent(synth, tiny_net):
    z = to_dev(synth.synth_z(3, seed=50)); xT = to_dev(synth.start_noise([7, 8, 9], 32, seed_base=1))
    sampler = DDIMSampler(NoiseScheduler(1000, "cosine", DEV), eta=0.0)
    full = sampler.sample(tiny_net, z, (3, 3, 32, 32), steps=4, x_T=xT)
    for i in range(3):
        one = sampler.sample(tiny_net, z[i:i + 1], (1, 3, 32, 32), steps=4, x_T=xT[i:i + 1])
        assert torch.equal(one[0], full[i]), i


def test_resblock_operator_and_training_is_rejected(golden, synth):
    g = golden("resblock.npz")
    rb = ResBlock(32, 256).to(DEV)
    rb.compute_dtype = "f16x3"
    spec = [(f"down.0.{k}", tuple(v.shape)) for k, v in rb.state_dict().items()]
    sd = synth.synth_state_dict(spec, seed=3)
    rb.load_state_dict({k[len("down.0."):]: torch.from_numpy(v) for k, v in sd.items()})
    y = rb(to_dev(g["x"]), to_dev(g["h"]))
    assert maxerr(y, torch.from_numpy(g["y"])) < 3e-5, maxerr(y, torch.from_numpy(g["y"]))
    with pytest.raises(ValueError, match=r"(?s)fp32.*bf16"):
        _native.NativeTrainer(512, 32, (1, 2), 256, 3, dtype="f16x3", device=DEV)


# ---------------------------------------------------------------- C2
def _check_routes(lines, want_kernel):
    seen = set()
    for ln in lines:
        f = ln.split()
        kind, kernel = f[1], f[2]
        kv = dict(x.split("=") for x in f[3:])
        assert "ops" in kv, ln
        if kind in ("C3S1", "CT4"):
            assert kv["ops"] == "f16x3" and kernel in ("ws", "fr"), ln
            assert (kernel == "fr") == (kv["th"] == "8"), ln
            seen.add(kernel)
        else:
            assert kind in ("STEM", "HEAD", "C3S2") and kv["ops"] == "f32" and kernel not in ("ws", "fr"), ln
    assert want_kernel in seen, (want_kernel, seen)
    assert sum(ln.split()[1] == "C3S1" for ln in lines) == 28 and sum(ln.split()[1] == "CT4" for ln in lines) == 3, lines


def test_c2_forward_batch1_and_routes(golden, synth, c2_sd, c2_net):
    """Batch 1: 4-row tiles, the ws kernel."""
    g = golden("c2_sample.npz")
    xT = to_dev(synth.start_noise([0], 256, seed_base=100)); z = to_dev(synth.synth_z(1))
    e0 = c2_net(xT, z, to_dev(np.array([999], np.int64)))
    _check_routes(route_lines(c2_net.native()), "ws")
    e1 = c2_net(xT * 0.5, z, to_dev(np.array([500], np.int64)))
    check_packed("eps_t999", e0, g, TOL_EPS_FP32)
    check_packed("eps_t500_halfx", e1, g, TOL_EPS_FP32)
    c2_net.native().poll_errors()
    # the two existing modes print what they printed before
    n32 = make_net(c2_sd, 128, (1, 2, 2), dtype="fp32")
    n32(xT, z, to_dev(np.array([999], np.int64)))
    assert not any("ops=" in ln for ln in route_lines(n32.native()))


def test_c2_forward_batch8_and_routes(golden, synth, c2_net):
    """Record 0 of batch 8 (the bench workload's shape): 8-row tiles, the fr kernel."""
    g = golden("c2_sample.npz")
    z = to_dev(synth.synth_z(8)); xT = to_dev(synth.start_noise(range(8), 256, seed_base=100))
    t = to_dev(np.full((8,), 999, np.int64))
    eps = c2_net(xT, z, t)
    _check_routes(route_lines(c2_net.native()), "fr")
    check_packed("eps_t999", eps[0:1], g, TOL_EPS_FP32)
    e1 = c2_net(xT * 0.5, z, to_dev(np.full((8,), 500, np.int64)))
    check_packed("eps_t500_halfx", e1[0:1], g, TOL_EPS_FP32)
    c2_net.native().poll_errors()


def test_ragged_batch_against_the_fp32_mode(synth, c2_sd, c2_net):
    """8 x 200 x 168 (partial column and row tiles at every level) against the fp32 mode: two results that are each within
    TOL_EPS_FP32 of the oracle; the rows / columns that partial tiles cover asserted on their own."""
    B, H, W = 8, 200, 168
    g = torch.Generator("cpu").manual_seed(3)
    x = to_dev(torch.randn((B, 3, H, W), generator=g)); z = to_dev(synth.synth_z(B))
    t = to_dev(np.array([999, 800, 650, 500, 350, 200, 50, 0], np.int64))
    e = c2_net(x, z, t)
    e32 = make_net(c2_sd, 128, (1, 2, 2), dtype="fp32")(x, z, t)
    d, d_rows, d_cols = maxerr(e, e32), maxerr(e[:, :, -4:, :], e32[:, :, -4:, :]), maxerr(e[:, :, :, -8:], e32[:, :, :, -8:])
    print(f"f16x3 ragged 200x168 vs fp32 mode: {d:.3e}; last 4 rows {d_rows:.3e}; last 8 columns {d_cols:.3e}")
    assert torch.isfinite(e).all() and d < 2 * TOL_EPS_FP32, d
    assert d_rows < 2 * TOL_EPS_FP32 and d_cols < 2 * TOL_EPS_FP32, (d_rows, d_cols)
    c2_net.native().poll_errors()


def test_c2_50_steps_vs_reference(golden, synth, c2_net):
    """The headline gate of the mode: 256 px, 50 DDIM steps against the reference's CPU run, at the fp32 mode's 1e-3."""
    g = golden("c2_sample.npz")
    xT = to_dev(synth.start_noise([0], 256, seed_base=100)); z = to_dev(synth.synth_z(1))
    x = DDIMSampler(NoiseScheduler(1000, "cosine", DEV), 0.0).sample(c2_net, z, (1, 3, 256, 256), steps=50, x_T=xT)
    err = check_packed("x_final", x, g, TOL_E2E_FP32)
    print(f"C2 50-step f16x3 max-abs vs reference: {err:.3e}")
    c2_net.native().poll_errors()


def _rms(a):
    return float(a.double().pow(2).mean().sqrt())


def test_conv_transpose_exact_operand_replay(synth, c2_sd, c2_net):
    """The three ConvTransposes at C2 have no GroupNorm in front, so read_activation gives the kernel's exact input.  `got` against a
    float64 conv_transpose2d of the fp32 input and fp32 weights (+ bias + skip), and against the two references that omit one cross
    term (a_lo w_hi, a_hi w_lo; built on the host from the same split): the kernel must be at least 10x closer to the full product
    than either omission is, in RMS over all outputs.  Torch's fp32 accumulation of the three products clears this by 36x or more
    (ratios 365, 517, 720 on N(0, 2) inputs of these layers) and an omitted term misses it by as much."""
    xT = to_dev(synth.start_noise([0], 256, seed_base=100)); z = to_dev(synth.synth_z(1))
    c2_net(xT, z, to_dev(np.array([999], np.int64)))
    torch.cuda.synchronize()
    layers = [("up.2", "up.1", "down.7", 512, 256, 32), ("up.5", "up.4", "down.4", 256, 128, 64), ("up.8", "up.7", "down.1", 128, 128, 128)]
    for name, src, skip, cin, cout, s in layers:
        got = c2_net.read_activation(name, (1, cout, 2 * s, 2 * s)).cpu().double()
        a = c2_net.read_activation(src, (1, cin, s, s)).cpu()
        sk = c2_net.read_activation(skip, (1, cout, 2 * s, 2 * s)).cpu().double()
        w = torch.from_numpy(c2_sd[f"{name}.weight"]); b = torch.from_numpy(c2_sd[f"{name}.bias"]).double()
        sc = split_emulation.weight_scale(w)
        wh, wl = split_emulation.split(w * sc)
        ah, al = split_emulation.split(a)
        assert float((ah + al - a).abs().max()) <= 2.0 ** -21 * float(a.abs().max())

        def ct(x, ww):
            return F.conv_transpose2d(x.double(), ww.double(), None, stride=2, padding=1)
        rest = b.view(1, -1, 1, 1) + sk
        full = ct(a, w) + rest
        no_alwh = ct(ah, wh + wl) / sc + rest
        no_ahwl = ct(ah + al, wh) / sc + rest
        r_got, r1, r2 = _rms(got - full), _rms(no_alwh - full), _rms(no_ahwl - full)
        print(f"{name}: rms(got - full) {r_got:.3e}; omitting a_lo w_hi {r1:.3e} ({r1 / r_got:.0f}x), a_hi w_lo {r2:.3e} ({r2 / r_got:.0f}x); "
              f"max |got - full| {float((got - full).abs().max()):.3e}")
        assert 10 * r_got <= r1 and 10 * r_got <= r2, (name, r_got, r1, r2)


def test_range_guard_reports_once_and_leaves_the_process_usable(golden, synth, c2_sd):
    """Activations beyond fp16's range (norm1 scaled by 1e6 in front of a split conv): the operand saturates, the forward stays
    finite, and the handle reports it once; a net on the unscaled weights afterwards matches the fixture."""
    g = golden("c2_sample.npz")
    bad = dict(c2_sd)
    bad["down.0.norm1.weight"] = (c2_sd["down.0.norm1.weight"] * np.float32(1e6)).astype(np.float32)
    net = make_net(bad, 128, (1, 2, 2))
    xT = to_dev(synth.start_noise([0], 256, seed_base=100)); z = to_dev(synth.synth_z(1)); t = to_dev(np.array([999], np.int64))
    eps = net(xT, z, t)
    torch.cuda.synchronize()
    assert torch.isfinite(eps).all()
    with pytest.raises(RuntimeError, match=r"(?s)f16x3.*fp32"):
        net.native().poll_errors()
    net.native().poll_errors()                                   # reported once
    good = make_net(c2_sd, 128, (1, 2, 2))
    check_packed("eps_t999", good(xT, z, t), g, TOL_EPS_FP32)
    torch.cuda.synchronize()
    good.native().poll_errors()
