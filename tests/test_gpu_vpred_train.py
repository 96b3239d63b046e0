"""The v objective on the GPU: ``ccn_diffusion_loss_grad_v`` against the float64 closed form of tests/vpred_ref.py and torch's fp32
autograd, its zero-weight form against ``ccn_mse_loss_grad``, and ``train_step(prediction="v")`` against the oracle loop.

Bounds (U = 2^-24; S, T and K_V = 9 from vpred_ref: S takes s where the eps form has s / a, T is the allowance for the three roundings
of the target a noise - s x0):
  gradient, kernel vs float64 closed form      |err| <= K_V U S + T per element
  gradient, kernel vs torch fp32 autograd      |err| <= 2 K_V U S per element (both form the same fp32 target: T drops out)
  loss terms, kernel vs float64                the bounds of test_gpu_objective.check_terms_against_float64 (1.01 U relative), the MSE
                                               on the fp32 target as an operand
  clamp mask / auxiliary-gradient set          no mismatch: raw = a x_t - s v_hat is two products and a subtraction, bit-equal to torch
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))
import vpred_ref as R  # noqa: E402

from clip_feature_codec import _native  # noqa: E402
from clip_feature_codec.models.unet import CLIPCondUNet  # noqa: E402
from clip_feature_codec.diffusion.scheduler import NoiseScheduler  # noqa: E402
from clip_feature_codec.train.diffusion_train import FusedAdamW, train_step  # noqa: E402
from clip_feature_codec.utils import synth  # noqa: E402
from oracle import ref_unet, ref_train, ref_diffusion  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEP = np.load(HERE / "golden" / "train_step.npz")
RECON_W, TV_W = 0.05, 1e-4
U = R.U
SHAPES = [(1, 3, 2, 2), (2, 3, 40, 24), (3, 1, 17, 130), (1, 2, 18, 523)]


def dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(DEV)


def col(c):
    return c.view(-1, 1, 1, 1)


def make_inputs(shape, seed):
    """As ``make_inputs`` of tests/test_gpu_objective.py: saturated rows and columns of x0, t from {0, 120, 400, 700, 930, 999}; the
    prediction is the target plus noise of 0.3."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randint(0, 256, shape, generator=g).float() / 127.5 - 1.0
    x0[0, :, : max(1, H // 8), :] = 1.0
    x0[-1, :, :, : max(1, W // 8)] = -1.0
    t = torch.tensor([(0, 120, 400, 700, 930, 999)[i % 6] for i in range(B)]) if B > 1 else torch.tensor([400])
    noise = torch.randn(shape, generator=g)
    tables = ref_diffusion.scheduler_tables(1000, "cosine")
    a = tables["sqrt_alphas_cumprod"][t].contiguous(); s = tables["sqrt_one_minus_alphas_cumprod"][t].contiguous()
    target = col(a) * noise - col(s) * x0                              # three fp32 ops, each rounded
    v_hat = target + 0.3 * torch.randn(shape, generator=g)
    x_t = ref_diffusion.q_sample(tables, x0, t, noise)
    jitter = torch.randn(shape, generator=g)
    return x0, t, noise, v_hat, x_t, a, s, target, jitter


def run_kernel(v_hat, noise, x_t, x0, a, s, recon_w, tv_w):
    terms, d = _native.diffusion_loss_grad_v(dev(v_hat), dev(noise), dev(x_t), dev(x0), dev(a), dev(s), recon_w, tv_w)
    torch.cuda.synchronize()
    return terms.cpu().numpy(), d.cpu().numpy()


def torch_v_objective(v_hat, noise, x_t, x0, a, s, recon_w, tv_w):
    """The v objective in torch ops (the test's own statement of it)."""
    target = col(a) * noise - col(s) * x0
    x0_pred = (col(a) * x_t - col(s) * v_hat).clamp(-1, 1)
    mse = F.mse_loss(v_hat, target)
    l1 = F.l1_loss(x0_pred, x0)
    tv = (x0_pred[:, :, 1:, :] - x0_pred[:, :, :-1, :]).abs().mean() + (x0_pred[:, :, :, 1:] - x0_pred[:, :, :, :-1]).abs().mean()
    return mse + recon_w * l1 + tv_w * tv, (mse, l1, tv)


def check_terms_against_float64(terms, cf, recon_w, tv_w, what):
    """The bounds of tests/test_gpu_objective.py."""
    ref = cf["terms"]
    bound = 1.01 * U * ref
    bound[0] += U * (recon_w * ref[2] + tv_w * ref[3])
    err = np.abs(terms.astype(np.float64) - ref)
    print(f"{what}: loss terms {terms}, error / bound {err / bound}")
    assert np.all(err <= bound), (what, err / bound)


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_against_float64_and_torch_autograd(shape):
    x0, t, noise, v_hat, x_t, a, s, target, jitter = make_inputs(shape, seed=sum(shape))
    leaf = v_hat.clone().requires_grad_(True)
    loss, (mse, l1, tv) = torch_v_objective(leaf, noise, x_t, x0, a, s, RECON_W, TV_W)
    loss.backward()
    raw = col(a) * x_t - col(s) * v_hat
    cf = R.closed_form_v(v_hat.numpy(), noise.numpy(), raw.numpy(), x0.numpy(), a.numpy(), s.numpy(), RECON_W, TV_W, target32=target.numpy())
    terms, d = run_kernel(v_hat, noise, x_t, x0, a, s, RECON_W, TV_W)
    frac = float(cf["mask"].mean())
    assert shape[2] * shape[3] < 16 or 0.02 < frac < 0.98, frac                  # both sides of the clamp
    ratio = R.worst_ratio_v(d, cf, k=2 * R.K_V, ref=leaf.grad.numpy())
    ratio64 = R.worst_ratio_v(d, cf)
    print(f"{shape}: {100 * (1 - frac):.1f} % clamped; kernel vs torch fp32 autograd, worst |err| / (2 K U S) = {ratio:.3f}; "
          f"vs float64 closed form / (K U S + T) = {ratio64:.3f} (K = {R.K_V})")
    assert ratio <= 1.0 and ratio64 <= 1.0, (ratio, ratio64)
    check_terms_against_float64(terms, cf, RECON_W, TV_W, str(shape))
    n = v_hat.numel()
    tb = (3 + np.ceil(np.log2(n)) + 2 + 1.01) * U                                 # torch's pairwise fp32 sums (tests/test_objective_host.py)
    ref_terms = np.array([float(v.detach()) for v in (loss, mse, l1, tv)])
    assert np.all(np.abs(terms - ref_terms) <= tb * np.abs(ref_terms)), (terms, ref_terms)
    # the set of elements with an auxiliary gradient: with v_hat := the fp32 target the MSE part of d_v is exactly 0, and x_t is moved
    # so that raw = a x_t - s v_hat still lands on both sides of the clamp
    x_t2 = x_t + 0.4 * jitter / col(a)
    raw2 = col(a) * x_t2 - col(s) * target
    cf2 = R.closed_form_v(target.numpy(), noise.numpy(), raw2.numpy(), x0.numpy(), a.numpy(), s.numpy(), RECON_W, TV_W, target32=target.numpy())
    _, d2 = run_kernel(target, noise, x_t2, x0, a, s, RECON_W, TV_W)
    want = cf2["aux"] != 0
    mism = int(((d2 != 0) != want).sum())
    print(f"{shape}: {int(want.sum())} of {want.size} elements with an auxiliary gradient, {mism} mismatches")
    assert shape[2] * shape[3] < 16 or (want.sum() > 0.05 * want.size and (~want).sum() > 0.02 * want.size)
    assert mism == 0
    # d_v_dev may be NULL: the terms alone
    t3, none = _native.diffusion_loss_grad_v(dev(v_hat), dev(noise), dev(x_t), dev(x0), dev(a), dev(s), RECON_W, TV_W, want_grad=False)
    assert none is None and np.array_equal(t3.cpu().numpy(), terms)


@pytest.mark.parametrize("shape", SHAPES)
def test_zero_weights_are_the_mse_kernels_bit_for_bit(shape):
    x0, t, noise, v_hat, x_t, a, s, target, _ = make_inputs(shape, seed=7)
    target_dev = col(dev(a)) * dev(noise) - col(dev(s)) * dev(x0)                  # materialised by the same three fp32 ops
    assert torch.equal(target_dev.cpu(), target)
    terms, d = _native.diffusion_loss_grad_v(dev(v_hat), dev(noise), torch.full_like(dev(x_t), float("nan")), dev(x0), dev(a), dev(s), 0.0, 0.0)
    loss, d_mse = _native.mse_loss_grad(dev(v_hat), target_dev)
    assert torch.equal(d, d_mse)
    assert torch.equal(terms[0], loss) and torch.equal(terms[1], loss)
    assert float(terms[2]) == 0.0 and float(terms[3]) == 0.0


@pytest.mark.parametrize("shape", [(3, 1, 17, 130), (2, 3, 40, 24)])
def test_two_runs_are_bit_identical(shape):
    x0, t, noise, v_hat, x_t, a, s, _, _ = make_inputs(shape, seed=5)
    t1, d1 = run_kernel(v_hat, noise, x_t, x0, a, s, RECON_W, TV_W)
    t2, d2 = run_kernel(v_hat, noise, x_t, x0, a, s, RECON_W, TV_W)
    assert np.array_equal(t1.view(np.uint32), t2.view(np.uint32)) and np.array_equal(d1.view(np.uint32), d2.view(np.uint32))


def test_degenerate_images_are_rejected():
    c = torch.ones(1, device=DEV)
    for shape in ((1, 1, 1, 8), (1, 1, 8, 1)):
        x = torch.zeros(shape, device=DEV)
        with pytest.raises(ValueError, match="at least 2"):
            _native.diffusion_loss_grad_v(x, x, x, x, c, c, RECON_W, TV_W)
        with pytest.raises(ValueError, match="at least 2"):
            _native.diffusion_loss_grad_v(x, x, x, x, c, c, 0.0, 0.0)


def make_net(sd):
    net = CLIPCondUNet(z_dim=512, base=32, ch_mult=(1, 2), dtype="fp32").to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.train()


def oracle_v_grads(sd, tables, x0, z, t, noise):
    x_t = ref_diffusion.q_sample(tables, x0, t, noise)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    v_hat = ref_unet.unet_forward(leaves, x_t, z, t)
    a = tables["sqrt_alphas_cumprod"][t]; s = tables["sqrt_one_minus_alphas_cumprod"][t]
    loss, terms = torch_v_objective(v_hat, noise, x_t, x0, a, s, RECON_W, TV_W)
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return loss.detach(), {k: g for k, g in zip(leaves, grads)}, [float(v.detach()) for v in terms]


def test_train_step_v_matches_the_oracle_over_three_steps():
    """train_step(prediction="v", recon_w=0.05, tv_w=1e-4) for three steps against the oracle model under CPU autograd with the test's
    torch v objective on top: shape, inputs and bounds of test_train_step_with_the_objective_matches_the_oracle_over_three_steps
    (5e-5 relative loss and terms, 5 % of the Adam movement)."""
    sd = synth.synth_state_dict(synth.unet_param_spec(512, 32, (1, 2)))
    tables = ref_diffusion.scheduler_tables(1000, "cosine")
    x0, z, t, noise = (torch.from_numpy(STEP[k]) for k in ("x0", "z", "t", "noise"))
    net = make_net(sd)
    sch = NoiseScheduler(1000, "cosine", device=DEV)
    opt = FusedAdamW(net, lr=2e-4)
    state = net.train_state()
    ref = ref_unet.as_torch_sd(sd)
    m = {k: torch.zeros_like(v) for k, v in ref.items()}; v2 = {k: torch.zeros_like(v) for k, v in ref.items()}
    for step in range(1, 4):
        loss = train_step(net, sch, opt, x0.to(DEV), z.to(DEV), t.to(DEV), noise.to(DEV), recon_w=RECON_W, tv_w=TV_W, prediction="v")
        terms = state.last_loss_terms.cpu().numpy()
        rloss, rg, rterms = oracle_v_grads(ref, tables, x0, z, t, noise)
        rel = abs(float(loss) - float(rloss)) / float(rloss)
        print(f"step {step}: loss {float(loss):.7f} oracle {float(rloss):.7f} (relative {rel:.2e}); terms {terms} oracle {rterms}")
        assert float(loss) == float(terms[0])
        assert rel < 5e-5, (step, float(loss), float(rloss))
        assert abs(terms[1] - rterms[0]) < 5e-5 * rterms[0] and abs(terms[2] - rterms[1]) < 5e-5 * rterms[1] and abs(terms[3] - rterms[2]) < 5e-5 * rterms[2]
        for k in ref:
            ref[k], m[k], v2[k] = ref_train.adamw_update(ref[k], rg[k], m[k], v2[k], step)
    got = {k: p.detach().cpu() for k, p in net.named_parameters()}
    init = ref_unet.as_torch_sd(sd)
    worst = 0.0
    for k in ref:
        moved = (ref[k] - init[k]).abs().max()
        worst = max(worst, float((got[k] - ref[k]).abs().max()) / float(moved))
        assert float((got[k] - ref[k]).abs().max()) <= 0.05 * float(moved) + 1e-7, k
    print(f"worst parameter distance from the oracle after three v steps: {worst:.4f} of the Adam movement (bound 0.05)")
    assert net.train_state().fp.intact()
    # the zero-weight v step is the v-MSE: the kernel's terms are total = mse, l1 = tv = 0
    loss = train_step(net, sch, opt, x0.to(DEV), z.to(DEV), t.to(DEV), noise.to(DEV), prediction="v")
    terms = state.last_loss_terms.cpu().numpy()
    assert float(loss) == float(terms[0]) == float(terms[1]) and terms[2] == 0 and terms[3] == 0
    # and an eps MSE-only step afterwards is the old step: no terms
    train_step(net, sch, opt, x0.to(DEV), z.to(DEV), t.to(DEV), noise.to(DEV))
    assert state.last_loss_terms is None


@pytest.mark.parametrize("weights", [(0.0, 0.0), (RECON_W, TV_W)])
def test_default_route_is_unchanged(weights):
    """prediction="eps" spelled out against a second net that is never given the argument, three steps on the same inputs.  Bit for
    bit: every step's loss, and the first step's network output and d loss / d eps_hat (everything in front of the backward).  The
    parameters themselves are not bit-reproducible from run to run on ANY route: the backward accumulates the conditioning and bias
    gradients with float atomicAdd (docs/EXPERIMENTS.md R11.2: parent against parent differs in 12,555 parameters after one step,
    max 2.6e-7), so they are held to the bound the oracle test above uses, 5 % of the Adam movement.  The v step on the same inputs
    is a different step."""
    sd = synth.synth_state_dict(synth.unet_param_spec(512, 32, (1, 2)))
    x0, z, t, noise = (torch.from_numpy(STEP[k]).to(DEV) for k in ("x0", "z", "t", "noise"))
    sch = NoiseScheduler(1000, "cosine", device=DEV)
    nets = [make_net(sd) for _ in range(3)]
    opts = [FusedAdamW(n, lr=2e-4) for n in nets]
    kw = dict(recon_w=weights[0], tv_w=weights[1])
    for step in range(3):
        l_arg = train_step(nets[0], sch, opts[0], x0, z, t, noise, prediction="eps", **kw).clone()
        l_old = train_step(nets[1], sch, opts[1], x0, z, t, noise, **kw).clone()
        l_v = train_step(nets[2], sch, opts[2], x0, z, t, noise, prediction="v", **kw).clone()
        assert torch.equal(l_arg, l_old), step
        assert float(l_v) != float(l_old)
        if step == 0:
            sb = [n.train_state().static_buffers(x0, z) for n in nets]
            assert torch.equal(sb[0]["eps"], sb[1]["eps"]) and torch.equal(sb[0]["d_eps"], sb[1]["d_eps"])
            assert torch.equal(sb[0]["eps"], sb[2]["eps"]) and not torch.equal(sb[0]["d_eps"], sb[2]["d_eps"])
    init = ref_unet.as_torch_sd(sd)
    worst = 0.0
    for (k, p), (_, q) in zip(nets[0].named_parameters(), nets[1].named_parameters()):
        moved = float((q.detach().cpu() - init[k]).abs().max())
        d = float((p.detach() - q.detach()).abs().max())
        worst = max(worst, d / moved)
        assert d <= 0.05 * moved + 1e-7, k
    print(f"weights {weights}: prediction='eps' vs no argument after three steps: worst parameter distance {worst:.2e} of the Adam movement")
    assert any(not torch.equal(p.detach(), r.detach()) for p, r in zip(nets[1].parameters(), nets[2].parameters()))
    assert (nets[0].train_state().last_loss_terms is None) == (weights == (0.0, 0.0))
    assert (nets[1].train_state().last_loss_terms is None) == (weights == (0.0, 0.0))
