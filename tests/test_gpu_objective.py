"""The fused MSE + L1 + TV objective on the GPU: ``ccn_diffusion_loss_grad`` against the float64 closed form (tests/objective_ref.py,
which tests/test_objective_host.py pins to the reference's fp32 autograd run), ``train_step(recon_w=, tv_w=)`` against the oracle
loop, and ``train_diffusion``'s two routes against each other.

Bounds (U = 2^-24, S = the term-by-term absolute sum of the closed form, K = objective_ref.K = 10 from the count of roundings):
  gradient, kernel vs float64 closed form      |err| <= K U S per element
  gradient, kernel vs torch fp32 autograd      |err| <= 2 K U S per element (two fp32 evaluations of one exact value)
  loss terms, kernel vs float64                1.01 U relative (fp64 accumulation of exact fp64 summands, one fp32 rounding; the total
                                               also carries the fp32 rounding of the two weights)
  clamp mask                                   no mismatch: raw is evaluated as ccn_predict_x0 does, which is bit-equal to torch
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))
import objective_ref as R  # noqa: E402

from clip_feature_codec import _native  # noqa: E402
from clip_feature_codec.models.unet import CLIPCondUNet  # noqa: E402
from clip_feature_codec.diffusion.scheduler import NoiseScheduler  # noqa: E402
from clip_feature_codec.train.diffusion_train import FusedAdamW, train_step  # noqa: E402
from clip_feature_codec.utils import synth  # noqa: E402
from oracle import ref_unet, ref_train, ref_diffusion  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(HERE / "golden" / "train_objective.npz")
STEP = np.load(HERE / "golden" / "train_step.npz")
RECON_W, TV_W = 0.05, 1e-4
U = R.U


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_kernel(eps, noise, x_t, x0, a, s, recon_w, tv_w):
    terms, d = _native.diffusion_loss_grad(dev(eps), dev(noise), dev(x_t), dev(x0), dev(a), dev(s), recon_w, tv_w)
    torch.cuda.synchronize()
    return terms.cpu().numpy(), d.cpu().numpy()


def aux_set(eps, x_t, x0, a, s, recon_w, tv_w):
    """Elements whose L1 + TV gradient is non-zero: with noise := eps the MSE part of d_eps is exactly 0 (raw does not read noise)."""
    _, d = run_kernel(eps, eps, x_t, x0, a, s, recon_w, tv_w)
    return d != 0


def check_terms_against_float64(terms, cf, recon_w, tv_w, what):
    ref = cf["terms"]
    bound = 1.01 * U * ref
    bound[0] += U * (recon_w * ref[2] + tv_w * ref[3])
    err = np.abs(terms.astype(np.float64) - ref)
    print(f"{what}: loss terms {terms}, error / bound {err / bound}")
    assert np.all(err <= bound), (what, err / bound)


def torch_objective(eps_hat, noise, x_t, x0, a, s, recon_w, tv_w):
    """The objective as train/diffusion_train.py:124-128 writes it, in torch ops (the test's own restatement)."""
    x0_pred = ((x_t - s.view(-1, 1, 1, 1) * eps_hat) / a.view(-1, 1, 1, 1)).clamp(-1, 1)
    mse = F.mse_loss(eps_hat, noise)
    l1 = F.l1_loss(x0_pred, x0)
    tv = (x0_pred[:, :, 1:, :] - x0_pred[:, :, :-1, :]).abs().mean() + (x0_pred[:, :, :, 1:] - x0_pred[:, :, :, :-1]).abs().mean()
    return mse + recon_w * l1 + tv_w * tv, (mse, l1, tv)


def test_kernel_against_the_reference_fixture():
    g = GOLD
    cf = R.closed_form(g["eps_hat"], g["noise"], g["raw"], g["x0"], g["a"], g["s"], RECON_W, TV_W)
    terms, d = run_kernel(g["eps_hat"], g["noise"], g["x_t"], g["x0"], g["a"], g["s"], RECON_W, TV_W)
    got = aux_set(g["eps_hat"], g["x_t"], g["x0"], g["a"], g["s"], RECON_W, TV_W)
    want = cf["aux"] != 0
    assert want.sum() > 0.3 * want.size and (~want).sum() > 0.3 * want.size
    mism = int((got != want).sum())
    print(f"fixture: {int(want.sum())} elements with an auxiliary gradient, {mism} mismatches")
    assert mism == 0
    ratio = R.worst_ratio(d, cf)
    print(f"fixture: kernel d_eps vs float64 closed form, worst |err| / (K U S) = {ratio:.3f} (K = {R.K}; K = 1: {ratio * R.K:.2f})")
    assert ratio <= 1.0, ratio
    check_terms_against_float64(terms, cf, RECON_W, TV_W, "fixture")
    # d_eps_dev may be NULL: the terms alone
    t2, none = _native.diffusion_loss_grad(dev(g["eps_hat"]), dev(g["noise"]), dev(g["x_t"]), dev(g["x0"]), dev(g["a"]), dev(g["s"]),
                                           RECON_W, TV_W, want_grad=False)
    assert none is None and np.array_equal(t2.cpu().numpy(), terms)


def test_zero_weights_are_the_mse_kernels_bit_for_bit():
    g = GOLD
    terms, d = _native.diffusion_loss_grad(dev(g["eps_hat"]), dev(g["noise"]), dev(g["x_t"]), dev(g["x0"]), dev(g["a"]), dev(g["s"]), 0.0, 0.0)
    loss, d_mse = _native.mse_loss_grad(dev(g["eps_hat"]), dev(g["noise"]))
    assert torch.equal(d, d_mse)
    assert torch.equal(terms[0], loss) and torch.equal(terms[1], loss)
    assert float(terms[2]) == 0.0 and float(terms[3]) == 0.0


def make_inputs(shape, seed):
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randint(0, 256, shape, generator=g).float() / 127.5 - 1.0
    x0[0, :, : max(1, H // 8), :] = 1.0
    x0[-1, :, :, : max(1, W // 8)] = -1.0
    t = torch.tensor([(0, 120, 400, 700, 930, 999)[i % 6] for i in range(B)]) if B > 1 else torch.tensor([400])
    noise = torch.randn(shape, generator=g)
    eps = noise + 0.3 * torch.randn(shape, generator=g)
    tables = ref_diffusion.scheduler_tables(1000, "cosine")
    a = tables["sqrt_alphas_cumprod"][t].contiguous(); s = tables["sqrt_one_minus_alphas_cumprod"][t].contiguous()
    x_t = ref_diffusion.q_sample(tables, x0, t, noise)
    return x0, t, noise, eps, x_t, a, s


# (1, 2, 18, 523): five x tiles of 128 columns, the last one 11 wide, W odd
@pytest.mark.parametrize("shape", [(1, 3, 2, 2), (2, 3, 40, 24), (3, 1, 17, 130), (2, 3, 64, 257), (4, 3, 256, 256), (1, 2, 18, 523)])
def test_shapes_that_stress_tiling_against_torch_autograd(shape):
    x0, t, noise, eps, x_t, a, s = make_inputs(shape, seed=sum(shape))
    leaf = eps.clone().requires_grad_(True)
    loss, (mse, l1, tv) = torch_objective(leaf, noise, x_t, x0, a, s, RECON_W, TV_W)
    loss.backward()
    ref_d = leaf.grad.numpy()
    raw = ((x_t - s.view(-1, 1, 1, 1) * eps) / a.view(-1, 1, 1, 1))
    raw_gpu = _native.predict_x0(x_t.to(DEV), eps.to(DEV), a.to(DEV), s.to(DEV)).cpu()
    raw_diff = int((raw_gpu != raw).sum())
    cf = R.closed_form(eps.numpy(), noise.numpy(), raw.numpy(), x0.numpy(), a.numpy(), s.numpy(), RECON_W, TV_W)
    terms, d = run_kernel(eps.numpy(), noise.numpy(), x_t.numpy(), x0.numpy(), a.numpy(), s.numpy(), RECON_W, TV_W)
    got = aux_set(eps.numpy(), x_t.numpy(), x0.numpy(), a.numpy(), s.numpy(), RECON_W, TV_W)
    mism = int((got != (cf["aux"] != 0)).sum())
    print(f"{shape}: raw differs between CPU and GPU in {raw_diff} elements; auxiliary-gradient set mismatches {mism}")
    assert raw_diff == 0 and mism == 0
    ratio = R.worst_ratio(d, dict(cf, d_eps=ref_d.astype(np.float64)), k=2 * R.K)
    ratio64 = R.worst_ratio(d, cf)
    print(f"{shape}: kernel vs torch fp32 autograd, worst |err| / (2 K U S) = {ratio:.3f}; vs float64 closed form / (K U S) = {ratio64:.3f}")
    assert ratio <= 1.0 and ratio64 <= 1.0, (ratio, ratio64)
    check_terms_against_float64(terms, cf, RECON_W, TV_W, str(shape))
    # and against torch's own fp32 terms: their pairwise fp32 sums carry up to (3 + ceil(log2 n) + 2) U (tests/test_objective_host.py)
    n = eps.numel()
    tb = (3 + np.ceil(np.log2(n)) + 2 + 1.01) * U
    ref_terms = np.array([float(v.detach()) for v in (loss, mse, l1, tv)])
    assert np.all(np.abs(terms - ref_terms) <= tb * np.abs(ref_terms)), (terms, ref_terms)


def test_degenerate_images_are_rejected():
    x = torch.zeros((1, 1, 1, 8), device=DEV); c = torch.ones(1, device=DEV)
    with pytest.raises(Exception):
        _native.diffusion_loss_grad(x, x, x, x, c, c, RECON_W, TV_W)
    x = torch.zeros((1, 1, 8, 1), device=DEV)
    with pytest.raises(Exception):
        _native.diffusion_loss_grad(x, x, x, x, c, c, RECON_W, TV_W)


@pytest.mark.parametrize("shape", [(4, 3, 256, 256), (3, 1, 17, 130)])
def test_two_runs_are_bit_identical(shape):
    x0, t, noise, eps, x_t, a, s = make_inputs(shape, seed=5)
    args = [v.numpy() for v in (eps, noise, x_t, x0, a, s)]
    t1, d1 = run_kernel(*args, RECON_W, TV_W)
    t2, d2 = run_kernel(*args, RECON_W, TV_W)
    assert np.array_equal(t1.view(np.uint32), t2.view(np.uint32)) and np.array_equal(d1.view(np.uint32), d2.view(np.uint32))


def make_net(sd, base, ch_mult, dtype="fp32"):
    net = CLIPCondUNet(z_dim=512, base=base, ch_mult=ch_mult, dtype=dtype).to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.train()


def oracle_objective_grads(sd, tables, x0, z, t, noise):
    """ref_train.train_step_grads with the objective on top of the oracle network."""
    x_t = ref_diffusion.q_sample(tables, x0, t, noise)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    eps = ref_unet.unet_forward(leaves, x_t, z, t)
    a = tables["sqrt_alphas_cumprod"][t]; s = tables["sqrt_one_minus_alphas_cumprod"][t]
    loss, terms = torch_objective(eps, noise, x_t, x0, a, s, RECON_W, TV_W)
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return loss.detach(), {k: g for k, g in zip(leaves, grads)}, eps.detach(), x_t, [float(v.detach()) for v in terms]


def mask_of(x_t, eps, a, s):
    raw = (x_t - s.view(-1, 1, 1, 1) * eps) / a.view(-1, 1, 1, 1)
    return (raw >= -1) & (raw <= 1)


def test_train_step_with_the_objective_matches_the_oracle_over_three_steps():
    """train_step(recon_w=0.05, tv_w=1e-4) for three steps against the oracle loop with the test's torch objective on top: the shape,
    inputs and bounds of test_fused_loss_and_adamw_match_oracle_over_three_steps (5e-5 relative loss, 5 % of the Adam movement).
    Clamp-mask flips between the GPU's and the oracle's eps_hat are counted and printed, not absorbed in a bound."""
    sd = synth.synth_state_dict(synth.unet_param_spec(512, 32, (1, 2)))
    tables = ref_diffusion.scheduler_tables(1000, "cosine")
    x0, z, t, noise = (torch.from_numpy(STEP[k]) for k in ("x0", "z", "t", "noise"))
    net = make_net(sd, 32, (1, 2))
    sch = NoiseScheduler(1000, "cosine", device=DEV)
    opt = FusedAdamW(net, lr=2e-4)
    state = net.train_state()
    ref = ref_unet.as_torch_sd(sd)
    m = {k: torch.zeros_like(v) for k, v in ref.items()}; v2 = {k: torch.zeros_like(v) for k, v in ref.items()}
    a = tables["sqrt_alphas_cumprod"][t]; s = tables["sqrt_one_minus_alphas_cumprod"][t]
    for step in range(1, 4):
        loss = train_step(net, sch, opt, x0.to(DEV), z.to(DEV), t.to(DEV), noise.to(DEV), recon_w=RECON_W, tv_w=TV_W)
        terms = state.last_loss_terms.cpu().numpy()
        eps_gpu = state.static_buffers(x0.to(DEV), z.to(DEV))["eps"].cpu()
        rloss, rg, reps, x_t, rterms = oracle_objective_grads(ref, tables, x0, z, t, noise)
        flips = int((mask_of(x_t, eps_gpu, a, s) != mask_of(x_t, reps, a, s)).sum())
        rel = abs(float(loss) - float(rloss)) / float(rloss)
        print(f"step {step}: loss {float(loss):.7f} oracle {float(rloss):.7f} (relative {rel:.2e}); terms {terms} oracle {rterms}; "
              f"clamp-mask flips {flips} of {eps_gpu.numel()}")
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
    print(f"worst parameter distance from the oracle after three steps: {worst:.4f} of the Adam movement (bound 0.05)")
    assert net.train_state().fp.intact()
    # an MSE-only step afterwards is the old step: no terms
    train_step(net, sch, opt, x0.to(DEV), z.to(DEV), t.to(DEV), noise.to(DEV))
    assert state.last_loss_terms is None


class _KeepGrads:
    """An optimiser that leaves parameters and gradients alone: train_step then ends with the step's gradient in the flat buffer."""

    def step(self):
        pass

    def zero_grad(self):
        pass


def _step_grads(sd, dtype, x0, z, t, noise, recon_w, tv_w):
    net = make_net(sd, 128, (1, 2, 2), dtype=dtype)
    st = net.train_state()
    st.fp.grad.zero_()
    loss = train_step(net, NoiseScheduler(1000, "cosine", device=DEV), _KeepGrads(), x0.to(DEV), z.to(DEV), t.to(DEV), noise.to(DEV),
                      recon_w=recon_w, tv_w=tv_w)
    torch.cuda.synchronize()
    eps = st.static_buffers(x0.to(DEV), z.to(DEV))["eps"].cpu().clone()
    return float(loss), {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}, eps


def _bf16_vs_fp32(g16, g32):
    worst_cos, worst_norm = ("", 1.0), ("", 1.0)
    for k, r in g32.items():
        a = g16[k].double().flatten(); b = r.double().flatten()
        cos = float((a @ b) / (a.norm() * b.norm() + 1e-30)); nr = float(a.norm() / (b.norm() + 1e-30))
        if cos < worst_cos[1]:
            worst_cos = (k, cos)
        if abs(nr - 1) > abs(worst_norm[1] - 1):
            worst_norm = (k, nr)
    return worst_cos, worst_norm


def test_bf16_step_with_the_objective_against_fp32_mode():
    """One step at base 128, (1,2,2), batch 2, 64 px with the objective on: the parameter gradients of the bf16 mode against the fp32
    mode, with the bounds of test_bf16_gradients_at_c2_widths_against_fp32_mode (loss 2e-2 relative, cosine > 0.97, norm ratio within
    10 %).  The MSE-only figures of the same step are printed next to them."""
    sd = synth.synth_state_dict(synth.unet_param_spec(512, 128, (1, 2, 2)))
    B, S = 2, 64
    g = torch.Generator("cpu").manual_seed(21)
    x0 = torch.randint(0, 256, (B, 3, S, S), generator=g).float() / 127.5 - 1.0
    z = torch.from_numpy(synth.synth_z(B)); t = torch.tensor([450, 980]); noise = torch.randn((B, 3, S, S), generator=g)
    tables = ref_diffusion.scheduler_tables(1000, "cosine")
    a = tables["sqrt_alphas_cumprod"][t]; s = tables["sqrt_one_minus_alphas_cumprod"][t]
    x_t = ref_diffusion.q_sample(tables, x0, t, noise)
    res = {}
    for name, (rw, tw) in (("objective", (RECON_W, TV_W)), ("mse only", (0.0, 0.0))):
        l32, g32, e32 = _step_grads(sd, "fp32", x0, z, t, noise, rw, tw)
        l16, g16, e16 = _step_grads(sd, "bf16", x0, z, t, noise, rw, tw)
        wc, wn = _bf16_vs_fp32(g16, g32)
        flips = int((mask_of(x_t, e16, a, s) != mask_of(x_t, e32, a, s)).sum())
        print(f"bf16 vs fp32 mode, {name}: loss {l16:.6f} vs {l32:.6f} (relative {abs(l16 - l32) / l32:.2e}); worst cosine {wc[1]:.4f} ({wc[0]}); "
              f"worst norm ratio {wn[1]:.4f} ({wn[0]}); clamp-mask flips {flips} of {e16.numel()}")
        res[name] = (l16, l32, wc, wn)
    l16, l32, wc, wn = res["objective"]
    assert abs(l16 - l32) < 2e-2 * l32
    assert wc[1] > 0.97, wc
    assert 0.9 < wn[1] < 1.1, wn


def test_train_diffusion_fused_objective_against_the_autograd_route(tmp_path, monkeypatch):
    """Same store, same seed: the per-epoch logged losses of the fused route and of the autograd route.  Both compute one function
    with the same forward and backward kernels; they differ in the rounding of d_eps (K U S per element, against the 5e-5 relative
    loss agreement the oracle test holds per step across a CPU/GPU difference that is orders larger) and in the log line's four
    decimals (0.5e-4 per value).  Bound per epoch e of three steps: 1e-4 + 5e-5 * e * loss."""
    from clip_feature_codec.io import bitstream
    from clip_feature_codec.train import diffusion_train as dt
    store = tmp_path / "store"
    synth.write_synth_store(store, 12, 32, write_clp=bitstream.write_bitstream)
    calls = []
    real = _native.diffusion_loss_grad
    monkeypatch.setattr(_native, "diffusion_loss_grad", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    out = {}
    for fused in (True, False):
        lines = []
        calls.clear()
        torch.manual_seed(0)
        dt.train_diffusion(store, out_size=32, epochs=3, batch_size=4, lr=1e-3, device=DEV, save_dir=tmp_path / f"ckpt{int(fused)}", base=32,
                           ch_mult=(1, 2), dtype="fp32", num_workers=0, clip_w=0.0, log=lines.append, fused_objective=fused)
        out[fused] = [float(ln.split("loss=")[1]) for ln in lines if "epoch" in ln]
        assert len(calls) == (9 if fused else 0), (fused, len(calls))
    print(f"train_diffusion per-epoch losses: fused {out[True]}, autograd {out[False]}")
    assert len(out[True]) == 3 and all(np.isfinite(out[True]))
    for e, (lf, la) in enumerate(zip(out[True], out[False]), start=1):
        assert abs(lf - la) <= 1e-4 + 5e-5 * e * la, (e, lf, la)
    sd_f = torch.load(tmp_path / "ckpt1" / "diffusion_unet_final.pt", map_location="cpu", weights_only=True)
    assert set(sd_f) == {k for k, _ in synth.unet_param_spec(512, 32, (1, 2))}


def _ddp_objective_rank(rank, world, port, out):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    sd = synth.synth_state_dict(synth.unet_param_spec(512, 32, (1, 2)))
    net = make_net(sd, 32, (1, 2))
    st = net.train_state()
    x0, x, z, t, noise = (torch.from_numpy(STEP[k]) for k in ("x0", "x_t", "z", "t", "noise"))
    tables = ref_diffusion.scheduler_tables(1000, "cosine")
    a = tables["sqrt_alphas_cumprod"][t].contiguous(); s = tables["sqrt_one_minus_alphas_cumprod"][t].contiguous()
    B = x.shape[0]
    lo, hi = rank * B // world, (rank + 1) * B // world
    x0, x, z, t, noise, a, s = (v[lo:hi].contiguous().to(DEV) for v in (x0, x, z, t, noise, a, s))
    eps = st.trainer.forward(st.fp.flat, x, z, t)
    terms, d = _native.diffusion_loss_grad(eps, noise, x, x0, a, s, RECON_W, TV_W)
    d.mul_(1.0 / world)
    st.fp.grad.zero_()
    works = []
    st.trainer.backward(st.fp.flat, st.fp.grad, x, z, d, bucket_floats=200_000,
                        bucket_cb=(lambda lo_, hi_: works.append(dist.all_reduce(st.fp.grad[lo_:hi_], async_op=True))) if world > 1 else None)
    for w in works:
        w.wait()
    torch.cuda.synchronize()
    if rank == 0:
        np.save(out, st.fp.grad.cpu().numpy())
    if world > 1:
        dist.destroy_process_group()


def test_two_ranks_with_the_objective_give_the_full_batch_gradient(tmp_path):
    """Half of the fixture's batch per rank, the objective's gradient scaled by 1 / world, every bucket all-reduced as the backward
    hands it out (gloo on one card): the reduced flat gradient equals the single-process full-batch gradient to 1e-5 of its max --
    every term of the objective is a mean over equal shards, so the mean of the shard gradients is the full-batch gradient."""
    import torch.multiprocessing as mp
    _ddp_objective_rank(0, 1, 0, str(tmp_path / "g1.npy"))
    mp.spawn(_ddp_objective_rank, args=(2, 29581, str(tmp_path / "g2.npy")), nprocs=2, join=True)
    g1, g2 = np.load(tmp_path / "g1.npy"), np.load(tmp_path / "g2.npy")
    assert np.abs(g1).max() > 0
    assert np.abs(g1 - g2).max() <= 1e-5 * np.abs(g1).max(), np.abs(g1 - g2).max() / np.abs(g1).max()
