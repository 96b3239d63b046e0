"""Classifier-free guidance on the GPU: the combine-and-update kernel bit for bit against the torch-CPU op sequence, the fused guided
loop (``ccn_sample_guided``) against the CPU oracle evaluated twice per step, its routes and identities, and the embedding dropout of
the training step.  All on the C1-sized model (base 32, ``(1, 2)``), B = 2, 32 px, 6 steps unless a test says otherwise."""
import numpy as np
import pytest
import torch

from clip_feature_codec import _native
from clip_feature_codec.models.unet import CLIPCondUNet
from clip_feature_codec.diffusion.scheduler import NoiseScheduler
from clip_feature_codec.diffusion.ddim import DDIMSampler
from oracle import ref_unet, ref_diffusion

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

TOL_E2E_FP32 = 1e-3       # tests/test_gpu_parity.py: BASELINE.json north_star, max-abs on the reconstructed tensor
TOL_COND_PATHS = 1e-5     # test_graph_equals_stepwise_and_is_deterministic: hoisted table vs the int64 conditioning path
B, S, T, W_G = 2, 32, 6, 3.0


def to_dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a))).to(DEV)


def maxerr(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


def make_net(sd, dtype="fp32"):
    net = CLIPCondUNet(z_dim=512, base=32, ch_mult=(1, 2), dtype=dtype).to(DEV).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net


def oracle_guided(model, w, null_row):
    """The reference model wrapped as the guided prediction: eu + w * (ec - eu), eu from the null embedding."""
    def f(x, z, t):
        eu = model(x, null_row.expand(x.shape[0], -1), t)
        ec = model(x, z, t)
        return eu + w * (ec - eu)
    return f


@pytest.fixture(scope="module")
def tiny_net(tiny_sd):
    return make_net(tiny_sd)


@pytest.fixture(scope="module")
def cpu_model(tiny_sd):
    return ref_unet.make_model(ref_unet.as_torch_sd(tiny_sd))


@pytest.fixture(scope="module")
def inputs(synth):
    return torch.from_numpy(synth.synth_z(B)), torch.from_numpy(synth.start_noise(range(B), S))


@pytest.fixture(scope="module")
def ref_guided_cosine(cpu_model, inputs):
    """The oracle's guided sample (cosine, w = 3, zero null embedding); shared, never written to."""
    z, xT = inputs
    with torch.no_grad():
        return ref_diffusion.ddim_sample(oracle_guided(cpu_model, W_G, torch.zeros(512)), z, xT, steps=T)


@pytest.fixture(scope="module")
def gpu_guided_cosine(tiny_net, inputs):
    """The fused guided sample of the same inputs (first call: capture + replay)."""
    z, xT = inputs
    sampler = DDIMSampler(NoiseScheduler(1000, "cosine", DEV), guided=True)
    return sampler, sampler.sample(tiny_net, to_dev(z), (B, 3, S, S), steps=T, cfg_scale=W_G, x_T=to_dev(xT))


# ------------------------------------------------------------------------------------------------------------------ 1. the kernel
N_STRIDE = 2048 * 256 * 4 + 3 * 256 * 4 + 3      # past the grid cap of the four-wide form: every lane strides, three-element tail


def _kernel_case(golden, n, w, row, with_noise, with_dup, offset=0):
    """One launch against ``ref_diffusion.ddim_update(x, eu + w * (ec - eu), coef_row, noise)`` on the CPU.  ``offset``: the tensors
    are views that many floats into their buffers (an offset of 1 takes the one-element-per-lane form)."""
    coef = golden("scheduler.npz")["coef.10"][row].astype(np.float32).copy()       # (see test_ddim_step_bit_exact: the table's bits
    sigma = np.float32(0.3) if with_noise else np.float32(0.0)                     #  are those of the host that made the fixture)
    coef[4] = sigma
    g = torch.Generator().manual_seed(1000 * row + n % 997)
    x, ec, eu, nz = (torch.randn(n, generator=g) for _ in range(4))
    x = float(coef[1]) * 1.2 * x + float(coef[0]) * (eu + w * (ec - eu))           # x0 ~ 1.2 N(0, 1): both sides of the clamp
    ref =ref_diffusion.ddim_update(x, eu + w * (ec - eu), coef, nz if with_noise else None)

    def view(t):
        return torch.cat([torch.zeros(offset), t]).to(DEV)[offset:]
    xd, ecd, eud = view(x), view(ec), view(eu)
    nzd = view(nz) if with_noise else None
    dup = view(torch.full((n,), 7.0)) if with_dup else None
    assert xd.data_ptr() % 16 == (4 * offset) % 16
    _native.cfg_ddim_step(xd, ecd, eud, w, coef[:4], float(sigma), nzd, x_dup=dup)
    what = f"n={n} w={w} row={row} noise={with_noise} dup={with_dup} offset={offset}"
    assert np.array_equal(xd.cpu().numpy(), ref.numpy()), what
    if with_dup:
        assert torch.equal(dup, xd), what + ": x_dup differs from x"
    assert torch.equal(ecd.cpu(), ec) and torch.equal(eud.cpu(), eu), what + ": an input was written"


@pytest.mark.parametrize("n", [1, 255, 2 * 3 * 17 * 19, 2 * 3 * 64 * 64])
@pytest.mark.parametrize("w", [0.0, 1.3, 3.0, 7.5])
def test_cfg_ddim_step_bit_exact(golden, n, w):
    row = int(w * 10 + n) % 10
    for with_noise in (False, True):
        for with_dup in (False, True):
            _kernel_case(golden, n, w, row, with_noise, with_dup)


@pytest.mark.parametrize("n,offset", [(255, 1), (2 * 3 * 17 * 19, 1), (2 * 3 * 17 * 19, 2), (N_STRIDE, 0), (256 * 4096 + 5, 1)])
def test_cfg_ddim_step_bit_exact_other_paths(golden, n, offset):
    """Unaligned pointers (one element per lane), and sizes past the grid cap of either form (the grid-stride loop)."""
    _kernel_case(golden, n, 3.0, 4, True, True, offset)
    _kernel_case(golden, n, 1.3, 9, False, False, offset)


# ------------------------------------------------------------------------------------------------------- 2. fused loop vs the oracle
def test_guided_fused_matches_oracle_and_guidance_matters(cpu_model, inputs, ref_guided_cosine, gpu_guided_cosine):
    z, xT = inputs
    _, got = gpu_guided_cosine
    err = maxerr(got, ref_guided_cosine)
    with torch.no_grad():
        unguided = ref_diffusion.ddim_sample(cpu_model, z, xT, steps=T)
    gap = maxerr(ref_guided_cosine, unguided)
    print(f"guided fused vs oracle: max-abs {err:.3e}; oracle guided vs unguided: {gap:.3e}")
    assert got.shape == (B, 3, S, S) and got.device == torch.device(DEV)
    assert err < TOL_E2E_FP32, err
    assert gap > 10 * TOL_E2E_FP32, gap          # 7.3e-2 on these inputs: a sampler that ignores cfg_scale fails by 70x


# ------------------------------------------------------------------------------------------------------------------------ 3. routes
def test_guided_routes_agree(tiny_net, inputs, gpu_guided_cosine):
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sampler, a = gpu_guided_cosine
    b = sampler.sample(tiny_net, z, (B, 3, S, S), steps=T, cfg_scale=W_G, x_T=xT)          # graph replay
    assert torch.equal(a, b)
    plain = DDIMSampler(sampler.sch, guided=True)
    plain.use_graph = False
    c = plain.sample(tiny_net, z, (B, 3, S, S), steps=T, cfg_scale=W_G, x_T=xT)            # launch by launch
    assert torch.equal(a, c)
    d = sampler.sample(lambda x, zz, t: tiny_net(x, zz, t), z, (B, 3, S, S), steps=T, cfg_scale=W_G, x_T=xT)   # stepwise route
    # the 1e-5 between the two conditioning paths enters eps_c with weight |w| and eps_u with |1 - w|
    tol = (abs(W_G) + abs(W_G - 1)) * TOL_COND_PATHS
    assert maxerr(a, d) < tol, (maxerr(a, d), tol)


def test_guided_and_unguided_graphs_share_a_workspace(tiny_net, inputs, gpu_guided_cosine):
    """A guided call of batch B and an unguided one of batch 2B use the same plan, workspace and list of captured graphs, with the
    same timestep table and coefficients: each must find its own graph, and another scale is another capture."""
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sch = NoiseScheduler(1000, "cosine", DEV)
    z4, x4 = torch.cat([z, torch.zeros_like(z)]), torch.cat([xT, xT])
    unguided, guided = DDIMSampler(sch), DDIMSampler(sch, guided=True)
    u1 = unguided.sample(tiny_net, z4, (2 * B, 3, S, S), steps=T, x_T=x4)
    g1 = guided.sample(tiny_net, z, (B, 3, S, S), steps=T, cfg_scale=W_G, x_T=xT)
    u2 = unguided.sample(tiny_net, z4, (2 * B, 3, S, S), steps=T, x_T=x4)
    g2 = guided.sample(tiny_net, z, (B, 3, S, S), steps=T, cfg_scale=2.0, x_T=xT)
    g3 = guided.sample(tiny_net, z, (B, 3, S, S), steps=T, cfg_scale=W_G, x_T=xT)
    assert torch.equal(u1, u2)
    assert torch.equal(g1, gpu_guided_cosine[1]) and torch.equal(g3, g1)
    assert maxerr(g2, g1) > 10 * TOL_E2E_FP32


# -------------------------------------------------------------------------------------------------------------------- 4. identities
def test_guidance_identities(tiny_net, inputs):
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sch = NoiseScheduler(1000, "cosine", DEV)
    shape = (B, 3, S, S)
    unguided = DDIMSampler(sch)
    base = unguided.sample(tiny_net, z, shape, steps=T, x_T=xT)
    # the reference's behaviour, kept: without the flag cfg_scale is accepted and unused
    assert torch.equal(unguided.sample(tiny_net, z, shape, steps=T, cfg_scale=3.0, x_T=xT), base)
    guided = DDIMSampler(sch, guided=True)
    assert torch.equal(guided.sample(tiny_net, z, shape, steps=T, cfg_scale=1.0, x_T=xT), base)
    # w = 0: eu + 0 * (ec - eu) is eu exactly, the unconditional half alone
    w0 = guided.sample(tiny_net, z, shape, steps=T, cfg_scale=0.0, x_T=xT)
    zero = unguided.sample(tiny_net, torch.zeros_like(z), shape, steps=T, x_T=xT)
    err = maxerr(w0, zero)
    assert err < 1e-5, f"cfg_scale = 0 vs unguided on z = 0: not bit-equal, max-abs {err:.3e}"
    if not torch.equal(w0, zero):
        import warnings
        warnings.warn(f"cfg_scale = 0 vs unguided on z = 0: not bit-equal (max-abs {err:.3e}); only the plan's batch differs")
    assert maxerr(w0, base) > 10 * TOL_E2E_FP32


# ------------------------------------------------------------------------------------------------------------------------ 5. null_z
def test_nonzero_null_embedding(synth, tiny_net, cpu_model, inputs, ref_guided_cosine):
    """The null row is ``synth.synth_z(1, seed=77)[0]``: on the CPU oracle it moves the guided sample by 7.6e-2 from the zero-null
    one on these inputs."""
    z, xT = inputs
    row = torch.from_numpy(synth.synth_z(1, seed=77)[0])
    with torch.no_grad():
        ref = ref_diffusion.ddim_sample(oracle_guided(cpu_model, W_G, row), z, xT, steps=T)
    assert maxerr(ref, ref_guided_cosine) > 10 * TOL_E2E_FP32
    sampler = DDIMSampler(NoiseScheduler(1000, "cosine", DEV), guided=True, null_z=row)     # (a host tensor: moved by the sampler)
    got = sampler.sample(tiny_net, to_dev(z), (B, 3, S, S), steps=T, cfg_scale=W_G, x_T=to_dev(xT))
    assert maxerr(got, ref) < TOL_E2E_FP32, maxerr(got, ref)
    assert maxerr(got, ref_guided_cosine) > 10 * TOL_E2E_FP32


# ----------------------------------------------------------------------------------------------------------------------- 6. eta > 0
def test_guided_eta_positive(tiny_net, cpu_model, inputs):
    """Linear schedule, eta = 0.03, 6 steps (test_eta_positive_fused_graph_matches_oracle_and_stepwise: every coefficient real).
    One set of draws serves both halves; the oracle is fed the same draws."""
    eta = 0.03
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sch = NoiseScheduler(1000, "linear", DEV)
    assert np.isfinite(sch.ddim_coefficients(T, eta)).all() and (sch.ddim_coefficients(T, eta)[:-1, 4] > 0).all()
    sampler = DDIMSampler(sch, eta=eta, guided=True)
    torch.manual_seed(1234)
    a = sampler.sample(tiny_net, z, (B, 3, S, S), steps=T, cfg_scale=W_G, x_T=xT)
    draws = next(iter(sampler._noise.values())).cpu().clone()
    assert draws.shape == (T, B, 3, S, S)
    it = iter(range(T))
    with torch.no_grad():
        ref = ref_diffusion.ddim_sample(oracle_guided(cpu_model, W_G, torch.zeros(512)), inputs[0], inputs[1], steps=T, schedule="linear",
                                        eta=eta, noise_fn=lambda x: draws[next(it)])
    assert maxerr(a, ref) < TOL_E2E_FP32, maxerr(a, ref)
    torch.manual_seed(1234)
    b = sampler.sample(lambda x, zz, t: tiny_net(x, zz, t), z, (B, 3, S, S), steps=T, cfg_scale=W_G, x_T=xT)      # stepwise route
    assert maxerr(a, b) < (abs(W_G) + abs(W_G - 1)) * TOL_COND_PATHS, maxerr(a, b)
    torch.manual_seed(1234)
    c = sampler.sample(tiny_net, z, (B, 3, S, S), steps=T, cfg_scale=W_G, x_T=xT)                                   # replay
    assert torch.equal(a, c)


# ---------------------------------------------------------------------------------------------------------------- 7. a second shape
def test_guided_second_shape(synth, tiny_net, cpu_model):
    """B = 3 (six rows in the plan), 48 x 32 px, 4 steps."""
    b, h, w, steps = 3, 48, 32, 4
    z = torch.from_numpy(synth.synth_z(b, seed=50))
    xT = torch.randn((b, 3, h, w), generator=torch.Generator().manual_seed(48))
    with torch.no_grad():
        ref = ref_diffusion.ddim_sample(oracle_guided(cpu_model, W_G, torch.zeros(512)), z, xT, steps=steps)
    got = DDIMSampler(NoiseScheduler(1000, "cosine", DEV), guided=True).sample(tiny_net, to_dev(z), (b, 3, h, w), steps=steps,
                                                                                 cfg_scale=W_G, x_T=to_dev(xT))
    assert maxerr(got, ref) < TOL_E2E_FP32, maxerr(got, ref)


# -------------------------------------------------------------------------------------------------------------------------- 8. bf16
def test_guided_bf16_bounded(tiny_sd, inputs, gpu_guided_cosine):
    """bf16 mode: finite, and within the bounds the suite uses for bf16 trajectories (test_c2_bf16_reported_deviation: 0.6 max,
    0.065 mean).  They catch garbage, not rounding."""
    net = make_net(tiny_sd, dtype="bf16")
    x = DDIMSampler(NoiseScheduler(1000, "cosine", DEV), guided=True).sample(net, to_dev(inputs[0]), (B, 3, S, S), steps=T,
                                                                               cfg_scale=W_G, x_T=to_dev(inputs[1]))
    d = (x - gpu_guided_cosine[1]).abs()
    print(f"guided bf16 vs guided fp32 (C1 size, {T} steps, w = {W_G}): max-abs {float(d.max()):.3e} mean-abs {float(d.mean()):.3e}")
    assert bool(torch.isfinite(x).all())
    assert float(d.max()) < 0.6 and float(d.mean()) < 0.065, (float(d.max()), float(d.mean()))


# ------------------------------------------------------------------------------------------------------------------- 9. error paths
def test_guided_error_paths(tiny_net, inputs, gpu_guided_cosine):
    z, xT = to_dev(inputs[0]), to_dev(inputs[1])
    sch = NoiseScheduler(1000, "cosine", DEV)
    shape = (B, 3, S, S)
    for bad in (torch.zeros(511), torch.zeros(1, 512), torch.zeros(512, 1)):
        with pytest.raises(ValueError, match="null_z"):
            DDIMSampler(sch, guided=True, null_z=bad).sample(tiny_net, z, shape, steps=T, cfg_scale=W_G, x_T=xT)
    guided = DDIMSampler(sch, guided=True)
    for bad in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="finite"):
            guided.sample(tiny_net, z, shape, steps=T, cfg_scale=bad, x_T=xT)
        with pytest.raises(ValueError, match="finite"):
            guided.sample(lambda x, zz, t: tiny_net(x, zz, t), z, shape, steps=T, cfg_scale=bad, x_T=xT)
    with pytest.raises(ValueError, match="shape mismatch"):
        guided.sample(tiny_net, z[:1], shape, steps=T, cfg_scale=W_G, x_T=xT)
    with pytest.raises(ValueError, match="shape mismatch"):
        guided.sample(tiny_net, torch.cat([z, z]), shape, steps=T, cfg_scale=W_G, x_T=xT)
    # the library's own checks, below the Python ones
    nat = tiny_net.native()
    ts, coef = sch.ddim_timesteps(T), sch.ddim_coefficients(T, 0.0)
    with pytest.raises(ValueError, match="null_z"):
        nat.sample(z, xT, ts, coef[:, :4], w=W_G, z_null=torch.zeros(3, device=DEV))
    with pytest.raises(ValueError, match="finite"):
        nat.sample(z, xT, ts, coef[:, :4], w=float("nan"))
    again = guided.sample(tiny_net, z, shape, steps=T, cfg_scale=W_G, x_T=xT)
    torch.cuda.synchronize()
    tiny_net.native().poll_errors()
    assert torch.equal(again, gpu_guided_cosine[1])


# --------------------------------------------------------------------------------------------------------------------- 10. training
def test_train_step_z_drop(synth, tiny_sd):
    """z_drop = 1 zeroes every row: the gradient of z_proj.0.weight is then exactly zero, its moments stay zero and, without weight
    decay, the weight is bit-unchanged, while the bias moves.  z_drop = 0 with explicit t / noise leaves the device generator alone."""
    from clip_feature_codec.train.diffusion_train import FusedAdamW, train_step
    net = make_net(tiny_sd).train()
    sch = NoiseScheduler(1000, "cosine", device=DEV)
    opt = FusedAdamW(net, lr=2e-4, weight_decay=0.0)
    g = torch.Generator().manual_seed(21)
    x0 = to_dev(torch.rand((B, 3, S, S), generator=g) * 2 - 1); z = to_dev(synth.synth_z(B))
    noise = to_dev(torch.randn((B, 3, S, S), generator=g)); t = to_dev(torch.tensor([700, 20]))
    named = dict(net.named_parameters())
    w0, b0 = named["z_proj.0.weight"].detach().clone(), named["z_proj.0.bias"].detach().clone()
    rng = torch.cuda.get_rng_state(DEV)
    loss = train_step(net, sch, opt, x0, z, t=t, noise=noise, z_drop=1.0)
    assert np.isfinite(float(loss))
    assert not torch.equal(torch.cuda.get_rng_state(DEV), rng)             # the mask's draw
    assert torch.equal(named["z_proj.0.weight"].detach().view(torch.int32), w0.view(torch.int32))
    assert not torch.equal(named["z_proj.0.bias"].detach(), b0)
    assert torch.equal(net.train_state().static_buffers(x0, z)["z"], torch.zeros_like(z))
    rng = torch.cuda.get_rng_state(DEV)
    train_step(net, sch, opt, x0, z, t=t, noise=noise, z_drop=0.0)
    assert torch.equal(torch.cuda.get_rng_state(DEV), rng)
    assert torch.equal(net.train_state().static_buffers(x0, z)["z"], z)
    assert not torch.equal(named["z_proj.0.weight"].detach(), w0)         # with its embeddings back, the weight trains
    with pytest.raises(ValueError):
        train_step(net, sch, opt, x0, z, t=t, noise=noise, z_drop=1.5)
