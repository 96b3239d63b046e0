"""The weight EMA on the GPU: ccn_adamw_step_ema against the entry points it stands beside (same AdamW bits) and against the float64
closed form of tests/ema_ref.py, then FusedAdamW(ema_decay=) through train_step, the averaged weights for inference, the resumable
optimiser state and train_diffusion(ema_decay=, resume=)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "clip-neural-image-conpression_amd"), str(ROOT / "tests")]

from clip_feature_codec import _native  # noqa: E402
from clip_feature_codec.models.unet import CLIPCondUNet  # noqa: E402
from clip_feature_codec.diffusion.scheduler import NoiseScheduler  # noqa: E402
from clip_feature_codec.train.diffusion_train import FusedAdamW, GradScaler, train_step  # noqa: E402
from clip_feature_codec.utils import synth  # noqa: E402
import ema_ref  # noqa: E402
import guard_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(ROOT / "tests" / "golden" / "train_step.npz")
H = guard_ref.HYPER
GW = _native.GUARD_WORD
EW = _native.EMA_WORD
PAD = 4                   # floats of padding before and after every buffer's range
SENTINEL = 7.0
GRID_CAP = 8192           # launch_adamw's cap: workgroups of 256 threads, one 16-byte quad of each buffer per thread and trip
N_BIG = 4 * (GRID_CAP * 256 * 2 + 77) + 3          # two trips of the capped grid plus a ragged rest
Z5 = (0, 0, 0, 0, 0)
# (n, element offsets of p, g, m, v, ema off their 16-byte boundary): equal offsets keep the 16-byte kernel (with a scalar head),
# one odd buffer -- the gradient's, or the EMA's alone -- puts the call on the 4-byte kernel
CASES = [(1, Z5), (3, Z5), (255, Z5), (257, Z5), (10007, (1, 1, 1, 1, 1)), (10007, (0, 1, 0, 0, 0)), (10007, (0, 0, 0, 0, 1)), (N_BIG, Z5)]
IDS = [f"{n}-{''.join(map(str, o))}" for n, o in CASES]


class Kernels:
    """The C-ABI calls on raw buffers (what FusedAdamW.step issues with ema_decay=), the pattern of test_gpu_guard.py's helper with a
    fifth buffer.  Every buffer sits in an allocation with PAD sentinel floats on both sides of its range (plus its offset)."""

    def __init__(self, p0, offset=Z5, decay=0.999, warmup=False, guarded=False, init_scale=65536.0, growth_interval=2000):
        p0 = torch.as_tensor(p0)
        n = p0.numel()
        self.n, self.offset, self.decay, self.warmup, self.guarded = n, offset, decay, warmup, guarded
        self.base = [torch.full((n + 2 * PAD + 4,), SENTINEL, device=DEV) for _ in range(5)]
        self.p, self.g, self.m, self.v, self.ema = (b[PAD + o:PAD + o + n] for b, o in zip(self.base, offset))
        self.p.copy_(p0)
        for b in (self.g, self.m, self.v):
            b.zero_()
        self.ema.fill_(-3.0)                # never read before the first update: the value must not matter
        assert all(b.data_ptr() % 16 == 4 * o for b, o in zip((self.p, self.g, self.m, self.v, self.ema), offset))
        self.ema_block = torch.zeros(_native.EMA_WORDS, dtype=torch.int32, device=DEV)
        _native.ema_init(self.ema_block, 0)
        self.block = self.scratch = None
        self.cfg = (2.0, 0.5, growth_interval)
        if guarded:
            self.block = torch.zeros(_native.GUARD_WORDS, dtype=torch.int32, device=DEV)
            self.scratch = torch.empty(_native.GUARD_SCRATCH_FLOATS, device=DEV)
            _native.step_guard_init(self.block, init_scale)
        self.steps = 0

    def word(self, name):
        k = GW[name]
        return (self.block.view(torch.float32) if k < 6 else self.block)[k]

    def eword(self, name):
        return self.ema_block.view(torch.float32)[0] if name == "weight" else self.ema_block[EW[name]]

    def step(self, g_unscaled, zero_grad=True, max_grad_norm=0.0):
        self.g.copy_(torch.as_tensor(g_unscaled))
        if self.guarded:
            self.g.mul_(self.word("scale"))
            _native.grad_guard(self.g, self.block, self.scratch, max_grad_norm, H["betas"][0], H["betas"][1], *self.cfg)
        self.steps += 1
        _native.adamw_step_ema(self.p, self.g, self.m, self.v, self.ema, H["lr"], H["betas"][0], H["betas"][1], H["eps"], H["weight_decay"],
                               self.steps, self.decay, self.ema_block, zero_grad=zero_grad, ema_warmup=self.warmup, guard_block=self.block)

    def padding_intact(self):
        return all(bool((b[:PAD + o] == SENTINEL).all()) and bool((b[PAD + o + self.n:] == SENTINEL).all()) for b, o in zip(self.base, self.offset))


def inputs(n, steps=3, seed=3):
    g = torch.Generator(DEV).manual_seed(seed)
    p0 = torch.randn(n, generator=g, device=DEV)
    return p0, [torch.randn(n, generator=g, device=DEV) * 0.01 for _ in range(steps)]


def ulp32_dev(x):
    """Elementwise fp32 ulp of |x| as float64, from the exponent bits: 2^(E - 150) for biased exponent E (no smaller than 2^-126:
    the values here are nowhere near 2^-103)."""
    e = x.abs().float().contiguous().view(torch.int32) >> 23
    return ((e - 23).clamp(min=1) << 23).view(torch.float32).double()


def ema_update_error(ema_new, p_new, e_prev, w):
    """max over elements of |ema_new - (e_prev + w (p_new - e_prev))| / (2 ulp32(max(|p_new|, |e_prev|))), float64 on the device from
    the bits the device holds.  The bound is one rounding of the difference, scaled by w < 1, plus the one rounding of the fma."""
    exact = e_prev.double() + float(w) * (p_new.double() - e_prev.double())
    bound = 2 * ulp32_dev(torch.maximum(p_new.abs(), e_prev.abs()))
    return float(((ema_new.double() - exact).abs() / bound).max())


# ---- 1. the same AdamW bits as the entry points beside it ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["zero_grad", "keep_grad", "guarded"])
@pytest.mark.parametrize("n,offset", CASES, ids=IDS)
def test_same_adamw_bits_as_the_existing_entries(n, offset, mode):
    p0, grads = inputs(n)
    k = Kernels(p0, offset=offset, guarded=mode == "guarded")
    pr, gr, mr, vr = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    if mode == "guarded":
        rblock = torch.zeros(_native.GUARD_WORDS, dtype=torch.int32, device=DEV)
        rscratch = torch.empty(_native.GUARD_SCRATCH_FLOATS, device=DEV)
        _native.step_guard_init(rblock, 65536.0)
    for step, g in enumerate(grads, start=1):
        k.step(g, zero_grad=mode != "keep_grad")
        gr.copy_(g)
        if mode == "guarded":
            gr.mul_(rblock.view(torch.float32)[GW["scale"]])
            _native.grad_guard(gr, rblock, rscratch, 0.0, H["betas"][0], H["betas"][1], 2.0, 0.5, 2000)
            _native.adamw_step_guarded(pr, gr, mr, vr, H["lr"], H["betas"][0], H["betas"][1], H["eps"], H["weight_decay"], rblock)
        else:
            _native.adamw_step(pr, gr, mr, vr, H["lr"], H["betas"][0], H["betas"][1], H["eps"], H["weight_decay"], step, zero_grad=mode == "zero_grad")
        assert torch.equal(k.g, gr), step
        if mode == "keep_grad":
            assert torch.equal(k.g, g), step
        else:
            assert not k.g.any(), step
    assert torch.equal(k.p, pr) and torch.equal(k.m, mr) and torch.equal(k.v, vr)
    assert not torch.equal(k.p, p0) and k.padding_intact()
    if mode == "guarded":
        assert torch.equal(k.block, rblock) and int(k.word("good_steps")) == 3
    assert int(k.eword("updates")) == 3 and int(k.eword("apply")) == 1 and int(k.eword("first")) == 0


# ---- 2. the value of the average -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warmup", [False, True], ids=["const", "warmup"])
@pytest.mark.parametrize("decay", [0.999, 0.5])
@pytest.mark.parametrize("n,offset", CASES, ids=IDS)
def test_ema_value_per_update(n, offset, decay, warmup):
    p0, grads = inputs(n, seed=5)
    k = Kernels(p0, offset=offset, decay=decay, warmup=warmup)
    updates, weights = ema_ref.schedule(decay, warmup, [True] * len(grads))        # the closed form's counts and weights
    for u, g in enumerate(grads):
        e_prev = k.ema.clone()
        k.step(g)
        w = weights[u]
        assert int(k.eword("updates")) == updates[u] == u + 1 and int(k.eword("first")) == int(u == 0) and int(k.eword("apply")) == 1
        assert np.float32(float(k.eword("weight"))) == w, (u, float(k.eword("weight")), w)
        if u == 0:
            assert torch.equal(k.ema, k.p)
        else:
            err = ema_update_error(k.ema, k.p, e_prev, w)
            print(f"n={n} decay={decay} warmup={warmup} update {u}: worst error {err:.3f} of the 2-ulp bound")
            assert err <= 1.0, u
            assert not torch.equal(k.ema, k.p)
    assert k.padding_intact()


# ---- 3. a skipped step -----------------------------------------------------------------------------------------------------------
def _guarded_script(decay=0.9, warmup=True):
    n = 10007
    p0, grads = guard_ref.script(n)
    k = Kernels(p0, decay=decay, warmup=warmup, guarded=True, growth_interval=3)
    p_seq, applied, emas = [], [], []
    updates = 0
    for it, g in enumerate(grads, start=1):
        snap = (k.p.clone(), k.m.clone(), k.v.clone(), k.ema.clone())
        k.step(g, max_grad_norm=0.5)
        ok = bool(int(k.word("apply")))
        assert int(k.eword("apply")) == int(ok)
        if it in (3, 7):
            assert not ok
            assert all(torch.equal(a, b) for a, b in zip((k.p, k.m, k.v, k.ema), snap)), it
            assert int(k.eword("updates")) == updates, it
        else:
            assert ok and not torch.equal(k.p, snap[0]) and not torch.equal(k.ema, snap[3])
            updates += 1
            assert int(k.eword("updates")) == updates, it
        assert not k.g.any(), it
        p_seq.append(k.p.cpu().numpy()); applied.append(ok); emas.append(k.ema.clone())
    return k, p_seq, applied, emas


def test_a_skipped_step_moves_neither_the_average_nor_its_count():
    decay, warmup = 0.9, True
    k, p_seq, applied, emas = _guarded_script(decay, warmup)
    assert applied == [True, True, False, True, True, True, False, True, True, True]
    ref = ema_ref.closed_form(p_seq, decay, warmup, applied=applied)
    assert int(k.eword("updates")) == ref["updates"][-1] == 8 and int(k.word("good_steps")) == 8 and int(k.word("skipped_steps")) == 2
    assert np.float32(float(k.eword("weight"))) == ref["weights"][-1] == ema_ref.weight(decay, warmup, 7)
    # the whole trajectory against float64: every update after the copy adds at most 2 ulp32 of the largest value (test 2's bound),
    # and later updates only shrink earlier errors (factor 1 - w)
    for it, (e, r) in enumerate(zip(emas, ref["ema"])):
        err = float(np.abs(e.cpu().numpy().astype(np.float64) - r).max())
        bound = 2 * ema_ref.ulp32(np.abs(r).max()) * max(ref["updates"][it] - 1, 0)
        assert err <= bound, (it, err, bound)
    k2, _, applied2, emas2 = _guarded_script(decay, warmup)
    assert applied2 == applied and all(torch.equal(a, b) for a, b in zip(emas, emas2))
    assert torch.equal(k.p, k2.p) and torch.equal(k.m, k2.m) and torch.equal(k.v, k2.v) and torch.equal(k.ema_block, k2.ema_block)


# ---- 4. error paths ----------------------------------------------------------------------------------------------------------------
def test_error_paths():
    lib = _native.load_library()
    k = Kernels(np.zeros(16, dtype=np.float32), guarded=True)
    stream = _native.current_stream(torch.device(DEV))
    p, g, m, v, e, b, s = (t.data_ptr() for t in (k.p, k.g, k.m, k.v, k.ema, k.block, k.ema_block))
    einval = 1
    assert lib.ccn_ema_init(None, 0, stream) == einval
    assert lib.ccn_ema_init(s, -1, stream) == einval
    hyper = (3e-4, 0.9, 0.99, 1e-8, 0.05)

    def call(bufs=(p, g, m, v, e), n=16, step=1, zero=1, decay=0.9, guard=None, state=s):
        return lib.ccn_adamw_step_ema(*bufs, n, *hyper, step, zero, decay, 0, guard, state, stream)

    for i in range(5):
        bufs = [p, g, m, v, e]; bufs[i] = None
        assert call(bufs=tuple(bufs)) == einval, i
    assert call(state=None) == einval
    assert call(n=-1) == einval
    for bad in (1.0, 1.5, -0.1, float("nan")):
        assert call(decay=bad) == einval, bad
        assert b"ema_decay" in lib.ccn_last_error()
    assert call(zero=0, guard=b) == einval and b"zero_grad" in lib.ccn_last_error()
    assert call(step=0) == einval
    torch.cuda.synchronize()
    assert int(k.eword("updates")) == 0 and not k.p.any() and bool((k.ema == -3.0).all())          # none of them launched anything
    assert call(n=0) == 0 and call(decay=0.0) == 0
    torch.cuda.synchronize()
    assert int(k.eword("updates")) == 1
    args = (H["lr"], *H["betas"], H["eps"], H["weight_decay"], 1, 0.9)
    with pytest.raises(ValueError, match="ema"):
        _native.adamw_step_ema(k.p, k.g, k.m, k.v, k.ema.double(), *args, k.ema_block)
    with pytest.raises(ValueError, match="ema"):
        _native.adamw_step_ema(k.p, k.g, k.m, k.v, k.ema.cpu(), *args, k.ema_block)
    with pytest.raises(ValueError, match="ema"):
        _native.adamw_step_ema(k.p, k.g, k.m, k.v, k.ema[:8], *args, k.ema_block)
    with pytest.raises(ValueError, match="params"):
        _native.adamw_step_ema(k.base[0][::2][:16], k.g, k.m, k.v, k.ema, *args, k.ema_block)
    with pytest.raises(ValueError, match="EMA state block"):
        _native.adamw_step_ema(k.p, k.g, k.m, k.v, k.ema, *args, k.ema_block[:4])
    with pytest.raises(ValueError, match="EMA state block"):
        _native.adamw_step_ema(k.p, k.g, k.m, k.v, k.ema, *args, k.ema_block.cpu())
    with pytest.raises(ValueError, match="EMA state block"):
        _native.ema_init(k.ema_block.float())
    with pytest.raises(ValueError, match="guard block"):
        _native.adamw_step_ema(k.p, k.g, k.m, k.v, k.ema, *args, k.ema_block, zero_grad=True, guard_block=k.block[:8])
    with pytest.raises(ValueError, match="ema_decay"):
        _native.adamw_step_ema(k.p, k.g, k.m, k.v, k.ema, *args[:-1], 1.0, k.ema_block)
    sd = synth.synth_state_dict(synth.unet_param_spec(512, 32, (1, 2)))
    net = make_net(sd)
    with pytest.raises(ValueError, match="ema_decay"):
        FusedAdamW(net, ema_decay=1.0)
    x0, z, t, noise = (torch.from_numpy(GOLD[n]).to(DEV) for n in ("x0", "z", "t", "noise"))
    sch = NoiseScheduler(1000, "cosine", device=DEV)
    with pytest.raises(TypeError, match="torch.optim.swa_utils.AveragedModel"):
        train_step(net, sch, torch.optim.AdamW(net.parameters()), x0, z, t, noise, ema_decay=0.9)
    with pytest.raises(ValueError, match="ema_decay"):
        train_step(net, sch, FusedAdamW(net, ema_decay=0.5), x0, z, t, noise, ema_decay=0.9)
    plain = FusedAdamW(net)
    assert plain.ema is None and plain.ema_block is None
    for fn in (plain.ema_state_dict, plain.ema_weights, plain.ema_updates):
        with pytest.raises(RuntimeError, match="ema_decay"):
            fn()


# ---- 5 - 9. through the network ------------------------------------------------------------------------------------------------------
def make_net(sd, dtype="fp32"):
    net = CLIPCondUNet(z_dim=512, base=32, ch_mult=(1, 2), dtype=dtype).to(DEV)
    net.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    return net.train()


@pytest.fixture(scope="module")
def c1():
    sd = synth.synth_state_dict(synth.unet_param_spec(512, 32, (1, 2)))
    return dict(sd=sd, batch=tuple(torch.from_numpy(GOLD[k]) for k in ("x0", "z", "t", "noise")))


def setup(c1, dtype="fp32", **kw):
    net = make_net(c1["sd"], dtype)
    sch = NoiseScheduler(1000, "cosine", device=DEV)
    opt = FusedAdamW(net, lr=2e-4, **kw)
    return net, sch, opt, tuple(a.to(DEV) for a in c1["batch"])


def ema_word(opt, name):
    return opt.ema_block.view(torch.float32)[0] if name == "weight" else opt.ema_block[EW[name]]


@pytest.mark.parametrize("warmup", [False, True], ids=["const", "warmup"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_three_train_steps_keep_the_average(c1, dtype, warmup):
    decay = 0.9
    net, sch, opt, (x0, z, t, noise) = setup(c1, dtype, ema_decay=decay, ema_warmup=warmup)
    fp = net.train_state().fp
    assert torch.equal(opt.ema, fp.flat) and opt.ema.data_ptr() != fp.flat.data_ptr()
    for u in range(3):
        e_prev = opt.ema.clone()
        loss = float(train_step(net, sch, opt, x0, z, t, noise, ema_decay=decay))
        assert np.isfinite(loss)
        w = ema_ref.weight(decay, warmup, u)
        assert np.float32(float(ema_word(opt, "weight"))) == w and opt.ema_updates() == u + 1
        if u == 0:
            assert torch.equal(opt.ema, fp.flat)
        else:
            assert ema_update_error(opt.ema, fp.flat, e_prev, w) <= 1.0, u
            assert not torch.equal(opt.ema, fp.flat)
    assert opt.steps == 3 and fp.intact() and not fp.grad.any()


def test_a_poisoned_batch_leaves_the_average_alone(c1):
    net, sch, opt, (x0, z, t, noise) = setup(c1, "fp32", ema_decay=0.9)
    scaler = GradScaler()
    fp = net.train_state().fp
    assert np.isfinite(float(train_step(net, sch, opt, x0, z, t, noise, scaler=scaler)))
    assert np.isfinite(float(train_step(net, sch, opt, x0, z, t, noise, scaler=scaler)))
    snap = (fp.flat.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.ema.clone(), opt.ema_block.clone())
    assert opt.ema_updates() == 2
    bad = noise.clone(); bad[1, 2, 5, 7] = float("inf")
    assert not np.isfinite(float(train_step(net, sch, opt, x0, z, t, bad, scaler=scaler)))
    assert all(torch.equal(a, b) for a, b in zip((fp.flat, opt.exp_avg, opt.exp_avg_sq, opt.ema), snap))
    assert opt.ema_updates() == 2 and int(ema_word(opt, "apply")) == 0 and not fp.grad.any()
    assert int(scaler.stats()["skipped_steps"]) == 1 and int(scaler.stats()["good_steps"]) == 2
    assert np.isfinite(float(train_step(net, sch, opt, x0, z, t, noise, scaler=scaler)))
    assert opt.ema_updates() == 3 and int(ema_word(opt, "apply")) == 1
    assert not torch.equal(opt.ema, snap[3]) and not torch.equal(fp.flat, snap[0])
    assert ema_update_error(opt.ema, fp.flat, snap[3], ema_ref.weight(0.9, False, 2)) <= 1.0
    assert bool(torch.isfinite(opt.ema).all())


def test_the_averaged_weights_for_inference(c1):
    net, sch, opt, (x0, z, t, noise) = setup(c1, "fp32", ema_decay=0.5)
    for _ in range(3):
        train_step(net, sch, opt, x0, z, t, noise)
    fp = net.train_state().fp
    before = fp.flat.clone(); ema_before = opt.ema.clone()
    esd = opt.ema_state_dict()
    nsd = net.state_dict()
    assert list(esd) == list(nsd) and all(esd[k].shape == nsd[k].shape and esd[k].data_ptr() != nsd[k].data_ptr() for k in nsd)
    assert any(not torch.equal(esd[k], nsd[k]) for k in nsd)
    other = CLIPCondUNet.from_state_dict(esd).to(DEV).eval()
    with torch.no_grad():
        eps_other = other(x0, z, t)
        net.eval()
        eps_raw = net(x0, z, t).clone()
        with opt.ema_weights():
            net.eval()
            assert torch.equal(fp.flat, ema_before) and torch.equal(opt.ema, before)
            eps_ema = net(x0, z, t).clone()
            with pytest.raises(RuntimeError, match="ema_weights"):
                opt.step()
        assert torch.equal(net(x0, z, t), eps_raw)                     # back on the raw weights
    assert torch.equal(eps_ema, eps_other) and not torch.equal(eps_ema, eps_raw)
    assert torch.equal(fp.flat, before) and torch.equal(opt.ema, ema_before) and fp.intact()
    with pytest.raises(KeyError):                                      # swapped back on an exception as well
        with opt.ema_weights():
            raise KeyError("x")
    assert torch.equal(fp.flat, before) and torch.equal(opt.ema, ema_before)
    net.train()
    assert np.isfinite(float(train_step(net, sch, opt, x0, z, t, noise)))
    assert opt.ema_updates() == 4 and not torch.equal(fp.flat, before)


def _four_steps(c1, guarded, split):
    """Four opt.step() calls on gradients written straight into fp.grad (no backward: deterministic); ``split``: after two of them
    the state goes through state_dict() into a fresh net and optimiser (and scaler)."""
    kw = dict(ema_decay=0.9, ema_warmup=True)
    net, _, opt, _ = setup(c1, "fp32", **kw)
    scaler = GradScaler(growth_interval=3) if guarded else None
    gen = torch.Generator(DEV).manual_seed(21)
    n = opt.exp_avg.numel()
    # the flat buffers pad every tensor to a multiple of four floats; a backward leaves the padding's gradient at zero (so the padding
    # stays zero for good, and no checkpoint needs to carry it): the test's gradients do the same
    mask = torch.zeros(n, device=DEV)
    for _, off, cnt in net.train_state().fp.views:
        mask[off:off + cnt] = 1.0
    grads = [torch.randn(n, generator=gen, device=DEV) * 0.01 * mask for _ in range(4)]
    for i, g in enumerate(grads):
        if split and i == 2:
            osd, nsd = opt.state_dict(), {k: v.clone() for k, v in net.state_dict().items()}
            ssd = scaler.state_dict() if guarded else None
            assert osd["steps"] == 2 and osd["ema_updates"] == 2
            net = make_net(nsd)
            opt = FusedAdamW(net, lr=1.0, betas=(0.5, 0.5), eps=1.0, weight_decay=0.5, **kw)      # all of it comes from the state
            opt.load_state_dict(osd)
            if guarded:
                scaler = GradScaler()
                scaler.load_state_dict(ssd)
        fp = net.train_state().fp
        fp.grad.copy_(g)
        if guarded:
            fp.grad.mul_(scaler.scale_tensor(DEV))
            opt.step(zero_grad=True, guard=scaler)
        else:
            opt.step(zero_grad=True)
    return net, opt, scaler


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
def test_resume_from_state_dict_continues_bit_for_bit(c1, guarded):
    net_a, opt_a, sc_a = _four_steps(c1, guarded, split=False)
    net_b, opt_b, sc_b = _four_steps(c1, guarded, split=True)
    a, b = opt_a.state_dict(), opt_b.state_dict()
    assert torch.equal(net_a.train_state().fp.flat, net_b.train_state().fp.flat)
    for key in ("exp_avg", "exp_avg_sq", "ema"):
        assert torch.equal(a[key], b[key]), key
    assert a["steps"] == b["steps"] == 4 and a["ema_updates"] == b["ema_updates"] == 4
    assert (a["lr"], a["betas"], a["eps"], a["weight_decay"], a["ema_decay"], a["ema_warmup"]) == \
           (b["lr"], b["betas"], b["eps"], b["weight_decay"], b["ema_decay"], b["ema_warmup"])
    assert torch.equal(opt_a.ema_block, opt_b.ema_block)
    if guarded:
        assert sc_a.state_dict() == sc_b.state_dict() and sc_a.state_dict()["good_steps"] == 4 and sc_a.get_scale() == 131072.0


def test_mismatched_state_is_refused(c1):
    net, _, with_ema, _ = setup(c1, ema_decay=0.9)
    without = FusedAdamW(net)
    with pytest.raises(ValueError, match="built without ema_decay"):
        without.load_state_dict(with_ema.state_dict())
    with pytest.raises(ValueError, match="holds no EMA"):
        with_ema.load_state_dict(without.state_dict())
    sd = with_ema.state_dict()
    sd["exp_avg"] = sd["exp_avg"][:-1]
    with pytest.raises(ValueError, match="parameters"):
        with_ema.load_state_dict(sd)
    ptrs = (with_ema.exp_avg.data_ptr(), with_ema.exp_avg_sq.data_ptr(), with_ema.ema.data_ptr(), with_ema.ema_block.data_ptr())
    with_ema.load_state_dict(with_ema.state_dict())
    assert ptrs == (with_ema.exp_avg.data_ptr(), with_ema.exp_avg_sq.data_ptr(), with_ema.ema.data_ptr(), with_ema.ema_block.data_ptr())


def test_train_diffusion_writes_ema_checkpoints_and_resumes(tmp_path):
    from clip_feature_codec.io import bitstream
    from clip_feature_codec.train.diffusion_train import train_diffusion
    store = tmp_path / "store"
    synth.write_synth_store(store, 8, 32, write_clp=bitstream.write_bitstream)
    kw = dict(out_size=32, batch_size=4, lr=1e-3, device=DEV, base=32, ch_mult=(1, 2), dtype="bf16", num_workers=0, clip_w=0.0,
              grad_scaler=True, max_grad_norm=1.0, ema_decay=0.99)
    lines = []
    torch.manual_seed(0)
    ck = tmp_path / "ckpt"
    final = train_diffusion(store, epochs=2, save_dir=ck, log=lines.append, **kw)
    assert final == ck / "diffusion_unet_final.pt" and final.exists()
    assert [ln for ln in lines if "loss=" in ln][0].startswith("[train] epoch 1/2")
    for raw, ema in (("diffusion_unet_ep1.pt", "diffusion_unet_ep1_ema.pt"), ("diffusion_unet_ep2.pt", "diffusion_unet_ep2_ema.pt"),
                     ("diffusion_unet_final.pt", "diffusion_unet_final_ema.pt")):
        a = torch.load(ck / raw, map_location="cpu", weights_only=True); b = torch.load(ck / ema, map_location="cpu", weights_only=True)
        assert list(a) == list(b) and any(not torch.equal(a[k], b[k]) for k in a)
        CLIPCondUNet(z_dim=512, base=32, ch_mult=(1, 2)).load_state_dict(b, strict=True)
        assert all(bool(torch.isfinite(v).all()) for v in b.values())
    st = torch.load(ck / "train_state.pt", map_location="cpu", weights_only=True)
    assert st["epoch"] == 2 and st["opt"]["steps"] == 4 and st["opt"]["ema_updates"] == 4 and st["scaler"]["good_steps"] == 4
    assert not (ck / "train_state.pt.tmp").exists()
    # one epoch, then resume up to two
    ck2 = tmp_path / "ckpt2"
    torch.manual_seed(0)
    train_diffusion(store, epochs=1, save_dir=ck2, log=lambda s: None, **kw)
    assert torch.load(ck2 / "train_state.pt", map_location="cpu", weights_only=True)["opt"]["steps"] == 2
    lines2 = []
    final2 = train_diffusion(store, epochs=2, save_dir=ck2, log=lines2.append, resume=ck2 / "train_state.pt", **kw)
    assert lines2 and lines2[0].startswith("[train] epoch 2/2") and sum("loss=" in ln for ln in lines2) == 1, lines2
    st2 = torch.load(ck2 / "train_state.pt", map_location="cpu", weights_only=True)
    assert st2["epoch"] == 2 and st2["opt"]["steps"] == 4 and st2["opt"]["ema_updates"] == 4
    assert final2.exists() and (ck2 / "diffusion_unet_final_ema.pt").exists() and (ck2 / "diffusion_unet_ep2_ema.pt").exists()
    # another architecture is refused
    with pytest.raises(ValueError, match="architecture"):
        train_diffusion(store, epochs=2, save_dir=tmp_path / "ckpt3", log=lambda s: None, resume=ck2 / "train_state.pt",
                        **{**kw, "base": 64})
