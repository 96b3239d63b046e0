"""The training step of ``CLIPCondUNet`` on libccn_hip.so: epsilon-MSE, optionally with the reference's L1 and TV terms.

Reference: ``train/diffusion_train.py:119-124,137-140`` -- per batch::

    t = randint(0, T, (b,)); noise = randn_like(x0)
    x_t = sch.q_sample(x0, t, noise); eps_hat = net(x_t, z, t); loss = F.mse_loss(eps_hat, noise)
    loss.backward(); opt.step(); opt.zero_grad()

Here ``net(x_t, z, t)`` of a ``CLIPCondUNet`` in training mode returns an ``eps_hat`` that carries an autograd node
(``UNetFunction``) whose backward is the library's hand-written backward pass, so the three reference lines run
unchanged with any torch optimiser.  The parameters are re-homed as views into ONE flat fp32 buffer (what the C ABI
reads); ``FusedAdamW`` is the matching one-launch optimiser, and ``train_step`` is the loop body above with the
fused loss kernel.

The reference's default objective adds two terms on ``x0_pred = predict_x0_from_eps(x_t, t, eps_hat).clamp(-1, 1)`` (:125-128):
``recon_w * l1(x0_pred, x0) + tv_w * total_variation(x0_pred)``.  ``train_step(..., recon_w=, tv_w=)`` evaluates them and their
gradient in the same single pass as the MSE (``ccn_diffusion_loss_grad``), and ``train_diffusion`` runs its batches through it.
Still not provided: the CLIP-alignment term (``clip_w``, :129-136), which needs ``open_clip`` with downloaded weights
(SURVEY.md section 8, row a18).

The reference's ``scaler.scale(loss).backward(); scaler.step(opt); scaler.update()`` (:137-139) runs with this module's ``GradScaler``
and ``FusedAdamW``: the loss scale, the skipped step on a non-finite gradient, the scale update and (optionally) gradient-norm
clipping are decided on the device by one extra read of the flat gradient buffer (``ccn_grad_guard``), and the guarded AdamW
kernel only reads that decision -- no host sync.  ``train_step(..., scaler=, max_grad_norm=)`` and
``train_diffusion(..., grad_scaler=, max_grad_norm=)`` use it; everything is off by default.

``FusedAdamW(net, ema_decay=)`` also keeps an exponential moving average of the parameters -- the weights a diffusion decoder is
sampled from (``torch.optim.swa_utils.AveragedModel`` with ``get_ema_multi_avg_fn(decay)``).  The average is taken inside the AdamW
kernel, which reads the guard's decision on the device: a skipped step neither moves the average nor counts as an update.
``opt.ema_state_dict()`` is the checkpoint to evaluate, ``with opt.ema_weights():`` runs this model on the averaged weights, and
``opt.state_dict()`` / ``load_state_dict()`` with ``train_diffusion(resume=)`` continue a run that stopped.

With ``torch.distributed`` initialised, ``train_step(..., ddp=True)`` averages the flat gradient buffer over the ranks
with one all-reduce (RCCL over xGMI on a GPU node): the data-parallel step of BASELINE.json configs[4].
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from .. import _native


class FlatParams:
    """Flat fp32 homes of a module's parameters and gradients, in the trainer's layout."""

    def __init__(self, net: nn.Module, trainer: "_native.NativeTrainer") -> None:
        named = dict(net.named_parameters())
        keys = [k for k, _, _ in trainer.layout]
        if set(keys) != set(named):
            raise RuntimeError(f"parameter keys differ from the library's: {sorted(set(keys) ^ set(named))[:6]}")
        dev = trainer.device
        self.flat = torch.zeros(trainer.total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(trainer.total, dtype=torch.float32, device=dev)
        self.views: List[Tuple[nn.Parameter, int, int]] = []
        with torch.no_grad():
            for name, shape, off in trainer.layout:
                p = named[name]
                if tuple(p.shape) != tuple(shape):
                    raise RuntimeError(f"{name}: shape {tuple(p.shape)} != {tuple(shape)}")
                n = p.numel()
                view = self.flat[off:off + n].view(shape)
                view.copy_(p.detach().to(dev, torch.float32))
                p.data = view
                p.grad = self.grad[off:off + n].view(shape)
                self.views.append((p, off, n))

    def intact(self) -> bool:
        base = self.flat.data_ptr()
        return all(p.data_ptr() == base + 4 * off for p, off, _ in self.views)

    def params(self) -> List[nn.Parameter]:
        return [p for p, _, _ in self.views]

    def grads_bound(self) -> Optional[str]:
        """'views' if every ``p.grad`` is its view of the flat gradient buffer, 'none' if every one is None, else None (foreign)."""
        base = self.grad.data_ptr()
        n_none = sum(1 for p, _, _ in self.views if p.grad is None)
        if n_none == len(self.views):
            return "none"
        if n_none == 0 and all(p.grad.data_ptr() == base + 4 * off for p, off, _ in self.views):
            return "views"
        return None

    def rebind_grads(self) -> None:
        """Make every ``p.grad`` a view of the flat gradient buffer again (after ``zero_grad(set_to_none=True)``)."""
        for p, off, n in self.views:
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * off:
                p.grad = self.grad[off:off + n].view(p.shape)


class UNetFunction(torch.autograd.Function):
    """eps_hat = UNet(x_t, z, t) with the library's backward.  Inputs after ``t`` are the parameters (autograd leaves).

    The trainer keeps the activations of ONE forward (its workspace), so every forward takes a serial number and a backward whose
    serial is no longer the trainer's latest raises instead of differentiating the wrong activations (two forwards before one
    backward: micro-batches, teacher/student double calls).  When every ``p.grad`` is the parameter's view of the flat gradient
    buffer (or None), the library accumulates straight into that buffer and the node returns no parameter gradients -- no
    per-step 130 MB scratch, no second accumulation pass by autograd; otherwise (foreign ``p.grad`` tensors) it falls back to a
    scratch buffer that autograd accumulates."""

    @staticmethod
    def forward(ctx, state, x_t, z, t, *params):
        x = _native.require_dev(x_t, "x_t"); zz = _native.require_dev(z, "z_clip"); tt = _native.require_dev(t, "t", torch.int64)
        eps = state.trainer.forward(state.fp.flat, x, zz, tt)
        ctx.state = state
        ctx.save_for_backward(x, zz)
        ctx.version = state.fp.flat._version
        ctx.serial = state.trainer.serial
        return eps

    @staticmethod
    def backward(ctx, d_eps):
        state = ctx.state
        x, zz = ctx.saved_tensors
        if state.fp.flat._version != ctx.version:
            raise RuntimeError("parameters were modified between the training forward and its backward")
        if state.trainer.serial != ctx.serial:
            raise RuntimeError("another training forward of this model ran before this backward: the library keeps the activations "
                               "of one forward at a time (run forward -> backward pairs, e.g. one micro-batch after the other)")
        fp = state.fp
        d = _native.require_dev(d_eps, "d_eps")
        mode = fp.grads_bound()
        if mode is not None:
            if mode == "none":                     # after zero_grad(set_to_none=True): the buffer holds stale sums
                fp.grad.zero_()
            fp.rebind_grads()
            if state.ddp_bucketed and state.world() > 1:
                d = d * (1.0 / state.world())      # the sum over ranks is then already the mean
                # inside `with state.no_sync():` (all micro-batches but the last) the gradients only accumulate locally; the last
                # backward's bucket all-reduces then carry the whole accumulated sum -- torch DDP's no_sync semantics.  Without
                # it every backward would re-reduce the already averaged earlier micro-batches (x world).
                state.trainer.backward(fp.flat, fp.grad, x, zz, d, bucket_cb=state.enqueue_bucket if state.sync_grads else None)
            else:
                state.trainer.backward(fp.flat, fp.grad, x, zz, d)
            return (None,) * (4 + len(fp.views))
        # foreign .grad tensors (not views of the flat gradient buffer): the gradients go back through autograd.  Under data
        # parallelism they must still be averaged -- one blocking all-reduce of THIS backward's gradient here (also inside no_sync():
        # what autograd accumulates into foreign .grad tensors afterwards is out of the library's reach), never a silent per-rank one.
        g = torch.zeros_like(fp.flat)
        state.trainer.backward(fp.flat, g, x, zz, d)
        if state.ddp_bucketed and state.world() > 1:
            average_gradients(g)
        grads = tuple(g[off:off + n].view(p.shape) for p, off, n in fp.views)
        return (None, None, None, None) + grads


class TrainState:
    """Trainer handle + flat parameter homes of one CLIPCondUNet (created on its first training forward)."""

    def __init__(self, net: nn.Module, dtype: str, device) -> None:
        a = net.arch
        self.trainer = _native.NativeTrainer(a["z_dim"], a["base"], a["ch_mult"], a["time_dim"], a["img_ch"], groups=8,
                                             dtype=dtype, device=device)
        self.fp = FlatParams(net, self.trainer)
        self.dtype = dtype
        self.ddp_bucketed = False          # UNetFunction.backward all-reduces finished gradient ranges while it still runs
        self.sync_grads = True             # False inside no_sync(): gradient accumulation over micro-batches without communication
        # (4,) total, mse, l1, tv (l1, tv unweighted) of the last train_step with recon_w / tv_w: a view of a static buffer, read it
        # before the next step; None after an MSE-only step
        self.last_loss_terms: Optional[torch.Tensor] = None
        self._works: list = []

    def no_sync(self):
        """Context manager for gradient accumulation under data parallelism (torch DDP's ``no_sync``): backward passes inside it
        only accumulate into the local gradient buffer; run the LAST micro-batch's backward outside it, then ``wait_grad_sync()``."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            prev, self.sync_grads = self.sync_grads, False
            try:
                yield
            finally:
                self.sync_grads = prev
        return ctx()

    @staticmethod
    def world() -> int:
        import torch.distributed as dist
        return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1

    def enqueue_bucket(self, lo: int, hi: int) -> None:
        import torch.distributed as dist
        self._works.append(dist.all_reduce(self.fp.grad[lo:hi], async_op=True))

    def wait_grad_sync(self) -> None:
        """Join the bucket all-reduces the last backward enqueued (call before the optimiser step)."""
        for w in self._works:
            w.wait()
        self._works.clear()

    def apply(self, x_t, z, t):
        return UNetFunction.apply(self, x_t, z, t, *self.fp.params())

    def static_buffers(self, x0: torch.Tensor, z: torch.Tensor) -> dict:
        """Fixed-address tensors of the fused step for this batch shape (what lets the library replay captured graphs)."""
        key = (tuple(x0.shape), tuple(z.shape))
        bufs = getattr(self, "_static", None)
        if bufs is None or bufs["key"] != key:
            dev = x0.device
            bufs = dict(key=key, x_t=torch.empty_like(x0), eps=torch.empty_like(x0), d_eps=torch.empty_like(x0), noise=torch.empty_like(x0),
                        x0=torch.empty_like(x0), z=torch.empty_like(z), t=torch.empty(x0.shape[0], dtype=torch.int64, device=dev),
                        loss=torch.empty((), dtype=torch.float32, device=dev), scratch=torch.empty(1024, dtype=torch.float32, device=dev))
            self._static = bufs
        return bufs

    def objective_buffers(self, sb: dict) -> dict:
        """What the L1 / TV objective adds to ``static_buffers``: the gathered schedule coefficients, the four loss terms and the
        reduction scratch, at fixed addresses like the rest."""
        if "terms" not in sb:
            dev, b = sb["x0"].device, sb["x0"].shape[0]
            sb.update(a=torch.empty(b, dtype=torch.float32, device=dev), s=torch.empty(b, dtype=torch.float32, device=dev),
                      terms=torch.zeros(4, dtype=torch.float32, device=dev),
                      scratch_obj=torch.empty(_native.OBJECTIVE_SCRATCH_FLOATS, dtype=torch.float32, device=dev))
        return sb


class FusedAdamW:
    """``torch.optim.AdamW`` semantics over the flat buffers, one kernel launch per step (train/diffusion_train.py:105,138).

    ``ema_decay`` (0 <= decay < 1): the same pass also keeps ``self.ema``, the exponential moving average of the parameters that
    ``AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(ema_decay))`` with ``update_parameters`` after every applied step would
    hold: the first update copies the parameters, later ones are ``ema.lerp_(p, 1 - decay)``.  ``ema_warmup``: the decay of update
    ``u`` (from 0) is ``min(ema_decay, (1 + u) / (10 + u))``.  The count of updates lives in ``self.ema_block`` on the device and
    does not advance on a skipped step.  Without ``ema_decay`` nothing is allocated and every step is what it was."""

    def __init__(self, net, lr: float = 2e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 ema_decay: Optional[float] = None, ema_warmup: bool = False) -> None:
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), not {ema_decay}")
        self.net = net
        self.state: TrainState = net.train_state()
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        fp = self.state.fp
        self.exp_avg = torch.zeros_like(fp.flat)
        self.exp_avg_sq = torch.zeros_like(fp.flat)
        self.steps = 0
        self._guard: Optional["GradScaler"] = None      # the guard of the last guarded step: its block holds the step count from then on
        self._clip_guard: Optional["GradScaler"] = None
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.ema: Optional[torch.Tensor] = None
        self.ema_block: Optional[torch.Tensor] = None
        self._ema_swapped = False
        if self.ema_decay is not None:
            self.ema = fp.flat.detach().clone()
            self.ema_block = torch.zeros(_native.EMA_WORDS, dtype=torch.int32, device=fp.flat.device)
            _native.ema_init(self.ema_block, 0)

    def clip_guard(self) -> "GradScaler":
        """The internal guard of ``max_grad_norm`` without a scaler: scale 1, never grows, never backs off."""
        if self._clip_guard is None:
            self._clip_guard = GradScaler(init_scale=1.0, growth_factor=1.0, backoff_factor=1.0, growth_interval=2 ** 31 - 1)
        return self._clip_guard

    def step(self, zero_grad: bool = False, guard: Optional["GradScaler"] = None, max_grad_norm: Optional[float] = None) -> None:
        """``zero_grad=True``: ``step()`` + ``zero_grad()`` as one pass over the buffers (``ccn_adamw_step_zero_grad``).

        ``guard`` (a ``GradScaler``) and / or ``max_grad_norm`` > 0: the guarded step (train/diffusion_train.py:138-139).  The
        gradient buffer holds ``d (scale * loss)``; ``ccn_grad_guard`` reads it once and decides on the device whether the step is
        applied, then ``ccn_adamw_step_guarded`` applies ``g / scale * clip_coef`` or leaves parameters and moments untouched.  A
        guarded step always consumes the gradients and leaves the buffer at zero.  AdamW's step count then lives in the guard's
        control block (it advances on applied steps only); the first guarded step seeds it with the larger of ``self.steps`` and the
        count the guard already holds (a ``GradScaler`` restored with ``load_state_dict`` resumes its run's count), and an unguarded
        ``step()`` afterwards raises, because the host-side count would be wrong."""
        fp = self.state.fp
        if self._ema_swapped:
            raise RuntimeError("step() inside `with opt.ema_weights():` -- the flat buffer holds the averaged weights there, leave the "
                               "context before training on")
        if guard is not None and not guard.enabled:
            guard = None
        if guard is None and max_grad_norm is not None and max_grad_norm > 0:
            guard = self.clip_guard()
        if guard is not None:
            block = guard.block(fp.flat.device)
            if self._guard is not guard:             # seed the count of applied steps, on the device
                word = block[_native.GUARD_WORD["good_steps"]]
                if self._guard is None:
                    # the larger of this optimiser's count and the block's: a GradScaler restored with load_state_dict carries the
                    # count of a resumed run (FusedAdamW has no state_dict of its own), a fresh one holds 0
                    word.clamp_(min=self.steps)
                else:
                    word.copy_(self._guard.block(fp.flat.device)[_native.GUARD_WORD["good_steps"]])
                self._guard = guard
            _native.grad_guard(fp.grad, block, guard.scratch, max_grad_norm if max_grad_norm is not None else 0.0, self.betas[0],
                               self.betas[1], guard.growth_factor, guard.backoff_factor, guard.growth_interval)
            step, zero_grad = 0, True                # the count is the block's; a guarded step consumes the gradients
        elif self._guard is not None:
            raise RuntimeError("an unguarded step() after a guarded one: the count of applied steps lives in the guard's control block "
                               "(skipped steps do not advance it), keep passing guard= / max_grad_norm=")
        else:
            block = None
            self.steps += 1
            step = self.steps
        bufs = (fp.flat, fp.grad, self.exp_avg, self.exp_avg_sq)
        hyper = (self.lr, self.betas[0], self.betas[1], self.eps, self.weight_decay)
        if self.ema is not None:
            _native.adamw_step_ema(*bufs, self.ema, *hyper, step, self.ema_decay, self.ema_block, zero_grad=zero_grad,
                                   ema_warmup=self.ema_warmup, guard_block=block)
        elif block is not None:
            _native.adamw_step_guarded(*bufs, *hyper, block)
        else:
            _native.adamw_step(*bufs, *hyper, step, zero_grad=zero_grad)
        fp.flat[:1].add_(0)    # the kernel wrote behind torch's back: bump the (shared) version counter so that a stale forward is detected
        if zero_grad:
            fp.rebind_grads()

    def zero_grad(self, set_to_none: bool = False) -> None:
        self.state.fp.grad.zero_()
        self.state.fp.rebind_grads()

    # ---- the averaged weights ------------------------------------------------------------------------------------------------
    def _need_ema(self) -> None:
        if self.ema is None:
            raise RuntimeError("this FusedAdamW keeps no EMA: construct it with ema_decay=")

    def ema_updates(self) -> int:
        """EMA updates done so far (AveragedModel's ``n_averaged``) -- a host read (synchronises)."""
        self._need_ema()
        return int(self.ema_block[_native.EMA_WORD["updates"]])

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """``net.state_dict()`` with the averaged parameters: same keys, shapes and order, values cloned from ``self.ema`` -- the
        checkpoint to sample from (loads with ``CLIPCondUNet.from_state_dict``, ``cli.eval``, ``cli.reconstruct_diffusion``)."""
        self._need_ema()
        if self._ema_swapped:
            raise RuntimeError("ema_state_dict() inside `with opt.ema_weights():` -- the buffers are swapped there")
        where = {name: (off, shape) for name, shape, off in self.state.trainer.layout}
        out = {}
        for key, val in self.net.state_dict().items():
            if key in where:
                off, shape = where[key]
                out[key] = self.ema[off:off + val.numel()].view(tuple(shape)).clone()
            else:
                out[key] = val.detach().clone()
        return out

    def _swap_ema(self) -> None:
        """Exchange the contents of the flat parameter buffer and ``self.ema`` through a 4 MiB chunk (no second full-size buffer).
        The copies into ``flat`` bump its version counter: ``net.native()`` re-commits its weights from what the buffer then holds."""
        flat, ema = self.state.fp.flat, self.ema
        n = flat.numel()
        chunk = min(n, 1 << 20)
        tmp = torch.empty(chunk, dtype=torch.float32, device=flat.device)
        with torch.no_grad():
            for lo in range(0, n, chunk):
                a, b = flat[lo:lo + chunk], ema[lo:lo + chunk]
                t = tmp[:a.numel()]
                t.copy_(a); a.copy_(b); b.copy_(t)

    def ema_weights(self):
        """Context manager: inside it the model's parameters ARE the averaged weights (``net.eval()`` and the samplers see them);
        the raw iterate is parked in ``self.ema`` and swapped back on exit, also on an exception.  ``step()`` inside it raises."""
        import contextlib
        self._need_ema()

        @contextlib.contextmanager
        def ctx():
            if self._ema_swapped:
                raise RuntimeError("ema_weights() is not re-entrant")
            self._swap_ema()
            self._ema_swapped = True
            try:
                yield self.net
            finally:
                self._swap_ema()
                self._ema_swapped = False
        return ctx()

    # ---- resumable state --------------------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """Everything a resumed run needs: hyper-parameters, the count of applied steps (the guard block's when a guard owns it),
        both moments and, with an EMA, the average and its count of updates.  Host reads (synchronises); tensors are clones."""
        if self._ema_swapped:
            raise RuntimeError("state_dict() inside `with opt.ema_weights():` -- the buffers are swapped there")
        steps = self.steps
        if self._guard is not None:
            steps = int(self._guard.block(self.exp_avg.device)[_native.GUARD_WORD["good_steps"]])
        sd = dict(lr=self.lr, betas=tuple(self.betas), eps=self.eps, weight_decay=self.weight_decay, steps=int(steps),
                  exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone())
        if self.ema is not None:
            sd.update(ema=self.ema.clone(), ema_updates=self.ema_updates(), ema_decay=self.ema_decay, ema_warmup=self.ema_warmup)
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """Copies into the existing buffers (their addresses stay), re-initialises the EMA block and sets the step count; a guarded
        step afterwards seeds the guard's count with it (``step``'s seeding rule)."""
        if self._ema_swapped:
            raise RuntimeError("load_state_dict() inside `with opt.ema_weights():`")
        n = self.exp_avg.numel()
        for key in ("exp_avg", "exp_avg_sq") + (("ema",) if "ema" in sd else ()):
            if tuple(sd[key].shape) != (n,):
                raise ValueError(f"{key} has {tuple(sd[key].shape)} elements, this optimiser's model has {n} parameters")
        if "ema" in sd and self.ema is None:
            raise ValueError("the state holds an EMA but this FusedAdamW was built without ema_decay=")
        if "ema" not in sd and self.ema is not None:
            raise ValueError("this FusedAdamW was built with ema_decay= but the state holds no EMA")
        self.lr, self.betas, self.eps, self.weight_decay = sd["lr"], tuple(sd["betas"]), sd["eps"], sd["weight_decay"]
        self.exp_avg.copy_(sd["exp_avg"]); self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        if self.ema is not None:
            self.ema.copy_(sd["ema"])
            self.ema_decay, self.ema_warmup = float(sd["ema_decay"]), bool(sd["ema_warmup"])
            _native.ema_init(self.ema_block, int(sd["ema_updates"]))
        self.steps = int(sd["steps"])
        self._guard = None


class GradScaler:
    """``torch.amp.GradScaler`` for ``FusedAdamW`` (train/diffusion_train.py:106,137-139), with its state in device memory.

    ``scaler.scale(loss).backward(); scaler.step(opt); scaler.update()`` run unchanged.  ``step`` launches ``ccn_grad_guard`` (one read
    of the flat gradient buffer: any non-finite element skips the step and multiplies the scale by ``backoff_factor``; after
    ``growth_interval`` applied steps in a row the scale is multiplied by ``growth_factor``) and the guarded AdamW kernel; the host
    never learns the decision, so nothing synchronises.  ``update()`` is a no-op: the guard kernel has already updated the scale.
    ``step(opt, max_grad_norm=)`` also clips the unscaled gradient's L2 norm, as ``unscale_`` + ``clip_grad_norm_`` would.  The
    gradients stay scaled in the buffer until the step consumes and zeroes them; read the unscaled norm from ``stats()``.
    ``get_scale()``, ``state_dict()`` are host reads (they synchronise)."""

    def __init__(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5, growth_interval: int = 2000,
                 enabled: bool = True) -> None:
        if not (init_scale > 0 and growth_factor > 0 and backoff_factor > 0 and growth_interval >= 1):
            raise ValueError("init_scale, growth_factor, backoff_factor must be positive and growth_interval at least 1")
        self.growth_factor, self.backoff_factor, self.growth_interval, self.enabled = float(growth_factor), float(backoff_factor), int(growth_interval), bool(enabled)
        self._init = dict(scale=float(init_scale), _growth_tracker=0, good_steps=0, skipped_steps=0)
        self._block: Optional[torch.Tensor] = None
        self.scratch: Optional[torch.Tensor] = None

    def block(self, device) -> torch.Tensor:
        """The control block (``ccn_step_guard_t``) as 16 int32 words on ``device``; created and initialised on first use."""
        if self._block is None:
            device = torch.device(device)
            if device.type != "cuda":
                raise RuntimeError(f"the step guard lives on a HIP device, not on {device}")
            self._block = torch.zeros(_native.GUARD_WORDS, dtype=torch.int32, device=device)
            self.scratch = torch.empty(_native.GUARD_SCRATCH_FLOATS, dtype=torch.float32, device=device)
            i = self._init
            _native.step_guard_init(self._block, i["scale"], i["_growth_tracker"], i["good_steps"], i["skipped_steps"])
        elif self._block.device != torch.device(device):
            raise RuntimeError(f"this GradScaler lives on {self._block.device}, not on {device}")
        return self._block

    def _word(self, name: str, device=None) -> torch.Tensor:
        blk = self.block(device if device is not None else self._block.device)
        k = _native.GUARD_WORD[name]
        return (blk.view(torch.float32) if k < 6 else blk)[k]

    def scale_tensor(self, device) -> torch.Tensor:
        """The device-resident loss scale, a 0-dim fp32 view of the control block."""
        return self._word("scale", device)

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        return loss * self.scale_tensor(loss.device) if self.enabled else loss

    def step(self, opt, max_grad_norm: Optional[float] = None) -> None:
        if not isinstance(opt, FusedAdamW):
            raise TypeError(f"this GradScaler drives FusedAdamW (the flat-buffer optimiser), not {type(opt).__name__}: "
                            "use torch.amp.GradScaler with a torch.optim optimiser")
        opt.state.wait_grad_sync()                  # the guard must see the all-reduced gradients
        opt.step(zero_grad=True, guard=self, max_grad_norm=max_grad_norm)

    def update(self) -> None:
        """No-op: ``ccn_grad_guard`` updated the scale and the growth tracker when it took the decision."""

    def stats(self) -> Dict[str, torch.Tensor]:
        """0-dim views of the control block, no sync: the last step's unscaled ``grad_norm`` and ``applied`` (0 / 1), the current
        ``scale`` and the counts of applied (``good_steps``) and ``skipped_steps``."""
        if self._block is None:
            raise RuntimeError("no step has run yet")
        return dict(grad_norm=self._word("grad_norm"), applied=self._word("apply"), scale=self._word("scale"),
                    good_steps=self._word("good_steps"), skipped_steps=self._word("skipped_steps"))

    def get_scale(self) -> float:
        """The current scale -- a host read (synchronises)."""
        if not self.enabled:
            return 1.0
        return float(self._word("scale")) if self._block is not None else self._init["scale"]

    def state_dict(self) -> dict:
        """torch's keys plus the counts of applied / skipped steps -- a host read (synchronises)."""
        if self._block is None:
            st = dict(self._init)
        else:
            w = self._block.tolist()                # the one host read; the scale's bits are decoded on the host
            st = dict(scale=torch.tensor(w[_native.GUARD_WORD["scale"]], dtype=torch.int32).view(torch.float32).item(),
                      _growth_tracker=w[_native.GUARD_WORD["growth_tracker"]], good_steps=w[_native.GUARD_WORD["good_steps"]],
                      skipped_steps=w[_native.GUARD_WORD["skipped_steps"]])
        st.update(growth_factor=self.growth_factor, backoff_factor=self.backoff_factor, growth_interval=self.growth_interval)
        return st

    def load_state_dict(self, sd: dict) -> None:
        self.growth_factor = float(sd.get("growth_factor", self.growth_factor))
        self.backoff_factor = float(sd.get("backoff_factor", self.backoff_factor))
        self.growth_interval = int(sd.get("growth_interval", self.growth_interval))
        self._init = dict(scale=float(sd["scale"]), _growth_tracker=int(sd.get("_growth_tracker", 0)), good_steps=int(sd.get("good_steps", 0)),
                          skipped_steps=int(sd.get("skipped_steps", 0)))
        if self._block is not None:
            i = self._init
            _native.step_guard_init(self._block, i["scale"], i["_growth_tracker"], i["good_steps"], i["skipped_steps"])


def average_gradients(flat_grad: torch.Tensor) -> torch.Tensor:
    """Data-parallel gradient of the global batch: ONE all-reduce of the flat buffer (RCCL over xGMI on a GPU node, gloo in the
    CPU tests), then divide by the world size -- what DistributedDataParallel does bucket by bucket."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(flat_grad)
        flat_grad.div_(dist.get_world_size())
    return flat_grad


def z_dropout(z: torch.Tensor, p: float, generator: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Embedding dropout, the training half of classifier-free guidance: every row of ``z`` (B, ...) is replaced by zeros with
    probability ``p`` -- the null embedding ``DDIMSampler(guided=True)`` samples the unconditional branch with.  Returns
    ``(z_dropped, keep_mask)``, ``keep_mask`` a (B,) bool tensor on ``z``'s device.  One ``torch.rand(B)`` draw on that device, from
    its default generator unless ``generator`` is given; ``p == 0`` draws nothing and returns ``z`` itself.  Any device."""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"the dropout probability must be in [0, 1], not {p}")
    b = z.shape[0]
    if p == 0.0:
        return z, torch.ones(b, dtype=torch.bool, device=z.device)
    keep = torch.rand(b, device=z.device, generator=generator) >= p        # rand is in [0, 1): p = 1 drops every row
    return torch.where(keep.view((b,) + (1,) * (z.dim() - 1)), z, torch.zeros((), dtype=z.dtype, device=z.device)), keep


def train_step(net, sch, opt, x0: torch.Tensor, z: torch.Tensor, t: Optional[torch.Tensor] = None,
               noise: Optional[torch.Tensor] = None, ddp=False, graph: bool = False, recon_w: float = 0.0,
               tv_w: float = 0.0, scaler: Optional[GradScaler] = None, max_grad_norm: Optional[float] = None,
               ema_decay: Optional[float] = None, z_drop: float = 0.0, prediction: str = "eps") -> torch.Tensor:
    """One optimisation step; returns the (detached) loss.  ``t`` / ``noise`` default to the reference's draws.

    ``prediction="v"`` (default ``"eps"``, the reference's; anything else is a ``ValueError``): the network is trained to predict
    ``v = a noise - s x0`` (``NoiseScheduler.v_target``).  The loss and its gradient always come from ``ccn_diffusion_loss_grad_v``:
    ``mse(v_hat, v) + recon_w * l1(x0_pred, x0) + tv_w * TV(x0_pred)`` with ``x0_pred = clamp(a x_t - s v_hat, -1, 1)``, whose
    auxiliary gradient carries the factor ``s <= 1`` where the eps form has ``s/a`` (up to 6.4e4 on the cosine schedule); with both
    weights 0 it is the v-MSE step.  ``q_sample``, forward, backward, buckets, guard, EMA and ``z_drop`` are the same, and
    ``last_loss_terms`` is always filled (l1 and tv read 0 when their weights are 0).Sample such weights with ``DDIMSampler(..., prediction="v")``.
    A zero-terminal-SNR scheduler (``NoiseScheduler(rescale_zero_snr=True)``) needs ``prediction="v"`` -- at ``t = T-1`` the target is
    then ``-x0`` and ``x0_pred = -v_hat``, no division -- and is refused with ``"eps"``, whose ``x0_pred`` divides by ``a_t = 0``.

    ``z_drop`` (usually 0.1): ``z_dropout`` zeroes whole rows of ``z`` with that probability before the copy into the static buffer,
    which trains the unconditional branch that guided sampling needs.  Under data parallelism each rank draws its own mask.  With 0
    (the default) nothing is drawn and the step is what it was, launch for launch.

    The weight EMA belongs to the optimiser (``FusedAdamW(net, ema_decay=)``) and needs no argument here; ``ema_decay`` is only
    checked: a ``TypeError`` with any other optimiser, a ``ValueError`` if it is not the optimiser's own.

    ``recon_w`` / ``tv_w`` (the reference's ``train_diffusion`` defaults are 0.05 and 1e-4): the loss becomes
    ``mse + recon_w * l1(x0_pred, x0) + tv_w * total_variation(x0_pred)`` with ``x0_pred = predict_x0_from_eps(...).clamp(-1, 1)``
    (train/diffusion_train.py:124-128), evaluated with its gradient by one kernel on the static buffers; the four terms are then
    in ``net.train_state().last_loss_terms``.  With both 0 (the default) the step is the epsilon-MSE step, launch for launch.

    ``scaler`` (this module's ``GradScaler``; the reference trains with one, train/diffusion_train.py:106,137-139) and / or
    ``max_grad_norm`` > 0, with a ``FusedAdamW``: ``d_eps`` is multiplied by the device-resident loss scale before the backward, and
    after the gradient all-reduces the step runs guarded -- skipped (parameters and moments untouched, scale halved) when any
    gradient element is non-finite, the unscaled gradient clipped to ``max_grad_norm`` otherwise.  Under data parallelism no extra
    collective is needed: a non-finite element survives the all-reduce on every rank, so all ranks decide alike.  The returned
    loss is the unscaled one.  With ``scaler=None`` (or a disabled one) and no ``max_grad_norm`` the step is what it was, launch
    for launch.

    All tensors the library touches live at fixed addresses (``TrainState.static_buffers``), so with ``graph=True`` the forward and
    the backward are replayed as captured hipGraphs after the first step of a shape -- measured SLOWER than plain stream launches
    for this step (7.98 vs 7.33 ms; 7.53 without the side-stream branch), hence off by default.  The returned loss is a view of a
    static buffer: read it before the next step."""
    v_pred = _native.prediction_code(prediction) == _native.PRED_V
    check_zero_snr_prediction(getattr(sch, "rescale_zero_snr", False), prediction)
    state: TrainState = net.train_state()
    fp = state.fp
    fp.rebind_grads()
    if ema_decay is not None:
        if not isinstance(opt, FusedAdamW):
            raise TypeError(f"ema_decay= needs a FusedAdamW(net, ema_decay=), not {type(opt).__name__}: average a torch.optim optimiser's "
                            "weights with torch.optim.swa_utils.AveragedModel")
        if opt.ema_decay != float(ema_decay):
            raise ValueError(f"ema_decay={ema_decay} but the optimiser was built with ema_decay={opt.ema_decay}")
    guard = scaler if scaler is not None and scaler.enabled else None
    clip = max_grad_norm is not None and max_grad_norm > 0
    if (guard is not None or clip) and not isinstance(opt, FusedAdamW):
        raise TypeError("scaler= / max_grad_norm= need a FusedAdamW: drive a torch.optim optimiser with torch.amp.GradScaler")
    if not 0.0 <= z_drop <= 1.0:
        raise ValueError(f"z_drop must be in [0, 1], not {z_drop}")
    z_dev = _native.require_dev(z, "z")
    if z_drop > 0:
        z = z_dev = z_dropout(z_dev, z_drop)[0]
    sb = state.static_buffers(_native.require_dev(x0, "x0"), z_dev)
    sb["x0"].copy_(x0); sb["z"].copy_(z)
    if t is None:
        sb["t"].random_(0, sch.timesteps)
    else:
        sb["t"].copy_(t)
    if noise is None:
        sb["noise"].normal_()
    else:
        sb["noise"].copy_(noise)
    state.trainer.set_graph(graph)
    if recon_w < 0 or tv_w < 0:
        raise ValueError("recon_w and tv_w must be non-negative")
    if recon_w > 0 or tv_w > 0 or v_pred:
        state.objective_buffers(sb)
        dev = sb["x0"].device
        torch.index_select(sch.sqrt_alphas_cumprod.to(dev), 0, sb["t"], out=sb["a"])
        torch.index_select(sch.sqrt_one_minus_alphas_cumprod.to(dev), 0, sb["t"], out=sb["s"])
        _native.q_sample(sb["x0"], sb["noise"], sb["a"], sb["s"], sb["x_t"])
        state.trainer.forward(fp.flat, sb["x_t"], sb["z"], sb["t"], out=sb["eps"])
        objective = _native.diffusion_loss_grad_v if v_pred else _native.diffusion_loss_grad
        terms, d_eps = objective(sb["eps"], sb["noise"], sb["x_t"], sb["x0"], sb["a"], sb["s"], recon_w, tv_w,
                                 bufs=(sb["terms"], sb["d_eps"], sb["scratch_obj"]))
        loss = terms[0]
        state.last_loss_terms = terms
    else:
        sch.q_sample(sb["x0"], sb["t"], sb["noise"], out=sb["x_t"])
        state.trainer.forward(fp.flat, sb["x_t"], sb["z"], sb["t"], out=sb["eps"])
        loss, d_eps = _native.mse_loss_grad(sb["eps"], sb["noise"], bufs=(sb["loss"], sb["d_eps"], sb["scratch"]))
        state.last_loss_terms = None
    import torch.distributed as dist
    have_pg = bool(ddp) and dist.is_available() and dist.is_initialized()
    world = dist.get_world_size() if have_pg else 1
    # ddp="always": the bucketed route whenever a process group exists, a one-rank group included (runs the RCCL all-reduces and the
    # stream joins of the N > 1 route on a single GPU: tests/test_gpu_rccl.py)
    if world > 1 or (have_pg and ddp == "always"):
        # data parallel: the flat gradient buffer is all-reduced bucket by bucket while the backward still runs (RCCL on its own
        # stream); d_eps is pre-scaled by 1 / world so that the sum is already the mean
        if guard is None:
            d_eps.mul_(1.0 / world)
        else:
            # scale / world into a static one-element buffer (a one-element launch, no allocation), then ONE pass over d_eps
            factor = sb.setdefault("scale_over_world", torch.empty((), dtype=torch.float32, device=d_eps.device))
            torch.mul(guard.scale_tensor(d_eps.device), 1.0 / world, out=factor)
            d_eps.mul_(factor)
        works = []
        state.trainer.backward(fp.flat, fp.grad, sb["x_t"], sb["z"], d_eps,
                               bucket_cb=lambda lo, hi: works.append(dist.all_reduce(fp.grad[lo:hi], async_op=True)))
        for w in works:
            w.wait()
    else:
        if guard is not None:
            d_eps.mul_(guard.scale_tensor(d_eps.device))
        state.trainer.backward(fp.flat, fp.grad, sb["x_t"], sb["z"], d_eps)
    if guard is not None or clip:
        opt.step(zero_grad=True, guard=guard, max_grad_norm=max_grad_norm)
    elif isinstance(opt, FusedAdamW):
        opt.step(zero_grad=True)
    else:
        opt.step()
        opt.zero_grad()
    return loss


# ---- the reference's entry point (train/diffusion_train.py:36-60,69-150) -----------------------------------------------------
class StoreDataset(torch.utils.data.Dataset):
    """(image in [-1, 1] as (3, S, S) fp32, L2-normalised CLIP embedding) per manifest record -- train/diffusion_train.py:36-60."""

    def __init__(self, store_dir, out_size: int = 256) -> None:
        import json
        from pathlib import Path
        import numpy as np
        self.store_dir = Path(store_dir)
        self.manifest = json.loads((self.store_dir / "manifest.json").read_text(encoding="utf-8"))
        meta = np.load(self.store_dir / "codec_meta.npz")
        self.scale = meta["scale"].astype("float32")
        self.zero = meta["zero"].astype("float32")
        self.out_size = out_size

    def __len__(self) -> int:
        return len(self.manifest)

    def __getitem__(self, i: int):
        from pathlib import Path
        import numpy as np
        from PIL import Image
        from ..io.bitstream import read_bitstream, decode_embedding
        rec = self.manifest[i]
        z = decode_embedding(read_bitstream(Path(rec["bitstream"])), self.scale, self.zero).astype(np.float32).reshape(-1)
        img = Image.open(rec["image"]).convert("RGB").resize((self.out_size, self.out_size), Image.BICUBIC)
        arr = (np.array(img).astype(np.float32) / 127.5 - 1.0).transpose(2, 0, 1)
        return torch.from_numpy(arr), torch.from_numpy(z)


def total_variation(x: torch.Tensor) -> torch.Tensor:
    return (x[:, :, 1:, :] - x[:, :, :-1, :]).abs().mean() + (x[:, :, :, 1:] - x[:, :, :, :-1]).abs().mean()


def autograd_objective_step(net, sch, opt, x0: torch.Tensor, z: torch.Tensor, t: torch.Tensor, noise: torch.Tensor,
                            recon_w: float = 0.0, tv_w: float = 0.0, scaler: Optional[GradScaler] = None,
                            max_grad_norm: Optional[float] = None, prediction: str = "eps") -> torch.Tensor:
    """The loop body of train/diffusion_train.py:119-128,137-140 through autograd: the objective from torch ops on (B, 3, S, S), the
    library's forward and backward behind ``UNetFunction``, ``opt.step()`` and ``opt.zero_grad()`` as two passes.  What
    ``train_step(recon_w=, tv_w=)`` fuses; kept as ``train_diffusion(fused_objective=False)`` and for A/B (tools/objective_ab.py).
    With ``scaler`` the last lines are the reference's ``scaler.scale(loss).backward(); scaler.step(opt); scaler.update()``.
    ``prediction="v"``: the target is ``sch.v_target`` and ``x0_pred = clamp(a x_t - s v_hat)``, as in ``train_step``."""
    import torch.nn.functional as F
    v_pred = _native.prediction_code(prediction) == _native.PRED_V
    state: TrainState = net.train_state()
    state.fp.rebind_grads()
    x_t = sch.q_sample(x0, t, noise)
    eps_hat = net(x_t, z, t)
    loss = F.mse_loss(eps_hat, sch.v_target(x0, t, noise) if v_pred else noise)
    if recon_w > 0 or tv_w > 0:
        # predict_x0_from_eps (diffusion/scheduler.py:51-55) written with torch ops: its gradient must reach eps_hat
        sg = sch.sqrt_one_minus_alphas_cumprod[t].view(-1, 1, 1, 1); ac = sch.sqrt_alphas_cumprod[t].view(-1, 1, 1, 1)
        x0_pred = (ac * x_t - sg * eps_hat if v_pred else (x_t - sg * eps_hat) / ac).clamp(-1, 1)
        if recon_w > 0:
            loss = loss + recon_w * F.l1_loss(x0_pred, x0)
        if tv_w > 0:
            loss = loss + tv_w * total_variation(x0_pred)
    if scaler is not None and scaler.enabled:
        scaler.scale(loss).backward()
        scaler.step(opt, max_grad_norm=max_grad_norm)
        scaler.update()
        return loss.detach()                        # the guarded step left the gradient buffer at zero: no second pass over it
    loss.backward()
    state.wait_grad_sync()
    if max_grad_norm is not None and max_grad_norm > 0:
        opt.step(max_grad_norm=max_grad_norm)       # guarded (scale 1): consumes and zeroes the gradients as well
        return loss.detach()
    opt.step()
    opt.zero_grad()
    return loss.detach()


def check_resume_prediction(ck, prediction: str, resume="the resumed state") -> None:
    """``train_state.pt`` records the parameterisation its weights were trained with (a file from before the option: ``"eps"``);
    continuing it with another one is a ``ValueError`` naming both."""
    _native.prediction_code(prediction)
    had = ck.get("prediction", "eps")
    if had != prediction:
        raise ValueError(f"{resume} was trained with prediction={had!r}, this run asks for prediction={prediction!r}")


def check_zero_snr_prediction(zero_snr: bool, prediction: str) -> None:
    """A zero-terminal-SNR schedule has ``sqrt(alphas_cumprod[T-1]) == 0`` and the eps form divides by it: only ``prediction="v"``
    trains on it; anything else is a ``ValueError`` naming both settings."""
    if zero_snr and prediction != "v":
        raise ValueError(f'zero_snr=True (a rescale_zero_snr scheduler) needs prediction="v", not prediction={prediction!r}: the eps form '
                         'divides by sqrt(alpha_bar_t), which is 0 at t = T-1')


def check_resume_zero_snr(ck, zero_snr: bool, resume="the resumed state") -> None:
    """``train_state.pt`` records whether its weights were trained on the zero-terminal-SNR schedule (a file from before the option:
    ``False``); continuing it on the other schedule is a ``ValueError`` naming both."""
    had = bool(ck.get("zero_snr", False))
    if had != bool(zero_snr):
        raise ValueError(f"{resume} was trained with zero_snr={had}, this run asks for zero_snr={bool(zero_snr)}")


def train_diffusion(store_dir, out_size: int = 256, epochs: int = 40, batch_size: int = 8, lr: float = 2e-4, timesteps: int = 1000,
                    schedule: str = "cosine", recon_w: float = 0.05, clip_w: float = 0.1, tv_w: float = 1e-4, device: str = "cuda",
                    save_dir=None, base: int = 128, ch_mult=(1, 2, 2), dtype: str = "bf16", num_workers: int = 2, log=print,
                    fused_objective: bool = True, grad_scaler: bool = False, max_grad_norm: Optional[float] = None,
                    ema_decay: Optional[float] = None, ema_warmup: bool = False, resume=None, z_drop: float = 0.0,
                    prediction: str = "eps", zero_snr: bool = False):
    """The reference's ``train_diffusion`` (same arguments, defaults, checkpoint names and log line) on the MI355X kernels.

    Per batch (train/diffusion_train.py:115-140): t ~ U{0..T-1}, noise ~ N, then ``train_step`` with the ``t`` / ``noise`` drawn here:
    x_t = q_sample, eps_hat = net(x_t, z, t), loss = mse(eps_hat, noise) + recon_w * L1(x0_pred, x0) + tv_w * TV(x0_pred) and its
    gradient from one kernel, the library's backward, the fused AdamW step.  The running loss is accumulated on the device and read
    once per epoch.  ``fused_objective=False`` keeps the earlier route for A/B: the same objective from torch ops on (B, 3, S, S)
    through autograd (``UNetFunction``), the loss read back every batch.  The CLIP-alignment term (clip_w, :129-136) needs
    ``open_clip`` with downloaded weights: it is skipped with a note.  ``grad_scaler=True`` is the reference's
    setting (its ``GradScaler``, :106,137-139): loss scaling with the skipped step on non-finite gradients, decided on the device
    (``GradScaler`` above); it is off by default here because the fp32 gradient buffer does not need the scale, only the guard.
    ``max_grad_norm`` > 0 clips the gradient's L2 norm in the same pass.  The number of skipped steps is logged per epoch, from the
    same host read as the loss.  Additions that default to the reference's behaviour: ``base`` / ``ch_mult`` / ``dtype``.  With
    ``torch.distributed`` initialised the records are sharded over the ranks and the flat gradient buffer is all-reduced bucket
    by bucket while the backward runs.

    ``ema_decay``: ``FusedAdamW`` keeps the moving average of the weights and rank 0 also writes ``diffusion_unet_ep{N}_ema.pt`` and
    ``diffusion_unet_final_ema.pt`` -- the checkpoints to sample from; the reference's file names keep holding the raw iterate.
    Every epoch rank 0 also writes ``train_state.pt`` (to a temporary name, then ``os.replace``): epoch, weights, optimiser and scaler
    state, torch's CPU and device RNG states.  ``resume=<that file>`` restores all of it on every rank and continues with the next
    epoch (same ``[train] epoch k/N`` numbering); a file of another architecture or parameter count is refused.

    ``z_drop`` (usually 0.1): every batch's embeddings go through ``z_dropout`` -- whole rows zeroed with that probability, one
    ``torch.rand`` draw per batch on the device, each rank its own -- which trains the unconditional branch that
    ``DDIMSampler(guided=True)`` needs.  ``train_state.pt`` already carries the RNG states, so a resumed run continues the masks.

    ``prediction="v"`` trains the v-parameterisation (``train_step``).  The checkpoints keep the reference's key set, so they do NOT
    say how they were trained: pass the same ``prediction`` to the samplers and the CLIs.  ``train_state.pt`` does record it, and
    ``resume=`` with another one is a ``ValueError`` naming both.

    ``zero_snr=True`` trains on the schedule rescaled to zero terminal SNR (``NoiseScheduler(rescale_zero_snr=True)``), so that
    ``t = T-1``, where every sampler starts, is pure noise in training too.  It needs ``prediction="v"`` (a ``ValueError`` otherwise).
    Like ``prediction`` it is not in the checkpoints -- pass ``--zero_snr`` to the CLIs -- but ``train_state.pt`` records it and
    ``resume=`` with the other value is a ``ValueError`` naming both (a file from before the option reads as ``False``).
    """
    import os
    from pathlib import Path
    import torch.distributed as dist
    from ..models.unet import CLIPCondUNet
    from ..diffusion.scheduler import NoiseScheduler
    if not 0.0 <= z_drop <= 1.0:
        raise ValueError(f"z_drop must be in [0, 1], not {z_drop}")
    _native.prediction_code(prediction)
    check_zero_snr_prediction(zero_snr, prediction)
    save_dir = Path(save_dir or store_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    ds = StoreDataset(store_dir, out_size=out_size)
    ddp = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    sampler = torch.utils.data.distributed.DistributedSampler(ds, shuffle=True) if ddp else None
    dl = torch.utils.data.DataLoader(ds, batch_size=batch_size, shuffle=sampler is None, sampler=sampler, num_workers=num_workers,
                                     pin_memory=True)
    z_dim = ds[0][1].numel()
    net = CLIPCondUNet(z_dim=z_dim, base=base, ch_mult=tuple(ch_mult), img_ch=3, dtype=dtype).to(device)
    ck = None
    if resume is not None:
        from ..models.unet import infer_arch
        ck = torch.load(resume, map_location="cpu", weights_only=True)
        check_resume_prediction(ck, prediction, resume)
        check_resume_zero_snr(ck, zero_snr, resume)
        if infer_arch(ck["net"]) != net.arch:
            raise ValueError(f"{resume} holds a model of architecture {infer_arch(ck['net'])}, this run builds {net.arch}")
        net.load_state_dict(ck["net"], strict=True)        # the optimiser's load_state_dict below refuses another parameter count
    if ddp:                                                    # same initial weights on every rank
        for p in net.parameters():
            dist.broadcast(p.data, src=0)
    sch = NoiseScheduler(timesteps=timesteps, schedule=schedule, device=device, rescale_zero_snr=zero_snr)
    net.train()
    state = net.train_state(device)
    # data parallel: finished ranges of the flat gradient buffer are all-reduced (RCCL) while the backward still runs
    state.ddp_bucketed = ddp
    opt = FusedAdamW(net, lr=lr, ema_decay=ema_decay, ema_warmup=ema_warmup)
    scaler = GradScaler() if grad_scaler else None
    skipped_before, first_ep = 0, 0
    if ck is not None:
        if (ck["scaler"] is None) != (scaler is None):
            raise ValueError(f"{resume} was written {'with' if ck['scaler'] is not None else 'without'} grad_scaler, this run is the reverse")
        opt.load_state_dict(ck["opt"])          # the hyper-parameters of the stopped run included: `lr` is then the file's
        if scaler is not None:
            scaler.load_state_dict(ck["scaler"])
            skipped_before = int(ck["scaler"]["skipped_steps"])
        torch.set_rng_state(ck["rng_cpu"])
        torch.cuda.set_rng_state(ck["rng_device"], device)
        first_ep = int(ck["epoch"])
    if clip_w > 0:
        try:
            import open_clip  # noqa: F401
            raise ImportError("the CLIP-alignment term is not wired to this build's kernels")
        except ImportError as exc:
            log(f"[train] clip_w={clip_w} ignored: {exc}")
    rank0 = not ddp or dist.get_rank() == 0
    final_path = save_dir / "diffusion_unet_final.pt"
    for ep in range(first_ep, epochs):
        if sampler is not None:
            sampler.set_epoch(ep)
        running, seen = 0.0, 0
        running_dev = torch.zeros((), dtype=torch.float64, device=device)
        for x0, z in dl:
            x0 = x0.to(device); z = z.to(device)
            b = x0.size(0)
            t = torch.randint(0, timesteps, (b,), device=device, dtype=torch.long)
            noise = torch.randn_like(x0)
            if fused_objective:
                loss = train_step(net, sch, opt, x0, z, t=t, noise=noise, ddp=ddp, recon_w=max(recon_w, 0.0), tv_w=max(tv_w, 0.0),
                                  scaler=scaler, max_grad_norm=max_grad_norm, z_drop=z_drop, prediction=prediction)
                running_dev += loss.double() * b          # the loss is a view of a static buffer: consumed here, in stream order
            else:
                if z_drop > 0:
                    z = z_dropout(z, z_drop)[0]
                running += float(autograd_objective_step(net, sch, opt, x0, z, t, noise, recon_w, tv_w, scaler=scaler,
                                                                 max_grad_norm=max_grad_norm, prediction=prediction)) * b
            seen += b
        skipped, loss_scale = 0, 1.0
        if opt._guard is not None:                        # the one host read of the epoch carries the guard's counters too
            st = opt._guard.stats()
            got = torch.stack([running_dev, st["skipped_steps"].double(), st["scale"].double()]).tolist()
            skipped, loss_scale = int(got[1]) - skipped_before, got[2]
            skipped_before = int(got[1])
            if fused_objective:
                running = got[0]
        elif fused_objective:
            running = float(running_dev)                  # the one host read of the epoch
        if rank0:
            torch.save(net.state_dict(), save_dir / f"diffusion_unet_ep{ep + 1}.pt")
            if opt.ema is not None:
                torch.save(opt.ema_state_dict(), save_dir / f"diffusion_unet_ep{ep + 1}_ema.pt")
            tmp_path = save_dir / "train_state.pt.tmp"
            torch.save(dict(epoch=ep + 1, net=net.state_dict(), opt=opt.state_dict(), scaler=None if scaler is None else scaler.state_dict(),
                            rng_cpu=torch.get_rng_state(), rng_device=torch.cuda.get_rng_state(device), prediction=prediction,
                            zero_snr=bool(zero_snr)), tmp_path)
            os.replace(tmp_path, save_dir / "train_state.pt")
            log(f"[train] epoch {ep + 1}/{epochs} loss={running / max(seen, 1):.4f}")
            if skipped:
                log(f"[train] epoch {ep + 1}/{epochs}: {skipped} step(s) skipped on non-finite gradients, loss scale now {loss_scale:g}")
    if rank0:
        torch.save(net.state_dict(), final_path)
        if opt.ema is not None:
            torch.save(opt.ema_state_dict(), save_dir / "diffusion_unet_final_ema.pt")
    return final_path
