"""The script that pins the bits of the optimiser tail: three steps of every AdamW entry point on host-seeded inputs.

tests/golden/make_optimizer_golden.py runs it against the library of an earlier commit and records a SHA-256 of every buffer after
every step in tests/golden/optimizer_steps.npz; tests/test_gpu_optimizer_bits.py runs it against the library under test and compares.
Both go through the public ``_native`` wrappers, so the library is whatever ``CCN_HIP_LIB`` names (the built one by default).

Modes: the plain step keeping / zeroing the gradients, the guarded step, and the same three with the fused EMA (the guarded one with
warm-up).  The guarded modes clip at ``MAX_NORM`` and grow the scale after every good step, and their second step's gradient holds
one ``inf``: that step must leave p / m / v / ema / ``updates`` alone, zero g and back the scale off (asserted here, so that neither
the fixture nor the test can go blind).

Cases ``(n, element offsets of p, g, m, v, ema off their 16-byte boundary)`` are the smallest at which the head / quad / tail walk can
go wrong; every buffer sits between ``PAD`` sentinel floats, which are checked after every step.
"""
from __future__ import annotations

import functools
import hashlib

import numpy as np
import torch

import guard_ref
from clip_feature_codec import _native

DEV = "cuda:0"
H = guard_ref.HYPER
GW = _native.GUARD_WORD
EW = _native.EMA_WORD
PAD = 4
SENTINEL = 7.0
STEPS = 3
GRID_CAP = 8192                                    # workgroups of 256 threads, one 16-byte quad of each buffer per thread and trip
N_BIG = 4 * (GRID_CAP * 256 * 2 + 77) + 3          # tests/test_gpu_ema.py's: two trips of the capped grid plus a ragged rest
KEEP_ARRAYS_UP_TO = 1033                           # the final arrays of these cases are stored as well, to locate a mismatch
MAX_NORM = 0.5                                     # below the gradient norm 0.01 sqrt(n) of the larger cases: the clip is active there
EMA_DECAY = 0.999
INIT_SCALE = 65536.0
BUFFERS = ("p", "g", "m", "v", "ema", "guard", "ema_block")

# mode -> (guarded, ema, zero_grad, warmup)
MODES = {
    "plain_keep": (False, False, False, False),
    "plain_zero": (False, False, True, False),
    "guarded": (True, False, True, False),
    "ema_keep": (False, True, False, False),
    "ema_zero": (False, True, True, False),
    "ema_guarded_warmup": (True, True, True, True),
}
Z5 = (0, 0, 0, 0, 0)
_SHAPES = [
    (1, Z5), (3, Z5),                # head only
    (5, Z5),                         # one quad + tail
    (255, Z5), (257, Z5),            # around one wave-multiple
    (1033, (1, 1, 1, 1, 1)),         # head 3, 257 quads (a second workgroup), tail 2
    (10007, (0, 1, 0, 0, 0)),        # the gradient buffer alone is odd: the 4-byte path
    (10007, (0, 0, 0, 0, 1)),        # the EMA buffer alone is odd (EMA modes only)
    (N_BIG, Z5),
]
# the modes without an EMA buffer skip the one shape that differs from another in the EMA's offset alone
CASES = [(n, off, mode) for n, off in _SHAPES for mode, (_, ema, _, _) in MODES.items() if ema or off != (0, 0, 0, 0, 1)]
assert len(CASES) == 9 * 6 - 3


def case_id(n, off, mode) -> str:
    return f"{n}-{''.join(map(str, off))}-{mode}"


IDS = [case_id(*c) for c in CASES]


@functools.lru_cache(maxsize=1)
def inputs(n: int):
    """Parameters randn(n) and STEPS gradients 0.01 randn(n), fp32, from numpy's generator on the host (one stream per n)."""
    rng = np.random.default_rng(20260 + n)
    p0 = rng.standard_normal(n, dtype=np.float32)
    return p0, [rng.standard_normal(n, dtype=np.float32) * np.float32(0.01) for _ in range(STEPS)]


def _sha(t: torch.Tensor) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(t.contiguous().cpu().numpy()).digest(), dtype=np.uint8)


def run(n: int, off, mode: str):
    """Run the script; returns (digests uint8 [STEPS][len(BUFFERS)][32] (zeros for a buffer the mode does not have),
    final arrays fp32 [4 or 5][n] or None above KEEP_ARRAYS_UP_TO, final blocks int32 [GUARD_WORDS + EMA_WORDS] (zeros if absent))."""
    guarded, with_ema, zero, warmup = MODES[mode]
    p0, grads = inputs(n)
    nbuf = 5 if with_ema else 4
    base = [torch.full((n + 2 * PAD + 4,), SENTINEL, device=DEV) for _ in range(nbuf)]
    bufs = [b[PAD + o:PAD + o + n] for b, o in zip(base, off)]
    assert all(b.data_ptr() % 16 == 4 * o for b, o in zip(bufs, off))
    p, g, m, v = bufs[:4]
    ema = bufs[4] if with_ema else None
    p.copy_(torch.from_numpy(p0))
    g.zero_(); m.zero_(); v.zero_()
    block = scratch = ema_block = None
    if with_ema:
        ema.fill_(-3.0)                             # never read before the first update: the value must not matter
        ema_block = torch.zeros(_native.EMA_WORDS, dtype=torch.int32, device=DEV)
        _native.ema_init(ema_block, 0)
    if guarded:
        block = torch.zeros(_native.GUARD_WORDS, dtype=torch.int32, device=DEV)
        scratch = torch.empty(_native.GUARD_SCRATCH_FLOATS, device=DEV)
        _native.step_guard_init(block, INIT_SCALE)
    named = dict(zip(BUFFERS, (p, g, m, v, ema, block, ema_block)))
    digests = np.zeros((STEPS, len(BUFFERS), 32), dtype=np.uint8)
    hyper = (H["lr"], H["betas"][0], H["betas"][1], H["eps"], H["weight_decay"])
    for it in range(STEPS):
        step = it + 1
        g.copy_(torch.from_numpy(grads[it]))
        if guarded:
            if step == 2:
                g[n // 2] = float("inf")
            scale_before = float(block.view(torch.float32)[GW["scale"]])
            g.mul_(block.view(torch.float32)[GW["scale"]])
            _native.grad_guard(g, block, scratch, MAX_NORM, H["betas"][0], H["betas"][1], 2.0, 0.5, 1)
        if with_ema:
            _native.adamw_step_ema(p, g, m, v, ema, *hyper, step, EMA_DECAY, ema_block, zero_grad=zero, ema_warmup=warmup, guard_block=block)
        elif guarded:
            _native.adamw_step_guarded(p, g, m, v, *hyper, block)
        else:
            _native.adamw_step(p, g, m, v, *hyper, step, zero_grad=zero)
        for k, name in enumerate(BUFFERS):
            if named[name] is not None:
                digests[it, k] = _sha(named[name])
        for b, o in zip(base, off):
            assert bool((b[:PAD + o] == SENTINEL).all()) and bool((b[PAD + o + n:] == SENTINEL).all()), (step, "padding overwritten")
        # what the script is about, whatever the library
        if zero:
            assert not g.any(), step
        else:
            assert np.array_equal(g.cpu().numpy(), grads[it]), step
        if guarded:
            skipped = step == 2
            assert int(block[GW["apply"]]) == int(not skipped), step
            assert float(block.view(torch.float32)[GW["scale"]]) == scale_before * (0.5 if skipped else 2.0), step
            if skipped:
                same = [k for k, name in enumerate(BUFFERS) if name in ("p", "m", "v", "ema")]
                assert np.array_equal(digests[it, same], digests[it - 1, same]), "a skipped step moved p / m / v / ema"
        if with_ema:
            assert int(ema_block[EW["updates"]]) == (step - (1 if guarded and step >= 2 else 0)), step
    finals = torch.stack(bufs).cpu().numpy() if n <= KEEP_ARRAYS_UP_TO else None
    blocks = np.zeros(_native.GUARD_WORDS + _native.EMA_WORDS, dtype=np.int32)
    if guarded:
        blocks[:_native.GUARD_WORDS] = block.cpu().numpy()
    if with_ema:
        blocks[_native.GUARD_WORDS:] = ema_block.cpu().numpy()
    return digests, finals, blocks
