"""The training step's per-shape plan (csrc/ccn_train.hip, StepPlan) against the walks it replaced and against its own properties.

``tests/golden/train_plan_parent.json`` holds what the last library with the three bump-allocator walks gave for the shapes of
tests/train_plan_cases.py: ``ccn_train_workspace_bytes`` and the text of ``ccn_internal_train_routes`` after a forward + backward, plain
and bucketed (made by tests/golden/make_train_plan_golden.py from the commit the fixture names).  Sizes and launch decisions are compared
exactly; numerics are not compared with the parent's (the training buffers are not bit-reproducible from run to run, docs/EXPERIMENTS.md
R11.2) but between the run-time forms of one library, with the bounds test_gpu_train.py uses between plain launches and a graph replay.
"""
import ctypes
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "clip-neural-image-conpression_amd"), str(ROOT / "tests")]

import train_plan_cases as tpc  # noqa: E402
from clip_feature_codec import _native  # noqa: E402
from clip_feature_codec.models.unet import CLIPCondUNet  # noqa: E402
from clip_feature_codec.utils import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = tpc.DEV
FIX = json.loads((ROOT / "tests" / "golden" / "train_plan_parent.json").read_text())
STEP_CASES = [cid for cid, c in tpc.CASES.items() if c[7]]


def layout(trainer, B, H, W):
    """(text, [(name, off, bytes)], total) of ccn_internal_train_layout."""
    lib = trainer.lib
    lib.ccn_internal_train_layout.restype = ctypes.c_int
    lib.ccn_internal_train_layout.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p, ctypes.c_size_t]
    n = lib.ccn_internal_train_layout(trainer.h, B, H, W, None, 0)
    assert n > 0
    buf = ctypes.create_string_buffer(n + 1)
    assert lib.ccn_internal_train_layout(trainer.h, B, H, W, buf, n + 1) == n
    text = buf.value.decode()
    lines = text.splitlines()
    assert lines[-1].startswith("total=")
    regions = []
    for ln in lines[:-1]:
        name, off, size = ln.split()
        assert off.startswith("off=") and size.startswith("bytes=")
        regions.append((name, int(off[4:]), int(size[6:])))
    return text, regions, int(lines[-1][6:])


def test_the_fixture_covers_the_cases_and_the_launch_forms():
    """All twelve cases are in the fixture, and its OWN bf16 route texts contain every form the comparison claims to cover: both side
    forms and the fused pre-pass of the forward norm, the persistent kernel for the 3x3, the stride-2 conv and the ConvTranspose as forward
    and as data gradient, one of them in the 4x4 form."""
    assert list(FIX["cases"]) == list(tpc.CASES) and len(FIX["cases"]) == 12
    assert len(FIX["commit"]) >= 7 and FIX["device"]
    for cid, c in tpc.CASES.items():
        got = FIX["cases"][cid]
        assert got["bytes"] > 0
        assert ("routes" in got and "routes_bucketed" in got and len(got["routes"].splitlines()) > 100) if c[7] else set(got) == {"bytes"}
    have = tpc.bf16_coverage(FIX["cases"][cid][k] for cid in STEP_CASES if cid.startswith("bf16") for k in ("routes", "routes_bucketed"))
    assert all(have.values()), [k for k, v in have.items() if not v]


@pytest.mark.parametrize("cid", list(tpc.CASES))
def test_workspace_bytes_and_routes_are_the_parents(cid):
    got, want = tpc.record(cid), FIX["cases"][cid]
    assert got["bytes"] == want["bytes"]
    assert set(got) == set(want)
    for k in ("routes", "routes_bucketed"):
        if k in want:
            a, b = got[k].splitlines(), want[k].splitlines()
            diff = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
            assert not diff and len(a) == len(b), (k, len(a), len(b), diff[:5])


@pytest.mark.parametrize("cid", list(tpc.CASES))
def test_layout_regions_are_aligned_disjoint_and_inside_the_workspace(cid):
    """activations are not aliased.  Nothing is launched."""
    dtype, base, ch_mult, B, H, W, variant, _ = tpc.CASES[cid]
    lib = tpc.library()
    old = lib.ccn_internal_set_conv_variant(variant) if variant is not None else None
    tr = _native.NativeTrainer(512, base, ch_mult, tpc.TIME_DIM, 3, dtype=dtype, device=DEV)
    try:
        _, regions, total = layout(tr, B, H, W)
        assert total == tpc.workspace_bytes(tr, B, H, W) == FIX["cases"][cid]["bytes"]
    finally:
        tr.close()
        if old is not None:
            lib.ccn_internal_set_conv_variant(old)
    assert len(regions) > 100 and len({name for name, _, _ in regions}) == len(regions)
    end, last = 0, None
    for name, off, size in sorted(regions, key=lambda r: r[1]):
        assert off % 256 == 0 and size > 0, (name, off, size)
        assert off >= end, f"{name} at {off} overlaps {last}, which ends at {end}"
        assert off + size <= total, (name, off, size, total)
        end, last = off + size, name


def make_net(base, dtype):
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, (1, 2)))
    net = CLIPCondUNet(z_dim=512, base=base, ch_mult=(1, 2), time_dim=tpc.TIME_DIM, dtype=dtype).to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return net.train()


def step_data(B, H, W, seed):
    g = torch.Generator("cpu").manual_seed(seed)
    x = torch.randn((B, 3, H, W), generator=g).to(DEV)
    target = torch.randn((B, 3, H, W), generator=g).to(DEV)
    return x, torch.from_numpy(synth.synth_z(B)).to(DEV), torch.linspace(0, 999, B).round().long().to(DEV), target


class Runner:
    """Forward, fused MSE and backward of one trainer on fixed buffers (a captured graph is keyed by their addresses)."""

    def __init__(self, tr, flat, B, H, W, seed=5):
        self.tr, self.flat = tr, flat
        self.x, self.z, self.t, self.target = step_data(B, H, W, seed)
        self.eps, self.g = torch.empty_like(self.x), torch.zeros_like(flat)
        self.bufs = (torch.empty((), device=DEV), torch.empty_like(self.x), torch.empty(1024, device=DEV))

    def step(self, backward=True):
        """(loss, eps, flat gradient) on the host."""
        self.g.zero_()
        self.tr.forward(self.flat, self.x, self.z, self.t, out=self.eps)
        loss, d = _native.mse_loss_grad(self.eps, self.target, bufs=self.bufs)
        if backward:
            self.tr.backward(self.flat, self.g, self.x, self.z, d)
        torch.cuda.synchronize()
        return float(loss), self.eps.cpu().clone(), self.g.cpu().clone()


def assert_as_graph_replay_against_plain(ref, got, what):
    """The comparison of test_graph_replay_of_forward_and_backward_matches_plain_launches: the losses with np.allclose(rtol=1e-5); a
    buffer's largest difference at most 0.05 of the buffer's own scale -- there the parameters' largest movement, here the largest
    entry of the plain run's eps and of its gradient."""
    assert np.allclose(ref[0], got[0], rtol=1e-5), (what, ref[0], got[0])
    for name, a, b in (("eps", ref[1], got[1]), ("gradient", ref[2], got[2])):
        assert bool(torch.isfinite(b).all()), (what, name)
        diff, scale = float((a - b).abs().max()), float(a.abs().max())
        print(f"{what}: {name} max difference {diff:.3e}, scale {scale:.3e}")
        assert scale > 0 and diff <= 0.05 * scale, (what, name, diff, scale)


def test_side_forms_graph_replay_and_profiling_share_one_plan():
    """bf16, base 128, 2 x 136 x 200 on one trainer: plain launches (side forms of the ResBlocks, pack split, weight gradients beside the
    data gradients), a captured and replayed graph (pre-pass forms, everything on one stream at capture), profiling on (no side
    stream).  The run-time choices work over the same planned regions: the layout report is the same text after each, and eps and
    gradients stay with the plain run's."""
    B, H, W = 2, 136, 200
    net = make_net(128, "bf16")
    st = net.train_state()
    tr = st.trainer
    run = Runner(tr, st.fp.flat, B, H, W)
    plain = run.step()
    assert "norm side-" in tpc.routes(tr)
    text = layout(tr, B, H, W)[0]
    tr.set_graph(True)
    run.step()                                                  # capture
    replay = run.step()
    assert "norm side-" not in tpc.routes(tr)
    assert layout(tr, B, H, W)[0] == text
    assert_as_graph_replay_against_plain(plain, replay, "graph replay")
    tr.set_graph(False)
    tr.profile(True)
    prof = run.step()
    fams = tr.profile_read()
    tr.profile(False)
    assert sum(f["calls"] for f in fams) > 100
    assert layout(tr, B, H, W)[0] == text
    assert_as_graph_replay_against_plain(plain, prof, "profiling")


def test_backward_after_the_shape_cache_is_warm():
    """forward(shape 1), forward + backward(shape 2), forward + backward(shape 1) on one trainer and one workspace that holds either:
    the last backward finds its tensors through the cached plan of shape 1, not through anything the calls in between left behind."""
    s1, s2 = (2, 32, 32), (2, 48, 64)
    net = make_net(128, "bf16")
    st = net.train_state()
    tr = st.trainer
    big = _native.Workspace(max(tpc.workspace_bytes(tr, *s) for s in (s1, s2)), tr.device)
    tr._ws = {s1: big, s2: big}
    r1, r2 = Runner(tr, st.fp.flat, *s1, seed=5), Runner(tr, st.fp.flat, *s2, seed=6)
    r1.step(backward=False)
    other = r2.step()
    assert bool(torch.isfinite(other[2]).all())
    got = r1.step()
    net2 = make_net(128, "bf16")
    st2 = net2.train_state()
    ref = Runner(st2.trainer, st2.fp.flat, *s1, seed=5).step()
    assert_as_graph_replay_against_plain(ref, got, "shape 1 after shape 2")
