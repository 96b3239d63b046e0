"""The seven fixed-shape loop entries (``ccn_sample`` .. ``ccn_sample_guided_ms``), called directly through ctypes.  The Python route
goes through ``ccn_sample_run``, so this file is what still calls the wrappers: each one launch by launch, then captured, then replayed,
bit for bit against ``NativeUNet.sample`` with the corresponding keywords on another workspace slot.  The C1-sized model (base 32,
``(1, 2)``), B = 2, 16 px, 6 steps: the smallest shape with a guided 2B layout and a seeded step of more than one record."""
import ctypes

import numpy as np
import pytest
import torch

from clip_feature_codec import _native
from clip_feature_codec.models.unet import CLIPCondUNet
from clip_feature_codec.diffusion.scheduler import NoiseScheduler
from clip_feature_codec.diffusion.dpm_solver import DPMSolverSampler

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, S, T, W_G, ETA, THR_P = 2, 16, 6, 3.0, 0.03, 0.9
SHAPE = (B, 3, S, S)
SEEDS = [7, 2 ** 63 + 8]
VARIANTS = ("plain", "eta", "guided", "seeded", "guided_seeded", "ms", "guided_ms")
MOST_FIELDS = ("guided_seeded", "guided_ms")       # the two entries whose records use the most fields
CASES = [(v, "eps", None) for v in VARIANTS] + [(v, "v", None) for v in MOST_FIELDS] + [(v, "eps", THR_P) for v in MOST_FIELDS]


@pytest.fixture(scope="module")
def nets(tiny_sd):
    def make(dtype):
        net = CLIPCondUNet(z_dim=512, base=32, ch_mult=(1, 2), dtype=dtype).to(DEV).eval()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in tiny_sd.items()}, strict=True)
        return net
    return {d: make(d) for d in ("fp32", "bf16")}


@pytest.fixture(scope="module")
def inputs(synth):
    """Tables and tensors of every variant, made once; never written to (the scratches are per test)."""
    sch = NoiseScheduler(1000, "linear", DEV)
    coef = sch.ddim_coefficients(T, ETA)
    assert np.isfinite(coef).all() and (coef[:-1, 4] > 0).all()
    ms_ts, ms_coef = DPMSolverSampler(sch).tables(T)
    assert (ms_coef[1:-1, 4] != 0).all()
    c = lambda a, t: np.ascontiguousarray(a, dtype=t)
    return dict(z=torch.from_numpy(synth.synth_z(B)).to(DEV), x_T=_native.normal_fill(SEEDS, SHAPE, 0, device=DEV),
                ts=c(sch.ddim_timesteps(T), np.int32), coef=c(coef[:, :4], np.float32), sigma=c(coef[:, 4], np.float32),
                noise=torch.stack([_native.normal_fill(SEEDS, SHAPE, 1 + i, device=DEV) for i in range(T)]),
                seeds=_native.seeds_tensor(SEEDS, B, DEV), ms_ts=c(ms_ts, np.int32), ms_coef=c(ms_coef, np.float32))


def reference(nat, variant, a, thr):
    """``NativeUNet.sample`` with the keywords of the variant, on slot 0.  Leaves the handle's dynamic threshold as the run had it."""
    kw = dict(slot=0, dynamic_threshold=thr)
    if "guided" in variant:
        kw["w"] = W_G
    if variant.endswith("ms"):
        return nat.sample(a["z"], a["x_T"], a["ms_ts"], a["ms_coef"], **kw)
    if variant in ("eta", "guided"):
        kw.update(sigma=a["sigma"], noise=a["noise"])
    if "seeded" in variant:
        kw.update(sigma=a["sigma"], seeds=SEEDS)
    return nat.sample(a["z"], a["x_T"], a["ts"], a["coef"], **kw)


def entry(nat, variant, a, ws, scratch, hist, use_graph):
    """One direct call of the variant's own entry point; the result."""
    lib, out = nat.lib, torch.empty_like(a["x_T"])
    ms = variant.endswith("ms")
    ts, coef = (a["ms_ts"], a["ms_coef"]) if ms else (a["ts"], a["coef"])
    zn = (None,) if "guided" in variant else ()                    # z_null_dev NULL: zeros
    head = (nat.h, a["z"].data_ptr(), *zn, a["x_T"].data_ptr(), out.data_ptr(), B, S, S, len(ts), ts.ctypes.data, coef.ctypes.data)
    tail = (ws.ptr, ws.nbytes, _native.current_stream(torch.device(DEV)), use_graph)
    sigma, noise, seeds = a["sigma"].ctypes.data, a["noise"].data_ptr(), a["seeds"].data_ptr()
    own = {"plain": (lib.ccn_sample, ()),
           "eta": (lib.ccn_sample_eta, (sigma, noise)),
           "guided": (lib.ccn_sample_guided, (sigma, noise, W_G, scratch.data_ptr())),
           "seeded": (lib.ccn_sample_seeded, (sigma, seeds, scratch.data_ptr())),
           "guided_seeded": (lib.ccn_sample_guided_seeded, (sigma, seeds, W_G, scratch.data_ptr())),
           "ms": (lib.ccn_sample_ms, (hist.data_ptr(),)),
           "guided_ms": (lib.ccn_sample_guided_ms, (W_G, scratch.data_ptr(), hist.data_ptr()))}
    fn, mid = own[variant]
    with torch.cuda.device(DEV):
        _native.check(fn(*head, *mid, *tail))
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("variant,pred,thr", CASES)
def test_entry_equals_the_descriptor_route(nets, inputs, dtype, variant, pred, thr):
    nat = nets[dtype].native()
    captures = lambda: nat.lib.ccn_internal_graph_captures(nat.h)
    PB = 2 * B if "guided" in variant else B
    steps = len(inputs["ms_ts"] if variant.endswith("ms") else inputs["ts"])
    scratch = torch.empty((PB,) + SHAPE[1:], device=DEV)
    hist = torch.empty(SHAPE, device=DEV)
    try:
        nat.set_prediction(pred)
        ref = reference(nat, variant, inputs, thr)                  # (the handle keeps this run's dynamic threshold for the calls below)
        assert bool(torch.isfinite(ref).all())
        ws = nat.workspace(PB, S, S, steps, slot=1)
        before = captures()
        eager = entry(nat, variant, inputs, ws, scratch, hist, 0)
        assert captures() == before                                 # launch by launch: nothing is captured
        first = entry(nat, variant, inputs, ws, scratch, hist, 1)
        # the documented key (tables, addresses, w, the handle's prediction and threshold) is new on this workspace: one capture ...
        assert captures() == before + 1
        again = entry(nat, variant, inputs, ws, scratch, hist, 1)
        assert captures() == before + 1                             # ... and the same call again replays it
        torch.cuda.synchronize()
        nat.poll_errors()
        for name, got in (("launch by launch", eager), ("captured", first), ("replayed", again)):
            assert torch.equal(got, ref), (name, float((got - ref).abs().max()))
    finally:
        nat.set_prediction("eps")
        _native.check(nat.lib.ccn_set_dynamic_threshold(nat.h, 0.0, 0.0, None, 0))


def test_modes_change_the_result(nets, inputs):
    """The repeated cases are not the plain ones over again: v-prediction and the dynamic threshold each move the output."""
    nat = nets["fp32"].native()
    try:
        base = reference(nat, "guided_seeded", inputs, None)
        assert not torch.equal(reference(nat, "guided_seeded", inputs, THR_P), base)
        nat.set_prediction("v")
        assert not torch.equal(reference(nat, "guided_seeded", inputs, None), base)
    finally:
        nat.set_prediction("eps")
        _native.check(nat.lib.ccn_set_dynamic_threshold(nat.h, 0.0, 0.0, None, 0))
