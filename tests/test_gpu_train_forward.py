"""The bf16 training forward, layer by layer, against float64 recomputations from the exact operands each kernel consumed.

The backward half of the bf16 step is pinned kernel by kernel (tests/test_gpu_train_kernels.py, tests/test_gpu_dgrad.py), starting from
the tensors the forward pass wrote.  This file pins those tensors.  Per case one ``trainer.forward`` runs on the GPU; the forward part
of its workspace is copied to the host once and replayed by tests/train_forward_ref.py:

  (a) every conv layer (stem, both convs of every ResBlock, stride-2 convs, ConvTransposes, the head into eps) within the inference
      replay's element-wise rounding bound, with its three wrong references rejected on at least MIN_VIOLATED of the outputs they change;
  (b) every activated copy ``.xa`` / ``.ya`` within the flip width of the float64 GroupNorm + SiLU of its raw input, and of the same
      transform with the device's own table -- in the side forms the only check that the tensor the weight-gradient kernel reads is the
      function the conv applied;
  (c) every ``.st`` / ``.ab`` table, out_norm's included, against float64 statistics of the stored input (train_forward_ref.table_bounds:
      an rstd bound of 2^-10.1 to 2^-11.9 relative on T1, T2 and T4, to 2^-9.2 on T3's 180-pixel middle; 2^-8 on the one or two tables
      per case that the persistent kernel's bias-only stride-2 epilogue feeds, whose rounding the statistics do not see is one number
      per channel and binade), and ``.ab`` against ``.st`` of the same norm to fp32 roundoff;
  (d) the conditioning regions temb, t1, tp, zpv, h, film against oracle/ref_unet's formulas in float64;
  (e) the routes and forward-norm forms the shape matrix reaches, as the library reports them, against ROUTES_TRAIN_BF16 /
      NORM_FORMS_TRAIN_BF16;
  (f) T1 and T2 once more under ``set_graph(True)``: the main-stream pre-pass forms over the same planned regions, replayed on their
      own, and compared with the default (side-stream) run.

Measured on an MI355X (docs/EXPERIMENTS.md R25): conv layers at most 0.999 of their bound (the stem, whose only rounding is the
store), wrong references rejected on at least 0.83 of the outputs they change; activated copies at most one flip (ratio 1.000) against
either transform, padded statistics rejected on at least 0.75; tables at most 0.60, ``.ab`` against ``.st`` 0.57 of 4 u; conditioning
at most 0.28 (temb).  A library whose rstd is 0.1 % too large fails test_norm_tables in all six runs.

Not reached: the ResBlock ``prologue`` form (the pre-pass kernel refuses more than 256 sixteen-byte slices per pixel: ``r.C / 8 > 256``,
a level of more than 2048 channels; no network is built for it -- out_norm reaches ``prologue``, as test_gpu_train_routes.py says of
the same form in fp32) and the free-running kernel on 3x3 convs (8-row tiles at a width the persistent kernel does not take: one more
batch-3 case at 136 x 200 px; its ConvTranspose form is reached by T4).
"""
import ctypes
import sys
import time
from pathlib import Path

import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))
import train_forward_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIME_DIM = 256
CH_MULT = (1, 2)      # two stride-2 convs: levels at H x W and H/2 x W/2 of `base` channels, the middle at H/4 x W/4 of 2 x base

# id -> (base, B, H, W); confirmed with the route hook (the reports are in docs/EXPERIMENTS.md)
CASES = {
    # 3x3 on the persistent kernel, 8-row tiles at level 0 (4 x 17 x 4 = 272 tiles) with a partial row tile (132 = 16 x 8 + 4) and a
    # partial column tile (104 = 3 x 32 + 8), 4-row tiles at 66 x 52 (128 ch) and 33 x 26 (256 ch, two N tiles).  The first stride-2 conv
    # on the persistent kernel with 4 x 9 x 2 = 72 eight-row tiles (training's window 64..127); both ConvTransposes on its 8-row form, the
    # one at 33 x 26 (4 x 5 x 1 x 4 = 80 tiles) where conv_tile_rows alone gives 4.  side-stats+act (68 slots at level 0: the consumer
    # reduces at most 64 itself) and side-fused.  stem2, head2.
    "T1": (128, 4, 132, 104),
    # batch 2: 3x3 on the persistent kernel's 4-row tiles on every level (2 x 17 x 4 = 136 < 256); side-stats+act with 132 slots;
    # stride-2 convs on igemm at 128-wide N tiles (36 and 20 eight-row tiles); ConvTranspose on ws (40 tiles) and forced onto the
    # persistent kernel's 8-row form (2 x 9 x 2 x 4 = 144 tiles, conv_tile_rows gives 4)
    "T2": (128, 2, 132, 104),
    # no fragment operands: igemm at 48 channels (BN 32, GroupNorm groups of 6 channels straddling the N tiles), ws at 96; generic stem
    # and head; igemm stride-2 conv and ConvTranspose; the pre-pass `fused` form everywhere
    "T3": (48, 3, 40, 72),
    # 238 partial-sum slots at level 0: the separate statistics launch (`stats+act`) on the main stream; ws at BN 64; the ConvTranspose
    # on the free-running kernel's 8-row tiles at BN 64; the 128-channel middle on the persistent kernel (side-fused)
    "T4": (64, 2, 136, 200),
}
RUNS = [(c, False) for c in CASES] + [("T1", True), ("T2", True)]      # (case, set_graph)
RUN_IDS = [c + ("-graph" if g else "") for c, g in RUNS]

# Every (kind, kernel, th) the bf16 training forward launches over RUNS, read off conv_route under Planner::route's policy
# {pr, s2_min_tiles8 = 64, ct_like_s2, no split-K} and conv_kernel_for; one entry per reachable route, the case that reaches it
ROUTES_TRAIN_BF16 = {
    ("STEM", "stem2", 4),      # T1, T2, T4 (64 and 128 channels)
    ("STEM", "igemm", 4),      # T3: 48 is not a stem2 width
    ("C3S1", "pr", 8),         # T1 level 0
    ("C3S1", "pr", 4),         # T1 deeper levels, T2 every level, T4's middle
    ("C3S1", "ws", 4),         # T3's 96-channel middle, T4 at 64 channels (BN 64)
    ("C3S1", "igemm", 4),      # T3 at 48 channels (BN 32)
    ("C3S2", "pr", 8),         # T1 down.2: 72 eight-row tiles, the window only training takes (inference: more than 128)
    ("C3S2", "igemm", 4),      # T1 down.5 (20 tiles x 2 N tiles = 40), T2, T3, T4
    ("CT4", "pr", 8),          # T1 up.2 and T2 up.5: forced to 8 rows where conv_tile_rows gives 4 (ct_like_s2); T1 up.5
    ("CT4", "ws", 4),          # T2 up.2 (40 tiles), T4 up.2
    ("CT4", "igemm", 4),       # T3 (BN 32)
    ("CT4", "fr", 8),          # T4 up.5: 8-row tiles (2 x 9 x 4 x 4 = 288) at BN 64, which the persistent kernel does not take
    ("HEAD", "head2", 0),      # T1, T2, T4 (Step::forward notes head2 without a tile geometry)
    ("HEAD", "igemm", 4),      # T3
}
# Step::forward / norm_fwd / norm_conv_fwd_side
NORM_FORMS_TRAIN_BF16 = {
    "side-fused",              # T1, T2, T4: both convs on the persistent kernel, at most 64 slots per group
    "side-stats+act",          # T1 level 0 (68 slots), T2 level 0 (132)
    "fused",                   # T3; T4 below level 0; T1-graph, T2-graph (a capture takes no side stream)
    "stats+act",               # T4 level 0 (238 slots > 128); T2-graph level 0 (132)
    "prologue",                # out_norm, every case (the ResBlock form needs more than 2048 channels: module docstring)
}

_RUN = {}


def hook_text(fn, *args):
    fn.restype = ctypes.c_int
    n = fn(*args, None, 0)
    assert n > 0
    buf = ctypes.create_string_buffer(n + 1)
    assert fn(*args, buf, n + 1) == n
    return buf.value.decode()


def inputs(cid):
    from clip_feature_codec.utils import synth
    base, B, H, W = CASES[cid]
    sd = synth.synth_state_dict(synth.unet_param_spec(512, base, CH_MULT))
    g = torch.Generator("cpu").manual_seed(2000 + int(cid[1:]))
    x = torch.randn((B, 3, H, W), generator=g)
    z = torch.from_numpy(synth.synth_z(B))
    t = torch.linspace(0, 999, B).round().long()
    return sd, x, z, t


def run(cid, graph):
    """one forward call of one case, replayed once: everything the tests below look at"""
    key = (cid, graph)
    if key in _RUN:
        return _RUN[key]
    from clip_feature_codec import _native
    from clip_feature_codec.models.unet import CLIPCondUNet
    base, B, H, W = CASES[cid]
    sd, x, z, t = inputs(cid)
    L = _native.load_library()
    L.ccn_internal_train_routes.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    L.ccn_internal_train_layout.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p, ctypes.c_size_t]
    net = CLIPCondUNet(z_dim=512, base=base, ch_mult=CH_MULT, time_dim=TIME_DIM, dtype="bf16").to(DEV)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    st = net.train().train_state()
    tr, flat = st.trainer, st.fp.flat
    if graph:
        tr.set_graph(True)
    t0 = time.perf_counter()
    eps = tr.forward(flat, x.to(DEV), z.to(DEV), t.to(DEV))
    torch.cuda.synchronize()
    routes = hook_text(L.ccn_internal_train_routes, tr.h).splitlines()
    layout = hook_text(L.ccn_internal_train_layout, tr.h, B, H, W)
    ws = tr.workspace(B, H, W)
    shift = ws.ptr - ws.buf.data_ptr()
    fwd_bytes = R.parse_layout(layout)[0]["dfilm"][0]               # the backward's regions follow the forward's in planning order
    raw = ws.buf[shift:shift + fwd_bytes].cpu()                     # the one copy
    eps = eps.cpu()
    gpu_s = time.perf_counter() - t0
    del net, st, tr, ws
    torch.cuda.empty_cache()
    out = R.replay(R.Regions(layout, raw), routes, sd, base, CH_MULT, B, H, W, x, z, t, eps, TIME_DIM,
                   f"{cid}{' set_graph' if graph else ''} base {base} {B}x{H}x{W}", rng_seed=B + H, keep=cid in ("T1", "T2"))
    out["route_lines"] = [ln for ln in routes if ln.startswith(("conv fwd", "norm"))]
    print(f"{cid}{'-graph' if graph else ''}: forward + copy {gpu_s:.2f} s, replay {time.perf_counter() - t0 - gpu_s:.1f} s")
    _RUN[key] = out
    return out


@pytest.mark.parametrize("cid,graph", RUNS, ids=RUN_IDS)
def test_conv_layers(cid, graph):
    """(a): max |got - ref| / bound <= 1 for every conv layer, and every wrong reference (a zeroed tap, a column shift inside the last
    column tile, padded statistics) outside the bound on at least MIN_VIOLATED of the outputs it changes."""
    from test_gpu_layer_replay import check_rows
    rows = run(cid, graph)["rows"]
    assert len(rows) == 2 + 2 * 10 + 4                              # stem, head, ten ResBlocks, two stride-2 convs, two ConvTransposes
    check_rows(rows)


@pytest.mark.parametrize("cid,graph", RUNS, ids=RUN_IDS)
def test_activated_copies(cid, graph):
    """(b): every .xa / .ya element is a bf16 value within the flip width of the float64 transform of the raw input region."""
    acts = run(cid, graph)["acts"]
    assert len(acts) == 20
    R.check_act_rows(acts)


@pytest.mark.parametrize("cid,graph", RUNS, ids=RUN_IDS)
def test_norm_tables(cid, graph):
    """(c): every .st / .ab table against float64 statistics of the stored input region."""
    tables = run(cid, graph)["tables"]
    assert len(tables) == 21
    R.check_table_rows(tables)


@pytest.mark.parametrize("cid,graph", RUNS, ids=RUN_IDS)
def test_conditioning(cid, graph):
    """(d): temb within 2e-4 of the CPU's; t1, tp, zpv, h and film within ETA_COND (sum |W||x| + |b|) of float64."""
    R.check_cond_rows(run(cid, graph)["cond"])


def test_route_coverage():
    """(e): the union of the route reports is exactly ROUTES_TRAIN_BF16 and NORM_FORMS_TRAIN_BF16; every route has a rounding model."""
    from test_gpu_layer_replay import ROUNDING
    seen, forms = set(), set()
    for (cid, graph), rid in zip(RUNS, RUN_IDS):
        out = run(cid, graph)
        k, f = R.route_keys(out["routes"])
        seen |= k; forms |= f
        print(f"\n{rid}:\n  " + "\n  ".join(out["route_lines"]))
    for kind, kernel, th in seen:
        assert (kernel, 1) in ROUNDING or (kind == "HEAD" and kernel == "igemm"), (kind, kernel, th)
    assert seen == ROUTES_TRAIN_BF16, (sorted(ROUTES_TRAIN_BF16 - seen), sorted(seen - ROUTES_TRAIN_BF16))
    assert forms == NORM_FORMS_TRAIN_BF16, (sorted(NORM_FORMS_TRAIN_BF16 - forms), sorted(forms - NORM_FORMS_TRAIN_BF16))


@pytest.mark.parametrize("cid", ["T1", "T2"])
def test_stream_settings_agree(cid):
    """(f): the side forms (default) and the main-stream pre-pass forms (set_graph) write the same planned regions.  Tables: where
    both runs read the same stored input they reduce the same partial sums, in float64, in another order: they agree to fp32
    roundoff (4 u of the entry; for c of |beta| + |mean a|).  Where the inputs differ (a flipped operand upstream changes the tensors
    downstream) each run is within its bound of (c) of its own reference.  Activated copies: they differ only where one run's width
    around the transform with its own table is non-zero, or the tables or the raw inputs themselves differ."""
    a, b = run(cid, False), run(cid, True)
    fa, fb = R.route_keys(a["routes"])[1], R.route_keys(b["routes"])[1]
    assert fa & {"side-fused", "side-stats+act"} and not fb & {"side-fused", "side-stats+act"}, (fa, fb)
    worst, same_in = 0.0, 0
    for ta, tb in zip(a["tables"], b["tables"]):
        assert ta["name"] == tb["name"]
        if not all(bool((ta["ref"][k] == tb["ref"][k]).all()) for k in ta["got"]):
            continue
        same_in += 1
        cpg = ta["got"]["a"].shape[1] // ta["got"]["mean"].shape[1]
        scale = dict(ta["ref"], c=(ta["ref"]["c"] + ta["ref"]["mean"].repeat_interleave(cpg, 1) * ta["ref"]["a"]).abs()
                     + (ta["ref"]["mean"].repeat_interleave(cpg, 1) * ta["ref"]["a"]).abs())
        for k in ta["got"]:
            r = float(((ta["got"][k] - tb["got"][k]).abs() / (4 * R.U32 * scale[k].abs() + 1e-300)).max())
            worst = max(worst, r)
            assert r <= 1.0, (ta["name"], k, r)
    assert same_in >= 1                                              # at least the first norm reads the same tensor in both runs
    n_diff = n_all = n_wide = 0
    for xa, xb, ta, tb in zip(a["acts"], b["acts"], [t for t in a["tables"] if t["name"] != "out_norm"],
                              [t for t in b["tables"] if t["name"] != "out_norm"]):
        assert xa["name"] == xb["name"] and xa["name"].startswith(ta["name"][:-3])
        tab_differs = ((ta["got"]["a"] != tb["got"]["a"]) | (ta["got"]["c"] != tb["got"]["c"]))[:, :, None, None]
        differ = xa["got"] != xb["got"]
        assert bool((~differ | xa["wide"] | xb["wide"] | tab_differs | (xa["x"] != xb["x"])).all()), xa["name"]
        n_diff += int(differ.sum()); n_all += differ.numel(); n_wide += int((xa["wide"] | xb["wide"]).sum())
    print(f"{cid}: {same_in} tables read the same input in both stream settings, worst ratio to 4 u {worst:.3f}; activated copies that "
          f"differ: {n_diff} of {n_all} ({n_wide} with a non-zero own-table width)")
