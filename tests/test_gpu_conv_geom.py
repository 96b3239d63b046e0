"""Fixed-geometry instantiations of the persistent conv (csrc/ccn_conv_pr.hip, PrGeom) against its run-time instantiations.

The same operations run in the same order; only where the geometry operands come from differs.  So everything here is compared for
equality: one handle plans and launches with the instantiations allowed (conv variant 4, the default), a second one on the same
weights with them switched off (variant 5).  The model is the headline one (base 128, ch_mult (1,2,2)) at 256 px, kept small through
the batch.

Which layers match depends on the batch, because the plan's tile rows, its input-GroupNorm form and the kernel itself do
(conv_tile_rows / conv_route / conv_in_kernel_stats count tiles over the whole batch): from batch 4 up every 3x3, stride-2 and
ConvTranspose layer of this model takes the forms the instantiations are compiled for.  Batch 8 (the benchmark's) is therefore the case
that asserts "every layer"; at batch 1 and 2 the 128- and 64-pixel levels run 4-row tiles with a scale / shift table, the stride-2
convs leave the persistent kernel, so there the test asserts the layers that must match (the 256- and 32-pixel levels), and that
nothing matches whose route line differs from batch 8's.  The first conv of the 32-pixel level reads the sums of the stride-2 conv in
front of it: 4 slots per N tile from the persistent kernel's 8-row tiles at batch 8, 8 from the 4-row kernel that runs at batch 1 and
2 -- two instantiations, told apart by name.

The kernel word comes from ``ccn_internal_plan_kernels`` / ``_of``: the route report with the instantiation's name ("pr:...") in place
of "pr".  ``ccn_internal_plan_routes`` itself keeps its text (tests/test_gpu_infer_plan.py compares it with the parent commit's).
"""
import contextlib
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))
import infer_plan_cases as ipc  # noqa: E402
from clip_feature_codec import _native  # noqa: E402
from clip_feature_codec.diffusion.scheduler import NoiseScheduler  # noqa: E402
from clip_feature_codec.utils import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = ipc.DEV
PX = 256
HEADLINE = (128, (1, 2, 2))
GEOM_ON, GEOM_OFF = 4, 5                        # ccn_internal_set_conv_variant: persistent kernel with / without the instantiations
CONV_KINDS = ("C3S1", "C3S2", "CT4")
# batch 1 and 2: the levels whose launch forms do not depend on the batch (module docstring)
MATCH_AT_ANY_BATCH = {f"{blk}{sfx}" for blk in ("down.0", "down.1", "mid1", "mid2", "up.0", "up.1") for sfx in (".film", "")}


def _lib():
    lib = ipc.library()
    lib.ccn_internal_set_conv_variant.restype = ctypes.c_int
    lib.ccn_internal_set_conv_variant.argtypes = [ctypes.c_int]
    lib.ccn_internal_plan_kernels.restype = ctypes.c_int
    lib.ccn_internal_plan_kernels.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    lib.ccn_internal_plan_kernels_of.restype = ctypes.c_int
    lib.ccn_internal_plan_kernels_of.argtypes = [ctypes.c_void_p] + [ctypes.c_int32] * 4 + [ctypes.c_char_p, ctypes.c_size_t]
    return lib


@contextlib.contextmanager
def variant(v):
    """The switch is read when a plan is built (the report) and when a launch is issued or captured (the kernel)."""
    lib = _lib()
    old = lib.ccn_internal_set_conv_variant(v)
    try:
        yield
    finally:
        lib.ccn_internal_set_conv_variant(old)


def make_handle(base, ch_mult):
    nat = _native.NativeUNet(512, base, ch_mult, ipc.TIME_DIM, 3, dtype="bf16", device=DEV)
    nat.load_state_dict(synth.synth_state_dict(synth.unet_param_spec(512, base, ch_mult, ipc.TIME_DIM)))
    return nat


@pytest.fixture(scope="module")
def pair():
    """(handle used under variant 4, handle used under variant 5) of the headline model, same weights."""
    assert _lib().ccn_internal_set_conv_variant(GEOM_ON) == GEOM_ON, "the default variant allows the instantiations"
    on, off = make_handle(*HEADLINE), make_handle(*HEADLINE)
    yield on, off
    on.close()
    off.close()
    torch.cuda.empty_cache()


def kernels_of(nat, B, px=PX, steps=1):
    return ipc.parse_routes(ipc._report(_lib().ccn_internal_plan_kernels_of, nat.h, B, px, px, steps))


def conv_lines(routes):
    return {n: r for n, r in routes.items() if r["kind"] in CONV_KINDS}


def inputs(B):
    z = torch.from_numpy(synth.synth_z(B, seed=77)).to(DEV)
    x = torch.from_numpy(np.ascontiguousarray(synth.start_noise(range(B), PX, 300))).to(DEV)
    t = torch.linspace(0, 999, B).round().long().to(DEV)
    return z, x, t


def activation_shapes(nat, B):
    """(name, NCHW shape) of every activation a conv-family launch of the plan writes (the head writes the caller's tensor)."""
    sizes = {}
    for ln in ipc.layout_text(nat, B, PX, PX, 1).splitlines()[:-1]:
        name, _, nbytes = ln.split()
        sizes[name] = int(nbytes[len("bytes="):])
    out, H = [], PX
    for name, r in ipc.parse_routes(ipc.route_text_of(nat, B, PX, PX, 1)).items():
        if r["kind"] == "HEAD":
            continue
        H = H // 2 if r["kind"] == "C3S2" else (H * 2 if r["kind"] == "CT4" else H)
        C, rem = divmod(sizes[name], B * H * H * 2)
        assert rem == 0 and C > 0, (name, sizes[name], H)
        out.append((name, (B, C, H, H)))
    return out


@pytest.mark.parametrize("B", [1, 2, 8])
def test_forward_and_every_activation_are_bit_equal_with_and_without_the_instantiations(pair, B):
    on, off = pair
    z, x, t = inputs(B)
    eps_on = on.forward(x, z, t)
    with variant(GEOM_OFF):
        eps_off = off.forward(x, z, t)
    torch.cuda.synchronize()
    assert any(r["kernel"].startswith("pr:") for r in ipc.parse_routes(ipc._report(_lib().ccn_internal_plan_kernels, on.h)).values())
    assert not any(r["kernel"].startswith("pr:") for r in ipc.parse_routes(ipc._report(_lib().ccn_internal_plan_kernels, off.h)).values())
    assert torch.isfinite(eps_on).all()
    assert torch.equal(eps_on, eps_off)
    shapes = activation_shapes(on, B)
    assert len(shapes) == 35, len(shapes)                                   # stem, 14 ResBlocks x 2 convs, 3 stride-2, 3 ConvTranspose
    for name, shape in shapes:
        a, b = on.read_activation(name, shape), off.read_activation(name, shape)
        assert torch.equal(a, b), name
        del a, b
    on.poll_errors()                                                        # the handle's error word is 0 (raises otherwise)
    off.poll_errors()


@pytest.mark.parametrize("B", [1, 2])
def test_three_step_sample_graph_and_launch_by_launch_all_four_equal(pair, B):
    on, off = pair
    z, x, _ = inputs(B)
    sched = NoiseScheduler(1000, "cosine", DEV)
    ts, coef = sched.ddim_timesteps(3), sched.ddim_coefficients(3)[:, :4]
    outs = {"on graph": on.sample(z, x, ts, coef, use_graph=True), "on graph replay": on.sample(z, x, ts, coef, use_graph=True),
            "on launches": on.sample(z, x, ts, coef, use_graph=False)}
    with variant(GEOM_OFF):
        outs["off graph"] = off.sample(z, x, ts, coef, use_graph=True)
        outs["off graph replay"] = off.sample(z, x, ts, coef, use_graph=True)
        outs["off launches"] = off.sample(z, x, ts, coef, use_graph=False)
    torch.cuda.synchronize()
    ref = outs["off launches"]
    assert torch.isfinite(ref).all() and not torch.equal(ref, x)
    for k, v in outs.items():
        assert torch.equal(v, ref), k
    on.poll_errors()
    off.poll_errors()


def test_every_conv_layer_of_the_headline_model_runs_an_instantiation_at_the_benchmark_batch(pair):
    on, off = pair
    got = conv_lines(kernels_of(on, 8, steps=50))
    assert len(got) == 34
    for name, r in got.items():
        assert r["kernel"].startswith("pr:"), (name, r)
    with variant(GEOM_OFF):
        for B in (1, 2, 8):
            assert not any(r["kernel"].startswith("pr:") for r in kernels_of(off, B).values()), B
    # the plain route report does not change with the switch
    with variant(GEOM_OFF):
        plain_off = ipc.route_text_of(off, 8, PX, PX, 50)
    assert ipc.route_text_of(on, 8, PX, PX, 50) == plain_off
    assert "pr:" not in plain_off


@pytest.mark.parametrize("B", [1, 2])
def test_small_batches_match_only_the_batch_independent_levels(pair, B):
    on, _ = pair
    at8, atB = conv_lines(kernels_of(on, 8)), conv_lines(kernels_of(on, B))
    plain8 = ipc.parse_routes(ipc.route_text_of(on, 8, PX, PX, 1))
    plainB = ipc.parse_routes(ipc.route_text_of(on, B, PX, PX, 1))
    matched = {n for n, r in atB.items() if r["kernel"].startswith("pr:")}
    print(B, sorted(matched))
    assert MATCH_AT_ANY_BATCH <= matched, MATCH_AT_ANY_BATCH - matched
    for n in matched:
        assert plainB[n] == plain8[n], n                                   # same kernel, tile rows, split, N tiles, GroupNorm form
        if n == "mid1.film":                                                # (the layout of the stride-2 conv's sums: module docstring)
            assert (atB[n]["kernel"], at8[n]["kernel"]) == ("pr:c3.512x32.film", "pr:c3.512x32.film.s4")
        else:
            assert atB[n]["kernel"] == at8[n]["kernel"], n


@pytest.mark.parametrize("what,base,ch_mult,px", [("224 px", 128, (1, 2, 2), 224), ("base 64", 64, (1, 2, 2), PX), ("two levels", 128, (1, 2), PX)])
def test_other_models_and_sizes_run_the_run_time_instantiations(pair, what, base, ch_mult, px):
    """Selection is by exact match of the geometry, not by model: another size or width matches nothing.  The two-level model's first
    level IS the headline model's (128 channels at 256 px): its FiLM convs do not match (another FiLM row stride); its residual convs
    and the ConvTranspose back to 256 px (the headline model's up.8) -- whose instantiations fix nothing the two models differ in --
    do, and nothing else does."""
    nat = pair[0] if (base, ch_mult) == HEADLINE else make_handle(base, ch_mult)
    try:
        routes = kernels_of(nat, 1, px=px)
        assert conv_lines(routes)
        matched = {n for n, r in routes.items() if r["kernel"].startswith("pr:")}
        assert matched == ({"down.0", "down.1", "up.5"} if what == "two levels" else set()), (what, matched)
        assert not any(routes[n]["kernel"].endswith(".film") for n in matched)
    finally:
        if nat is not pair[0]:
            nat.close()
