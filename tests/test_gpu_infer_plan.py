"""The inference plan (csrc/ccn_api.hip: ShapePlan, launch) against the library of the commit before it.

tests/golden/infer_plan_parent.json was recorded by running the parent commit's library (tests/golden/make_infer_plan_golden.py): per
shape its workspace size, its route report, its algorithmic work and -- the inference kernels are run-to-run deterministic -- SHA-256 of
what ccn_forward, ccn_sample (launch by launch, captured, replayed), ccn_sample_eta and ccn_resblock_forward wrote.  The plan must give
the same sizes and the same launches with the same arguments in the same order, so everything here is compared for equality.  The
sampler's tables come from the fixture (the host's libm stays out of it).  The layout report of the new hook is checked for what a bump
allocator must guarantee, and the two caches (plans per shape, bindings per workspace address) for what include/ccn_hip.h promises.
"""
import json
import sys
from pathlib import Path

import pytest
import torch

HERE = Path(__file__).resolve().parent
if str(HERE) not in sys.path:
    sys.path.insert(0, str(HERE))
import infer_plan_cases as ipc  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURE = json.loads((HERE / "golden" / "infer_plan_parent.json").read_text())


@pytest.fixture(scope="module", autouse=True)
def _handles():
    yield
    ipc.close_handles()


def test_fixture_covers_every_case_and_every_launch_form():
    assert set(FIXTURE["cases"]) == set(ipc.CASES)
    assert len(FIXTURE["commit"]) >= 7 and FIXTURE["device"]
    for cid, case in ipc.CASES.items():
        rec = FIXTURE["cases"][cid]
        assert rec["bytes"] > 0 and rec["routes"] and len(rec["work"]) == 2, cid
        assert ("sha256" in rec) == case["run"] == ("tables" in rec), cid
        if case["run"]:
            want = {"forward", "sample", "sample_graph"} | ({"sample_eta", "sample_eta_graph"} if case.get("eta") else set()) \
                | ({"resblock"} if case.get("resblock") else set())
            assert set(rec["sha256"]) == want, cid
            assert len(rec["tables"]["eta0"]["ts"]) == case["shape"][3], cid
    have = ipc.coverage(FIXTURE["cases"])
    assert all(have.values()), have
    steps9 = [c for c in ipc.CASES.values() if c["run"] and c["shape"][3] > 8 and c["model"][3] == "phases" and c["model"][0] == "bf16"]
    assert steps9, "no case wraps the weight version index"


@pytest.mark.parametrize("cid", list(ipc.CASES))
def test_sizes_routes_work_and_output_bits_equal_the_parents(cid):
    want = FIXTURE["cases"][cid]
    got = ipc.record(cid, want.get("tables"))
    print(cid, got["bytes"], got["work"], got.get("sha256"))
    assert got["bytes"] == want["bytes"]
    assert got["routes"].splitlines() == want["routes"].splitlines()
    assert got["work"] == want["work"]
    assert got.get("sha256") == want.get("sha256")


@pytest.mark.parametrize("cid", list(ipc.CASES))
def test_layout_regions_are_named_aligned_disjoint_and_inside_the_total(cid):
    B, H, W, steps = ipc.CASES[cid]["shape"]
    nat = ipc.handle(ipc.CASES[cid]["model"])
    lines = ipc.layout_text(nat, B, H, W, steps).splitlines()
    assert lines[-1].startswith("total=")
    total = int(lines[-1][len("total="):])
    regions = []
    for ln in lines[:-1]:
        name, off, nbytes = ln.split()
        regions.append((name, int(off[len("off="):]), int(nbytes[len("bytes="):])))
    assert len(regions) > 20, len(regions)
    assert len({r[0] for r in regions}) == len(regions), "region names must be unique"
    assert all(off % 256 == 0 for _, off, _ in regions)
    spans = sorted((off, off + n, name) for name, off, n in regions)
    for (a0, a1, an), (b0, b1, bn) in zip(spans, spans[1:]):
        assert a1 <= b0, (an, bn)
    assert spans[-1][1] <= total
    assert total == ipc.workspace_bytes(nat, B, H, W, steps)


def test_two_workspaces_share_one_plan_and_give_the_same_bits():
    cid = "bf16-128-122-2x64x64"
    B, H, W, steps = ipc.CASES[cid]["shape"]
    nat = ipc.handle(ipc.CASES[cid]["model"])
    ts, coef5 = ipc.tables_from_bits(FIXTURE["cases"][cid]["tables"]["eta0"])
    z, x, _ = ipc.inputs(cid)
    before = ipc.layout_text(nat, B, H, W, steps)
    outs = [ipc.digest(nat.sample(z, x, ts, coef5[:, :4], use_graph=g, slot=slot)) for slot in (0, 1) for g in (False, True)]
    assert nat.workspace(B, H, W, steps, 0).ptr != nat.workspace(B, H, W, steps, 1).ptr
    assert set(outs) == {FIXTURE["cases"][cid]["sha256"]["sample"]}, outs
    assert ipc.layout_text(nat, B, H, W, steps) == before
    nat.poll_errors()


def test_size_and_work_queries_do_not_change_the_last_used_plan():
    cid = "bf16-48-12-2x32x32"
    B, H, W, _ = ipc.CASES[cid]["shape"]
    nat = ipc.handle(ipc.CASES[cid]["model"])
    z, x, t = ipc.inputs(cid)
    nat.forward(x, z, t)
    routes = ipc.route_text(nat)
    act = nat.read_activation("down.2", (B, 48, H // 2, W // 2)).cpu()
    assert ipc.workspace_bytes(nat, 1, 64, 96, 5) != ipc.workspace_bytes(nat, B, H, W, 1)
    nat.algorithmic_work(1, 64, 96)
    ipc.layout_text(nat, 1, 64, 96, 5)
    ipc.route_text_of(nat, 1, 64, 96, 5)
    assert ipc.route_text(nat) == routes
    # (shape 2's down.2 has three times the elements: reading it into this buffer would be refused)
    assert torch.equal(nat.read_activation("down.2", (B, 48, H // 2, W // 2)).cpu(), act)
