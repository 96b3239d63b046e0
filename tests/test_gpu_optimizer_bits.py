"""The optimiser tail bit for bit against what an earlier commit's library computed (tests/golden/optimizer_steps.npz, made by
tests/golden/make_optimizer_golden.py from the commit the fixture names): plain, guarded and EMA steps share one AdamW kernel and
cannot check one another, so the recorded bits are the reference.  The script, its modes and its cases are tests/optimizer_bits.py's."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "clip-neural-image-conpression_amd"), str(ROOT / "tests")]

import optimizer_bits as ob  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(ROOT / "tests" / "golden" / "optimizer_steps.npz", allow_pickle=False)


def test_the_fixture_covers_the_script():
    assert len(GOLD["ids"]) == 51 and {f"1033-11111-{m}" for m in ob.MODES} <= set(GOLD["ids"])      # 9 shapes x 6 modes - 3
    assert list(GOLD["ids"]) == ob.IDS and list(GOLD["buffers"]) == list(ob.BUFFERS)
    assert GOLD["sha256"].shape == (len(ob.CASES), ob.STEPS, len(ob.BUFFERS), 32)
    assert len(str(GOLD["commit"])) >= 7 and str(GOLD["device"])          # where the bits come from
    assert sorted(k for k in GOLD.files if k.startswith("final/")) == sorted("final/" + ob.case_id(*c) for c in ob.CASES if c[0] <= ob.KEEP_ARRAYS_UP_TO)


def _where(got, want):
    """First differing element of every final array that differs (cases whose arrays are stored)."""
    out = []
    for name, a, b in zip(ob.BUFFERS, got.view(np.uint32), want.view(np.uint32)):
        bad = np.flatnonzero(a != b)
        if bad.size:
            i = int(bad[0])
            out.append(f"{name}[{i}]: {a.view(np.float32)[i]!r} != {b.view(np.float32)[i]!r} ({bad.size} of {a.size} differ)")
    return out


@pytest.mark.parametrize("n,off,mode", ob.CASES, ids=ob.IDS)
def test_same_bits_as_the_recorded_library(n, off, mode):
    i = ob.IDS.index(ob.case_id(n, off, mode))
    digests, finals, blocks = ob.run(n, off, mode)
    want = GOLD["sha256"][i]
    bad = [(step + 1, ob.BUFFERS[k]) for step in range(ob.STEPS) for k in range(len(ob.BUFFERS)) if not np.array_equal(digests[step, k], want[step, k])]
    detail = _where(finals, GOLD["final/" + ob.IDS[i]]) if bad and finals is not None else []
    assert not bad, (f"(step, buffer) whose SHA-256 differs from commit {GOLD['commit']}'s: {bad}", detail, blocks.tolist(), GOLD["blocks"][i].tolist())
    assert np.array_equal(blocks, GOLD["blocks"][i])
    if finals is not None:
        assert np.array_equal(finals.view(np.uint32), GOLD["final/" + ob.IDS[i]].view(np.uint32))
