"""The record-keyed noise source without a GPU: the numpy reference (tests/rng_ref.py) against the Random123 known answers, the
exactness of its uniforms in fp32, the moments and independence of its normals, and the device header's integer core
(csrc/ccn_philox.h), compiled by the host compiler into tools/philox_words.cpp, against the reference word for word."""
import os
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import rng_ref  # noqa: E402

REPO = Path(__file__).resolve().parent.parent
CSRC = REPO / "clip-neural-image-conpression_amd" / "csrc"

KAT = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_known_answers():
    for ctr, key, want in KAT:
        assert _hex(rng_ref.philox4x32_10(ctr, key)) == want


def test_counter_and_key_layout():
    """A draw's key is the two halves of the seed, its counter (q, d, 0, 0); a negative seed is its two's-complement bits."""
    s = (0x299F31D0 << 32) | 0xA4093822
    assert _hex(rng_ref.draw_words(s, 7, [11])[0]) == _hex(rng_ref.philox4x32_10((11, 7, 0, 0), (0xA4093822, 0x299F31D0)))
    assert np.array_equal(rng_ref.draw_words(-1, 0, [0, 1]), rng_ref.draw_words(2 ** 64 - 1, 0, [0, 1]))
    assert rng_ref.seed_bits(-(2 ** 63) + 5) == 2 ** 63 + 5


def test_uniforms_are_exact_in_fp32_and_inside_the_unit_interval():
    words = np.concatenate([rng_ref.draw_words(99, 3, np.arange(4096)).reshape(-1), np.array([0, 0x1FF, 0x200, 0xFFFFFFFF], dtype=np.uint32)])
    u = rng_ref.uniforms(words)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)            # representable: fp32 holds the same numbers
    # ... and fp32 arithmetic in the kernel's order reaches them without rounding
    f = ((words >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    assert f.dtype == np.float32 and np.array_equal(f.astype(np.float64), u)
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24
    assert np.sqrt(-2.0 * np.log(u.min())) <= 5.77                               # the range of a normal


def test_moments():
    n = rng_ref.normal_record(99, 3, 3 * 256 * 256)
    mean, var = n.mean(), n.var()
    kurt = ((n - mean) ** 4).mean() / var ** 2
    print(f"mean {mean:.4f} var {var:.4f} kurtosis {kurt:.4f} max |n| {np.abs(n).max():.3f}")
    assert abs(mean) < 0.01 and abs(var - 1.0) < 0.01 and abs(kurt - 3.0) < 0.05
    assert np.isfinite(n).all() and np.abs(n).max() <= 5.77


def test_seeds_and_draws_are_uncorrelated():
    a, b = rng_ref.normal_record(5, 0, 768), rng_ref.normal_record(6, 0, 768)
    c = rng_ref.normal_record(5, 1, 768)
    r_seed, r_draw = np.corrcoef(a, b)[0, 1], np.corrcoef(a, c)[0, 1]
    print(f"correlation across seeds {r_seed:.4f}, across draws {r_draw:.4f}")
    assert abs(r_seed) < 0.05 and abs(r_draw) < 0.05


def test_prefix_property():
    """Element j does not depend on the record's length: a shorter record is a prefix (what lets a tail go element by element)."""
    full = rng_ref.normal_record(2 ** 63 + 5, 1, 768)
    assert np.array_equal(rng_ref.normal_record(2 ** 63 + 5, 1, 105), full[:105])
    assert np.array_equal(rng_ref.normal_fill([3, 2 ** 63 + 5], 768, 1)[1], full)


def _host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_device_header_integer_core(tmp_path):
    """csrc/ccn_philox.h through a host compiler, on its own: the known answers, and the words of a few hundred (seed, draw, q)."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.fail("no host C++ compiler (CXX, c++, g++, clang++) to build tools/philox_words.cpp with")
    exe = tmp_path / "philox_words"
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", str(CSRC), str(REPO / "tools" / "philox_words.cpp"), "-o", str(exe)], check=True)
    kat = subprocess.run([str(exe), "kat"], check=True, capture_output=True, text=True).stdout.split("\n")
    assert [line.strip() for line in kat if line.strip()] == [want for _, _, want in KAT]
    groups = [(0, 0, 0, 40), (2 ** 32 - 1, 1, 0, 40), (2 ** 63 + 5, 7, 190, 40), (99, 3, 49000, 40), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 20, 40),
              (0x123456789ABCDEF0, 51, 2 ** 31 - 20, 40)]
    args = [str(v) for g in groups for v in g]
    lines = [line for line in subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True).stdout.split("\n") if line.strip()]
    assert len(lines) == sum(g[3] for g in groups) == 240
    k = 0
    for seed, draw, q0, nq in groups:
        q = (q0 + np.arange(nq, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
        ref = rng_ref.draw_words(seed, draw, q)
        for i in range(nq):
            left, right = lines[k].split(":")
            assert [int(v) for v in left.split()] == [seed, draw, int(q[i])]
            assert right.strip() == _hex(ref[i]), (seed, draw, int(q[i]))
            k += 1


def test_capped_sigma_table():
    """``ddim_coefficients(..., cap_sigma=True)``, the seeded samplers' table: the default table bit for bit wherever that is real, and
    on the rows where the reference's sqrt(ab_s - sigma^2) is NaN sigma = sqrt(ab_s) with a zero direction coefficient."""
    from clip_feature_codec.diffusion.scheduler import NoiseScheduler
    for schedule, steps, eta in (("cosine", 6, 0.03), ("cosine", 50, 0.5), ("linear", 6, 0.03), ("cosine", 6, 0.001), ("cosine", 10, 0.0)):
        sch = NoiseScheduler(1000, schedule, device="cpu")
        ref, cap = sch.ddim_coefficients(steps, eta), sch.ddim_coefficients(steps, eta, cap_sigma=True)
        bad = np.isnan(ref[:, 3])
        assert np.isfinite(cap).all()
        assert np.array_equal(cap[~bad].view(np.uint32), ref[~bad].view(np.uint32))
        assert np.array_equal(cap[bad][:, :3].view(np.uint32), ref[bad][:, :3].view(np.uint32))
        assert (cap[bad][:, 3] == 0).all() and np.array_equal(cap[bad][:, 4], ref[bad][:, 2]) and (cap[bad][:, 4] < ref[bad][:, 4]).all()
        assert bad.any() == ((schedule, eta) in (("cosine", 0.03), ("cosine", 0.5)))
