"""ccn_psnr_ssim_f32 / ccn_psnr_ssim_u8 on the GPU against their exact-integer restatement (tests/score_ref.py) and the host metrics.

The kernel's tile is 16 x 64 window positions (SC_TY x SC_TX, 22 x 80 staged pixels): 45 x 141 and 45 x 144 give two full tiles plus a
ragged one in each direction, the second on the 16-byte access path (W % 16 == 0); the other shapes sit inside one tile.
SSE must be the int64 sum exactly.  SSIM: the kernel and the restatement differ in the order of an fp64 sum over at most a few
thousand quotients of magnitude at most 1 and share one fp64 division per position -- about 1e-13; the bound is 1e-10.
"""
import ctypes

import numpy as np
import pytest
import torch

import score_ref
from clip_feature_codec import _native

pytestmark = pytest.mark.gpu
DEV = "cuda"
SSIM_TOL = 1e-10
IDS = ["x".join(map(str, s)) for s in score_ref.SHAPES]
assert (score_ref.TILE_Y, score_ref.TILE_X) == (16, 64)
TILED = [(1, 3, 45, 141), (3, 1, 45, 144)]                         # > 2 * 16 + 6 rows, > 2 * 64 + 6 columns
assert all(s in score_ref.SHAPES for s in TILED)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.cpu().numpy().view(np.uint64)


def check_block(block, a, b, what):
    """(B,2) float64 from the device against the restatement and the host's per-plane mean."""
    sse, ssim = score_ref.score(a, b)
    host = score_ref.plane_mean_ssim(a, b)
    got = block.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (a.shape[0], 2)
    for i in range(a.shape[0]):
        print(f"{what}[{i}]: sse {got[i, 0]:.0f} (want {sse[i]}), ssim {got[i, 1]!r} (restated {ssim[i]!r}, host {host[i]!r})")
        assert got[i, 0] == float(sse[i]), (what, i)
        if np.isnan(ssim[i]):
            assert np.isnan(got[i, 1]) and np.isnan(host[i]), (what, i)
        else:
            assert abs(got[i, 1] - ssim[i]) <= SSIM_TOL and abs(got[i, 1] - host[i]) <= SSIM_TOL, (what, i)
    return got


def f32_image(a_u8, rng):
    """An fp32 image in the sampler's range whose conversion is interesting: values spread inside their uint8 cell, then some outside
    [-1, 1], some exactly +-1, and some on and just either side of a truncation boundary."""
    x = ((a_u8.astype(np.float64) + rng.uniform(0.05, 0.95, a_u8.shape)) / 127.5 - 1.0).astype(np.float32)
    flat = x.reshape(-1)
    n = flat.size
    pick = rng.permutation(n)
    k = max(n // 8, 1)
    flat[pick[:k]] = rng.uniform(-1.6, 1.6, k).astype(np.float32)
    flat[pick[k:k + 3]] = (1.0, -1.0, 0.0)[:len(pick[k:k + 3])]
    edge = (rng.integers(1, 255, k).astype(np.float64) / 127.5 - 1.0).astype(np.float32)     # (x + 1) * 127.5 next to an integer
    step = rng.integers(-1, 2, k)
    edge = np.where(step < 0, np.nextafter(edge, np.float32(-2)), np.where(step > 0, np.nextafter(edge, np.float32(2)), edge))
    sel = pick[k + 3:2 * k + 3]
    flat[sel] = edge[:len(sel)]
    return x


@pytest.mark.parametrize("shape", score_ref.SHAPES, ids=IDS)
def test_u8_entry_matches_reference(shape):
    for content in score_ref.CONTENTS:
        a, b = score_ref.images(shape, content)
        got = check_block(_native.psnr_ssim(dev(a), dev(b)), a, b, content)
        windows = shape[2] >= score_ref.WIN and shape[3] >= score_ref.WIN
        if content == "identical":
            assert (got[:, 0] == 0).all() and (not windows or (got[:, 1] == 1.0).all())
        if content == "checker" and windows:
            assert (got[:, 1] < 0).all()


@pytest.mark.parametrize("shape", score_ref.SHAPES, ids=IDS)
def test_f32_entry_converts_like_to_uint8_and_agrees_with_u8_entry(shape):
    rng = np.random.default_rng(sum(shape))
    a, b = score_ref.images(shape, "smooth")
    x = f32_image(a, rng)
    want_u8 = score_ref.to_uint8(x)
    from clip_feature_codec.eval.metrics import _to_uint8
    assert np.array_equal(want_u8, _to_uint8(x))
    xd, bd = dev(x), dev(b)
    out_u8 = torch.full(shape, 77, dtype=torch.uint8, device=DEV)
    blk = _native.psnr_ssim(xd, bd, recon_u8_out=out_u8)
    assert np.array_equal(out_u8.cpu().numpy(), want_u8)
    check_block(blk, want_u8, b, "f32")
    assert np.array_equal(bits(blk), bits(_native.psnr_ssim(out_u8, bd)))          # the u8 entry on the same images: the same bits
    assert np.array_equal(bits(blk), bits(_native.psnr_ssim(xd, bd)))              # without the byte output, and a second call


@pytest.mark.parametrize("shape", [(3, 3, 23, 37)] + TILED, ids=lambda s: "x".join(map(str, s)))
def test_record_bits_do_not_depend_on_the_batch(shape):
    rng = np.random.default_rng(5)
    a, b = score_ref.images(shape, "random")
    x = f32_image(a, rng)
    whole = bits(_native.psnr_ssim(dev(x), dev(b)))
    whole_u8 = bits(_native.psnr_ssim(dev(a), dev(b)))
    for i in range(shape[0]):
        assert np.array_equal(bits(_native.psnr_ssim(dev(x[i:i + 1]), dev(b[i:i + 1])))[0], whole[i])
        assert np.array_equal(bits(_native.psnr_ssim(dev(a[i:i + 1]), dev(b[i:i + 1])))[0], whole_u8[i])


@pytest.mark.parametrize("shape", [(3, 3, 23, 37), (1, 3, 9, 16)] + TILED, ids=lambda s: "x".join(map(str, s)))
def test_pointer_alignment_does_not_change_a_bit(shape):
    rng = np.random.default_rng(6)
    a, b = score_ref.images(shape, "smooth")
    x = f32_image(a, rng)
    n = x.size
    xd, bd = dev(x), dev(b)
    out = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    ref = bits(_native.psnr_ssim(xd, bd, recon_u8_out=out))
    # the originals one byte, the reconstruction four bytes and the byte output three bytes off a 16-byte boundary
    b_off = torch.empty(n + 16, dtype=torch.uint8, device=DEV)[1:n + 1].view(shape); b_off.copy_(bd)
    x_off = torch.empty(n + 4, dtype=torch.float32, device=DEV)[1:n + 1].view(shape); x_off.copy_(xd)
    out_off = torch.zeros(n + 16, dtype=torch.uint8, device=DEV)[3:n + 3].view(shape)
    assert b_off.data_ptr() % 16 == 1 and x_off.data_ptr() % 16 == 4 and xd.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0
    assert np.array_equal(bits(_native.psnr_ssim(x_off, b_off, recon_u8_out=out_off)), ref)
    assert torch.equal(out_off, out)
    assert np.array_equal(bits(_native.psnr_ssim(out_off, b_off)), ref)
    assert np.array_equal(bits(_native.psnr_ssim(xd, b_off)), ref) and np.array_equal(bits(_native.psnr_ssim(x_off, bd)), ref)


def test_bufs_are_used_and_sliced():
    shape = (3, 3, 23, 37)
    a, b = score_ref.images(shape, "random")
    out = torch.full((4, 2), -1.0, dtype=torch.float64, device=DEV)
    scratch = torch.empty(_native.score_scratch_bytes(4, 3, 23, 37), dtype=torch.uint8, device=DEV)
    got = _native.psnr_ssim(dev(a), dev(b), bufs=(out, scratch))
    assert got.data_ptr() == out.data_ptr() and got.shape == (3, 2)
    assert np.array_equal(bits(got), bits(_native.psnr_ssim(dev(a), dev(b)))) and float(out[3, 0]) == -1.0


def test_non_finite_input_is_documented_choice():
    x = torch.zeros((1, 1, 7, 7), dtype=torch.float32, device=DEV)
    x[0, 0, 0, :3] = torch.tensor([float("inf"), float("-inf"), float("nan")])
    out = torch.empty((1, 1, 7, 7), dtype=torch.uint8, device=DEV)
    _native.psnr_ssim(x, torch.zeros_like(out), recon_u8_out=out)
    assert out[0, 0, 0, :4].tolist() == [255, 0, 0, 127]


def test_psnr_ssim_device_wrapper():
    from clip_feature_codec.eval import metrics
    shape = (3, 3, 23, 37)
    a, b = score_ref.images(shape, "smooth")
    psnr, ssim = metrics.psnr_ssim_device(a, b)
    assert psnr.dtype == np.float64 and ssim.dtype == np.float64 and psnr.shape == ssim.shape == (3,)
    sse, want = score_ref.score(a, b)
    for i in range(3):
        assert abs(psnr[i] - metrics.psnr_u8(a[i], b[i])) <= 1e-4 and psnr[i] == metrics.psnr_from_sse(sse[i], a[i].size)
        assert abs(ssim[i] - want[i]) <= SSIM_TOL


def test_error_cases_return_einval():
    lib = _native.load_library()
    B, C, H, W = 1, 3, 9, 16
    x = torch.zeros((B, C, H, W), dtype=torch.float32, device=DEV)
    o = torch.zeros((B, C, H, W), dtype=torch.uint8, device=DEV)
    out = torch.zeros((B, 2), dtype=torch.float64, device=DEV)
    need = _native.score_scratch_bytes(B, C, H, W)
    scratch = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    st = _native.current_stream(x.device)
    EINVAL = 1

    def f32(xp, op, outp, dims, sp, sbytes):
        return lib.ccn_psnr_ssim_f32(xp, op, None, outp, *dims, sp, sbytes, st)

    def u8(xp, op, outp, dims, sp, sbytes):
        return lib.ccn_psnr_ssim_u8(xp, op, outp, *dims, sp, sbytes, st)

    good = (x.data_ptr(), o.data_ptr(), out.data_ptr(), (B, C, H, W), scratch.data_ptr(), need)
    assert f32(*good) == 0 and u8(o.data_ptr(), *good[1:]) == 0
    for call, first in ((f32, x.data_ptr()), (u8, o.data_ptr())):
        assert call(None, *good[1:]) == EINVAL
        assert call(first, None, *good[2:]) == EINVAL
        assert call(first, good[1], None, *good[3:]) == EINVAL
        assert call(first, good[1], good[2], good[3], None, need) == EINVAL
        for bad in ((0, C, H, W), (B, -1, H, W), (B, C, 0, W), (B, C, H, 0)):
            assert call(first, good[1], good[2], bad, good[4], need) == EINVAL
        assert call(first, good[1], good[2], good[3], good[4], need - 1) == EINVAL          # too small
        assert call(first, good[1], good[2], good[3], good[4] + 4, need) == EINVAL          # not 8-byte aligned
    assert b"" != lib.ccn_last_error()
    torch.cuda.synchronize()
