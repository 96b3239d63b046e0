"""What ccn_psnr_ssim_{f32,u8} compute, restated in exact integers and float64 (numpy), and the images the score tests share.

The five 7 x 7 window sums come from a 2-D cumulative sum in int64, the variances from ``49 Saa - Sa^2`` and its siblings, and only the
quotient per window position and the mean over positions are floating point:

    ssim = ((2 Sa Sb + 49^2 c1) (2 Nab + 48 49 c2)) / ((Sa^2 + Sb^2 + 49^2 c1) (Na + Nb + 48 49 c2))

which is ``eval/metrics.py:_ssim_plane`` with numerator and denominator scaled by the same powers of 49 and 48.
"""
import numpy as np

WIN = 7
TILE_Y, TILE_X = 16, 64            # window positions per workgroup of score_partial_kernel (SC_TY, SC_TX in csrc/ccn_metrics.hip)
C1, C2 = (0.01 * 255.0) * (0.01 * 255.0), (0.03 * 255.0) * (0.03 * 255.0)
K1, K2 = C1 * 2401.0, C2 * 2352.0

# (B, C, H, W): one window; a few; no window (NaN SSIM, SSE still exact) in either direction; odd sizes inside one tile; two full tiles
# plus a ragged remainder in both directions (39 x 135 positions); the same with W % 16 == 0, where the kernel's 16-byte path runs
# (39 x 138 positions), and a small shape on that path
SHAPES = [(1, 1, 7, 7), (1, 3, 8, 9), (3, 1, 6, 20), (1, 3, 20, 5), (3, 3, 23, 37), (1, 3, 45, 141), (3, 1, 45, 144), (1, 3, 9, 16)]
CONTENTS = ("random", "identical", "const", "checker", "smooth")


def to_uint8(x: np.ndarray) -> np.ndarray:
    """eval/metrics.py:_to_uint8 on an fp32 array: two rounded fp32 operations, clip, truncation."""
    x = np.asarray(x, dtype=np.float32)
    return ((x + np.float32(1.0)) * np.float32(127.5)).clip(0, 255).astype(np.uint8)


def box_sums(p: np.ndarray) -> np.ndarray:
    """Sums of every WIN x WIN window that lies inside the (H, W) int64 plane: (H-6, W-6), empty if there is none."""
    H, W = p.shape
    if H < WIN or W < WIN:
        return np.zeros((max(H - WIN + 1, 0), max(W - WIN + 1, 0)), dtype=np.int64)
    c = np.zeros((H + 1, W + 1), dtype=np.int64)
    c[1:, 1:] = p.cumsum(0).cumsum(1)
    return c[WIN:, WIN:] - c[:-WIN, WIN:] - c[WIN:, :-WIN] + c[:-WIN, :-WIN]


def ssim_positions(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The SSIM quotient at every window position of one uint8 plane pair, float64."""
    a = a.astype(np.int64); b = b.astype(np.int64)
    sa, sb, saa, sbb, sab = box_sums(a), box_sums(b), box_sums(a * a), box_sums(b * b), box_sums(a * b)
    na, nb, nab = 49 * saa - sa * sa, 49 * sbb - sb * sb, 49 * sab - sa * sb
    assert max(np.abs(x).max(initial=0) for x in (2 * sa * sb, sa * sa + sb * sb, na + nb, 2 * nab)) < 2 ** 31   # the kernel's int32
    num = ((2 * sa * sb).astype(np.float64) + K1) * ((2 * nab).astype(np.float64) + K2)
    den = ((sa * sa + sb * sb).astype(np.float64) + K1) * ((na + nb).astype(np.float64) + K2)
    return num / den


def score(a_u8: np.ndarray, b_u8: np.ndarray):
    """(sse int64 (B,), ssim float64 (B,)) of two (B,C,H,W) uint8 batches; SSIM is NaN where no window fits."""
    B, C = a_u8.shape[:2]
    d = a_u8.astype(np.int64) - b_u8.astype(np.int64)
    sse = (d * d).reshape(B, -1).sum(1)
    ssim = np.full(B, np.nan)
    for i in range(B):
        pos = np.stack([ssim_positions(a_u8[i, c], b_u8[i, c]) for c in range(C)])
        if pos.size:
            ssim[i] = pos.sum() / float(pos.size)
    return sse, ssim


def images(shape, content: str, seed: int = 0):
    """A (recon_u8, orig_u8) pair of uint8 (B,C,H,W) batches."""
    B, C, H, W = shape
    rng = np.random.default_rng(1000 * seed + 7 * H + W + 31 * CONTENTS.index(content))
    if content == "random":
        return rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
    if content == "identical":
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        return a, a.copy()
    if content == "const":
        return np.full(shape, 255, np.uint8), np.full(shape, 254, np.uint8)
    if content == "checker":
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        a = np.broadcast_to((((yy + xx) & 1) * 255).astype(np.uint8), shape).copy()
        return a, (255 - a).astype(np.uint8)
    if content == "smooth":
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        base = 128.0 + 90.0 * np.sin(yy / 5.0 + np.arange(C)[:, None, None]) * np.cos(xx / 7.0 + np.arange(B)[:, None, None, None])
        a = base.clip(0, 255).astype(np.uint8)
        b = (base + rng.normal(0.0, 6.0, shape)).clip(0, 255).astype(np.uint8)
        return a, b
    raise ValueError(content)


def plane_mean_ssim(a_u8: np.ndarray, b_u8: np.ndarray) -> np.ndarray:
    """The host's definition: ``_ssim_plane`` averaged over the channels of each record (NaN where its crop is empty)."""
    from clip_feature_codec.eval.metrics import _ssim_plane
    out = np.full(a_u8.shape[0], np.nan)
    if a_u8.shape[2] < WIN or a_u8.shape[3] < WIN:
        return out
    for i in range(a_u8.shape[0]):
        out[i] = np.mean([_ssim_plane(a_u8[i, c], b_u8[i, c]) for c in range(a_u8.shape[1])])
    return out
