"""A numpy reference of the record-keyed noise source (Noise): Philox4x32-10 with the Random123 constants,
then Box-Muller.  The integers are exact; the normals are float64 (the device computes them in fp32 with the precise library
functions, so it agrees with this to a few fp32 ulps of its logf / sqrtf / sinpif / cospif, not bit for bit).

Element ``j`` of draw ``d`` of the record with 64-bit seed ``s``: key ``(s & 0xffffffff, s >> 32)``, counter ``(j >> 2, d, 0, 0)``;
the output words ``r0..r3`` serve elements ``4q .. 4q+3``: pair ``p = (j & 3) >> 1`` has ``u1 = ((r[2p] >> 9) + 0.5) 2^-23``,
``u2 = ((r[2p+1] >> 9) + 0.5) 2^-23``, ``rad = sqrt(-2 ln u1)``; an even ``j`` is ``rad cos(2 pi u2)``, an odd one ``rad sin(2 pi u2)``.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """``ctr``: four uint32 arrays (or ints) of one shape, ``key``: two.  Returns the four output words as uint64 arrays < 2^32."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in ctr)
    c0, c1, c2, c3 = np.broadcast_arrays(c0, c1, c2, c3)
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    sh, m = np.uint64(32), np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2               # < 2^64: exact in uint64
        n0 = (p1 >> sh) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> sh) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & m, n2, p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def seed_bits(seed):
    """Any Python int as the 64 bits the device sees (a negative one: two's complement)."""
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def draw_words(seed, draw, q):
    """The (len(q), 4) uint32 words of quads ``q`` of draw ``draw`` of the record with seed ``seed``."""
    s = seed_bits(seed)
    q = np.asarray(q, dtype=np.uint64)
    r = philox4x32_10((q, np.uint64(draw), np.uint64(0), np.uint64(0)), (s & MASK, s >> 32))
    return np.stack(r, axis=-1).astype(np.uint32)


def uniforms(words):
    """``((r >> 9) + 0.5) 2^-23`` in float64 (each is a 24-bit number: exact in fp32 too)."""
    return ((words >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normal_record(seed, draw, per):
    """The ``per`` float64 normals of one record's draw."""
    nq = (per + 3) // 4
    u = uniforms(draw_words(seed, draw, np.arange(nq)))              # (nq, 4): u1, u2 of pair 0, u1, u2 of pair 1
    out = np.empty((nq, 4), dtype=np.float64)
    for p in (0, 1):
        rad = np.sqrt(-2.0 * np.log(u[:, 2 * p]))
        out[:, 2 * p] = rad * np.cos(2.0 * np.pi * u[:, 2 * p + 1])
        out[:, 2 * p + 1] = rad * np.sin(2.0 * np.pi * u[:, 2 * p + 1])
    return out.reshape(-1)[:per]


def normal_fill(seeds, per, draw=0):
    """(len(seeds), per) float64: what ``_native.normal_fill(seeds, (B, per), draw)`` approximates in fp32."""
    return np.stack([normal_record(s, draw, per) for s in seeds])
