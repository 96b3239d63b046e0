// Reconstruction scores on the device (eval/metrics.py: _to_uint8, psnr_u8, _ssim_plane): per record the sum of squared differences
// of the two uint8 images and the SSIM skimage's defaults define -- 7 x 7 uniform window, sample covariance, K1 = 0.01, K2 = 0.03,
// data_range = 255, mean over the channels and the valid interior.  Like the optimiser tail (ccn_optim.hip) the kernels, their
// launcher and the extern "C" entry points of include/ccn_hip.h sit in one file and work on raw buffers: no handle, no allocation,
// no synchronisation.
//
// A workgroup takes SC_TY x SC_TX window positions of one (record, channel) plane.  Position (i, j) is the window whose top left
// pixel is (i, j), so the tile needs the pixels [y0, y0 + SC_TY + 6) x [x0, x0 + SC_TX + 6) of both images:
//   1. stage    16-pixel chunks of that rectangle (rounded up to SC_PW columns) into LDS, two bytes per pixel (a | b << 8), the fp32
//               reconstruction converted on the way in.  The thread that stages a pixel the tile OWNS adds it to the SSE and writes
//               the converted byte out: a tile owns its first SC_TY rows and SC_TX columns, the last tile of a direction also the
//               rest of the rectangle, so every pixel of the plane has exactly one owner although up to four tiles load it;
//   2. rows     horizontal 7-sums of a, b, a^2, b^2, ab for every row of the rectangle, eight neighbouring columns per thread
//               (sliding: one pixel enters, one leaves), 16 bytes per column back into LDS;
//   3. columns  vertical 7-sums of those, four neighbouring rows per thread (sliding again), then the SSIM quotient in fp64.
// Everything up to the quotient is integer arithmetic and exact: with S* the window sums,
//   49 u = S,   48 * 49 v_a = 49 Saa - Sa^2 =: Na,   48 * 49 v_ab = 49 Sab - Sa Sb =: Nab        (all below 2^31)
//   ssim = ((2 Sa Sb + 2401 c1) (2 Nab + 2352 c2)) / ((Sa^2 + Sb^2 + 2401 c1) (Na + Nb + 2352 c2))
// which is _ssim_plane's expression with both factors of the numerator and of the denominator scaled by 49^2 and 48 * 49.  For
// equal windows the numerator and the denominator have the same bits: identical images score exactly 1.
// Sums: fp64 (SSIM) and integer (SSE) per thread -> wave shuffle tree -> one pair of doubles per workgroup in scratch, indexed
// [record][channel][tile row][tile column] -> score_final_kernel, one wave per record, adds them in index order.  No atomics:
// bit-reproducible, and a record's bits do not depend on what else is in the batch.
#include "ccn_device.h"
#include "../../include/ccn_hip.h"

#include <cmath>
#include <cstdint>
#include <string>

namespace ccn {
namespace {

constexpr int SC_WIN = 7;
constexpr int SC_TX = 64, SC_TY = 16;                                // window positions per workgroup
constexpr int SC_PH = SC_TY + SC_WIN - 1;                            // 22 pixel rows
constexpr int SC_PW = 80;                                            // SC_TX + 6 pixel columns, rounded up to whole 16-pixel chunks
constexpr int SC_NCH = SC_PW / 16;
constexpr int SC_HLD = SC_TX + SC_TX / 8;                            // row of horizontal sums: a 16-byte pad after every 8 columns
static_assert(SC_PW >= SC_TX + SC_WIN - 1 && SC_PW % 16 == 0 && SC_TX % 16 == 0, "chunking");
static_assert(SC_PH * SC_NCH <= 256 && SC_PH * (SC_TX / 8) <= 256 && SC_TX * (SC_TY / 4) == 256, "one task per thread and phase");

// _to_uint8: (x + 1) * 127.5 as two rounded fp32 operations, clip to [0, 255], truncate.  NaN -> 0 (fmaxf returns the other operand)
__device__ __forceinline__ unsigned to_u8(float x)
{
    const float t = __fmul_rn(__fadd_rn(x, 1.0f), 127.5f);
    return (unsigned)fminf(fmaxf(t, 0.0f), 255.0f);
}

// F32: the reconstruction is fp32 in [-1, 1] (converted here), else uint8.  VEC: W % 16 == 0 and every image pointer 16-byte
// aligned, so that a 16-pixel chunk that starts inside the image lies inside it as a whole and is one (u8) or four (fp32) 16-byte
// accesses; otherwise one access per pixel.  Both forms hand the same bytes to the same arithmetic.
template <bool F32, bool VEC>
__global__ __launch_bounds__(256) void score_partial_kernel(const void* __restrict__ recon_v, const uint8_t* __restrict__ orig,
                                                             uint8_t* __restrict__ recon_u8_out, int H, int W, int nty, int ntx,
                                                             double* __restrict__ scratch)
{
    __shared__ __attribute__((aligned(16))) uint16_t pix[SC_PH][SC_PW];
    __shared__ __attribute__((aligned(16))) u32x4 hs[SC_PH][SC_HLD];  // .x = Sa | Sb << 16, .y = Saa, .z = Sbb, .w = Sab of a row's 7 pixels
    __shared__ double red_s[4];
    __shared__ unsigned red_e[4];
    const int tid = threadIdx.x;
    const int tx = (int)(blockIdx.x % (unsigned)ntx), ty = (int)((blockIdx.x / (unsigned)ntx) % (unsigned)nty);
    const size_t plane = blockIdx.x / ((unsigned)ntx * (unsigned)nty);
    const int x0 = tx * SC_TX, y0 = ty * SC_TY;
    const size_t pbase = plane * (size_t)H * (size_t)W;
    const int own_h = ty == nty - 1 ? SC_PH : SC_TY, own_w = tx == ntx - 1 ? SC_PW : SC_TX;
    unsigned sse = 0;                                                 // at most 22 * 80 * 255^2 per workgroup

    // ---- 1. stage ------------------------------------------------------------------------------------------------------------
    if (tid < SC_PH * SC_NCH) {
        const int r = tid / SC_NCH, k = tid % SC_NCH;
        const int y = y0 + r, x = x0 + 16 * k;
        unsigned a[16], b[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) { a[e] = 0; b[e] = 0; }
        const bool in = y < H && x < W;
        const size_t o = pbase + (size_t)(in ? y : 0) * (size_t)W + (size_t)(in ? x : 0);
        if (in) {
            if (VEC) {
                const u32x4 qb = *(const u32x4*)(orig + o);
#pragma unroll
                for (int e = 0; e < 16; ++e) b[e] = (qb[e >> 2] >> (8 * (e & 3))) & 255u;
                if (F32) {
                    const f32x4* p = (const f32x4*)((const float*)recon_v + o);
                    const f32x4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
#pragma unroll
                    for (int e = 0; e < 4; ++e) { a[e] = to_u8(q0[e]); a[4 + e] = to_u8(q1[e]); a[8 + e] = to_u8(q2[e]); a[12 + e] = to_u8(q3[e]); }
                } else {
                    const u32x4 qa = *(const u32x4*)((const uint8_t*)recon_v + o);
#pragma unroll
                    for (int e = 0; e < 16; ++e) a[e] = (qa[e >> 2] >> (8 * (e & 3))) & 255u;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    if (x + e < W) {
                        b[e] = orig[o + e];
                        a[e] = F32 ? to_u8(((const float*)recon_v)[o + e]) : (unsigned)((const uint8_t*)recon_v)[o + e];
                    }
                }
            }
        }
        u32x4 w0, w1;                                                 // pixels outside the image are staged as zeros
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w0[e] = (a[2 * e] | (b[2 * e] << 8)) | ((a[2 * e + 1] | (b[2 * e + 1] << 8)) << 16);
            w1[e] = (a[8 + 2 * e] | (b[8 + 2 * e] << 8)) | ((a[9 + 2 * e] | (b[9 + 2 * e] << 8)) << 16);
        }
        *(u32x4*)&pix[r][16 * k] = w0;
        *(u32x4*)&pix[r][16 * k + 8] = w1;
        if (in && r < own_h && 16 * k < own_w) {                      // own_w is a whole number of chunks
#pragma unroll
            for (int e = 0; e < 16; ++e) { const int d = (int)a[e] - (int)b[e]; sse += (unsigned)(d * d); }   // 0 outside the image
            if (F32 && recon_u8_out) {
                if (VEC) {
                    u32x4 q;
#pragma unroll
                    for (int e = 0; e < 4; ++e) q[e] = a[4 * e] | (a[4 * e + 1] << 8) | (a[4 * e + 2] << 16) | (a[4 * e + 3] << 24);
                    *(u32x4*)(recon_u8_out + o) = q;
                } else {
#pragma unroll
                    for (int e = 0; e < 16; ++e) if (x + e < W) recon_u8_out[o + e] = (uint8_t)a[e];
                }
            }
        }
    }
    __syncthreads();

    // ---- 2. rows: columns 8 g .. 8 g + 7 of row r from the pixels 8 g .. 8 g + 13 -----------------------------------------------
    if (tid < SC_PH * (SC_TX / 8)) {
        const int r = tid >> 3, g = tid & 7;
        const u32x4 w0 = *(const u32x4*)&pix[r][8 * g], w1 = *(const u32x4*)&pix[r][8 * g + 8];
        unsigned a[16], b[16];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            a[2 * e] = w0[e] & 255u; b[2 * e] = (w0[e] >> 8) & 255u; a[2 * e + 1] = (w0[e] >> 16) & 255u; b[2 * e + 1] = w0[e] >> 24;
            a[8 + 2 * e] = w1[e] & 255u; b[8 + 2 * e] = (w1[e] >> 8) & 255u; a[9 + 2 * e] = (w1[e] >> 16) & 255u; b[9 + 2 * e] = w1[e] >> 24;
        }
        // The unpacked bytes are made opaque to the optimiser: left visible, hipcc (ROCm 7.2) rewrites the sliding ab sum below into
        // v_dot4_u32_u8 chains that keep the product of the pixel that has left the window -- every column but the first of each
        // group of eight then came out wrong on the GPU.  __umul24 keeps the products at full rate without that knowledge.
#pragma unroll
        for (int e = 0; e < 16; ++e) { asm volatile("" : "+v"(a[e])); asm volatile("" : "+v"(b[e])); }
        unsigned sa = 0, sb = 0, saa = 0, sbb = 0, sab = 0;
#pragma unroll
        for (int e = 0; e < SC_WIN; ++e) {
            sa += a[e]; sb += b[e]; saa += __umul24(a[e], a[e]); sbb += __umul24(b[e], b[e]); sab += __umul24(a[e], b[e]);
        }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int j = 8 * g + t;
            hs[r][j + (j >> 3)] = u32x4{sa | (sb << 16), saa, sbb, sab};
            if (t < 7) {
                const unsigned ai = a[t + SC_WIN], bi = b[t + SC_WIN], ao = a[t], bo = b[t];
                sa += ai - ao; sb += bi - bo;
                saa += __umul24(ai, ai) - __umul24(ao, ao); sbb += __umul24(bi, bi) - __umul24(bo, bo); sab += __umul24(ai, bi) - __umul24(ao, bo);
            }
        }
    }
    __syncthreads();

    // ---- 3. columns: positions (4 seg .. 4 seg + 3, j); the window of row i is rows i .. i + 6 of hs -----------------------------
    double ss = 0.0;
    {
        const int j = tid & 63, seg = tid >> 6, jc = j + (j >> 3);
        const bool col_ok = x0 + j < W - (SC_WIN - 1);
        constexpr double c1 = (0.01 * 255.0) * (0.01 * 255.0), c2 = (0.03 * 255.0) * (0.03 * 255.0);
        constexpr double k1 = c1 * 2401.0, k2 = c2 * 2352.0;         // 49^2 c1, 48 * 49 c2
        u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < SC_WIN; ++e) v += hs[4 * seg + e][jc];    // the packed .x adds without a carry: both halves stay below 2^16
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int i = 4 * seg + t;
            if (col_ok && y0 + i < H - (SC_WIN - 1)) {
                const int sa = (int)(v[0] & 0xffffu), sb = (int)(v[0] >> 16);
                const int na = 49 * (int)v[1] - sa * sa, nb = 49 * (int)v[2] - sb * sb, nab = 49 * (int)v[3] - sa * sb;
                const double num = ((double)(2 * sa * sb) + k1) * ((double)(2 * nab) + k2);
                const double den = ((double)(sa * sa + sb * sb) + k1) * ((double)(na + nb) + k2);
                ss += num / den;
            }
            if (t < 3) v += hs[i + SC_WIN][jc] - hs[i][jc];           // true differences are never negative per field
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { ss += __shfl_xor(ss, m); sse += (unsigned)__shfl_xor((int)sse, m); }
    if ((tid & 63) == 0) { red_s[tid >> 6] = ss; red_e[tid >> 6] = sse; }
    __syncthreads();
    if (tid == 0) {
        scratch[(size_t)blockIdx.x * 2] = (double)((red_e[0] + red_e[1]) + (red_e[2] + red_e[3]));
        scratch[(size_t)blockIdx.x * 2 + 1] = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    }
}

// one wave per record, fixed order (mse_final_kernel's scheme) over the record's workgroup pairs; cnt = C (H - 6) (W - 6), 0 if none
__global__ void score_final_kernel(const double* __restrict__ scratch, int per_rec, double cnt, double* __restrict__ out)
{
    const double* p = scratch + (size_t)blockIdx.x * (size_t)per_rec * 2;
    double e = 0.0, s = 0.0;
    for (int i = (int)threadIdx.x; i < per_rec; i += 64) { e += p[2 * (size_t)i]; s += p[2 * (size_t)i + 1]; }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { e += __shfl_xor(e, m); s += __shfl_xor(s, m); }
    if (threadIdx.x == 0) {
        out[(size_t)blockIdx.x * 2] = e;
        out[(size_t)blockIdx.x * 2 + 1] = cnt > 0.0 ? s / cnt : __builtin_nan("");
    }
}

struct ScoreGeom { int nty, ntx; int64_t per_rec, total; };
// the tiling of one plane: at least one tile in each direction, so that an image without a window position still gets its SSE
ScoreGeom score_geom(int B, int C, int H, int W)
{
    const int py = H - (SC_WIN - 1), px = W - (SC_WIN - 1);
    ScoreGeom g;
    g.nty = py > 0 ? (py + SC_TY - 1) / SC_TY : 1;
    g.ntx = px > 0 ? (px + SC_TX - 1) / SC_TX : 1;
    g.per_rec = (int64_t)C * g.nty * g.ntx;
    g.total = g.per_rec * B;
    return g;
}

int score(const void* recon, bool f32, const uint8_t* orig, uint8_t* recon_u8_out, double* out, int B, int C, int H, int W, void* scratch,
          size_t scratch_bytes, hipStream_t s)
{
    if (!recon || !orig || !out || !scratch) return fail(CCN_EINVAL, "a buffer is NULL");
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(CCN_EINVAL, "B, C, H and W must be positive");
    const ScoreGeom g = score_geom(B, C, H, W);
    if (g.per_rec > INT32_MAX || g.total > INT32_MAX) return fail(CCN_EINVAL, "too many tiles");
    if (((uintptr_t)scratch & 7) != 0 || ((uintptr_t)out & 7) != 0) return fail(CCN_EINVAL, "scratch_dev and out_dev must be 8-byte aligned");
    if (scratch_bytes < (size_t)g.total * 16) return fail(CCN_EINVAL, "scratch is smaller than ccn_score_scratch_bytes asks for");
    if (f32 && ((uintptr_t)recon & 3) != 0) return fail(CCN_EINVAL, "recon_dev must be 4-byte aligned");
    const uintptr_t bits = (uintptr_t)recon | (uintptr_t)orig | (uintptr_t)recon_u8_out;
    const bool vec = W % 16 == 0 && (bits & 15) == 0;
    const dim3 grid((unsigned)g.total), block(256);
#define CCN_SCORE(F, V) hipLaunchKernelGGL((score_partial_kernel<F, V>), grid, block, 0, s, recon, orig, recon_u8_out, H, W, g.nty, g.ntx, (double*)scratch)
    if (f32) { if (vec) CCN_SCORE(true, true); else CCN_SCORE(true, false); }
    else { if (vec) CCN_SCORE(false, true); else CCN_SCORE(false, false); }
#undef CCN_SCORE
    const int py = H - (SC_WIN - 1), px = W - (SC_WIN - 1);
    const double cnt = py > 0 && px > 0 ? (double)C * (double)py * (double)px : 0.0;
    hipLaunchKernelGGL(score_final_kernel, dim3((unsigned)B), dim3(64), 0, s, (const double*)scratch, (int)g.per_rec, cnt, out);
    if (hipGetLastError() != hipSuccess) return fail(CCN_EHIP, "score launch failed");
    return CCN_OK;
}

}  // namespace
}  // namespace ccn

using namespace ccn;

extern "C" {

int ccn_score_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W, size_t* bytes)
{
    if (!bytes || B <= 0 || C <= 0 || H <= 0 || W <= 0) return fail(CCN_EINVAL, "bad argument");
    const ScoreGeom g = score_geom(B, C, H, W);
    if (g.per_rec > INT32_MAX || g.total > INT32_MAX) return fail(CCN_EINVAL, "too many tiles");
    *bytes = (size_t)g.total * 16;
    return CCN_OK;
}

int ccn_psnr_ssim_f32(const float* recon_dev, const uint8_t* orig_u8_dev, uint8_t* recon_u8_out_dev, double* out_dev, int32_t B, int32_t C,
                      int32_t H, int32_t W, void* scratch_dev, size_t scratch_bytes, void* stream)
{
    return score(recon_dev, true, orig_u8_dev, recon_u8_out_dev, out_dev, B, C, H, W, scratch_dev, scratch_bytes, (hipStream_t)stream);
}

int ccn_psnr_ssim_u8(const uint8_t* recon_u8_dev, const uint8_t* orig_u8_dev, double* out_dev, int32_t B, int32_t C, int32_t H, int32_t W,
                     void* scratch_dev, size_t scratch_bytes, void* stream)
{
    return score(recon_u8_dev, false, orig_u8_dev, nullptr, out_dev, B, C, H, W, scratch_dev, scratch_bytes, (hipStream_t)stream);
}

}  // extern "C"
