// The low-resolution guide (Low-resolution guide; ILVR, Choi et al. 2021; the super-resolution case of DDNM, Wang
// et al. 2022, in x0 space): per record, channel and N x N block of the image the step's x0 prediction is moved so that its block mean
// goes towards the guide's value g,
//     x0' = x0 + d,     d = (float)(lambda * (g - m)),     m = S / (N^2 2^30),     S = sum over the block of q(x0)
// with q(v) = __float2ll_rn(v * 2^30) (guide_fixed, ccn_device.h): |x0| <= 1 after the clamp, so the product is exact in fp32, S is an
// int64 sum of at most 4096 terms of magnitude <= 2^30, exact in ANY order, and (double)S is exact too.  d is therefore a function of
// the block's values alone: not of the launch shape, of B, of the record's position, of pointer alignment or of the load width.
//
// guide_strip_kernel: a strip -- the N rows of one plane that hold one row of blocks -- is N W contiguous floats, and the strips of a
// (B, C, H, W) tensor follow each other without a gap.  A workgroup of 256 owns whole strips (grid-stride over them): it zeroes one
// int64 per block of the strip in LDS, every lane walks the strip's quads (VEC: every pointer 16-byte aligned, 16-byte loads; N W is
// always a multiple of 4, so every strip then starts aligned) or its elements (4-byte loads), forms x0 by X0Form::x0 of X0Form::y
// (ccn_device.h) -- what the LR form of sampler_step_kernel goes through: the same combine, rescale multiply and clamp -- keeps a running sum
// while it stays inside one block (a quad may straddle two blocks, N = 2, or two rows, W % 4 != 0: the column is tracked per element) and adds
// it to the block's LDS word with one 64-bit integer atomic when it leaves the block.  After a barrier, lane t forms d of block t and
// stores it.  No global partial sums, no zeroed scratch, no floating-point atomics, one launch.  A strip of more than kSlots blocks
// (W / N > 1024) is walked once per kSlots blocks.
// PLAIN: the same sum over clamp(v, -1, 1) of a plain image, and the store is (float)m: the guide of an original (ccn_block_mean).
//
// Non-finite values are not looked for.  The static clamp maps a NaN to -1 (fmaxf returns its other operand) and +-inf to +-1, so a
// block's sum stays defined.  Under a NaN threshold every x0 of the record is NaN, the conversion of a NaN to int64 is whatever the
// hardware gives, d of that record's blocks is unspecified -- and x0' = NaN + d is NaN whatever d is, as the update is without a guide.
#include "ccn_device.h"
#include "../../include/ccn_hip.h"

#include <cmath>
#include <cstdint>
#include <string>

namespace ccn {
namespace {

constexpr int kThreads = 256, kSlots = 1024;

struct GuideArgs {
    X0Operands o;                      // PLAIN: x alone
    const float* guide;                // (strips, W / N)
    float* out;                        // (strips, W / N): d, or the block means (PLAIN)
    float strength;
    int W, lgN, WB;                    // WB = W / N blocks per strip
    long long strips;                  // B C (H / N)
    int strips_per_record;             // C (H / N)
};

template <bool VEC, bool PLAIN>
__global__ __launch_bounds__(kThreads) void guide_strip_kernel(GuideArgs a)
{
    __shared__ unsigned long long acc[kSlots];
    const unsigned tid = threadIdx.x, W = (unsigned)a.W, SW = W << a.lgN;     // SW: elements of a strip (the caller keeps it below 2^31)
    const double scale = (double)(1u << (2 * a.lgN)) * 1073741824.0;
    for (long long sid = blockIdx.x; sid < a.strips; sid += gridDim.x) {
        const long long base = sid * (long long)SW;
        const float* x = a.o.x + base;
        X0Form f;
        const float *yc = nullptr, *yu = nullptr;
        if constexpr (!PLAIN) {
            const long long b = sid / a.strips_per_record;
            yc = a.o.out_c + base;
            if (a.o.out_u) yu = a.o.out_u + base;
            f.pred = a.o.pred; f.c0 = a.o.c0; f.c1 = a.o.c1; f.w = a.o.w;
            f.guided = yu != nullptr; f.rescaled = a.o.gscale != nullptr; f.thr = a.o.thr != nullptr;
            if (f.thr) f.s = a.o.thr[b];
            if (f.rescaled) f.k = a.o.gscale[b];
        }
        auto value = [&](float xv, float yv, float uv) {
            if constexpr (PLAIN) return fminf(fmaxf(xv, -1.0f), 1.0f);
            else return f.x0(xv, f.y(yv, uv));
        };
        for (int blk0 = 0; blk0 < a.WB; blk0 += kSlots) {
            const int nb = a.WB - blk0 < kSlots ? a.WB - blk0 : kSlots;
            __syncthreads();                                        // the previous round's readers are done
            for (int t = tid; t < nb; t += kThreads) acc[t] = 0ull;
            __syncthreads();
            long long run = 0;
            int cur = -1;
            auto flush = [&] { if (cur >= 0) atomicAdd(&acc[cur], (unsigned long long)run); };
            auto add = [&](unsigned col, float v) {
                const int blk = (int)(col >> a.lgN) - blk0;
                if ((unsigned)blk >= (unsigned)nb) return;          // (only a strip of more than kSlots blocks has other rounds)
                if (blk != cur) { flush(); cur = blk; run = 0; }
                run += guide_fixed(v);
            };
            if constexpr (VEC) {
                for (unsigned q = tid; q < SW / 4; q += kThreads) {
                    const float4 xv = ((const float4*)x)[q];
                    float4 yv = make_float4(0.f, 0.f, 0.f, 0.f), uv = yv;
                    if constexpr (!PLAIN) {
                        yv = ((const float4*)yc)[q];
                        if (yu) uv = ((const float4*)yu)[q];
                    }
                    unsigned col = (q * 4) % W;
                    add(col, value(xv.x, yv.x, uv.x)); if (++col == W) col = 0;
                    add(col, value(xv.y, yv.y, uv.y)); if (++col == W) col = 0;
                    add(col, value(xv.z, yv.z, uv.z)); if (++col == W) col = 0;
                    add(col, value(xv.w, yv.w, uv.w));
                }
            } else {
                for (unsigned e = tid; e < SW; e += kThreads) {
                    float yv = 0.f, uv = 0.f;
                    if constexpr (!PLAIN) { yv = yc[e]; if (yu) uv = yu[e]; }
                    add(e % W, value(x[e], yv, uv));
                }
            }
            flush();
            __syncthreads();
            for (int t = tid; t < nb; t += kThreads) {
                const long long idx = sid * a.WB + blk0 + t;
                const double m = (double)(long long)acc[t] / scale;
                if constexpr (PLAIN) a.out[idx] = (float)m;
                else a.out[idx] = (float)((double)a.strength * ((double)a.guide[idx] - m));
            }
        }
    }
}

int log2_of(int N)
{
    int lg = 0;
    while ((1 << lg) < N) ++lg;
    return lg;
}

template <bool PLAIN>
hipError_t launch_strips(GuideArgs& a, int64_t planes, int C, int H, int W, int N, bool vec, hipStream_t s)
{
    if (!guide_block_ok(N, H, W) || planes <= 0 || C <= 0 || planes % C) return hipErrorInvalidValue;
    a.W = W; a.lgN = log2_of(N); a.WB = W / N;
    a.strips = planes * (H / N); a.strips_per_record = C * (H / N);
    const int grid = (int)(a.strips < 2048 ? a.strips : 2048);     // 256 CUs x 8 workgroups, grid-stride beyond
    if (vec) hipLaunchKernelGGL((guide_strip_kernel<true, PLAIN>), dim3(grid), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL((guide_strip_kernel<false, PLAIN>), dim3(grid), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace

bool guide_block_ok(int N, int H, int W)
{
    return N >= 2 && N <= 64 && !(N & (N - 1)) && H > 0 && W > 0 && H % N == 0 && W % N == 0 && (int64_t)W * N <= INT32_MAX;
}

hipError_t launch_lowres_delta(const X0Operands& o, int C, int H, int W, int N, const float* guide, float strength, float* delta, hipStream_t s)
{
    if (o.records <= 0 || o.records > 65535 || !o.x || !o.out_c || !guide || !delta) return hipErrorInvalidValue;
    GuideArgs a{};
    a.o = o; a.guide = guide; a.out = delta; a.strength = strength;
    const bool vec = !(((uintptr_t)o.x | (uintptr_t)o.out_c | (uintptr_t)o.out_u) & 15);
    return launch_strips<false>(a, o.records * C, C, H, W, N, vec, s);
}

hipError_t launch_block_mean(const float* x, int64_t planes, int H, int W, int N, float* out, hipStream_t s)
{
    if (!x || !out) return hipErrorInvalidValue;
    GuideArgs a{};
    a.o.x = const_cast<float*>(x); a.out = out;
    return launch_strips<true>(a, planes, 1, H, W, N, !((uintptr_t)x & 15), s);
}

}  // namespace ccn

using namespace ccn;

// the block geometry every guide entry takes (ccn_api.hip's checks call it too)
int ccn::guide_check(int32_t H, int32_t W, int32_t N)
{
    if (N < 2 || N > 64 || (N & (N - 1))) return fail(CCN_EINVAL, "N must be a power of two in 2..64");
    if (H <= 0 || W <= 0) return fail(CCN_EINVAL, "H and W must be positive");
    if (H % N || W % N) return fail(CCN_EINVAL, "H and W must be multiples of N: whole blocks only");
    if ((int64_t)W * N > INT32_MAX) return fail(CCN_EINVAL, "N rows of the image must hold fewer than 2^31 elements");
    return CCN_OK;
}

int ccn_block_mean(const float* x_dev, int64_t planes, int32_t H, int32_t W, int32_t N, float* out_dev, void* stream)
{
    if (!x_dev || !out_dev) return fail(CCN_EINVAL, "a tensor pointer is NULL");
    if (planes <= 0) return fail(CCN_EINVAL, "planes must be positive");
    if (int rc = guide_check(H, W, N)) return rc;
    if (launch_block_mean(x_dev, planes, H, W, N, out_dev, (hipStream_t)stream) != hipSuccess) return fail(CCN_EHIP, "block_mean launch failed");
    return CCN_OK;
}

int ccn_lowres_delta(const float* x_dev, const float* out_c_dev, const float* out_u_dev, int32_t pred, float w, float c0, float c1, int32_t B,
                     int32_t C, int32_t H, int32_t W, int32_t N, const float* guide_dev, float strength, const float* thr_dev,
                     const float* gscale_dev, float* delta_dev, void* stream)
{
    X0Operands o;
    o.x = const_cast<float*>(x_dev); o.out_c = out_c_dev; o.out_u = out_u_dev; o.gscale = gscale_dev; o.thr = thr_dev;
    o.pred = pred; o.w = w; o.c0 = c0; o.c1 = c1; o.records = B;
    if (!guide_dev || !delta_dev) return fail(CCN_EINVAL, "a tensor pointer is NULL");
    if (C <= 0) return fail(CCN_EINVAL, "C must be positive");
    if (int rc = guide_check(H, W, N)) return rc;
    o.per_record = (int64_t)C * H * W;
    if (int rc = check_x0_operands(o, false)) return rc;
    if (!(strength > 0.0f && strength <= 1.0f)) return fail(CCN_EINVAL, "the guide strength must be in (0, 1]");
    if (launch_lowres_delta(o, C, H, W, N, guide_dev, strength, delta_dev, (hipStream_t)stream) != hipSuccess)
        return fail(CCN_EHIP, "lowres_delta launch failed");
    return CCN_OK;
}
