// Dynamic thresholding of x0 (Saharia et al. 2022, Imagen section 2.3; DESIGN.md section 1, Thresholding): the per-record order
// statistic behind  s = min(max(Q_p(|x0|), 1), s_max),  x0 <- clamp(x0, -s, s) / s.
//
// Q_p is the linearly interpolated quantile (torch.quantile's default): with v the ascending |x0| of a record of `per` elements,
// pos = p (per - 1), k = floor(pos), frac = pos - k (host, double), q = v[k] + frac * (v[min(k+1, per-1)] - v[k]) in three separately
// rounded fp32 ops.  v[k] and v[k+1] are found EXACTLY, by a radix select on the bit pattern of |x0| (sign bit cleared: non-negative
// floats order as their bits do) -- 11 + 10 + 10 bits, most significant first, both ranks at once.  NaN patterns lie above +inf in
// that order, so NaNs sort last: a rank that lands on one makes q, the threshold and with it the record's update NaN (nothing here
// looks for them), +inf is an ordinary largest value, -0 and +0 are one key, denormals keep their order.
//
// The raw x0 of an element is X0Form::raw of X0Form::y (ccn_device.h), the formation the sampler update itself goes through: the same
// guidance combine and, with `gscale`, the same multiplication by the record's guidance-rescale factor (ccn_rescale.hip): the
// quantile is taken on the bits the update clamps.
//
// Launches (all on the caller's stream, nothing synchronises, nothing is allocated):
//   thr_zero_kernel            zeroes the select state of the B records: any scratch contents are fine, every call starts from zero
//   thr_pass_kernel<0>         grid (gx, B): histogram of the top 11 key bits; a workgroup counts in LDS, then adds its non-empty bins
//                              to the record's 64-bit global histogram with integer atomics
//   thr_pass_kernel<1>, <2>    every workgroup first picks the previous pass's digit of both ranks from that histogram (an integer
//                              prefix sum), then counts the next 10 bits of the elements that carry the picked prefix
//   thr_final_kernel           grid (1, B): the last pick, the interpolation, the clamp to [1, max_value]
// Integer counts only: the result has no summation order in it, so it does not depend on the grid, on B, on the record's position in
// the batch or on which access width ran.  VEC (every pointer 16-byte aligned and per % 4 == 0) reads 16 bytes per lane, else 4.
#include "ccn_device.h"
#include "../../include/ccn_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

namespace ccn {
namespace {

// One record's select state: H0 (2048 bins), H1 and H2 (two ranks x 1024 bins) as 64-bit counts -- a record has up to 2^34
// elements -- then the picks handed from one pass kernel to the next (written by workgroup 0 of a record, read by the NEXT launch).
constexpr int kBins0 = 2048, kBins = 1024;
struct Sel { uint32_t prefix[2]; uint32_t pad[2]; unsigned long long rank[2]; };       // the key bits picked so far, the rank inside them
constexpr size_t kHistBytes = (size_t)(kBins0 + 4 * kBins) * 8;
constexpr size_t kRecBytes = kHistBytes + 2 * sizeof(Sel);
static_assert(sizeof(Sel) == 32 && kRecBytes % 16 == 0, "the records of the scratch stay 16-byte aligned");

struct ThrArgs {
    X0Operands o;                      // (o.thr is not read: this is what computes it)
    unsigned long long k0, k1;         // the two ranks: k and min(k + 1, per - 1)
    float frac, max_value;
    float* thr;
    char* scratch;
};

__global__ __launch_bounds__(256) void thr_zero_kernel(uint4* __restrict__ p, long long n16)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long long)gridDim.x * blockDim.x)
        p[i] = make_uint4(0u, 0u, 0u, 0u);
}

// The bin of `hist` (NB 64-bit counts) that holds rank `rank`, and the rank inside that bin.  Called by all 256 threads; every
// thread returns the result.  `wtot`, `res` are LDS words of the caller.  A rank beyond the total (it cannot be: the counts of a
// prefix sum to the rank space it was picked from) would give the last bin.
template <int NB>
__device__ __forceinline__ void pick(const unsigned long long* __restrict__ hist, unsigned long long rank, unsigned long long* wtot,
                                     unsigned long long* res, int tid, uint32_t& digit, unsigned long long& inside)
{
    constexpr int PER = NB / 256;
    const int lane = tid & 63, wave = tid >> 6;
    unsigned long long c[PER], sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { c[j] = hist[tid * PER + j]; sum += c[j]; }
    unsigned long long incl = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) wtot[wave] = incl;
    if (tid == 0) { res[0] = NB - 1; res[1] = 0; }
    __syncthreads();
    unsigned long long below = incl - sum;
    for (int v = 0; v < wave; ++v) below += wtot[v];
    if (rank >= below && rank - below < sum) {                      // one thread: the bins are disjoint rank ranges
        unsigned long long r = rank - below;
        int j = 0;
#pragma unroll
        for (; j < PER - 1; ++j) { if (r < c[j]) break; r -= c[j]; }
        res[0] = (unsigned long long)(tid * PER + j); res[1] = r;
    }
    __syncthreads();
    digit = (uint32_t)res[0]; inside = res[1];
    __syncthreads();                                                // (res and wtot are reused by the next pick)
}

// the picks up to and including pass PASS - 1, for both ranks; `same`: both ranks lie in one prefix, which then has ONE histogram
template <int PASS>
__device__ __forceinline__ void picks_so_far(const ThrArgs& a, char* rec, unsigned long long* wtot, unsigned long long* res, int tid,
                                             uint32_t* pre, unsigned long long* rk)
{
    unsigned long long* H0 = (unsigned long long*)rec;
    unsigned long long* H1 = H0 + kBins0;
    Sel* st = (Sel*)(rec + kHistBytes);
    pre[0] = pre[1] = 0u; rk[0] = a.k0; rk[1] = a.k1;
    if constexpr (PASS == 0) return;
    else if constexpr (PASS == 1) {
#pragma unroll
        for (int t = 0; t < 2; ++t) pick<kBins0>(H0, rk[t], wtot, res, tid, pre[t], rk[t]);
    } else {
        // H(PASS-1) was counted under the picks of the launch before it: st[PASS - 2], written by that launch
        const Sel s = st[PASS - 2];
        const unsigned long long* H = H1 + (size_t)(PASS - 2) * 2 * kBins;
        const bool same = s.prefix[0] == s.prefix[1];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            uint32_t d;
            pick<kBins>(H + (same ? 0 : t * kBins), s.rank[t], wtot, res, tid, d, rk[t]);
            pre[t] = (s.prefix[t] << 10) | d;
        }
    }
    if constexpr (PASS == 1 || PASS == 2) if (blockIdx.x == 0 && tid == 0) {   // for the next launch
        Sel o;
        o.prefix[0] = pre[0]; o.prefix[1] = pre[1]; o.pad[0] = o.pad[1] = 0u; o.rank[0] = rk[0]; o.rank[1] = rk[1];
        st[PASS - 1] = o;
    }
}

template <int PASS, bool VEC>
__global__ __launch_bounds__(256) void thr_pass_kernel(ThrArgs a)
{
    constexpr int SH = PASS == 0 ? 20 : PASS == 1 ? 10 : 0;         // the digit of this pass: key >> SH, 11 bits (PASS 0) or 10
    __shared__ uint32_t lh[kBins0];                                 // PASS 0: one histogram; else [rank][1024]
    __shared__ unsigned long long wtot[4], res[2];
    const int b = blockIdx.y, tid = threadIdx.x;
    char* rec = a.scratch + (size_t)b * kRecBytes;
    uint32_t pre[2];
    unsigned long long rk[2];
    picks_so_far<PASS>(a, rec, wtot, res, tid, pre, rk);
    for (int i = tid; i < kBins0; i += 256) lh[i] = 0u;
    __syncthreads();

    const long long per = a.o.per_record, off = (long long)b * per;
    const float* x = a.o.x + off;
    const float* yc = a.o.out_c + off;
    const float* yu = a.o.out_u ? a.o.out_u + off : nullptr;
    const uint32_t pre0 = pre[0], pre1 = pre[1];
    X0Form f;
    f.pred = a.o.pred; f.c0 = a.o.c0; f.c1 = a.o.c1; f.w = a.o.w;
    f.guided = yu != nullptr; f.rescaled = a.o.gscale != nullptr;
    if (f.rescaled) f.k = a.o.gscale[b];
    auto count = [&](float xv, float yv, float uv) {
        const uint32_t key = __float_as_uint(f.raw(xv, f.y(yv, uv))) & 0x7fffffffu;
        if (PASS == 0) atomicAdd(&lh[key >> SH], 1u);
        else {
            const uint32_t hi = key >> (SH + 10), d = (key >> SH) & (uint32_t)(kBins - 1);
            if (hi == pre0) atomicAdd(&lh[d], 1u);
            else if (hi == pre1) atomicAdd(&lh[kBins + d], 1u);
        }
    };
    const long long t0 = (long long)blockIdx.x * blockDim.x + tid, nthr = (long long)gridDim.x * blockDim.x;
    const long long n4 = VEC ? per / 4 : 0;
    for (long long q = t0; q < n4; q += nthr) {
        const float4 xv = ((const float4*)x)[q], yv = ((const float4*)yc)[q];
        float4 uv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (yu) uv = ((const float4*)yu)[q];
        count(xv.x, yv.x, uv.x); count(xv.y, yv.y, uv.y); count(xv.z, yv.z, uv.z); count(xv.w, yv.w, uv.w);
    }
    for (long long i = n4 * 4 + t0; i < per; i += nthr) count(x[i], yc[i], yu ? yu[i] : 0.f);
    __syncthreads();

    unsigned long long* H = (unsigned long long*)rec + (PASS == 0 ? 0 : kBins0 + (PASS - 1) * 2 * kBins);
    for (int i = tid; i < kBins0; i += 256) {
        const uint32_t v = lh[i];
        if (v) atomicAdd(H + i, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(256) void thr_final_kernel(ThrArgs a)
{
    __shared__ unsigned long long wtot[4], res[2];
    const int b = blockIdx.y, tid = threadIdx.x;
    uint32_t key[2];
    unsigned long long rk[2];
    picks_so_far<3>(a, a.scratch + (size_t)b * kRecBytes, wtot, res, tid, key, rk);
    if (tid == 0) {
        const float v_lo = __uint_as_float(key[0]), v_hi = __uint_as_float(key[1]);
        const float q = __fadd_rn(v_lo, __fmul_rn(a.frac, __fsub_rn(v_hi, v_lo)));
        // min(max(q, 1), max_value) by comparisons: the same value for every number, and a NaN q stays NaN (fmaxf would drop it)
        float t = q < 1.0f ? 1.0f : q;
        t = t > a.max_value ? a.max_value : t;
        a.thr[b] = t;
    }
}

}  // namespace

size_t x0_threshold_scratch_bytes(int B) { return (size_t)(B > 0 ? B : 0) * kRecBytes; }

hipError_t launch_x0_threshold(const X0Operands& o, double p, float max_value, float* thr, void* scratch, hipStream_t s)
{
    const int64_t per = o.per_record, B = o.records;
    if (B <= 0 || B > 65535 || per <= 0 || per >= kThrMaxPerRecord || !(p >= 0.0 && p <= 1.0)) return hipErrorInvalidValue;
    ThrArgs a;
    a.o = o;
    const double pos = p * (double)(per - 1);
    double kf = std::floor(pos);
    if (kf > (double)(per - 1)) kf = (double)(per - 1);
    a.k0 = (unsigned long long)kf;
    a.k1 = a.k0 + 1 < (unsigned long long)per ? a.k0 + 1 : (unsigned long long)per - 1;
    a.frac = (float)(pos - kf);
    a.max_value = max_value; a.thr = thr; a.scratch = (char*)scratch;

    const bool vec = !(((uintptr_t)o.x | (uintptr_t)o.out_c | (uintptr_t)o.out_u) & 15) && !(per & 3);
    // about four workgroups per CU over the batch, never more than the record has work for; a workgroup's LDS counts are 32-bit,
    // so it takes at most 2^30 elements
    const int64_t work = vec ? per / 4 : per, blocks = (work + 255) / 256, want = 1024 / B > 0 ? 1024 / B : 1, least = (per >> 30) + 1;
    const int gx = (int)std::max<int64_t>(std::min<int64_t>(blocks, want), least);
    const dim3 grid(gx, (unsigned)B), one(1, (unsigned)B);

    const long long n16 = (long long)(x0_threshold_scratch_bytes(B) / 16);
    const int zb = (int)std::min<long long>((n16 + 255) / 256, 1024);
    hipLaunchKernelGGL(thr_zero_kernel, dim3(zb), dim3(256), 0, s, (uint4*)scratch, n16);
    if (vec) {
        hipLaunchKernelGGL((thr_pass_kernel<0, true>), grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL((thr_pass_kernel<1, true>), grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL((thr_pass_kernel<2, true>), grid, dim3(256), 0, s, a);
    } else {
        hipLaunchKernelGGL((thr_pass_kernel<0, false>), grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL((thr_pass_kernel<1, false>), grid, dim3(256), 0, s, a);
        hipLaunchKernelGGL((thr_pass_kernel<2, false>), grid, dim3(256), 0, s, a);
    }
    hipLaunchKernelGGL(thr_final_kernel, one, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace ccn

using namespace ccn;

int ccn_x0_threshold_scratch_bytes(int32_t B, int64_t per_record, size_t* bytes)
{
    if (!bytes) return fail(CCN_EINVAL, "null argument");
    X0Operands o;
    o.records = B; o.per_record = per_record;
    if (int rc = check_x0_operands(o, false, false)) return rc;
    *bytes = x0_threshold_scratch_bytes(B);
    return CCN_OK;
}

int ccn_x0_threshold(const float* x_dev, const float* out_c_dev, const float* out_u_dev, int32_t pred, float w, float c0, float c1,
                     int32_t B, int64_t per_record, double p, float max_value, float* thr_dev, void* scratch_dev, size_t scratch_bytes,
                     void* stream)
{
    return ccn_x0_threshold_rs(x_dev, out_c_dev, out_u_dev, pred, w, c0, c1, B, per_record, p, max_value, thr_dev, scratch_dev, scratch_bytes,
                               nullptr, stream);
}

int ccn_x0_threshold_rs(const float* x_dev, const float* out_c_dev, const float* out_u_dev, int32_t pred, float w, float c0, float c1,
                        int32_t B, int64_t per_record, double p, float max_value, float* thr_dev, void* scratch_dev, size_t scratch_bytes,
                        const float* gscale_dev, void* stream)
{
    X0Operands o;
    o.x = const_cast<float*>(x_dev); o.out_c = out_c_dev; o.out_u = out_u_dev; o.gscale = gscale_dev;
    o.pred = pred; o.w = w; o.c0 = c0; o.c1 = c1; o.per_record = per_record; o.records = B;
    if (!thr_dev) return fail(CCN_EINVAL, "a tensor pointer is NULL");
    if (int rc = check_x0_operands(o, false)) return rc;
    if (!(p >= 0.0 && p <= 1.0)) return fail(CCN_EINVAL, "the quantile p must be in [0, 1]");
    if (!(max_value >= 1.0f)) return fail(CCN_EINVAL, "max_value must be at least 1 (+inf: no upper bound)");
    if (!scratch_dev || ((uintptr_t)scratch_dev & 15)) return fail(CCN_EINVAL, "the scratch must be non-null and 16-byte aligned");
    if (scratch_bytes < x0_threshold_scratch_bytes(B))
        return fail(CCN_EINVAL, "the scratch is too small: need " + std::to_string(x0_threshold_scratch_bytes(B)) + " bytes");
    if (launch_x0_threshold(o, p, max_value, thr_dev, scratch_dev, (hipStream_t)stream) != hipSuccess)
        return fail(CCN_EHIP, "x0_threshold launch failed");
    return CCN_OK;
}
