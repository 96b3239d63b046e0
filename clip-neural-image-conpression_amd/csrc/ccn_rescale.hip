// Guidance rescale (Lin et al. 2023, Common Diffusion Noise Schedules and Sample Steps are Flawed, section 3.4; DESIGN.md section 1,
// Guidance rescale): the per-record factor that matches the standard deviation of the combined output to the conditional one's,
//     y = y_u + w (y_c - y_u)   (three separately rounded fp32 ops, as in the step kernel)
//     k_b = phi * std(y_c[b]) / std(y[b]) + (1 - phi)         unbiased std over the whole record, double, rounded ONCE to fp32
// The step kernel and the threshold passes then use y' = k_b * y (one __fmul_rn per element).
//
// The sums  S(y_c), S(y_c^2), S(y), S(y^2)  are accumulated in double (the square of an fp32 value is exact in double), in an order
// that is a function of (j, per) only:
//   rs_partial_kernel   grid (gx, B), gx = clamp(ceil(per / 4096), 1, 64), 256 threads.  Quad q = j >> 2 of the record belongs to thread
//                       q mod (256 gx) of the row, which adds its quads in increasing q and a quad's elements in increasing j.  VEC (every
//                       pointer 16-byte aligned and per % 4 == 0) loads a quad as 16 bytes, else its elements as 4 bytes each: the same
//                       values in the same order.  Lanes combine by an xor-shuffle tree (32, 16, .., 1), the four waves in index order
//                       through LDS, and the workgroup writes its four doubles to slot [b][blockIdx.x] of the scratch.
//   rs_final_kernel     one thread per record adds the gx slots in index order, forms k_b and stores one float.
// No floating-point atomics, nothing zeroed: every slot read was written by the same call.  Neither B, the record's position, the
// pointer alignment nor the load width enters the order, so k_b is the same bits wherever the record stands.
// A NaN or an inf anywhere in a record makes a sum NaN (inf - inf in the variance), so k_b is NaN for that record alone.
#include "ccn_device.h"
#include "../../include/ccn_hip.h"

#include <cmath>
#include <cstdint>
#include <string>

namespace ccn {
namespace {

constexpr int kRsThreads = 256, kRsMaxGx = 64;
constexpr int64_t kRsPerBlock = 4096;

int rs_gx(int64_t per)
{
    const int64_t g = (per + kRsPerBlock - 1) / kRsPerBlock;
    return (int)(g < 1 ? 1 : g > kRsMaxGx ? kRsMaxGx : g);
}
size_t rs_factor_bytes(int B) { return ((size_t)B * 4 + 15) / 16 * 16; }

struct Sums { double c, cc, y, yy; };

__device__ __forceinline__ void rs_add(Sums& a, float c, float u, const X0Form& f)
{
    const float y = f.combine(c, u);            // (no k yet: this is what computes it)
    const double dc = (double)c, dy = (double)y;
    a.c += dc; a.cc += dc * dc; a.y += dy; a.yy += dy * dy;
}

template <bool VEC>
__global__ __launch_bounds__(kRsThreads) void rs_partial_kernel(const float* __restrict__ out_c, const float* __restrict__ out_u, float w,
                                                                long long per, double* __restrict__ part)
{
    __shared__ double wsum[kRsThreads / 64][4];
    const int b = blockIdx.y, tid = threadIdx.x;
    const float* c = out_c + (long long)b * per;
    const float* u = out_u + (long long)b * per;
    const long long nq = (per + 3) / 4, nthr = (long long)gridDim.x * kRsThreads;
    Sums a = {0.0, 0.0, 0.0, 0.0};
    X0Form f; f.w = w;
    // four quads of a lane in flight: the loads first, then the adds in increasing q
    for (long long q0 = (long long)blockIdx.x * kRsThreads + tid; q0 < nq; q0 += 4 * nthr) {
        float4 cv[4], uv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long q = q0 + i * nthr;
            cv[i] = make_float4(0.f, 0.f, 0.f, 0.f); uv[i] = cv[i];
            if (q < nq) {
                if constexpr (VEC) { cv[i] = ((const float4*)c)[q]; uv[i] = ((const float4*)u)[q]; }
                else {
                    const long long j = q * 4;
                    cv[i].x = c[j]; uv[i].x = u[j];
                    if (j + 1 < per) { cv[i].y = c[j + 1]; uv[i].y = u[j + 1]; }
                    if (j + 2 < per) { cv[i].z = c[j + 2]; uv[i].z = u[j + 2]; }
                    if (j + 3 < per) { cv[i].w = c[j + 3]; uv[i].w = u[j + 3]; }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long j = (q0 + i * nthr) * 4;
            if (j < per) rs_add(a, cv[i].x, uv[i].x, f);
            if (j + 1 < per) rs_add(a, cv[i].y, uv[i].y, f);
            if (j + 2 < per) rs_add(a, cv[i].z, uv[i].z, f);
            if (j + 3 < per) rs_add(a, cv[i].w, uv[i].w, f);
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        a.c += __shfl_xor(a.c, o); a.cc += __shfl_xor(a.cc, o); a.y += __shfl_xor(a.y, o); a.yy += __shfl_xor(a.yy, o);
    }
    if ((tid & 63) == 0) { double* d = wsum[tid >> 6]; d[0] = a.c; d[1] = a.cc; d[2] = a.y; d[3] = a.yy; }
    __syncthreads();
    if (tid < 4) {
        double t = wsum[0][tid];
#pragma unroll
        for (int v = 1; v < kRsThreads / 64; ++v) t += wsum[v][tid];
        part[((size_t)b * gridDim.x + blockIdx.x) * 4 + tid] = t;
    }
}

__global__ __launch_bounds__(64) void rs_final_kernel(const double* __restrict__ part, int gx, int B, double n, double phi, float* __restrict__ k)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double* p = part + (size_t)b * gx * 4;
    double s[4] = {p[0], p[1], p[2], p[3]};
    for (int g = 1; g < gx; ++g)
        for (int i = 0; i < 4; ++i) s[i] += p[g * 4 + i];
    double var_c = (s[1] - s[0] * s[0] / n) / (n - 1.0), var_y = (s[3] - s[2] * s[2] / n) / (n - 1.0);
    if (var_c < 0.0) var_c = 0.0;                                   // (a NaN stays a NaN)
    if (var_y < 0.0) var_y = 0.0;
    const double std_c = sqrt(var_c), std_y = sqrt(var_y);
    double f = phi * std_c / std_y + (1.0 - phi);
    if (std_y == 0.0 && std_c == std_c) f = 1.0;                    // nothing to rescale
    k[b] = (float)f;
}

}  // namespace

size_t guidance_rescale_scratch_bytes(int B, int64_t per) { return rs_factor_bytes(B) + (size_t)B * rs_gx(per) * 4 * sizeof(double); }
void* guidance_rescale_partials(void* scratch, int B) { return (char*)scratch + rs_factor_bytes(B); }

hipError_t launch_guidance_rescale(const X0Operands& o, double phi, float* k, void* partials, hipStream_t s)
{
    const float *out_c = o.out_c, *out_u = o.out_u, w = o.w;
    const int64_t per = o.per_record, B = o.records;
    if (B <= 0 || B > 65535 || per < 2 || per >= kThrMaxPerRecord || !out_c || !out_u || !k || !partials) return hipErrorInvalidValue;
    const int gx = rs_gx(per);
    const bool vec = !(((uintptr_t)out_c | (uintptr_t)out_u) & 15) && !(per & 3);
    const dim3 grid(gx, (unsigned)B);
    if (vec) hipLaunchKernelGGL((rs_partial_kernel<true>), grid, dim3(kRsThreads), 0, s, out_c, out_u, w, (long long)per, (double*)partials);
    else hipLaunchKernelGGL((rs_partial_kernel<false>), grid, dim3(kRsThreads), 0, s, out_c, out_u, w, (long long)per, (double*)partials);
    hipLaunchKernelGGL(rs_final_kernel, dim3((unsigned)(B + 63) / 64), dim3(64), 0, s, (const double*)partials, gx, (int)B, (double)per, phi, k);
    return hipGetLastError();
}

}  // namespace ccn

using namespace ccn;

int ccn_guidance_rescale_scratch_bytes(int32_t B, int64_t per_record, size_t* bytes)
{
    if (!bytes) return fail(CCN_EINVAL, "null argument");
    X0Operands o;
    o.records = B; o.per_record = per_record;
    if (int rc = check_x0_operands(o, true, false)) return rc;
    *bytes = guidance_rescale_scratch_bytes(B, per_record);
    return CCN_OK;
}

int ccn_guidance_rescale(const float* out_c_dev, const float* out_u_dev, float w, double phi, int32_t B, int64_t per_record, float* k_dev,
                         void* scratch_dev, size_t scratch_bytes, void* stream)
{
    X0Operands o;
    o.out_c = out_c_dev; o.out_u = out_u_dev; o.w = w; o.per_record = per_record; o.records = B;
    if (!k_dev) return fail(CCN_EINVAL, "a tensor pointer is NULL");
    if (int rc = check_x0_operands(o, true)) return rc;
    if (!std::isfinite(w)) return fail(CCN_EINVAL, "the guidance scale must be finite");
    if (!(phi >= 0.0 && phi <= 1.0)) return fail(CCN_EINVAL, "the rescale factor phi must be in [0, 1]");
    if (!scratch_dev || ((uintptr_t)scratch_dev & 15)) return fail(CCN_EINVAL, "the scratch must be non-null and 16-byte aligned");
    const size_t need = guidance_rescale_scratch_bytes(B, per_record);
    if (scratch_bytes < need) return fail(CCN_EINVAL, "the scratch is too small: need " + std::to_string(need) + " bytes");
    if (launch_guidance_rescale(o, phi, k_dev, guidance_rescale_partials(scratch_dev, B), (hipStream_t)stream) != hipSuccess)
        return fail(CCN_EHIP, "guidance_rescale launch failed");
    return CCN_OK;
}
