// Seeded device noise: fills a (B, per_record) fp32 tensor with the normals of one draw, row b from seeds[b] (ccn_normal_fill).
// The generator itself is ccn_philox.h (integer core) + draw_quad / draw_element of ccn_device.h; the sampler-step kernel
// (ccn_kernels.hip) calls the same two functions, so a filled tensor and the generated-in-place noise agree bit for bit.
#include "ccn_device.h"
#include "../../include/ccn_hip.h"

#include <cstdint>
#include <string>

namespace ccn {
namespace {

// grid (x, B): row blockIdx.y.  A row that starts 16-byte aligned goes a quad per lane with one 16-byte store each, its per % 4 tail
// an element per lane; a row that does not goes an element per lane throughout (4-byte stores, coalesced across the wave).
__global__ __launch_bounds__(256) void normal_fill_kernel(float* __restrict__ out, const uint64_t* __restrict__ seeds, int64_t per, uint32_t draw)
{
    const int b = blockIdx.y;
    const uint64_t seed = seeds[b];
    float* row = out + (size_t)b * (size_t)per;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    const int64_t nq = ((uintptr_t)row & 15) ? 0 : per >> 2;       // block-uniform
    for (int64_t q = tid; q < nq; q += nthr) ((float4*)row)[q] = draw_quad(seed, draw, (uint32_t)q);
    for (int64_t j = nq * 4 + tid; j < per; j += nthr) row[j] = draw_element(seed, draw, j);
}

}  // namespace
}  // namespace ccn

using namespace ccn;

int ccn_normal_fill(float* out_dev, const uint64_t* seeds_dev, int32_t B, int64_t per_record, uint32_t draw, void* stream)
{
    if (!out_dev || !seeds_dev) return fail(CCN_EINVAL, "a buffer is NULL");
    if (((uintptr_t)out_dev & 3) || ((uintptr_t)seeds_dev & 7)) return fail(CCN_EINVAL, "out_dev must be 4-byte and seeds_dev 8-byte aligned");
    if (B <= 0 || B > 65535 || per_record <= 0) return fail(CCN_EINVAL, "B must be in [1, 65535] and per_record positive");
    if (per_record >= kDrawMaxPerRecord) return fail(CCN_EINVAL, "per_record must be below 2^34: the quad index is one 32-bit counter word");
    // sized for the quad path (the common one); an unaligned row strides the same grid four times as often
    const int64_t blocks = ((per_record + 3) / 4 + 255) / 256;
    const int gx = (int)(blocks < 1024 ? blocks : 1024);
    hipLaunchKernelGGL(normal_fill_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, out_dev, seeds_dev, per_record, draw);
    if (hipGetLastError() != hipSuccess) return fail(CCN_EHIP, "normal_fill launch failed");
    return CCN_OK;
}
