// Known-answer test: does v_mfma_f32_32x32x16_f16 keep fp16 SUBNORMAL A / B operands (hipcc's default MODE.denorm), or flush them?
// The f16x3 mode stores the low half of every activation below 2^-3 as an fp16 subnormal, so a flush would
// cost it 100x in accuracy.  One wave, one MFMA per case, every product and sum exact in fp32:
//   A[i][k] = (i % 4 + 1) (k + 1) ua,  B[k][j] = (j + 1) ub   ->   D[i][j] = 136 (i % 4 + 1) (j + 1) ua ub
// with ua, ub = 2^-24 (the fp16 subnormal unit: every operand value is a subnormal) or 1 (normals).
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 mfma_f16_subnormals.hip -o mfma_f16_subnormals && ./mfma_f16_subnormals
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(64) void one_mfma(const _Float16* __restrict__ A, const _Float16* __restrict__ B, float* __restrict__ D)
{
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    f16x8 a, b;
    for (int e = 0; e < 8; ++e) { a[e] = A[r * 16 + 8 * h + e]; b[e] = B[(8 * h + e) * 32 + r]; }   // lane half h holds k = 8h .. 8h + 7
    f32x16 acc;
    for (int q = 0; q < 16; ++q) acc[q] = 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
    for (int q = 0; q < 16; ++q) D[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + r] = acc[q];
}

int main()
{
    _Float16 *A, *B; float* D;
    if (hipMallocManaged(&A, 32 * 16 * 2) != hipSuccess || hipMallocManaged(&B, 16 * 32 * 2) != hipSuccess || hipMallocManaged(&D, 32 * 32 * 4) != hipSuccess) {
        printf("hipMallocManaged failed\n");
        return 2;
    }
    const char* names[4] = {"A normal    x B normal   ", "A subnormal x B normal   ", "A normal    x B subnormal", "A subnormal x B subnormal"};
    int kept = 0;
    for (int c = 0; c < 4; ++c) {
        const float ua = (c & 1) ? ldexpf(1.f, -24) : 1.f, ub = (c & 2) ? ldexpf(1.f, -24) : 1.f;
        for (int i = 0; i < 32; ++i) for (int k = 0; k < 16; ++k) A[i * 16 + k] = (_Float16)((float)((i % 4 + 1) * (k + 1)) * ua);
        for (int k = 0; k < 16; ++k) for (int j = 0; j < 32; ++j) B[k * 32 + j] = (_Float16)((float)(j + 1) * ub);
        one_mfma<<<1, 64>>>(A, B, D);
        if (hipDeviceSynchronize() != hipSuccess) { printf("kernel failed\n"); return 2; }
        int bad = 0, zero = 0;
        for (int i = 0; i < 32; ++i)
            for (int j = 0; j < 32; ++j) {
                const float want = 136.f * (float)((i % 4 + 1) * (j + 1)) * ua * ub;
                if (D[i * 32 + j] != want) ++bad;
                if (D[i * 32 + j] == 0.f) ++zero;
            }
        printf("%s: %4d of 1024 outputs differ from the exact sum, %4d are zero  (D[3][31] = %.9g, exact %.9g)\n", names[c], bad, zero,
               (double)D[3 * 32 + 31], (double)(136.f * 4.f * 32.f * ua * ub));
        if (c && !bad) ++kept;
    }
    printf("verdict: fp16 subnormal MFMA operands are %s\n", kept == 3 ? "KEPT (exact results in all three subnormal cases)" : "NOT all kept: see above");
    return 0;
}
