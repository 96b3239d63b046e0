// Device-side helpers shared by the convolution kernels (types, 16-byte pack/unpack, MFMA wrappers,
// the GroupNorm+SiLU prologue transform).
#pragma once
#include "ccn_internal.h"
#include "ccn_philox.h"

namespace ccn {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

enum { A_NHWC = 0, A_IM2COL = 1 };
enum { EPI_NHWC = 0, EPI_HEAD = 1 };

__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ unsigned pack_bf2(float a, float b) {
    f32x2 v = {a, b};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));   // v_cvt_pk_bf16_f32, RNE
}

// ---- the sampler update of one element (DDIM, and DPM-Solver++ 2M on top of it) ---------------------------------------------------
// Every op rounds to fp32 on its own, like the torch op sequence (diffusion/ddim.py:38-43):
//     x0 = clamp((x - c0*e)/c1, -1, 1);  xn = c2*x0 + c3*e;  c4 != 0:  xn = xn + c4*(x0 - hist)
// `hist` is the previous step's x0 and only enters when c4 != 0 (the caller does not read it otherwise: on step 0 it holds nothing);
// the clamped x0 comes back through `x0_out`, the next step's history.  With c4 == 0 this is the DDIM update, bit for bit.
// sampler_tail is everything after (x0, e): shared by the two parameterisations below.
__device__ __forceinline__ float sampler_tail(float x0, float e, float c2, float c3, float c4, float hist, float& x0_out)
{
    float xn = __fadd_rn(__fmul_rn(c2, x0), __fmul_rn(c3, e));
    if (c4 != 0.f) xn = __fadd_rn(xn, __fmul_rn(c4, __fsub_rn(x0, hist)));
    x0_out = x0;
    return xn;
}
// The x0 prediction before any clamp, either parameterisation.  `pred` is wave-uniform (a kernel argument): PRED_EPS / PRED_V have the
// values of CCN_PRED_EPS / CCN_PRED_V.
// The v-parameterisation: the network output is y = v = a*noise - s*x0, and with the SAME table (c0 = s_t, c1 = a_t)
//     x0 = clamp(c1*x - c0*y, -1, 1);  e = c0*x + c1*y;  then the tail above.
// x0 is formed directly, not as the eps form applied to e: at the noisy end of the cosine table 1/c1 = 6.4e4 and s rounds to 1.0f,
// so (x - c0*e)/c1 cancels to nothing, while c1*x - c0*y has no division and no cancellation (Parameterisation).
enum { PRED_EPS = 0, PRED_V = 1 };
__device__ __forceinline__ float raw_x0_eps(float x, float e, float c0, float c1) { return __fdiv_rn(__fsub_rn(x, __fmul_rn(c0, e)), c1); }
__device__ __forceinline__ float raw_x0_v(float x, float y, float c0, float c1) { return __fsub_rn(__fmul_rn(c1, x), __fmul_rn(c0, y)); }
__device__ __forceinline__ float raw_x0_p(int pred, float x, float y, float c0, float c1)
{
    return pred == PRED_V ? raw_x0_v(x, y, c0, c1) : raw_x0_eps(x, y, c0, c1);
}
// The clamp.  thr false: the static one.  thr true, dynamic thresholding (Thresholding): the record's threshold
// s >= 1 replaces it,  x0 = clamp(raw, -s, s) / s;  s == 1 is the static clamp bit for bit (a division by 1.0f is exact).  A NaN
// threshold (a record whose quantile fell on a NaN) passes fmaxf / fminf through and makes every x0 of that record NaN.
__device__ __forceinline__ float clamped_x0_p(int pred, bool thr, float s, float x, float y, float c0, float c1)
{
    const float r = raw_x0_p(pred, x, y, c0, c1);
    return thr ? __fdiv_rn(fminf(fmaxf(r, -s), s), s) : fminf(fmaxf(r, -1.0f), 1.0f);
}
__device__ __forceinline__ float pred_e(int pred, float x, float y, float c0, float c1)
{
    return pred == PRED_V ? __fadd_rn(__fmul_rn(c0, x), __fmul_rn(c1, y)) : y;
}
// The ONE formation of y, x0 and e ("The same x0"): both head epilogues, every form of sampler_step_kernel, the
// dynamic threshold's quantile (raw), the low-resolution guide's block mean (x0) and the guidance rescale's statistics (combine) go
// through it, so the order statistic and the block mean are taken over the very bits the step clamps and corrects.  A kernel sets the
// parts it has.  Where a flag is the kernel's template argument it is a compile-time constant here too (the struct is a local of an
// inlined caller): a part that is off leaves no instruction behind -- no multiply by k = 1, no division by s = 1, no + 0.
struct X0Form {
    int pred = PRED_EPS;
    float c0 = 0.f, c1 = 1.f;
    bool guided = false, rescaled = false, thr = false, lr = false;
    float w = 0.f, k = 1.f, s = 1.f;       // guided: the guidance scale; rescaled: the record's factor; thr: the record's threshold
    // u + w (c - u) of the two network outputs, three separately rounded ops
    __device__ __forceinline__ float combine(float c, float u) const { return __fadd_rn(u, __fmul_rn(w, __fsub_rn(c, u))); }
    // "the network output" of everything below: the combine when guided (u is not looked at otherwise), times k when rescaled
    __device__ __forceinline__ float y(float c, float u) const
    {
        if (guided) c = combine(c, u);
        return rescaled ? __fmul_rn(k, c) : c;
    }
    __device__ __forceinline__ float raw(float x, float y) const { return raw_x0_p(pred, x, y, c0, c1); }
    __device__ __forceinline__ float x0(float x, float y) const { return clamped_x0_p(pred, thr, s, x, y, c0, c1); }
    __device__ __forceinline__ float e(float x, float y) const { return pred_e(pred, x, y, c0, c1); }
    // the update of one element; lr: the low-resolution guide's correction d of the element's block is added to the clamped x0 first
    // (no re-clamp: |x0'| <= 1 + |d|), and only then -- x0 + 0.0f would turn a -0.0f into +0.0f on its way to the history
    __device__ __forceinline__ float step(float x, float y, float d, float c2, float c3, float c4, float hist, float& x0_out) const
    {
        float v = x0(x, y);
        if (lr) v = __fadd_rn(v, d);
        return sampler_tail(v, e(x, y), c2, c3, c4, hist, x0_out);
    }
};
// The fixed-point form of a value in [-1, 1] that the guide's block sums add: v * 2^30 is exact in fp32 and the conversion rounds to
// nearest even, so a sum of N^2 <= 4096 of them fits int64 with room and is the same in any order.
__device__ __forceinline__ long long guide_fixed(float v) { return __float2ll_rn(__fmul_rn(v, 1073741824.0f)); }

// ---- record-keyed normals (Noise) ----------------------------------------------------------------------------
// Element j of draw d of the record with seed s: the Philox words of quad q = j >> 2 (ccn_philox.h), pair p = (j & 3) >> 1 of them
// through Box-Muller with the precise library functions.  u = ((r >> 9) + 0.5) * 2^-23 is exact in fp32 and inside (0, 1), so
// |n| <= sqrt(-2 ln 2^-24) = 5.768.  draw_quad (a lane owns elements 4q .. 4q+3) and draw_element (one element) run the same
// operations on the same words: the value of an element does not depend on which computed it.
__device__ __forceinline__ float draw_unit(uint32_t r) { return __fmul_rn(__fadd_rn((float)(r >> 9), 0.5f), 1.1920928955078125e-07f); }
__device__ __forceinline__ float draw_radius(uint32_t r) { return sqrtf(__fmul_rn(-2.0f, logf(draw_unit(r)))); }
__device__ __forceinline__ float draw_turn(uint32_t r) { return __fmul_rn(2.0f, draw_unit(r)); }      // cospif / sinpif argument
__device__ __forceinline__ float4 draw_quad(uint64_t seed, uint32_t draw, uint32_t q)
{
    const Philox4 r = draw_words(seed, draw, q);
    const float rad0 = draw_radius(r.v[0]), th0 = draw_turn(r.v[1]), rad1 = draw_radius(r.v[2]), th1 = draw_turn(r.v[3]);
    return make_float4(__fmul_rn(rad0, cospif(th0)), __fmul_rn(rad0, sinpif(th0)), __fmul_rn(rad1, cospif(th1)), __fmul_rn(rad1, sinpif(th1)));
}
__device__ __forceinline__ float draw_element(uint64_t seed, uint32_t draw, int64_t j)
{
    const Philox4 r = draw_words(seed, draw, (uint32_t)(j >> 2));
    const int p = (int)(j & 2);                                     // 2 * pair
    const float rad = draw_radius(r.v[p]), th = draw_turn(r.v[p + 1]);
    return __fmul_rn(rad, (j & 1) ? sinpif(th) : cospif(th));
}

template <typename T> __device__ __forceinline__ float silu_f(float v);
template <> __device__ __forceinline__ float silu_f<float>(float v) { return v / (1.0f + expf(-v)); }
template <> __device__ __forceinline__ float silu_f<__bf16>(float v) { return __fdividef(v, 1.0f + __expf(-v)); }

// 16 bytes of T -> EPC floats and back
template <typename T> struct Vec16;
template <> struct Vec16<float> {
    static constexpr int EPC = 4;
    static __device__ __forceinline__ void unpack(const u32x4& r, float* v) {
        v[0] = __uint_as_float(r.x); v[1] = __uint_as_float(r.y); v[2] = __uint_as_float(r.z); v[3] = __uint_as_float(r.w);
    }
    static __device__ __forceinline__ u32x4 pack(const float* v) {
        return u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
    }
};
template <> struct Vec16<__bf16> {
    static constexpr int EPC = 8;
    static __device__ __forceinline__ void unpack(const u32x4& r, float* v) {
        v[0] = bf_lo(r.x); v[1] = bf_hi(r.x); v[2] = bf_lo(r.y); v[3] = bf_hi(r.y);
        v[4] = bf_lo(r.z); v[5] = bf_hi(r.z); v[6] = bf_lo(r.w); v[7] = bf_hi(r.w);
    }
    static __device__ __forceinline__ u32x4 pack(const float* v) {
        return u32x4{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
    }
};

template <typename T> __device__ __forceinline__ void mfma16(f32x16& acc, const u32x4& a, const u32x4& b);
template <> __device__ __forceinline__ void mfma16<float>(f32x16& acc, const u32x4& a, const u32x4& b) {
    const f32x4 a4 = __builtin_bit_cast(f32x4, a), b4 = __builtin_bit_cast(f32x4, b);
#pragma unroll
    for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[q], b4[q], acc, 0, 0, 0);
}
template <> __device__ __forceinline__ void mfma16<__bf16>(f32x16& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
}

// ---- f16x3: fp32 in memory, fp16 hi + lo operand rows in LDS -----------------------------------------------------------------
// The third operand form of the ws / fr kernels (CCN_DTYPE_F16X3).  Everything on the global side is the fp32 form's (the tag is
// four bytes wide on purpose: every sizeof(T) in the address math stays an fp32 element, and Vec16 / GnCoef are the fp32 ones);
// what differs is the 128-byte LDS row of a pixel's (an output channel's) 32-channel Cin chunk: 32 fp16 "hi" then 32 fp16 "lo",
// x ~= hi + lo to 22-23 bits.  Sixteen-byte unit u of the row (u = 0..3 hi, 4..7 lo; channels 8 (u & 3) .. + 7) sits at the fp32
// form's swizzled position (u ^ (row >> 1)) & 7, so the consumers' fragment reads are those of the other forms: read kk = 0, 1 is
// the hi fragment of K step kk (lane half h holds k = 8h .. 8h + 7 of v_mfma_f32_32x32x16_f16), read 2 + kk its lo fragment.
struct f16x3_t { float v; };
template <> struct Vec16<f16x3_t> : Vec16<float> {};
template <typename T> struct OperandForm { static constexpr bool SPLIT = false; };
template <> struct OperandForm<f16x3_t> { static constexpr bool SPLIT = true; };

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// One 16-byte unit of the fp32 form (four channels) -> the same 16 bytes as {hi[0..3], lo[0..3]}.
// hi = RNE(x) (v_cvt_f16_f32), lo = RNE(x - hi) (the subtraction is exact).  |x| >= 65520 would round to inf: hi saturates to the
// largest finite fp16 and `ovf` is raised (-> bit 2 of the handle's error word); a NaN is flagged and staged as a finite value too.
__device__ __forceinline__ u32x4 split_pack(const u32x4& o, unsigned& ovf)
{
    f16x4 hi, lo;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float x = __uint_as_float(o[e]);
        if (!(fabsf(x) < 65520.0f)) ovf = 1u;
        const float c = fminf(fmaxf(x, -65504.0f), 65504.0f);
        const _Float16 hv = (_Float16)c;
        hi[e] = hv;
        lo[e] = (_Float16)(c - (float)hv);
    }
    const u32x2 h2 = __builtin_bit_cast(u32x2, hi), l2 = __builtin_bit_cast(u32x2, lo);
    return u32x4{h2.x, h2.y, l2.x, l2.y};
}
// ... and into the row of its pixel (`row` = the row's first byte, sw = row index >> 1) as two 8-byte writes: channels 4 ck .. 4 ck + 3
__device__ __forceinline__ void split_store(unsigned char* row, int sw, int ck, const u32x4& p)
{
    const int half = (ck & 1) << 3, u = ck >> 1;
    *(u32x2*)(row + (((u ^ sw) & 7) << 4) + half) = u32x2{p.x, p.y};
    *(u32x2*)(row + ((((u | 4) ^ sw) & 7) << 4) + half) = u32x2{p.z, p.w};
}
__device__ __forceinline__ void split_put(unsigned char* row, int sw, int ck, const u32x4& o, unsigned& ovf)
{
    split_store(row, sw, ck, split_pack(o, ovf));
}

// one v_mfma_f32_32x32x16_f16 on two fp16 fragments of a split row
__device__ __forceinline__ void mfma_f16(f32x16& acc, const u32x4& a, const u32x4& b)
{
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
}

// v_mfma_f32_16x16x32_bf16 on quarter q (registers 4q .. 4q+3) of a 16-register accumulator tuple
typedef float f32x4q __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void mfma16q(f32x16& acc, const int q, const u32x4& a, const u32x4& b) {
    f32x4q t = {acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]};
    t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), t, 0, 0, 0);
    acc[4 * q] = t[0]; acc[4 * q + 1] = t[1]; acc[4 * q + 2] = t[2]; acc[4 * q + 3] = t[3];
}


// ---- GroupNorm-apply (+ SiLU) on one 16-byte chunk while staging the A operand ----------------------------
// fp32 (parity mode): y = fma(x, a, c); silu(y) = y / (1 + expf(-y)) with full-precision expf and a true division.
// bf16 (throughput mode): packed fp32 math, exp2 with log2(e) folded into a second scale/shift pair, v_rcp.
template <typename T> struct GnCoef;
template <> struct GnCoef<float> {
    float a[4], c[4];
    // vector loads issued together, ONE branch (a per-element select makes hipcc wait for each load in turn)
    __device__ __forceinline__ void load(const float2* ab, bool valid) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = 1.f; c[e] = 0.f; }
        if (valid) {
            // table layout per channel pair: {scale(2p), scale(2p+1), shift(2p), shift(2p+1)}
            const f32x4 v0 = *(const f32x4*)ab, v1 = *(const f32x4*)(ab + 2);
            a[0] = v0[0]; a[1] = v0[1]; c[0] = v0[2]; c[1] = v0[3];
            a[2] = v1[0]; a[3] = v1[1]; c[2] = v1[2]; c[3] = v1[3];
        }
    }
    template <bool SILU> __device__ __forceinline__ u32x4 apply(const u32x4& raw) const {
        float v[4];
        Vec16<float>::unpack(raw, v);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float y = fmaf(v[e], a[e], c[e]);
            if (SILU) y = y / (1.0f + expf(-y));
            v[e] = y;
        }
        return Vec16<float>::pack(v);
    }
};
template <> struct GnCoef<f16x3_t> : GnCoef<float> {};     // f16x3: the parity mode's transform, bit for bit
// NO packed-fp32 instructions (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32) here or anywhere in a producer wave: next to a
// wave that streams MFMAs they are starved outright -- tools/ubench/dump_vs_mfma.hip: this transform goes from 150 to
// >2300 cycles per 16 bytes as soon as one v_pk_mul_f32 is in it, while v_fma_f32 / v_mul_f32 / v_exp_f32 lose ~25 %.
// The file is built with -fno-slp-vectorize so that scalar code stays scalar.
template <> struct GnCoef<__bf16> {
    float a[8], c[8];
    __device__ __forceinline__ void load(const float2* ab, bool valid) {
        f32x4 v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = f32x4{1.f, 1.f, 0.f, 0.f};
        if (valid) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = *(const f32x4*)(ab + 2 * e);        // 4 x 16 B, all in flight together
        }
        // pair-interleaved table {scale, scale, shift, shift}: pure renaming, nothing here waits for the loads
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[2 * e] = v[e][0]; a[2 * e + 1] = v[e][1]; c[2 * e] = v[e][2]; c[2 * e + 1] = v[e][3]; }
    }
    // scale = gamma * rstd, shift = beta - mean * scale from raw affine parameters and a group's statistics
    __device__ __forceinline__ void from_raw(const f32x4* g, const f32x4* bt, float mean, float rstd, bool valid) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float sc = g[e >> 2][e & 3] * rstd;
            a[e] = valid ? sc : 1.f;
            c[e] = valid ? fmaf(-mean, sc, bt[e >> 2][e & 3]) : 0.f;
        }
    }
    template <bool SILU> __device__ __forceinline__ u32x4 apply(const u32x4& raw) const {
        const float nl2e = -1.4426950408889634f;
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned u = raw[e];
            float y0 = fmaf(bf_lo(u), a[2 * e], c[2 * e]), y1 = fmaf(bf_hi(u), a[2 * e + 1], c[2 * e + 1]);
            if (SILU) {
                const float d0 = __builtin_amdgcn_exp2f(y0 * nl2e) + 1.0f, d1 = __builtin_amdgcn_exp2f(y1 * nl2e) + 1.0f;
                y0 *= __builtin_amdgcn_rcpf(d0); y1 *= __builtin_amdgcn_rcpf(d1);
            }
            o[e] = pack_bf2(y0, y1);
        }
        return o;
    }
};


// ---- GroupNorm partial sums: write-through publish + last-arriver finalize ---------------------------------------------
// Hand-off between workgroups of ONE launch, placement-independent (cdna_hip_programming.md Guideline 16, R1 with an
// arrival counter): every partial is ONE 8-byte agent-scope (sc1, write-through) store; every storing wave drains its
// stores; workgroup barrier; one lane adds to the sample's counter; the workgroup whose add returns fin_blocks-1 is the
// last one: one agent-scope acquire, barrier, sc1 loads of every partial of that sample in a fixed order.
__device__ __forceinline__ void part_store(float2* p, float s1, float s2)
{
    const unsigned long long v = ((unsigned long long)__float_as_uint(s2) << 32) | __float_as_uint(s1);
    __hip_atomic_store((unsigned long long*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float2 part_load(const float2* p)
{
    const unsigned long long v = __hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return make_float2(__uint_as_float((unsigned)v), __uint_as_float((unsigned)(v >> 32)));
}

// mean and 1/sqrt(var + eps) of group g of sample b from its partial sums; one wave per group, fixed summation order;
// every lane returns the result
__device__ __forceinline__ void gn_group_stats(const float2* part, int b, int g, int G, int nslot, int n_nt, int bn, int cpg,
                                               double count, float eps, int lane, double& mean, double& rstd)
{
    const int jlo = (g * cpg) / bn, jhi = ((g + 1) * cpg - 1) / bn, nj = jhi - jlo + 1;
    const int n_sp = nslot / n_nt, ne = n_sp * nj;
    const float2* base = part + (size_t)(b * G + g) * nslot;
    double s1 = 0.0, s2 = 0.0;
    for (int e = lane; e < ne; e += 64) {
        const int sp = e / nj, j = jlo + (e - sp * nj);
        const float2 v = part_load(base + (size_t)sp * n_nt + j);
        s1 += (double)v.x; s2 += (double)v.y;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { s1 += __shfl_xor(s1, s); s2 += __shfl_xor(s2, s); }
    mean = s1 / count;
    double var = s2 / count - mean * mean;
    if (var < 0.0) var = 0.0;
    rstd = 1.0 / sqrt(var + (double)eps);
}

// scale/shift of every channel of group g of sample b from its partial sums
__device__ __forceinline__ void gn_reduce_group(const float2* part, int b, int g, int G, int nslot, int n_nt, int bn, int cpg, int C,
                                                double count, const float* gamma, const float* beta, float eps, float2* ab, int lane)
{
    double mean, rstd;
    gn_group_stats(part, b, g, G, nslot, n_nt, bn, cpg, count, eps, lane, mean, rstd);
    for (int c = g * cpg + lane; c < (g + 1) * cpg; c += 64) {
        const double sc = (double)gamma[c] * rstd;
        // pair-interleaved: channels (2p, 2p+1) -> {scale, scale, shift, shift} (see GnCoef::load)
        float* const row = (float*)(ab + (size_t)b * C) + 4 * (c >> 1) + (c & 1);
        row[0] = (float)sc; row[2] = (float)((double)beta[c] - mean * sc);
    }
}

// call with ALL threads of the workgroup after its part_store()s; `flag` is a free LDS word
template <int NT>
__device__ __forceinline__ void gn_fused_finalize(const ConvArgs& a, int b, unsigned* flag, int tid)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");            // every storing wave drains its write-through stores
    __syncthreads();
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(a.fin_counter + b, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = (old == (unsigned)a.fin_blocks - 1u) ? 1u : 0u;
    }
    __syncthreads();
    if (*flag == 0u) return;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (int g = wave; g < a.G; g += NT / 64)
        gn_reduce_group(a.part, b, g, a.G, a.nslot, a.n_nt, a.bn, a.cpg, a.Cout, a.fin_count, a.fin_gamma, a.fin_beta, 1e-5f, a.fin_ab, lane);
    if (tid == 0) __hip_atomic_store(a.fin_counter + b, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
}

}  // namespace ccn
