// Hand-written gfx950 (CDNA4) kernels of the DDIM reconstruction path.
//
//   conv_igemm_kernel   every convolution of CLIPCondUNet as an LDS-tiled implicit GEMM on MFMA:
//                       3x3 s1 (models/blocks.py:34,36), 3x3 s2 (models/unet.py:63), ConvTranspose 4x4 s2 as four
//                       2x2-tap parity sub-convolutions (models/unet.py:75), stem (models/unet.py:55, im2col K=27)
//                       and head (models/unet.py:79) with the DDIM update (diffusion/ddim.py:34-45) in its epilogue.
//                       Prologue fusion: GroupNorm-apply + SiLU while staging the input halo tile (blocks.py:41,43).
//                       Epilogue fusion: bias, FiLM (blocks.py:22-25), residual / skip add (blocks.py:44, unet.py:104),
//                       and the NEXT GroupNorm's partial sums, so a normalised tensor is never re-read for statistics.
//   gn_finalize_kernel  partial sums -> per-(sample, channel) scale/shift (fp64 combine).
//   linear/temb         conditioning vector and FiLM tables for every step, computed once before the loop.
//   sampler_step/q_sample  stand-alone elementwise forms.
//
// Layout: activations NHWC (channel-contiguous), element type T = float (parity mode, v_mfma_f32_32x32x2_f32,
// bit-identical to an fmaf chain) or bf16 (throughput mode, v_mfma_f32_32x32x16_bf16, fp32 accumulate).
// Both types use the same byte geometry: one LDS row = 128 B = 8 chunks of 16 B = 32 floats or 64 bf16; lane
// half h reads chunk 2*kk+h of its A row (a pixel) and of its B row (an output channel), so the K order seen by
// the two operands is identical by construction.  LDS rows are XOR-swizzled by ((row>>1)&7) at 16-B granularity:
// 32 consecutive rows read at one chunk index hit 16 distinct 16-B slots per ds_read_b128 lane group.
#include "ccn_conv_tile.h"

#include <array>
#include <utility>

namespace ccn {

__host__ __device__ constexpr int cmax(int a, int b) { return a > b ? a : b; }

template <int AK, int IS> struct HaloGeom {
    static constexpr int HOFF = AK == A_NHWC ? 1 : 0;
    // IS*(TH-1)+3 with TH = 4; one more row at stride 2 so that a 4x4 kernel (taps -1..2: the data gradient of the
    // ConvTranspose, ccn_train.hip) fits the same staging
    static constexpr int ROWS = AK == A_NHWC ? (IS == 1 ? 6 : 10) : 4;
    static constexpr int PITCH = AK == A_NHWC ? (IS == 1 ? 34 : 66) : 32;  // >= IS*(TW-1)+3 with TW = 32
    static constexpr int BYTES = ROWS * PITCH * 128;
};
template <int AK, int IS, int BN> struct LdsGeom {
    static constexpr int A_BYTES = HaloGeom<AK, IS>::BYTES;
    static constexpr int B_BYTES = BN * 128;
    static constexpr int TOTAL = EpiLds<4, BN, 4>::total(A_BYTES + 2 * B_BYTES);
};

template <typename T, int AK, int IS, int EPI, int WM, int WN, int MF, int NF>
__global__ __launch_bounds__(256) void conv_igemm_kernel(const ConvArgs a)
{
    static_assert(WM * WN == 4 && WM * MF == 4, "4 waves, 4 M-fragments of 32 pixels (TH=4 rows of TW=32)");
    constexpr int BN = WN * NF * 32;
    constexpr int EPC = Vec16<T>::EPC;
    constexpr int CKE = 8 * EPC;
    using HG = HaloGeom<AK, IS>;
    using LG = LdsGeom<AK, IS, BN>;
    constexpr int TH = 4, NWAVES = 4;
    using E = EpiLds<TH, BN, NWAVES>;               // the epilogue's fp32 tile and reduction scratch, over the loop's buffers
    constexpr int HPITCH = HG::PITCH;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const As = smem;
    unsigned char* const Bs = smem + LG::A_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;

#include "tile/decode.inc"              // -> b, ty, tx, par, nt; my0, mx0, n0; py, px_, par_off

    const unsigned char* const wbase = (const unsigned char*)a.w;
    const unsigned char* const inb = (const unsigned char*)a.in;

    // ---- weight (B operand) staging: global -> registers -> LDS, double buffered -----------------
    constexpr int BU = BN * 8 / 256;
    u32x4 breg[BU];
#define CCN_LOAD_B(IT)                                                                                              \
    {                                                                                                               \
        const int chunk_ = (IT) / a.ntaps, tap_ = (IT) - chunk_ * a.ntaps;                                          \
        const int wt_ = a.tapinfo_w(par_off + tap_);                                                                \
        _Pragma("unroll") for (int u = 0; u < BU; ++u) {                                                            \
            const int idx = tid + 256 * u, n = idx >> 3, ck = idx & 7;                                              \
            const size_t off = ((size_t)(wt_ * a.Cout_pad + n0 + n) * a.Cin_pad + (size_t)chunk_ * CKE) * sizeof(T) + ck * 16; \
            breg[u] = *(const u32x4*)(wbase + off);                                                                 \
        }                                                                                                           \
    }
#define CCN_STORE_B(BUF)                                                                                            \
    {                                                                                                               \
        _Pragma("unroll") for (int u = 0; u < BU; ++u) {                                                            \
            const int idx = tid + 256 * u, n = idx >> 3, ck = idx & 7;                                              \
            *(u32x4*)(Bs + (BUF) * LG::B_BYTES + n * 128 + (((ck ^ (n >> 1)) & 7) << 4)) = breg[u];                \
        }                                                                                                           \
    }

    // ---- input (A operand) staging ---------------------------------------------------------------
    auto stage_A = [&](int chunk) __attribute__((always_inline)) {
        const int ck = tid & 7;
        if constexpr (AK == A_NHWC) {
            constexpr int AU = HG::ROWS * HPITCH * 8;
            constexpr int AIT = (AU + 255) / 256;
            constexpr int GRP = 7;
            const int cbase = chunk * CKE + ck * EPC;
            const bool cvalid = cbase < a.Cin;
            const bool gn = a.gn_ab != nullptr;
            GnCoef<T> gk;
            gk.load(a.gn_ab + (size_t)b * a.Cin + (cvalid ? cbase : 0), gn && cvalid);
            const int iy0 = IS * my0 - 1, ix0 = IS * mx0 - 1;
#pragma unroll
            for (int g0 = 0; g0 < AIT; g0 += GRP) {
                u32x4 raw[GRP]; unsigned okm = 0;
#pragma unroll
                for (int u = 0; u < GRP; ++u) {
                    const int i = g0 + u;
                    raw[u] = u32x4{0u, 0u, 0u, 0u};
                    if (i < AIT) {
                        const int px = (tid >> 3) + 32 * i;
                        const int hy = px / HPITCH, hx = px - hy * HPITCH;
                        const int iy = iy0 + hy, ix = ix0 + hx;
                        const bool okv = px < HG::ROWS * HPITCH && cvalid && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
                        if (okv) {
                            okm |= 1u << u;
                            raw[u] = *(const u32x4*)(inb + (((size_t)(b * a.Hin + iy) * a.Win + ix) * a.Cin + cbase) * sizeof(T));
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < GRP; ++u) {
                    const int i = g0 + u;
                    if (i < AIT) {
                        const int px = (tid >> 3) + 32 * i;
                        if (px < HG::ROWS * HPITCH) {
                            u32x4 o = raw[u];
                            if (((okm >> u) & 1u) && gn)       // zero padding applies AFTER GroupNorm+SiLU; head: no SiLU (unet.py:105)
                                o = gk.template apply<EPI == EPI_NHWC>(raw[u]);
                            *(u32x4*)(As + px * 128 + (((ck ^ (px >> 1)) & 7) << 4)) = o;
                        }
                    }
                }
            }
        } else {   // A_IM2COL: stem, K = Cin*9 taken from the NCHW fp32 image; row m = pixel of the 4x32 tile
            const float* xin = (const float*)a.in;
            const int kreal = a.Cin * 9;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int m = (tid >> 3) + 32 * i;
                const int y = my0 + (m >> 5), x = mx0 + (m & 31);
                float v[EPC];
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const int k = chunk * CKE + ck * EPC + e;
                    float val = 0.0f;
                    if (k < kreal) {
                        const int ci = k / 9, tp = k - ci * 9, ky = tp / 3, kx = tp - ky * 3;
                        const int iy = y + ky - 1, ix = x + kx - 1;
                        if (iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win)
                            val = xin[((size_t)(b * a.Cin + ci) * a.Hin + iy) * a.Win + ix];
                    }
                    v[e] = val;
                }
                *(u32x4*)(As + m * 128 + (((ck ^ (m >> 1)) & 7) << 4)) = Vec16<T>::pack(v);
            }
        }
    };

    // ---- main loop: (Cin chunk) x (tap), one barrier per iteration -------------------------------
    f32x16 acc[MF][NF];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.0f;

    int pbase[MF], nrow[NF];
#pragma unroll
    for (int i = 0; i < MF; ++i) pbase[i] = (IS * (wm * MF + i) + HG::HOFF) * HPITCH + IS * r + HG::HOFF;
#pragma unroll
    for (int j = 0; j < NF; ++j) nrow[j] = (wn * NF + j) * 32 + r;

    const int n_it = a.nchunk * a.ntaps;
    CCN_LOAD_B(0)
    for (int it = 0; it < n_it; ++it) {
        const int chunk = it / a.ntaps, tap = it - chunk * a.ntaps;
        if (tap == 0) {
            if (it > 0) __syncthreads();
            stage_A(chunk);
        }
        CCN_STORE_B(it & 1)
        __syncthreads();
        if (it + 1 < n_it) CCN_LOAD_B(it + 1)
        const int dy = a.tapinfo_dy(par_off + tap), dx = a.tapinfo_dx(par_off + tap);
        const unsigned char* const Bb = Bs + (it & 1) * LG::B_BYTES;
        int pa[MF];
#pragma unroll
        for (int i = 0; i < MF; ++i) pa[i] = pbase[i] + dy * HPITCH + dx;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            u32x4 av[MF], bv[NF];
#pragma unroll
            for (int i = 0; i < MF; ++i)
                av[i] = *(const u32x4*)(As + pa[i] * 128 + ((((2 * kk + h) ^ (pa[i] >> 1)) & 7) << 4));
#pragma unroll
            for (int j = 0; j < NF; ++j)
                bv[j] = *(const u32x4*)(Bb + nrow[j] * 128 + ((((2 * kk + h) ^ (nrow[j] >> 1)) & 7) << 4));
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int j = 0; j < NF; ++j) mfma16<T>(acc[i][j], av[i], bv[j]);
        }
    }

#undef CCN_LOAD_B
#undef CCN_STORE_B
    // ---- epilogue: accumulators -> LDS fp32 tile -> coalesced 16-B rows ----------------------------
    __syncthreads();
    float* const Cs = (float*)smem;
    constexpr int CP = E::CP;
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int m = (wm * MF + i) * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
                Cs[m * CP + (wn * NF + j) * 32 + r] = acc[i][j][q];
            }
    __syncthreads();

    if constexpr (EPI == EPI_HEAD) {
        if (tid < 128) {
            const int m = tid, my = my0 + (m >> 5), mx = mx0 + (m & 31);
            if (my < a.MH && mx < a.MW) {
                for (int c = 0; c < a.Cout; ++c) {
                    const float e = Cs[m * CP + c] + a.bias[c];
                    const size_t idx = ((size_t)(b * a.Cout + c) * a.Hout + my) * a.Wout + mx;
                    if (a.eps_out) a.eps_out[idx] = e;
                    if (a.do_ddim) {
                        // diffusion/ddim.py:38-43 -- every op rounds to fp32 separately, like the torch ops; x0_hist (multistep
                        // sampler): the previous step's x0 enters with c4 and this step's replaces it
                        const float x = a.x_state[idx];
                        const float c4 = a.x0_hist ? a.c4 : 0.f;
                        const float hv = c4 != 0.f ? a.x0_hist[idx] : 0.f;
                        float x0;
                        X0Form f;
                        f.pred = a.pred; f.c0 = a.c0; f.c1 = a.c1;
                        float xn = f.step(x, e, 0.f, a.c2, a.c3, c4, hv, x0);
                        if (a.noise) xn = __fadd_rn(xn, __fmul_rn(a.sigma, a.noise[idx]));      // eta > 0 (diffusion/ddim.py:44-45)
                        if (a.x0_hist) a.x0_hist[idx] = x0;
                        a.x_state[idx] = xn;
                    }
                }
            }
        }
    } else {
        constexpr int NOCT = BN / 8, PSL = 256 / NOCT, NIT = 128 / PSL;
        const int o = tid % NOCT, ps = tid / NOCT;
        const int nb = n0 + o * 8;
        const bool nvalid = nb < a.Cout;
        float bias8[8], f1[8], f2[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { bias8[e] = 0.f; f1[e] = 1.f; f2[e] = 0.f; }
        if (nvalid) {
#pragma unroll
            for (int e = 0; e < 8; ++e) bias8[e] = a.bias[nb + e];
            if (a.film) {
                const float* fp = a.film + (size_t)b * a.film_bstride;
#pragma unroll
                for (int e = 0; e < 8; ++e) { f1[e] = 1.0f + fp[nb + e]; f2[e] = fp[a.Cout + nb + e]; }
            }
        }
        float s1[8], s2[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
        unsigned char* const outb = (unsigned char*)a.out;
        const unsigned char* const resb = (const unsigned char*)a.res;
#pragma unroll
        for (int itp = 0; itp < NIT; ++itp) {
            const int m = itp * PSL + ps;
            const int my = my0 + (m >> 5), mx = mx0 + (m & 31);
            if (nvalid && my < a.MH && mx < a.MW) {
                const int oy = my * a.OS + py, ox = mx * a.OS + px_;
                const size_t eoff = ((size_t)(b * a.Hout + oy) * a.Wout + ox) * a.Cout + nb;
                float v[8];
                const f32x4 c0 = *(const f32x4*)(Cs + m * CP + o * 8), c1 = *(const f32x4*)(Cs + m * CP + o * 8 + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[e] = c0[e]; v[4 + e] = c1[e]; }
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = fmaf(v[e] + bias8[e], f1[e], f2[e]);
                if (resb) {
                    float rv[8];
                    if constexpr (EPC == 8) {
                        Vec16<T>::unpack(*(const u32x4*)(resb + eoff * sizeof(T)), rv);
                    } else {
                        Vec16<T>::unpack(*(const u32x4*)(resb + eoff * sizeof(T)), rv);
                        Vec16<T>::unpack(*(const u32x4*)(resb + eoff * sizeof(T) + 16), rv + 4);
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] += rv[e];
                }
                if constexpr (EPC == 8) {
                    *(u32x4*)(outb + eoff * sizeof(T)) = Vec16<T>::pack(v);
                } else {
                    *(u32x4*)(outb + eoff * sizeof(T)) = Vec16<T>::pack(v);
                    *(u32x4*)(outb + eoff * sizeof(T) + 16) = Vec16<T>::pack(v + 4);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) { s1[e] += v[e]; s2[e] = fmaf(v[e], v[e], s2[e]); }
            }
        }
        if (a.part) {
#include "tile/gn_part_tail.inc"        // s1, s2 -> GroupNorm partials (-> in-kernel finalize)
        }
    }
}

// ---- dispatch ----------------------------------------------------------------------------------------
int conv_bn_for(int cout, int kind)
{
    if (kind == KIND_HEAD) return 32;
    if (cout >= 128) return 128;
    if (cout >= 64) return 64;
    return 32;
}

template <int AK, int IS> static size_t lds_for(int bn)
{
    switch (bn) {
        case 128: return LdsGeom<AK, IS, 128>::TOTAL;
        case 64: return LdsGeom<AK, IS, 64>::TOTAL;
        default: return LdsGeom<AK, IS, 32>::TOTAL;
    }
}
size_t conv_lds_bytes(int dtype, int kind, int bn)
{
    (void)dtype;
    switch (kind) {
        case KIND_C3S2: return lds_for<A_NHWC, 2>(bn);
        case KIND_STEM: return lds_for<A_IM2COL, 1>(bn);
        default: return lds_for<A_NHWC, 1>(bn);
    }
}

typedef void (*conv_fn_t)(const ConvArgs);

template <typename T, int AK, int IS> static conv_fn_t pick_bn(int bn)
{
    switch (bn) {
        case 128: return conv_igemm_kernel<T, AK, IS, EPI_NHWC, 2, 2, 2, 2>;
        case 64: return conv_igemm_kernel<T, AK, IS, EPI_NHWC, 2, 2, 2, 1>;
        default: return conv_igemm_kernel<T, AK, IS, EPI_NHWC, 4, 1, 1, 1>;
    }
}
template <typename T> static conv_fn_t pick_kind(int kind, int bn)
{
    switch (kind) {
        case KIND_C3S2: return pick_bn<T, A_NHWC, 2>(bn);
        case KIND_STEM: return pick_bn<T, A_IM2COL, 1>(bn);
        case KIND_HEAD: return conv_igemm_kernel<T, A_NHWC, 1, EPI_HEAD, 4, 1, 1, 1>;
        default: return pick_bn<T, A_NHWC, 1>(bn);
    }
}
static conv_fn_t pick(int dtype, int kind, int bn)
{
    return dtype == 0 ? pick_kind<float>(kind, bn) : pick_kind<__bf16>(kind, bn);
}

hipError_t conv_prepare()
{
    static const int kinds[] = {KIND_C3S1, KIND_C3S2, KIND_STEM, KIND_HEAD};
    static const int bns[] = {32, 64, 128};
    for (int dt = 0; dt < 2; ++dt)
        for (int kind : kinds)
            for (int bn : bns) {
                if (kind == KIND_HEAD && bn != 32) continue;
                hipError_t e = hipFuncSetAttribute((const void*)pick(dt, kind, bn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)conv_lds_bytes(dt, kind, bn));
                if (e != hipSuccess) return e;
            }
    hipError_t e;
    if ((e = conv_ws_prepare()) != hipSuccess) return e;
    if ((e = conv_fr_prepare()) != hipSuccess) return e;
    return conv_pr_prepare();
}

bool conv_ws_enabled()
{
    static const int on = diag_env("CCN_CONV_V1") ? 0 : 1;      // CCN_CONV_V1=1: A/B switch back to the 4-wave kernel
    return on != 0;
}

int conv_tile_rows(int kind, int bn, int B, int MH, int MW, int npar, int n_nt)
{
    if (!conv_ws_enabled() || !conv_ws_supported(kind, bn)) return 4;
    // 8-row tiles halve the weight traffic through L2 and LDS (the 4-row tile is LDS-bandwidth bound: 1 KB of
    // fragment reads per MFMA plus 32 B/clk of weight ds_writes) and cut the halo overhead; keep every CU busy
    const long blocks8 = (long)B * ((MH + 7) / 8) * ((MW + 31) / 32) * npar * n_nt;
    static const long min8 = diag_env("CCN_MIN8") ? atol(diag_env("CCN_MIN8")) : 256;
    return blocks8 >= min8 ? 8 : 4;
}

// 0 (or 1) ws everywhere, 2 free-running everywhere, 3 free-running on 8-row tiles, 4 (default) persistent
// register-weight kernel where it applies, else as 3; 5 = 4 without the fixed-geometry instantiations of that kernel (every launch
// takes the run-time form).  CCN_CONV_DMA overrides; tests switch it between handles.
static int g_conv_variant = -1;
static int conv_variant()
{
    if (g_conv_variant < 0) g_conv_variant = diag_env("CCN_CONV_DMA") ? atoi(diag_env("CCN_CONV_DMA")) : 4;
    return g_conv_variant;
}
extern "C" int ccn_internal_set_conv_variant(int v) { const int old = conv_variant(); g_conv_variant = v; return old; }

bool conv_pr_selected(int dtype, int kind, int bn, int th)
{
    return dtype == 1 && conv_ws_enabled() && (conv_variant() == 4 || conv_variant() == 5) && conv_pr_supported(kind, bn, th);
}
bool conv_pr_geom_enabled() { return conv_variant() == 4; }

ConvGeom conv_geom(int kind, bool four, int Hin, int Win, int th)
{
    ConvGeom g{};
    switch (kind) {
        case KIND_C3S2: g.Hout = (Hin - 1) / 2 + 1; g.Wout = (Win - 1) / 2 + 1; g.MH = g.Hout; g.MW = g.Wout; g.OS = 1; g.npar = 1; g.ntaps = four ? 16 : 9; break;
        case KIND_CT4: g.Hout = Hin * 2; g.Wout = Win * 2; g.MH = Hin; g.MW = Win; g.OS = 2; g.npar = 4; g.ntaps = 4; break;
        case KIND_STEM: g.Hout = Hin; g.Wout = Win; g.MH = Hin; g.MW = Win; g.OS = 1; g.npar = 1; g.ntaps = 1; break;
        default: g.Hout = Hin; g.Wout = Win; g.MH = Hin; g.MW = Win; g.OS = 1; g.npar = 1; g.ntaps = 9; break;
    }
    g.n_ty = (g.MH + th - 1) / th; g.n_tx = (g.MW + 31) / 32;
    return g;
}

void fill_taps(int* tapinfo, int kind, bool four)
{
    for (int i = 0; i < 16; ++i) tapinfo[i] = 0;
    if (kind == KIND_STEM) { tapinfo[0] = ConvArgs::make_tap(0, 0, 0); return; }
    if (kind == KIND_CT4) {
        // out = 2*in - 1 + k (ConvTranspose2d k=4, s=2, p=1): even out <- k in {1 (d=0), 3 (d=-1)}; odd out <- k in {0 (d=+1), 2 (d=0)}
        static const int kk[2][2] = {{1, 3}, {0, 2}}, dd[2][2] = {{0, -1}, {1, 0}};
        for (int py = 0; py < 2; ++py)
            for (int px = 0; px < 2; ++px)
                for (int i = 0; i < 2; ++i)
                    for (int j = 0; j < 2; ++j)
                        tapinfo[(py * 2 + px) * 4 + i * 2 + j] = ConvArgs::make_tap(dd[py][i], dd[px][j], kk[py][i] * 4 + kk[px][j]);
        return;
    }
    const int k = four ? 4 : 3;                              // 4x4 s2 p1: in = 2 m + (k - 1), k = 0..3
    for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx) tapinfo[ky * k + kx] = ConvArgs::make_tap(ky - 1, kx - 1, ky * k + kx);
}

ConvRoute conv_route(const ConvQuery& q, const ConvPolicy& p)
{
    ConvRoute r{};
    r.q = q;
    r.n_nt = q.Cout_pad / q.BN;
    const ConvGeom g8 = conv_geom(q.kind, q.four, q.Hin, q.Win, 8);
    const long tiles8 = (long)q.B * g8.n_ty * g8.n_tx * g8.npar * r.n_nt;
    r.th = conv_tile_rows(q.kind, q.BN, q.B, g8.MH, g8.MW, g8.npar, r.n_nt);
    const int nch = q.Cin_pad / conv_cin_chunk(q.dtype);
    // The persistent register-weight kernel (ccn_conv_pr.hip): bf16, fragment-ordered weights, >= 2 Cin chunks, outputs below 2 GB.
    // 3x3 s1 on 8- or 4-row tiles; the stride-2 conv (plane passes) on 8-row tiles as soon as enough of the CUs get one (it is ~2.5x
    // more efficient per tile than the 4-wave kernel on 4-row tiles), the ConvTranspose (parities) likewise or where conv_tile_rows
    // gives 8 rows.  Neither of those forms has an input GroupNorm, nor a ConvTranspose in the 4x4 form.
    const double out_bytes = (double)q.B * g8.Hout * g8.Wout * q.Cout * (q.dtype == 1 ? 2 : 4);
    if (p.pr && q.frag && nch >= 2 && !(q.res && q.film) && out_bytes < 2.0e9) {
        if (q.kind == KIND_C3S1) r.pr = conv_pr_selected(q.dtype, q.kind, q.BN, r.th);
        else if (!q.gn_ab && (q.kind == KIND_C3S2 || (q.kind == KIND_CT4 && !q.four))) {
            if (q.kind == KIND_CT4 && !p.ct_like_s2) r.pr = conv_pr_selected(q.dtype, q.kind, q.BN, r.th);
            else if (conv_pr_selected(q.dtype, q.kind, q.BN, 8) && tiles8 >= p.s2_min_tiles8) { r.pr = true; r.th = 8; }
        }
    }
    // Split-K: small layers (at most #CUs/2 tiles of 8 rows: the 32-pixel level at C2) on 8-row tiles with the Cin chunks split over
    // two workgroups per tile.  Measured at C2: a single-tile-per-workgroup launch of the persistent kernel carries ~25 us of fixed cost
    // (cold first chunk, serial last epilogue, hand-off), so halving the K loop of the 32-pixel 3x3 s1 layers (56 us) does not beat the
    // 4-row kernel (53 us); it does help the stride-2 conv into that level (63 -> 56 us), whose alternative is 128 tiles.  The split-K
    // instantiation has no residual path.
    r.ksplit = 1;
    if (r.pr && p.split_k && !q.res && (q.kind == KIND_C3S2 || (q.kind == KIND_C3S1 && p.split_k_s1))) {
        const int nk = q.kind == KIND_C3S2 ? 5 * nch : nch;              // K steps (stride 2: five plane passes per chunk)
        if (tiles8 >= 32 && tiles8 <= 128 && nk >= 4 && (nch & 1) == 0) { r.ksplit = 2; r.th = 8; }
    }
    r.g = conv_geom(q.kind, q.four, q.Hin, q.Win, r.th);
    r.nchunk = nch; r.ntaps = r.g.ntaps;
    if (r.pr && q.kind == KIND_C3S2) {                                   // plane passes (ccn_conv_pr.hip)
        if (q.four) r.nchunk *= 4;                                       // 4x4: four passes of 2x2 taps (ntaps stays 16)
        else { r.nchunk *= 5; r.ntaps = 2; }                             // 3x3: five passes of two tap slots
    }
    r.gs_ok = r.pr && r.ksplit == 1 && q.kind == KIND_C3S1;
    // (the persistent kernel publishes ONE partial per tile: its four producer waves' sums are combined in LDS first)
    r.fin_blocks = r.g.n_ty * r.g.n_tx * r.g.npar * r.n_nt;
    r.nslot = r.fin_blocks;
    r.part_nsp = r.g.n_ty * r.g.n_tx * r.g.npar; r.part_nnt = r.n_nt; r.part_bn = q.BN;
    r.stem2 = p.stem2 && q.kind == KIND_STEM && q.frag && stem2_supported(q.dtype, q.Cin, q.Cout, q.G) && !q.gn_ab && !q.film && !q.res;
    if (r.stem2) {                                                       // one slot per wave
        r.nslot = 4 * stem2_blocks(q.Hin, q.Win, nullptr);
        r.part_nsp = r.nslot; r.part_nnt = 1; r.part_bn = 1 << 30;
    }
    return r;
}

void ConvRoute::fill(ConvArgs& a) const
{
    a.B = q.B; a.Hin = q.Hin; a.Win = q.Win; a.Cin = q.Cin; a.Cin_pad = q.Cin_pad;
    a.Hout = g.Hout; a.Wout = g.Wout; a.Cout = q.Cout; a.Cout_pad = q.Cout_pad;
    a.MH = g.MH; a.MW = g.MW; a.OS = g.OS; a.npar = g.npar; a.ntaps = ntaps;
    a.th = th; a.n_ty = g.n_ty; a.n_tx = g.n_tx; a.n_nt = n_nt; a.nchunk = nchunk;
    a.use_pr = pr ? 1 : 0; a.use_stem2 = stem2 ? 1 : 0; a.ksplit = ksplit;
    a.silu = 1;
    a.G = q.Cout < q.G ? q.Cout : q.G; a.cpg = q.Cout / a.G;
    a.nslot = nslot; a.fin_blocks = fin_blocks; a.bn = q.BN;
    fill_taps(a.tapinfo, q.kind, q.four);
}

// The persistent kernel can form the scale/shift of its input's GroupNorm itself from the producer's partial sums (every producer
// wave reduces 8 groups x 8 lanes): 8 groups, a thread's 8-channel slice inside one group, and few enough slots per group that the
// reduction (slots / 8 loads per lane, redone whenever a workgroup moves to another sample) stays cheaper than the ~6.5 us of a
// finalize launch + kernel boundary -- true below the 256-pixel level at C2.
bool conv_in_kernel_stats(int dtype, int C, int G, int n_sp, int bn)
{
    if (dtype != 1 || n_sp <= 0 || G != 8 || (C / G) % 8 != 0) return false;
    const int cpg = C / G;
    int nj = 1;
    for (int g = 0; g < G; ++g) { const int n = ((g + 1) * cpg - 1) / bn - (g * cpg) / bn + 1; if (n > nj) nj = n; }
    return (long)n_sp * nj <= 64;                                       // 8 slots per lane: one round of loads
}

ConvKernel conv_kernel_for(int kind, int bn, const ConvArgs& a)
{
    if (a.use_stem2) return CK_STEM2;
    if (a.use_pr && kind == KIND_C3S2) return CK_PR;
    if (conv_ws_enabled() && conv_ws_supported(kind, bn)) {
        if (a.use_pr) return CK_PR;                              // decided at plan time (variant 4, bf16, 8-row tiles)
        // free-running kernel on 8-row tiles only: on 4-row tiles a consumer wave would issue 8 DMA pieces per 16 MFMAs and
        // the private weight copies double the L2 traffic of the already weight-heavy 128-pixel tile
        const int variant = conv_variant();
        if (variant == 2 || (variant >= 3 && a.th == 8)) return CK_FR;
        return CK_WS;
    }
    return CK_IGEMM;
}

const char* conv_kernel_name(ConvKernel k)
{
    switch (k) {
        case CK_WS: return "ws";
        case CK_FR: return "fr";
        case CK_PR: return "pr";
        case CK_STEM2: return "stem2";
        default: return "igemm";
    }
}

hipError_t launch_conv(int dtype, int kind, int bn, const ConvArgs& a, hipStream_t s)
{
    const ConvKernel k = conv_kernel_for(kind, bn, a);
    if (k == CK_STEM2) return launch_stem2(a, s);
    if (k == CK_PR && kind == KIND_C3S2) return launch_conv_pr(dtype, a, s);
    if (a.ops && k != CK_WS && k != CK_FR) return hipErrorInvalidValue;      // split weight rows: those two kernels only
    if (k != CK_IGEMM) {
        static const int dbg = diag_env("CCN_DBG") ? atoi(diag_env("CCN_DBG")) : 0;
        ConvArgs d = a; d.dbg = dbg;
        if (k == CK_PR) return launch_conv_pr(dtype, d, s);
        if (k == CK_FR) return launch_conv_fr(dtype, bn, d, s);
        return launch_conv_ws(dtype, bn, d, s);
    }
    if (a.th != 4) return hipErrorInvalidValue;
    const conv_fn_t fn = pick(dtype, kind, bn);
    const unsigned grid = (unsigned)(a.B * a.n_ty * a.n_tx * a.npar * a.n_nt);
    hipLaunchKernelGGL(fn, dim3(grid), dim3(256), conv_lds_bytes(dtype, kind, bn), s, a);
    return hipGetLastError();
}

// ---- GroupNorm-apply + SiLU pre-pass ----------------------------------------------------------------------
bool conv_wants_preact(int kind, int bn, int n_nt)
{
    static const int mode = diag_env("CCN_PREACT") ? atoi(diag_env("CCN_PREACT")) : 1;    // 0 never, 1 when n_nt >= 2, 2 always
    if (!conv_ws_enabled() || !conv_ws_supported(kind, bn) || kind != KIND_C3S1) return false;
    return mode == 2 || (mode == 1 && n_nt >= 2);   // (launch_gn_act needs C/EPC <= 256; wider layers keep the fused prologue)
}

// thread -> fixed 16-byte channel slice (coefficients loaded once) x 4 pixels, all four loads in flight together
template <typename T>
__global__ __launch_bounds__(256) void gn_act_kernel(const T* __restrict__ x, const float2* __restrict__ ab, T* __restrict__ y,
                                                      int HW, int C)
{
    constexpr int EPC = Vec16<T>::EPC;
    const int nsl = C / EPC;                         // 16-byte slices per pixel (<= 256)
    const int pstep = 256 / nsl;                     // pixels covered by one pass of the block
    const int b = blockIdx.y, tid = threadIdx.x;
    const int sl = tid % nsl, pp = tid / nsl;
    if (pp >= pstep) return;
    const int p0 = blockIdx.x * 4 * pstep + pp;
    GnCoef<T> gk;
    gk.load(ab + (size_t)b * C + sl * EPC, true);
    u32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = p0 + k * pstep;
        v[k] = u32x4{0u, 0u, 0u, 0u};
        if (p < HW) v[k] = *(const u32x4*)(x + ((size_t)b * HW + p) * C + sl * EPC);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = p0 + k * pstep;
        if (p < HW) *(u32x4*)(y + ((size_t)b * HW + p) * C + sl * EPC) = gk.template apply<true>(v[k]);
    }
}
// The same pass with the GroupNorm finalize folded in: every workgroup first reduces the producer's partial sums of its
// sample (G groups x a few hundred slots, L2 resident; a fixed summation order, so deterministic) and
// forms its threads' scale/shift in registers -- one launch and one ~5 us dependency step less per pre-activated conv.
// `ab_out` / `stats_out` (training forward, else null): the first workgroup of every sample also writes the scale / shift table and
// (mean, rstd) per group, which the backward pass and the weight-gradient kernel read -- the separate gn_stats launch disappears.
template <typename T>
__global__ __launch_bounds__(256) void gn_act_fused_kernel(const T* __restrict__ x, T* __restrict__ y, int HW, int C,
                                                            const float2* __restrict__ part, int G, int nslot, int n_nt, int bn, int cpg,
                                                            double count, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                            float2* __restrict__ ab_out, float2* __restrict__ stats_out)
{
    constexpr int EPC = Vec16<T>::EPC;
    __shared__ double st[64][2];
    const int nsl = C / EPC, pstep = 256 / nsl;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sl = tid % nsl, pp = tid / nsl;
    const int p0 = blockIdx.x * 4 * pstep + pp;
    const bool act = pp < pstep;
    u32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                       // the data loads fly while the statistics are reduced
        const int p = p0 + k * pstep;
        v[k] = u32x4{0u, 0u, 0u, 0u};
        if (act && p < HW) v[k] = *(const u32x4*)(x + ((size_t)b * HW + p) * C + sl * EPC);
    }
    for (int g = wave; g < G; g += 4) {
        double mean, rstd;
        gn_group_stats(part, b, g, G, nslot, n_nt, bn, cpg, count, eps, lane, mean, rstd);
        if (lane == 0) { st[g][0] = mean; st[g][1] = rstd; }
    }
    __syncthreads();
    if (ab_out && blockIdx.x == 0) {
        for (int c = tid; c < C; c += 256) {
            const int g = c / cpg;
            const double sc = (double)gamma[c] * st[g][1];
            float* const row = (float*)(ab_out + (size_t)b * C) + 4 * (c >> 1) + (c & 1);      // pair-interleaved (GnCoef::load)
            row[0] = (float)sc; row[2] = (float)((double)beta[c] - st[g][0] * sc);
        }
        if (tid < G) stats_out[b * G + tid] = make_float2((float)st[tid][0], (float)st[tid][1]);
    }
    if (!act) return;
    GnCoef<T> gk;
#pragma unroll
    for (int e = 0; e < EPC; ++e) {
        const int c = sl * EPC + e, g = c / cpg;
        const double sc = (double)gamma[c] * st[g][1];
        gk.a[e] = (float)sc; gk.c[e] = (float)((double)beta[c] - st[g][0] * sc);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int p = p0 + k * pstep;
        if (p < HW) *(u32x4*)(y + ((size_t)b * HW + p) * C + sl * EPC) = gk.template apply<true>(v[k]);
    }
}
hipError_t launch_gn_act_fused(int dtype, const void* x, void* y, int B, int HW, int C, const float2* part, int G, int n_sp, int n_nt,
                               int bn, int cpg, double count, const float* gamma, const float* beta, float eps, hipStream_t s,
                               float2* ab_out, float2* stats_out)
{
    const int epc = dtype == 0 ? 4 : 8, nsl = C / epc;
    if (nsl > 256 || nsl <= 0 || G > 64) return hipErrorInvalidValue;
    const int pstep = 256 / nsl;
    const dim3 grid((HW + 4 * pstep - 1) / (4 * pstep), B);
    if (dtype == 0) hipLaunchKernelGGL(gn_act_fused_kernel<float>, grid, dim3(256), 0, s, (const float*)x, (float*)y, HW, C, part, G, n_sp * n_nt, n_nt, bn, cpg, count, gamma, beta, eps, ab_out, stats_out);
    else hipLaunchKernelGGL(gn_act_fused_kernel<__bf16>, grid, dim3(256), 0, s, (const __bf16*)x, (__bf16*)y, HW, C, part, G, n_sp * n_nt, n_nt, bn, cpg, count, gamma, beta, eps, ab_out, stats_out);
    return hipGetLastError();
}

hipError_t launch_gn_act(int dtype, const void* x, const float2* ab, void* y, int B, int HW, int C, hipStream_t s)
{
    const int epc = dtype == 0 ? 4 : 8, nsl = C / epc;
    if (nsl > 256 || nsl <= 0) return hipErrorInvalidValue;
    const int pstep = 256 / nsl;
    const dim3 grid((HW + 4 * pstep - 1) / (4 * pstep), B);
    if (dtype == 0) hipLaunchKernelGGL(gn_act_kernel<float>, grid, dim3(256), 0, s, (const float*)x, ab, (float*)y, HW, C);
    else hipLaunchKernelGGL(gn_act_kernel<__bf16>, grid, dim3(256), 0, s, (const __bf16*)x, ab, (__bf16*)y, HW, C);
    return hipGetLastError();
}

// ---- GroupNorm finalize ----------------------------------------------------------------------------------
// One workgroup of 256 threads per (sample, group): the launch is pure latency (a dependency step between two convs), so
// the slot loop is spread over four waves (plain loads: the producer kernel has completed) and combined in a fixed order.
__global__ __launch_bounds__(256) void gn_finalize_kernel(const float2* __restrict__ part, int G, int n_sp, int n_nt, int bn,
                                                           int cpg, int C, double count, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, float2* __restrict__ ab)
{
    __shared__ double red[4][2];
    const int bg = blockIdx.x, b = bg / G, g = bg % G, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int jlo = (g * cpg) / bn, jhi = ((g + 1) * cpg - 1) / bn, nj = jhi - jlo + 1, ne = n_sp * nj;
    const float2* base = part + (size_t)(b * G + g) * n_sp * n_nt;
    double s1 = 0.0, s2 = 0.0;
    for (int e = tid; e < ne; e += 256) {
        const int sp = e / nj, j = jlo + (e - sp * nj);
        const float2 v = base[(size_t)sp * n_nt + j];
        s1 += (double)v.x; s2 += (double)v.y;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { s1 += __shfl_xor(s1, s); s2 += __shfl_xor(s2, s); }
    if (lane == 0) { red[wave][0] = s1; red[wave][1] = s2; }
    __syncthreads();
    s1 = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    s2 = (red[0][1] + red[1][1]) + (red[2][1] + red[3][1]);
    const double mean = s1 / count;
    double var = s2 / count - mean * mean;
    if (var < 0.0) var = 0.0;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    for (int c = g * cpg + tid; c < (g + 1) * cpg; c += 256) {
        const double sc = (double)gamma[c] * rstd;
        // pair-interleaved: channels (2p, 2p+1) -> {scale, scale, shift, shift} (see GnCoef::load)
        float* const row = (float*)(ab + (size_t)b * C) + 4 * (c >> 1) + (c & 1);
        row[0] = (float)sc; row[2] = (float)((double)beta[c] - mean * sc);
    }
}

hipError_t launch_gn_finalize(const float2* part, int B, int G, int n_sp, int n_nt, int bn, int cpg, int C, double count,
                              const float* gamma, const float* beta, float eps, float2* ab, hipStream_t s)
{
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(B * G), dim3(256), 0, s, part, G, n_sp, n_nt, bn, cpg, C, count, gamma, beta, eps, ab);
    return hipGetLastError();
}

// GroupNorm partial sums of an NHWC tensor (operator-level entry points only; the hot path gets them from the
// producing conv's epilogue).  Block (slot, b): a contiguous pixel range; thread -> (group, sub-range), fixed order.
template <typename T>
__global__ __launch_bounds__(256) void gn_partials_kernel(const T* __restrict__ x, float2* __restrict__ part, int HW, int C,
                                                           int cpg, int G, int nslot)
{
    __shared__ float sh[256 * 2];
    const int slot = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int per = (HW + nslot - 1) / nslot;
    const int p0 = slot * per, p1 = min(HW, p0 + per);
    const int nsub = 256 / G;
    const int g = tid % G, sub = tid / G;
    float s1 = 0.f, s2 = 0.f;
    if (sub < nsub)
        for (int p = p0 + sub; p < p1; p += nsub) {
            const T* row = x + ((size_t)b * HW + p) * C + g * cpg;
            for (int j = 0; j < cpg; ++j) { const float v = (float)row[j]; s1 += v; s2 = fmaf(v, v, s2); }
        }
    sh[tid * 2] = s1; sh[tid * 2 + 1] = s2;
    __syncthreads();
    if (tid < G) {
        float t1 = 0.f, t2 = 0.f;
        for (int q = 0; q < nsub; ++q) { t1 += sh[(q * G + tid) * 2]; t2 += sh[(q * G + tid) * 2 + 1]; }
        part[(size_t)(b * G + tid) * nslot + slot] = make_float2(t1, t2);
    }
}
hipError_t launch_gn_partials(int dtype, const void* x, float2* part, int B, int HW, int C, int cpg, int G, int nslot, hipStream_t s)
{
    if (G > 256) return hipErrorInvalidValue;
    if (dtype == 0) hipLaunchKernelGGL(gn_partials_kernel<float>, dim3(nslot, B), dim3(256), 0, s, (const float*)x, part, HW, C, cpg, G, nslot);
    else hipLaunchKernelGGL(gn_partials_kernel<__bf16>, dim3(nslot, B), dim3(256), 0, s, (const __bf16*)x, part, HW, C, cpg, G, nslot);
    return hipGetLastError();
}

// ---- conditioning ------------------------------------------------------------------------------------------
// timestep_embedding (models/unet.py:33-36): freqs = exp(-ln(1e4) * i / half) in fp32, [cos(t f) | sin(t f)].
template <typename TI>
__global__ void temb_kernel(const TI* __restrict__ t, float* __restrict__ out, int n, int dim)
{
    const int half = dim / 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * dim) return;
    const int row = idx / dim, i = idx - row * dim;
    float v = 0.0f;
    if (i < 2 * half) {
        const int fi = i < half ? i : i - half;
        const float f = expf(__fdiv_rn(__fmul_rn(-9.210340371976184f, (float)fi), (float)half));
        const float arg = __fmul_rn((float)t[row], f);
        v = i < half ? cosf(arg) : sinf(arg);
    }
    out[idx] = v;   // odd dim: last column zero (F.pad, models/unet.py:37-38)
}
hipError_t launch_temb_i64(const int64_t* t, float* out, int n, int dim, hipStream_t s)
{
    hipLaunchKernelGGL(temb_kernel<int64_t>, dim3((n * dim + 255) / 256), dim3(256), 0, s, t, out, n, dim);
    return hipGetLastError();
}
hipError_t launch_temb_i32(const int32_t* t, float* out, int n, int dim, hipStream_t s)
{
    hipLaunchKernelGGL(temb_kernel<int32_t>, dim3((n * dim + 255) / 256), dim3(256), 0, s, t, out, n, dim);
    return hipGetLastError();
}

// One wave per output column n, 16 rows per block; lanes stride K, xor-shuffle reduce (fixed order).
__global__ __launch_bounds__(256) void linear_kernel(const float* __restrict__ xa, const float* __restrict__ xb, int a_div, int b_mod,
                                                      const float* __restrict__ W, const float* __restrict__ bias, float* __restrict__ y,
                                                      int R, int K, int N, int act_silu)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = blockIdx.x * 4 + wave;
    if (n >= N) return;
    const int r0 = blockIdx.y * 16, r1 = min(R, r0 + 16);
    const float* wrow = W + (size_t)n * K;
    for (int rr = r0; rr < r1; ++rr) {
        const float* pa = xa + (size_t)(rr / a_div) * K;
        const float* pb = xb ? xb + (size_t)(rr % b_mod) * K : nullptr;
        float acc = 0.f;
        for (int k = lane; k < K; k += 64) {
            float xv = pa[k];
            if (pb) xv += pb[k];
            acc = fmaf(xv, wrow[k], acc);
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) acc += __shfl_xor(acc, s);
        if (lane == 0) {
            float v = acc + (bias ? bias[n] : 0.f);
            if (act_silu) v = v / (1.0f + expf(-v));
            y[(size_t)rr * N + n] = v;
        }
    }
}
hipError_t launch_linear(const float* xa, const float* xb, int a_div, int b_mod, const float* W, const float* b, float* y,
                         int R, int K, int N, int act_silu, hipStream_t s)
{
    hipLaunchKernelGGL(linear_kernel, dim3((N + 3) / 4, (R + 15) / 16), dim3(256), 0, s, xa, xb, a_div, b_mod, W, b, y, R, K, N, act_silu);
    return hipGetLastError();
}

// ---- elementwise ----------------------------------------------------------------------------------------------
// The stand-alone sampler update, for either parameterisation (`pred`, wave-uniform: X0Form in ccn_device.h), every op rounded
// to fp32 on its own.  y = out_c, or out_u + w*(out_c - out_u) when out_u is given (classifier-free guidance); hist (nullable) is read
// when c4 != 0 and receives the clamped x0; noise (nullable) adds sigma*noise; x is updated in place and x_dup (nullable) receives the
// same values: the unconditional half of the guided loop's state.  VEC: every pointer is 16-byte aligned, four elements per lane and
// access; the n % 4 tail goes one by one.
// SEEDED: the value `noise` would have held is generated instead (Noise): x is gridDim.y records of `per`
// elements, the blocks of row blockIdx.y work on record b = blockIdx.y alone (one seed load per lane, no division), and element j
// of it is draw_quad / draw_element(seeds[b], draw, j).  VEC then also means per % 4 == 0, so that every record starts 16-byte
// aligned and a lane's four elements are one quad of it.  The unseeded instantiations (gridDim.y == 1) are the kernel as it was.
// THR: the same grid rows, and record b's dynamic threshold thr[b] replaces the +-1 clamp of x0 (X0Form::thr; DESIGN.md
// section 1, Thresholding); a noise tensor is then walked by record too.  Without THR nothing of it is compiled in.
// RS: the same grid rows, and record b's guidance-rescale factor gscale[b] multiplies y right after the combine (DESIGN.md section 1,
// Guidance rescale): everything downstream -- the raw x0, e, the history -- is formed from k y.  Without RS nothing of it is compiled in.
// LR: the same grid rows, and element j of record b adds delta[b][block(j)] to its x0 right after the clamp (X0Form::lr; DESIGN.md
// section 1, Low-resolution guide): with W the image's width, N = 2^lgN the block size and WB = W / N, row R = j / W of the record's
// C H rows lies in strip R >> lgN (H % N == 0: no strip crosses a plane) and block(j) = (R >> lgN) WB + ((j - R W) >> lgN).  A quad
// may straddle two blocks or two rows, so the row and the column are carried per element.  Without LR nothing of it is compiled in.
// The argument record comes by value.  No two of its tensors overlap (the caller's contract); the __restrict__ on the local copies
// records that, but the compiler makes little of it on locals -- nothing here needs it: an iteration loads everything it reads before
// its first store.
template <bool VEC, bool SEEDED, bool THR, bool RS, bool LR>
__global__ void sampler_step_kernel(const SamplerStep a)
{
    float *__restrict__ x = a.o.x, *__restrict__ x_dup = a.x_dup, *__restrict__ hist = a.hist;
    const float *__restrict__ out_c = a.o.out_c, *__restrict__ out_u = a.o.out_u, *__restrict__ noise = a.noise, *__restrict__ delta = a.delta;
    const int64_t per = a.o.per_record;
    const int lrW = a.lr_W, lgN = a.lr_lgN, lrWB = a.lr_WB;
    const uint32_t draw = a.draw;
    const float c2 = a.c2, c3 = a.c3, sigma = a.sigma;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    int64_t n = a.o.records * per;
    uint64_t seed = 0;
    // one element's y, x0, e and update: the rescale, the threshold and the guide only where they were asked for
    X0Form f;
    f.pred = a.o.pred; f.c0 = a.o.c0; f.c1 = a.o.c1; f.w = a.o.w;
    f.rescaled = RS; f.thr = THR; f.lr = LR;
    if constexpr (SEEDED || THR || RS || LR) {                      // this record's slice of every tensor
        const int64_t off = (int64_t)blockIdx.y * per;
        if constexpr (SEEDED) seed = a.seeds[blockIdx.y];
        if constexpr (THR) f.s = a.o.thr[blockIdx.y];
        if constexpr (RS) f.k = a.o.gscale[blockIdx.y];
        x += off; out_c += off; n = per;
        if (x_dup) x_dup += off;
        if (hist) hist += off;
        if (out_u) out_u += off;
        if constexpr (THR || RS || LR) { if (noise) noise += off; }
        if constexpr (LR) delta += (int64_t)blockIdx.y * ((per >> lgN) >> lgN);
    }
    f.guided = out_u != nullptr;
    const int64_t n4 = VEC ? n / 4 : 0;
    const float c4 = hist ? a.c4 : 0.f;
    // LR: the d of element j and of the three after it (row R, column col of the record's rows; one division per call)
    auto block_d = [&](int64_t j, float* d4, int count) {
        int64_t R = per <= 0x7fffffff ? (int64_t)((uint32_t)j / (uint32_t)lrW) : j / lrW;
        int col = (int)(j - R * lrW);
        for (int e = 0; e < count; ++e) {
            d4[e] = delta[(R >> lgN) * lrWB + (col >> lgN)];
            if (++col == lrW) { col = 0; ++R; }
        }
    };
    // (u is loaded, and the guided test made, once per quad / element: the guided arm is the combine, the other leaves it out)
    auto y4 = [&](float4 c, float4 u) { return make_float4(f.y(c.x, u.x), f.y(c.y, u.y), f.y(c.z, u.z), f.y(c.w, u.w)); };
    for (int64_t q = tid; q < n4; q += nthr) {
        const float4 xv = ((const float4*)x)[q];
        float4 yv = ((const float4*)out_c)[q];
        yv = f.guided ? y4(yv, ((const float4*)out_u)[q]) : y4(yv, make_float4(0.f, 0.f, 0.f, 0.f));
        float4 hv = make_float4(0.f, 0.f, 0.f, 0.f), o, p;
        if (c4 != 0.f) hv = ((const float4*)hist)[q];
        float dv[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (LR) block_d(q * 4, dv, 4);
        o.x = f.step(xv.x, yv.x, dv[0], c2, c3, c4, hv.x, p.x);
        o.y = f.step(xv.y, yv.y, dv[1], c2, c3, c4, hv.y, p.y);
        o.z = f.step(xv.z, yv.z, dv[2], c2, c3, c4, hv.z, p.z);
        o.w = f.step(xv.w, yv.w, dv[3], c2, c3, c4, hv.w, p.w);
        if (SEEDED || noise) {
            float4 nv;
            if constexpr (SEEDED) nv = draw_quad(seed, draw, (uint32_t)q);
            else nv = ((const float4*)noise)[q];
            o.x = __fadd_rn(o.x, __fmul_rn(sigma, nv.x)); o.y = __fadd_rn(o.y, __fmul_rn(sigma, nv.y));
            o.z = __fadd_rn(o.z, __fmul_rn(sigma, nv.z)); o.w = __fadd_rn(o.w, __fmul_rn(sigma, nv.w));
        }
        if (hist) ((float4*)hist)[q] = p;
        ((float4*)x)[q] = o;
        if (x_dup) ((float4*)x_dup)[q] = o;
    }
    for (int64_t i = n4 * 4 + tid; i < n; i += nthr) {
        const float y = f.guided ? f.y(out_c[i], out_u[i]) : f.y(out_c[i], 0.f);
        const float hv = c4 != 0.f ? hist[i] : 0.f;
        float p, dv = 0.f;
        if constexpr (LR) block_d(i, &dv, 1);
        float xn = f.step(x[i], y, dv, c2, c3, c4, hv, p);
        if constexpr (SEEDED) xn = __fadd_rn(xn, __fmul_rn(sigma, draw_element(seed, draw, i)));
        else if (noise) xn = __fadd_rn(xn, __fmul_rn(sigma, noise[i]));
        if (hist) hist[i] = p;
        x[i] = xn;
        if (x_dup) x_dup[i] = xn;
    }
}
// the 32 instantiations, indexed by the five bits VEC SEEDED THR RS LR (most significant first)
using StepLaunch = void (*)(const SamplerStep&, dim3, hipStream_t);
template <bool... F>
void step_launch(const SamplerStep& a, dim3 grid, hipStream_t s) { hipLaunchKernelGGL((sampler_step_kernel<F...>), grid, dim3(256), 0, s, a); }
template <size_t... I>
constexpr std::array<StepLaunch, sizeof...(I)> step_table(std::index_sequence<I...>)
{
    return {{&step_launch<(I >> 4 & 1) != 0, (I >> 3 & 1) != 0, (I >> 2 & 1) != 0, (I >> 1 & 1) != 0, (I & 1) != 0>...}};
}
// seeds given and sigma > 0: the seeded form; thr given: the threshold form; gscale given: the rescaled form; delta given: the
// low-resolution-guide form; each walks the state record by record, one grid row each (the caller has checked the record, and with
// delta that lr_N is a power of two and per_record a multiple of lr_W lr_N).  With seeds `noise` is not read.
hipError_t launch_sampler_step(const SamplerStep& step, hipStream_t s)
{
    SamplerStep a = step;
    const int64_t per = a.o.per_record, n = a.o.records * per;
    const bool seeded = a.seeds && a.sigma > 0.f;
    if (seeded) a.noise = nullptr;
    const bool rowed = seeded || a.o.thr || a.o.gscale || a.delta;
    if (a.delta) {
        if (a.lr_N < 2 || (a.lr_N & (a.lr_N - 1)) || a.lr_W <= 0 || a.lr_W % a.lr_N || per <= 0 || per % ((int64_t)a.lr_W * a.lr_N)) return hipErrorInvalidValue;
        a.lr_lgN = 0;
        while ((1 << a.lr_lgN) < a.lr_N) ++a.lr_lgN;
        a.lr_WB = a.lr_W / a.lr_N;
    }
    if (rowed && (per <= 0 || a.o.records <= 0 || a.o.records > 65535)) return hipErrorInvalidValue;      // one grid row per record
    const bool vec = !(((uintptr_t)a.o.x | (uintptr_t)a.x_dup | (uintptr_t)a.hist | (uintptr_t)a.o.out_c | (uintptr_t)a.o.out_u | (uintptr_t)a.noise) & 15) &&
                     !(rowed && (per & 3));
    const int64_t rows = rowed ? a.o.records : 1, row = rowed ? per : n;
    const int64_t work = vec ? (row + 3) / 4 : row, blocks = (work + 255) / 256;
    const int gx = (int)(blocks < 2048 ? (blocks > 0 ? blocks : 1) : 2048);        // 256 CUs x 8 blocks, grid-stride beyond
    static constexpr auto table = step_table(std::make_index_sequence<32>());
    table[vec << 4 | seeded << 3 | (a.o.thr != nullptr) << 2 | (a.o.gscale != nullptr) << 1 | (a.delta != nullptr)](a, dim3(gx, (unsigned)rows), s);
    return hipGetLastError();
}

__global__ void q_sample_kernel(float* __restrict__ out, const float* __restrict__ x0, const float* __restrict__ noise,
                                const float* __restrict__ a, const float* __restrict__ sg, int64_t per)
{
    const int b = blockIdx.y;
    const float ca = a[b], cs = sg[b];
    const size_t base = (size_t)b * per;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x)
        out[base + i] = __fadd_rn(__fmul_rn(ca, x0[base + i]), __fmul_rn(cs, noise[base + i]));
}
hipError_t launch_q_sample(float* out, const float* x0, const float* noise, const float* a, const float* sg, int B, int64_t per,
                           hipStream_t s)
{
    const int gx = (int)((per + 255) / 256 < 1024 ? (per + 255) / 256 : 1024);
    hipLaunchKernelGGL(q_sample_kernel, dim3(gx > 0 ? gx : 1, B), dim3(256), 0, s, out, x0, noise, a, sg, per);
    return hipGetLastError();
}

__global__ void predict_x0_kernel(float* __restrict__ out, const float* __restrict__ xt, const float* __restrict__ eps,
                                  const float* __restrict__ a, const float* __restrict__ sg, int64_t per)
{
    const int b = blockIdx.y;
    const float ca = a[b], cs = sg[b];
    const size_t base = (size_t)b * per;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x)
        out[base + i] = __fdiv_rn(__fsub_rn(xt[base + i], __fmul_rn(cs, eps[base + i])), ca);
}
hipError_t launch_predict_x0(float* out, const float* xt, const float* eps, const float* a, const float* sg, int B, int64_t per,
                             hipStream_t s)
{
    const int gx = (int)((per + 255) / 256 < 1024 ? (per + 255) / 256 : 1024);
    hipLaunchKernelGGL(predict_x0_kernel, dim3(gx > 0 ? gx : 1, B), dim3(256), 0, s, out, xt, eps, a, sg, per);
    return hipGetLastError();
}

// y = x*(1+s) + b on NCHW fp32 (stand-alone FiLM, models/blocks.py:25; the UNet path fuses this into conv1's epilogue)
__global__ void film_nchw_kernel(const float* __restrict__ x, const float* __restrict__ sc, const float* __restrict__ sh,
                                 float* __restrict__ y, int64_t hw)
{
    const int bc = blockIdx.y;
    const float s1 = __fadd_rn(1.0f, sc[bc]), b1 = sh[bc];
    const size_t base = (size_t)bc * hw;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (int64_t)gridDim.x * blockDim.x)
        y[base + i] = __fadd_rn(__fmul_rn(x[base + i], s1), b1);
}
hipError_t launch_film_nchw(const float* x, const float* sc, const float* sh, float* y, int B, int C, int64_t hw, hipStream_t s)
{
    const int gx = (int)((hw + 255) / 256 < 256 ? (hw + 255) / 256 : 256);
    hipLaunchKernelGGL(film_nchw_kernel, dim3(gx > 0 ? gx : 1, B * C), dim3(256), 0, s, x, sc, sh, y, hw);
    return hipGetLastError();
}

template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ src, T* __restrict__ dst, int C, int HW, int64_t total)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const int64_t bp = i / C, p = bp % HW, b = bp / HW;
        dst[i] = (T)src[((size_t)b * C + c) * HW + p];
    }
}
template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* __restrict__ src, float* __restrict__ dst, int C, int HW, int64_t total)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = i % HW, bc = i / HW;
        const int c = (int)(bc % C);
        const int64_t b = bc / C;
        dst[i] = (float)src[((size_t)b * HW + p) * C + c];
    }
}
hipError_t launch_nchw_to_nhwc(int dtype, const float* src, void* dst, int B, int C, int H, int W, hipStream_t s)
{
    const int64_t total = (int64_t)B * C * H * W;
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    if (dtype == 0) hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, dim3(grid), dim3(256), 0, s, src, (float*)dst, C, H * W, total);
    else hipLaunchKernelGGL(nchw_to_nhwc_kernel<__bf16>, dim3(grid), dim3(256), 0, s, src, (__bf16*)dst, C, H * W, total);
    return hipGetLastError();
}
hipError_t launch_nhwc_to_nchw(int dtype, const void* src, float* dst, int B, int C, int H, int W, hipStream_t s)
{
    const int64_t total = (int64_t)B * C * H * W;
    const int grid = (int)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    if (dtype == 0) hipLaunchKernelGGL(nhwc_to_nchw_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)src, dst, C, H * W, total);
    else hipLaunchKernelGGL(nhwc_to_nchw_kernel<__bf16>, dim3(grid), dim3(256), 0, s, (const __bf16*)src, dst, C, H * W, total);
    return hipGetLastError();
}

}  // namespace ccn
