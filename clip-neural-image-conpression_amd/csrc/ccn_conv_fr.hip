// "Free-running" warp-specialised implicit-GEMM convolution: no workgroup barrier inside a Cin chunk.
//
// Measurements on the barrier-per-stage kernels (ccn_conv_ws.hip and a shared LDS-DMA-ring variant of it) showed the consumer waves are the
// pole: they hardly wait at the barriers, but every stage restarts their LDS-read -> MFMA pipeline behind a barrier
// and the loop runs at ~50 % of the MFMA rate.  Here the consumers never synchronise with anybody inside a chunk:
//   * weights (B): every consumer wave owns a PRIVATE ring of three one-tap slots for the 32*NF output channels it
//     multiplies, fills it itself by LDS-DMA (buffer_load_dwordx4 ... lds) two taps ahead, and orders its own reads
//     with its own counted s_waitcnt vmcnt -- no cross-wave hand-off at all (the two waves that share channels each
//     fetch their copy: 2x weight traffic from L2, which an 8-row tile can afford);
//   * input (A): ONE LDS buffer per workgroup.  The four producer waves hold the next chunk in registers (requested a
//     whole chunk ahead), apply GroupNorm + SiLU in place while the consumers compute, and at the chunk boundary --
//     two barriers -- dump it into the buffer;
//   * so a tile costs 1 + 2*(nchunk-1) barriers in its main loop instead of nchunk*ntaps, the fragment prefetch runs
//     straight through tap boundaries, and the producers' ds_writes are confined to the boundaries.
//
// The workgroup decode, the operands' buffer descriptors, the stamps, the chunk-0 input prologue, the epilogue and the GroupNorm
// partial-sum tail are the same in ccn_conv_ws.hip and are included from tile/*.inc (ccn_conv_tile.h says why as text).  Here: the
// LDS layout with the private weight rings, the two roles and their loops.
//
// Three operand forms: T = float, __bf16 (storage type = operand type) and f16x3_t (ccn_device.h: fp32 storage, fp16 hi + lo rows in
// LDS, three fp16 MFMAs per product).  The f16x3 form shares everything on the global side with the float form; its producers split
// while they stage, and its consumers run tile/split_steps.inc instead of the step loop below.
#include "ccn_conv_tile.h"

namespace ccn {

namespace {

template <int TH, int BN, int NF> struct FrLds {
    static constexpr int NBUF = 3;
    static constexpr int A_BYTES = TileGeom<TH>::A_BYTES;
    static constexpr int BW_BYTES = NF * 32 * 128;           // one tap of one consumer wave's channels
    static constexpr int B_BYTES = 4 * NBUF * BW_BYTES;
    static constexpr int LOOP = A_BYTES + B_BYTES;
    static constexpr int TOTAL = EpiLds<TH, BN, 8>::total(LOOP);
};

}  // namespace

template <typename T, int MF, int NF, int NTAPS>
__global__ __launch_bounds__(512) void conv_fr_kernel(const ConvArgs a)
{
    constexpr int WM = 2, WN = 2;
    constexpr int TH = WM * MF;
    constexpr int BN = WN * NF * 32;
    constexpr int EPC = Vec16<T>::EPC;
    constexpr int CKE = 8 * EPC;
    constexpr bool SPLIT = OperandForm<T>::SPLIT;       // f16x3: fp16 hi + lo operand rows (ccn_device.h)
    [[maybe_unused]] unsigned ovf = 0;                  // ... and an activation that left the fp16 range while being staged
    constexpr int NA = 4, A0 = 4;               // waves 4..7 stage the input operand
    constexpr int NWAVES = 8;
    using G = TileGeom<TH>;
    using L = FrLds<TH, BN, NF>;
    using E = EpiLds<TH, BN, NWAVES>;
    constexpr int NBUF = L::NBUF;
    constexpr int HPITCH = G::HPITCH;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const As = smem;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;

#include "tile/decode.inc"              // -> b, ty, tx, par, nt; my0, mx0, n0; py, px_, par_off
    constexpr int STAMP_B0 = -1;                // stamp rows: consumers, (no weight producers), A producers
    constexpr bool LOOP_BARRIER_RAW = true;     // the chunk-boundary barriers must not drain the register prefetch and the LDS-DMA
#include "tile/stamps.inc"              // -> stamp(slot), raw_barrier(), loop_barrier(), stamp_wait(); stamps slot 0
#include "tile/operands.inc"            // -> gn, iy0, ix0, OOB, in_srd(chunk), w_srd(tap, chunk)

    // ------------------------------------------------------------------ prologue: chunk 0 by all 512 threads
    {
#include "tile/prologue_a_load.inc"     // Cin chunk 0 of the input halo requested -> raw[], okm, gk
#include "tile/prologue_a_write.inc"    // ... GroupNorm + SiLU, swizzled write into As
    }

    // ------------------------------------------------------------------ epilogue pieces (used by every role after its loop)
#include "tile/epilogue.inc"            // -> Cs, epi_init(), epi_all(); f1, f2, s1, s2
    // f16x3 range guard: each role reports once it has staged its last input unit (the flag is not carried through a main loop)
    [[maybe_unused]] auto report_ovf = [&]() __attribute__((always_inline)) {
        if (__ballot(ovf != 0u) != 0ull && lane == 0 && a.err) __hip_atomic_fetch_or(a.err, 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    const bool do_epi = !CCN_DBG_BIT(a, 8);

    if (wave >= A0) {
        // ------------------------------------------------------------------ A producers (4 waves)
        // registers hold chunk c+1 (requested during chunk c-1); GroupNorm + SiLU is applied in place while the consumers
        // work on chunk c; between the two boundary barriers the chunk is dumped into the single A buffer and the same
        // registers are re-requested for chunk c+2
        const int ptid = tid - A0 * 64, ck = ptid & 7;
        constexpr int AIT = (G::AU + NA * 64 - 1) / (NA * 64);
        u32x4 areg[AIT];
        GnCoef<T> gk;
        auto a_off = [&](int i) __attribute__((always_inline)) -> unsigned {
            const int px = (ptid >> 3) + NA * 8 * i;
            const int hy = px / HPITCH, hx = px - hy * HPITCH;
            const int iy = iy0 + hy, ix = ix0 + hx;
            const bool ok = px < G::HROWS * HPITCH && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
            return ok ? (unsigned)(((b * a.Hin + iy) * a.Win + ix) * a.Cin + ck * EPC) * (unsigned)sizeof(T) : OOB;
        };
        auto a_req_all = [&](int chunk) __attribute__((always_inline)) {
            const int cb = chunk * CKE + ck * EPC;
            const bool cv = chunk < a.nchunk && cb < a.Cin;
            gk.load(a.gn_ab + (size_t)b * a.Cin + (cv ? cb : 0), gn && cv);     // first: its wait must not wait for the HBM requests below
            const auto srd = in_srd(chunk < a.nchunk ? chunk : 0);
#pragma unroll
            for (int i = 0; i < AIT; ++i) areg[i] = __builtin_amdgcn_raw_buffer_load_b128(srd, cv ? a_off(i) : OOB, 0, 0);
        };
        a_req_all(1);
        raw_barrier();                                             // chunk 0 visible
        stamp(1);
        for (int chunk = 0; chunk + 1 < a.nchunk; ++chunk) {
            if (!CCN_DBG_BIT(a, 1)) {
                const bool cv = (chunk + 1) * CKE + ck * EPC < a.Cin;
                if (gn && cv) {
#pragma unroll
                    for (int i = 0; i < AIT; ++i)
                        if (a_off(i) != OOB) areg[i] = gk.template apply<true>(areg[i]);   // padding stays zero
                }
            }
            if constexpr (SPLIT) {                                 // f16x3: the split too happens outside the boundary, in place
#pragma unroll
                for (int i = 0; i < AIT; ++i) areg[i] = split_pack(areg[i], ovf);
            }
            loop_barrier();                                        // consumers are done with chunk `chunk`
            if (!CCN_DBG_BIT(a, 1)) {
#pragma unroll
                for (int i = 0; i < AIT; ++i) {
                    const int px = (ptid >> 3) + NA * 8 * i;
                    if constexpr (SPLIT) { if (px < G::HROWS * HPITCH) split_store(As + px * 128, px >> 1, ck, areg[i]); }
                    else if (px < G::HROWS * HPITCH) *(u32x4*)(As + px * 128 + (((ck ^ (px >> 1)) & 7) << 4)) = areg[i];
                }
            }
            loop_barrier();                                        // chunk `chunk + 1` visible
            if (!CCN_DBG_BIT(a, 1)) a_req_all(chunk + 2);
        }
        if constexpr (SPLIT) report_ovf();
        stamp(2); stamp_wait();
        if (do_epi) {
            __syncthreads();                                       // matches the consumers' barrier: LDS is about to become the fp32 tile
            epi_init(); epi_all();
        }
        stamp(3);
    } else {
        // ------------------------------------------------------------------ consumers (4 waves)
        if constexpr (SPLIT) report_ovf();
        __builtin_amdgcn_s_setprio(2);
        const int wm = wave / WN, wn = wave % WN;
        f32x16 acc[MF][NF];
#pragma unroll
        for (int i = 0; i < MF; ++i)
#pragma unroll
            for (int j = 0; j < NF; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.0f;
        auto rbase = [&](int row) __attribute__((always_inline)) { return row * 128 + ((((row >> 1) & 6)) << 4) + (((h ^ (row >> 1)) & 1) << 4); };
        int prow[MF], bbase[NF], toff[NTAPS];
#pragma unroll
        for (int i = 0; i < MF; ++i) prow[i] = ((wm * MF + i) + 1) * HPITCH + r + 1;
#pragma unroll
        for (int j = 0; j < NF; ++j) bbase[j] = rbase(j * 32 + r);             // row index inside this wave's private tile
#pragma unroll
        for (int t = 0; t < NTAPS; ++t)
            toff[t] = NTAPS == 9 ? (t / 3 - 1) * HPITCH + (t % 3 - 1)
                                 : a.tapinfo_dy(par_off + t) * HPITCH + a.tapinfo_dx(par_off + t);
        // private weight ring: slot s of this wave at Bs + (wave*NBUF + s)*BW_BYTES; a tap is PP one-KiB pieces (8 rows each)
        constexpr int PP = NF * 32 / 8;
        const int b_wave = (int)L::A_BYTES + wave * NBUF * (int)L::BW_BYTES;
        auto b_dma = [&](int tg) __attribute__((always_inline)) {             // tg: tap index counted from the start of the tile
            int chunk = tg / NTAPS, tap = tg - chunk * NTAPS;
            if (chunk >= a.nchunk) { chunk = a.nchunk - 1; }                  // past the end: harmless re-read, keeps vmcnt uniform
            const auto srd = w_srd(tap, chunk);
            [[maybe_unused]] const int slot = tg % NBUF;             // (used by the device pass only)
#pragma unroll
            for (int k = 0; k < PP; ++k) {
                const int row = 8 * k + (lane >> 3);                           // row inside the private tile
                const unsigned voff = (unsigned)((size_t)(n0 + wn * NF * 32 + row) * a.Cin_pad * sizeof(T)) + ((((lane & 7) ^ (row >> 1)) & 7) << 4);
#if defined(__HIP_DEVICE_COMPILE__)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(srd, (__attribute__((address_space(3))) void*)(smem + b_wave + slot * L::BW_BYTES + k * 1024),
                                                         16, voff, 0, 0, 0);
#else
                (void)voff; (void)srd;
#endif
            }
        };
        b_dma(0); b_dma(1);
        raw_barrier();                                             // chunk 0 visible; the two weight taps stay in flight
        stamp(1);
        int tg = 0;                                                // taps done since the start of the tile
        for (int chunk = 0; chunk < a.nchunk; ++chunk) {
#pragma unroll
            for (int i = 0; i < MF; ++i) asm volatile("" : "+v"(prow[i]));    // keep the address math inside the loop
            if constexpr (SPLIT) {
                constexpr int NT = NTAPS;
                constexpr int DPM = (PP + MF * NF - 1) / (MF * NF);
                int abase[MF];
                auto a_tap = [&](int tt) __attribute__((always_inline)) {
#pragma unroll
                    for (int i = 0; i < MF; ++i) abase[i] = rbase(prow[i] + toff[tt]);
                };
                auto b_tap = [&](int tt) __attribute__((always_inline)) { return b_wave + ((tg + tt) % NBUF) * (int)L::BW_BYTES; };
                // as below: DMA(x) is issued during tap x-2; at the start of tap x the ring holds x (needed now) and x+1 (may fly)
                auto tap_begin = [&](int tt) __attribute__((always_inline)) { b_dma(tg + tt + 2); };
                auto tap_landed = [&](int) __attribute__((always_inline)) { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PP) : "memory"); };
#include "tile/split_steps.inc"
            } else {
                constexpr int NSTEP = NTAPS * 4;                   // step = tap * 4 + kk
                u32x4 av[2][MF], bv[2][NF];
                int abase[MF];
                auto frag = [&](int j, int tg0, u32x4* av_, u32x4* bv_) __attribute__((always_inline)) {
                    const int tt = j >> 2, kk = j & 3;
                    if (kk == 0) {
#pragma unroll
                        for (int i = 0; i < MF; ++i) abase[i] = rbase(prow[i] + toff[tt]);
                    }
                    const int b_off = b_wave + ((tg0 + tt) % NBUF) * (int)L::BW_BYTES;
#pragma unroll
                    for (int i = 0; i < MF; ++i) av_[i] = *(const u32x4*)(smem + (abase[i] ^ (kk << 5)));
#pragma unroll
                    for (int jn = 0; jn < NF; ++jn) bv_[jn] = *(const u32x4*)(smem + b_off + (bbase[jn] ^ (kk << 5)));
                };
                // DMA(x) is issued during tap x-2, so at the start of tap tg the ring holds tg (needed now) and tg+1 (may fly)
                asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PP) : "memory");
                frag(0, tg, av[0], bv[0]);
#pragma unroll
                for (int j = 0; j < NSTEP; ++j) {
                    const bool tap_begin = (j & 3) == 0, tap_end = (j & 3) == 3;
                    __builtin_amdgcn_sched_barrier(0);
                    // the slot of the previous tap is free (its fragment reads fed MFMAs already issued): refill it two taps ahead
                    if (tap_begin) b_dma(tg + (j >> 2) + 2);
                    if (j + 1 < NSTEP) {
                        if (tap_end) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(PP) : "memory");   // next tap landed (the one after may fly)
                        frag(j + 1, tg, av[(j + 1) & 1], bv[(j + 1) & 1]);
                    }
#pragma unroll
                    for (int i = 0; i < MF; ++i)
#pragma unroll
                        for (int jn = 0; jn < NF; ++jn) mfma16<T>(acc[i][jn], av[j & 1][i], bv[j & 1][jn]);
                    // An in-order wave that issues its MFMAs back to back leaves 24 of every 32 cycles of issue bandwidth
                    // unused and then runs the next step's address math / ds_reads while the matrix pipe drains (measured:
                    // a pure MFMA stream at 76 % of the pipe rate).  Interleave: one MFMA, then the DMA pieces of this tap
                    // (first step only), one LDS read and up to two VALU of the NEXT step's fragment fetch in its shadow.
                    constexpr int DPM = (PP + MF * NF - 1) / (MF * NF);     // DMA pieces per MFMA shadow
#pragma unroll
                    for (int m = 0; m < MF * NF; ++m) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // 1 MFMA
                        if (tap_begin) __builtin_amdgcn_sched_group_barrier(0x020, DPM, 0);   // VMEM reads (LDS-DMA pieces)
                        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // 1 DS read
                        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);      // 2 VALU
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            tg += NTAPS;
            if (chunk + 1 < a.nchunk) { loop_barrier(); loop_barrier(); }     // A buffer released / refilled
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // no DMA may land after the epilogue starts reusing LDS
        __builtin_amdgcn_s_setprio(0);
        stamp(2); stamp_wait();
        if (do_epi) {
            __syncthreads();                                       // every wave's DMA drained, every wave done reading A/B
            epi_init();
#include "tile/acc_to_lds.inc"          // acc[][] -> fp32 tile Cs
            epi_all();
        }
        stamp(3);
    }
    if (!do_epi) return;
    if (a.part) {
#include "tile/gn_part_tail.inc"        // s1, s2 -> GroupNorm partials (-> in-kernel finalize)
    }
}

// ---- dispatch -------------------------------------------------------------------------------------------------
template <typename T> static tile_fn_t pick_fr_t(int ntaps, int th, int bn)
{
    if (ntaps == 9) {
        if (th == 8) { if (bn == 128) return conv_fr_kernel<T, 4, 2, 9>; return conv_fr_kernel<T, 4, 1, 9>; }
        if (bn == 128) return conv_fr_kernel<T, 2, 2, 9>;
        return conv_fr_kernel<T, 2, 1, 9>;
    }
    if (th == 8) { if (bn == 128) return conv_fr_kernel<T, 4, 2, 4>; return conv_fr_kernel<T, 4, 1, 4>; }
    if (bn == 128) return conv_fr_kernel<T, 2, 2, 4>;
    return conv_fr_kernel<T, 2, 1, 4>;
}
// dtype: the storage type, or CCN_DTYPE_F16X3 = 2 for fp32 storage with split operand rows (ConvArgs::ops)
static tile_fn_t pick_fr(int dtype, int ntaps, int th, int bn)
{
    if (dtype == 2) return pick_fr_t<f16x3_t>(ntaps, th, bn);
    return dtype == 0 ? pick_fr_t<float>(ntaps, th, bn) : pick_fr_t<__bf16>(ntaps, th, bn);
}
static size_t fr_lds(int /*ntaps*/, int th, int bn)
{
    if (th == 8) return bn == 128 ? FrLds<8, 128, 2>::TOTAL : FrLds<8, 64, 1>::TOTAL;
    return bn == 128 ? FrLds<4, 128, 2>::TOTAL : FrLds<4, 64, 1>::TOTAL;
}

hipError_t conv_fr_prepare() { return tiled_prepare(pick_fr, fr_lds); }

static StampBuf g_stamps;
extern "C" int ccn_internal_dump_stamps_fr(const char* path) { return g_stamps.dump(path); }

hipError_t launch_conv_fr(int dtype, int bn, const ConvArgs& a, hipStream_t s)
{
    const unsigned grid = (unsigned)(a.B * a.n_ty * a.n_tx * a.npar * a.n_nt);
    if (a.ops && dtype != 0) return hipErrorInvalidValue;       // split operand rows exist for fp32 storage only
    return launch_tiled(pick_fr(a.ops ? 2 : dtype, a.ntaps, a.th, bn), grid, fr_lds(a.ntaps, a.th, bn), a, s, g_stamps);
}

}  // namespace ccn
