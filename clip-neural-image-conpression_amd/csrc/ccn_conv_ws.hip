// Warp-specialised implicit-GEMM convolution for the stride-1 3x3 convs and the ConvTranspose parities (the
// 3x3-s1 ResBlock convs are 87 % of the path's FLOPs).
//
// One workgroup = 8 waves on one CU:
//   waves 0-3  consumers: nothing but ds_read_b128 + MFMA over the staged tiles (2x2 waves, MF x NF fragments each)
//   waves 4-7  producers: run one pipeline step ahead -- global loads of the next input-halo chunk and weight
//              stage, the GroupNorm-apply + SiLU transform (VALU, transcendental-heavy), ds_write into the
//              *other* LDS buffer
// so the VALU prologue fusion and the staging traffic overlap the matrix pipe instead of alternating with it
// (MFMA and VALU are separate pipes; a wave issues in order, so the overlap has to come from different waves).
// Both operands are double buffered; ONE workgroup barrier per (Cin-chunk, tap) iteration orders everything:
//   iteration it:  consumers read A[c&1], B[it&1];  producers write B[(it+1)&1] and a slice of A[(c+1)&1]
// The epilogue (accumulators -> LDS fp32 tile -> bias / FiLM / residual -> coalesced 16-B NHWC rows + the next
// GroupNorm's partial sums) is shared by all 8 waves, 128 pixels per pass, with the residual rows prefetched
// into registers before the pass barrier.
//
// Tile: TH x 32 output-space pixels (TH = 4*MF/2: 4 or 8 rows of 32) x BN = 64*NF output channels.
//
// The workgroup decode, the operands' buffer descriptors, the chunk-0 input prologue, the epilogue and the GroupNorm partial-sum
// tail are the same in ccn_conv_fr.hip and are included from tile/*.inc (ccn_conv_tile.h says why as text).  Here: the LDS ring
// layout, the three roles with their stamps, and their loops.
//
// Operand forms: T = float, __bf16, and f16x3_t (fp32 storage, fp16 hi + lo rows in LDS: ccn_device.h, ccn_conv_fr.hip).
#include "ccn_conv_tile.h"

namespace ccn {

namespace {

template <int TH, int BN, int TPS> struct WsLds {
    static constexpr int A_BYTES = TileGeom<TH>::A_BYTES;
    static constexpr int BT_BYTES = BN * 128;                // one tap of one stage
    static constexpr int B_BYTES = TPS * BT_BYTES;           // one stage
    static constexpr int LOOP = 2 * A_BYTES + 2 * B_BYTES;
    static constexpr int TOTAL = EpiLds<TH, BN, 8>::total(LOOP);
};

}  // namespace

template <typename T, int MF, int NF, int NTAPS, int TPS>
__global__ __launch_bounds__(512) void conv_ws_kernel(const ConvArgs a)
{
    constexpr int WM = 2, WN = 2;
    constexpr int TH = WM * MF;                 // tile rows of 32 pixels
    constexpr int BN = WN * NF * 32;
    constexpr int EPC = Vec16<T>::EPC;
    constexpr int CKE = 8 * EPC;
    constexpr bool SPLIT = OperandForm<T>::SPLIT;       // f16x3: fp16 hi + lo operand rows (ccn_device.h)
    [[maybe_unused]] unsigned ovf = 0;                  // ... and an activation that left the fp16 range while being staged
    constexpr int NSPC = NTAPS / TPS;           // stages (barriers) per Cin chunk
    // producer waves 4..7: NB weight waves then NA input waves.  8-row tiles move 16 KB of weights per stage (one wave
    // keeps up) and carry the GroupNorm+SiLU VALU work on 1.7x more input, so they get 3 input waves; 4-row tiles 2 + 2.
    constexpr int NB = MF == 4 ? 1 : 2, NA = 4 - NB;
    constexpr int A0 = 4 + NB;                  // first A-producer wave
    static_assert(NSPC * TPS == NTAPS && NSPC >= 2, "taps must split evenly into >= 2 stages per chunk");
    constexpr int NWAVES = 8;
    using G = TileGeom<TH>;
    using L = WsLds<TH, BN, TPS>;
    using E = EpiLds<TH, BN, NWAVES>;
    constexpr int HPITCH = G::HPITCH;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* const As = smem;                         // 2 chunk buffers
    unsigned char* const Bs = smem + 2 * L::A_BYTES;        // 2 stage buffers of TPS taps

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;

#include "tile/decode.inc"              // -> b, ty, tx, par, nt; my0, mx0, n0; py, px_, par_off
    constexpr int STAMP_B0 = 4;                 // stamp rows: consumers, B producers (first wave 4), A producers
    constexpr bool LOOP_BARRIER_RAW = false;    // the stage barrier also publishes the producers' ds_writes: full __syncthreads()
#include "tile/stamps.inc"              // -> stamp(slot), raw_barrier(), loop_barrier(), stamp_wait(); stamps slot 0
#include "tile/operands.inc"            // -> gn, iy0, ix0, OOB, in_srd(chunk), w_srd(tap, chunk)

    // ------------------------------------------------------------------ prologue: chunk 0 and stage 0 by all 512 threads
    {
#include "tile/prologue_a_load.inc"     // Cin chunk 0 of the input halo requested -> raw[], okm, gk
        constexpr int BU0 = TPS * BN * 8 / 512;
        u32x4 b0[BU0];
#pragma unroll
        for (int u = 0; u < BU0; ++u) {
            const int idx = tid + 512 * u, tt = idx / (BN * 8), rem = idx - tt * (BN * 8), n = rem >> 3, ckb = rem & 7;
            b0[u] = __builtin_amdgcn_raw_buffer_load_b128(w_srd(__builtin_amdgcn_readfirstlane(tt), 0), (unsigned)(((size_t)(n0 + n) * a.Cin_pad) * sizeof(T) + ckb * 16), 0, 0);
        }
#include "tile/prologue_a_write.inc"    // ... GroupNorm + SiLU, swizzled write into As
#pragma unroll
        for (int u = 0; u < BU0; ++u) {
            const int idx = tid + 512 * u, tt = idx / (BN * 8), rem = idx - tt * (BN * 8), n = rem >> 3, ckb = rem & 7;
            *(u32x4*)(Bs + tt * L::BT_BYTES + n * 128 + (((ckb ^ (n >> 1)) & 7) << 4)) = b0[u];
        }
    }

    // ------------------------------------------------------------------ epilogue pieces (used by every role after its loop)
#include "tile/epilogue.inc"            // -> Cs, epi_init(), epi_all(); f1, f2, s1, s2
    // f16x3 range guard: each role reports once it has staged its last input unit (the flag is not carried through a main loop)
    [[maybe_unused]] auto report_ovf = [&]() __attribute__((always_inline)) {
        if (__ballot(ovf != 0u) != 0ull && lane == 0 && a.err) __hip_atomic_fetch_or(a.err, 4u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    const bool do_epi = !CCN_DBG_BIT(a, 8);

    if (wave >= A0) {
        // ------------------------------------------------------------------ A producers (2 waves): input halo, ONE CHUNK AHEAD IN REGISTERS
        // Software pipeline in registers: while the consumers work on chunk c, these waves hold chunk c+1's 16-byte units
        // (requested a whole chunk earlier), retire a slice of them per stage -- GroupNorm-apply + SiLU, ds_write into the
        // other A buffer -- and immediately re-request the same slots for chunk c+2.  No wait on memory in steady state.
        const int ptid = tid - A0 * 64, ck = ptid & 7;
        constexpr int AIT = (G::AU + NA * 64 - 1) / (NA * 64);                  // units per A-producer thread per chunk
        constexpr int UPS = (AIT + NSPC - 1) / NSPC;              // units retired (and re-requested) per stage
        u32x4 areg[AIT];
        GnCoef<T> gk, gk_next;                   // coefficients of the chunk being retired / of the one after it
        // unit i of this thread: halo pixel (ptid>>3) + 16*i, channel slice ck
        auto a_off = [&](int i) __attribute__((always_inline)) -> unsigned {
            const int px = (ptid >> 3) + NA * 8 * i;
            const int hy = px / HPITCH, hx = px - hy * HPITCH;
            const int iy = iy0 + hy, ix = ix0 + hx;
            const bool ok = px < G::HROWS * HPITCH && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
            return ok ? (unsigned)(((b * a.Hin + iy) * a.Win + ix) * a.Cin + ck * EPC) * (unsigned)sizeof(T) : OOB;
        };
        auto a_req = [&](int chunk, int i) __attribute__((always_inline)) {          // zeros if the chunk / slice / pixel does not exist
            const bool cv = chunk < a.nchunk && chunk * CKE + ck * EPC < a.Cin;
            areg[i] = __builtin_amdgcn_raw_buffer_load_b128(in_srd(chunk < a.nchunk ? chunk : 0), cv ? a_off(i) : OOB, 0, 0);
        };
        // vmcnt retires in order: coefficient loads are always issued BEFORE the input requests of the same stage, so
        // waiting for them never waits for HBM
        auto gk_req = [&](GnCoef<T>& dst, int chunk) __attribute__((always_inline)) {
            const int cb = chunk * CKE + ck * EPC;
            const bool cv = chunk < a.nchunk && cb < a.Cin;
            dst.load(a.gn_ab + (size_t)b * a.Cin + (cv ? cb : 0), gn && cv);
        };
        gk_req(gk, 1);
#pragma unroll
        for (int i = 0; i < AIT; ++i) a_req(1, i);
        __syncthreads();                                           // prologue tiles visible
        stamp(1);
        for (int chunk = 0; chunk < a.nchunk; ++chunk) {
            const bool more = chunk + 1 < a.nchunk && !CCN_DBG_BIT(a, 1);
            unsigned char* const Ad = As + ((chunk + 1) & 1) * L::A_BYTES;
#pragma unroll
            for (int g = 0; g < NSPC; ++g) {
                if (more) {
                    if (g == NSPC - 1) gk_req(gk_next, chunk + 2);
#pragma unroll
                    for (int i = g * UPS; i < (g + 1) * UPS && i < AIT; ++i) {
                        const int px = (ptid >> 3) + NA * 8 * i;
                        if (px < G::HROWS * HPITCH) {
                            // padding / overhang units arrive as zeros and must stay zero: the activation applies to real pixels only
                            const bool real = a_off(i) != OOB && (chunk + 1) * CKE + ck * EPC < a.Cin;
                            u32x4 o = areg[i];
                            if (gn && real) o = gk.template apply<true>(areg[i]);
                            if constexpr (SPLIT) split_put(Ad + px * 128, px >> 1, ck, o, ovf);
                            else *(u32x4*)(Ad + px * 128 + (((ck ^ (px >> 1)) & 7) << 4)) = o;
                        }
                        a_req(chunk + 2, i);
                    }
                    if (g == NSPC - 1) gk = gk_next;
                }
                loop_barrier();
            }
        }
        if constexpr (SPLIT) report_ovf();
        stamp(2); stamp_wait();
        if (do_epi) { epi_init(); epi_all(); }
        stamp(3);
    } else if (wave >= 4) {
        // ------------------------------------------------------------------ B producers (NB waves): weights, ONE STAGE AHEAD IN REGISTERS
        // During stage s these waves write stage s+1 (requested a whole stage earlier) into the other stage buffer and
        // re-request the same registers for stage s+2.
        if constexpr (SPLIT) report_ovf();
        const int ptid = tid - 256;
        constexpr int BU = BN * 8 / (NB * 64);                     // units per thread per tap
        unsigned boff[BU];
#pragma unroll
        for (int u = 0; u < BU; ++u) {
            const int idx = ptid + NB * 64 * u;
            boff[u] = (unsigned)(((size_t)(n0 + (idx >> 3)) * a.Cin_pad * sizeof(T)) + (idx & 7) * 16);
        }
        u32x4 bset[TPS][BU];
        // stage -> (chunk, tap group); requests past the end re-read the last stage (harmless, keeps the stream branch-free)
        auto b_req = [&](int chunk, int g, int tt) __attribute__((always_inline)) {
            const int c = chunk < a.nchunk ? chunk : a.nchunk - 1;
            const auto srd = w_srd(g * TPS + tt, c);
#pragma unroll
            for (int u = 0; u < BU; ++u) bset[tt][u] = __builtin_amdgcn_raw_buffer_load_b128(srd, boff[u], 0, 0);
        };
#pragma unroll
        for (int tt = 0; tt < TPS; ++tt) b_req(NSPC > 1 ? 0 : 1, NSPC > 1 ? 1 : 0, tt);       // stage 1
        __syncthreads();                                           // prologue tiles visible
        stamp(1);
        int stage = 0;
        const int n_stage = a.nchunk * NSPC;
        for (int chunk = 0; chunk < a.nchunk; ++chunk) {
#pragma unroll
            for (int g = 0; g < NSPC; ++g, ++stage) {
                constexpr int dummy = 0; (void)dummy;
                const bool wr = stage + 1 < n_stage && !CCN_DBG_BIT(a, 2);
                unsigned char* const Bd = Bs + ((stage + 1) & 1) * L::B_BYTES;
#pragma unroll
                for (int tt = 0; tt < TPS; ++tt) {
                    if (wr) {
#pragma unroll
                        for (int u = 0; u < BU; ++u) {
                            const int idx = ptid + NB * 64 * u, n = idx >> 3, ckb = idx & 7;
                            *(u32x4*)(Bd + tt * L::BT_BYTES + n * 128 + (((ckb ^ (n >> 1)) & 7) << 4)) = bset[tt][u];
                        }
                    }
                    b_req(chunk + (g + 2) / NSPC, (g + 2) % NSPC, tt);                         // stage + 2
                }
                loop_barrier();
            }
        }
        stamp(2); stamp_wait();
        if (do_epi) { epi_init(); epi_all(); }
        stamp(3);
    } else {
        // ------------------------------------------------------------------ consumers (4 waves): ds_read_b128 + MFMA only
        if constexpr (SPLIT) report_ovf();
        __builtin_amdgcn_s_setprio(2);
        f32x16 acc[MF][NF];
#pragma unroll
        for (int i = 0; i < MF; ++i)
#pragma unroll
            for (int j = 0; j < NF; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.0f;
        const int wm = wave / WN, wn = wave % WN;
        // Swizzled LDS byte address of 16-byte chunk (2*kk + h) of row `row`:  row*128 + (((2*kk + h) ^ (row >> 1)) & 7) * 16
        //   = rbase(row) ^ (kk << 5)   with   rbase(row) = row*128 + (((row >> 1) & 6) << 4) + (((h ^ (row >> 1)) & 1) << 4)
        // so the four kk reads of a fragment cost one v_xor each from a per-(fragment, tap) base.
        auto rbase = [&](int row) __attribute__((always_inline)) { return row * 128 + ((((row >> 1) & 6)) << 4) + (((h ^ (row >> 1)) & 1) << 4); };
        int prow[MF], bbase[NF], toff[NTAPS];
#pragma unroll
        for (int i = 0; i < MF; ++i) prow[i] = ((wm * MF + i) + 1) * HPITCH + r + 1;
#pragma unroll
        for (int j = 0; j < NF; ++j) bbase[j] = rbase((wn * NF + j) * 32 + r);
#pragma unroll
        for (int t = 0; t < NTAPS; ++t)
            toff[t] = NTAPS == 9 ? (t / 3 - 1) * HPITCH + (t % 3 - 1)
                                 : a.tapinfo_dy(par_off + t) * HPITCH + a.tapinfo_dx(par_off + t);
        __syncthreads();                                           // prologue tiles visible
        stamp(1);
        int stage = 0;
        for (int chunk = 0; chunk < a.nchunk; ++chunk) {
            const int a_off = (chunk & 1) * L::A_BYTES;
#pragma unroll
            for (int i = 0; i < MF; ++i) asm volatile("" : "+v"(prow[i]));    // keep the address math inside the loop (no hoist + spill)
#pragma unroll
            for (int g = 0; g < NSPC; ++g, ++stage) {
                const int b_off = 2 * L::A_BYTES + (stage & 1) * L::B_BYTES;
                if constexpr (SPLIT) {
                    constexpr int NT = TPS, DPM = 0;
                    int abase[MF];
                    auto a_tap = [&](int tt) __attribute__((always_inline)) {
#pragma unroll
                        for (int i = 0; i < MF; ++i) abase[i] = a_off + rbase(prow[i] + toff[g * TPS + tt]);
                    };
                    auto b_tap = [&](int tt) __attribute__((always_inline)) { return b_off + tt * (int)L::BT_BYTES; };
                    auto tap_begin = [&](int) __attribute__((always_inline)) {};
                    auto tap_landed = [&](int) __attribute__((always_inline)) {};
#include "tile/split_steps.inc"
                } else {
                    // fragments of step j+1 are requested before the MFMAs of step j (step = tap * 4 + kk)
                    constexpr int PF = 1;                         // fragment prefetch distance in steps (2 measured no faster: the loop is LDS-bandwidth bound)
                    constexpr int NSTEP = TPS * 4;
                    u32x4 av[PF + 1][MF], bv[PF + 1][NF];
                    int abase[MF];
                    auto frag = [&](int j, u32x4* av_, u32x4* bv_) __attribute__((always_inline)) {
                        const int tt = j >> 2, kk = j & 3;
                        if (kk == 0) {
#pragma unroll
                            for (int i = 0; i < MF; ++i) abase[i] = a_off + rbase(prow[i] + toff[g * TPS + tt]);
                        }
#pragma unroll
                        for (int i = 0; i < MF; ++i) av_[i] = *(const u32x4*)(smem + (abase[i] ^ (kk << 5)));
#pragma unroll
                        for (int jn = 0; jn < NF; ++jn)
                            bv_[jn] = *(const u32x4*)(smem + b_off + tt * L::BT_BYTES + (bbase[jn] ^ (kk << 5)));
                    };
#pragma unroll
                    for (int j = 0; j < PF && j < NSTEP; ++j) frag(j, av[j % (PF + 1)], bv[j % (PF + 1)]);
#pragma unroll
                    for (int j = 0; j < NSTEP; ++j) {
                        __builtin_amdgcn_sched_barrier(0);
                        if (j + PF < NSTEP) frag(j + PF, av[(j + PF) % (PF + 1)], bv[(j + PF) % (PF + 1)]);
#pragma unroll
                        for (int i = 0; i < MF; ++i)
#pragma unroll
                            for (int jn = 0; jn < NF; ++jn) mfma16<T>(acc[i][jn], av[j % (PF + 1)][i], bv[j % (PF + 1)][jn]);
                        // An in-order wave that issues its MFMAs back to back leaves 24 of every 32 issue cycles unused and
                        // then runs the next step's address math / ds_reads while the matrix pipe drains (a pure MFMA
                        // stream measured 76 % of the pipe rate).  Interleave: one MFMA, then one LDS read and up to two
                        // VALU of the NEXT step's fragment fetch in its shadow; the wait before this step's first MFMA is
                        // then a counted lgkmcnt on reads issued a whole step ago.
#pragma unroll
                        for (int m = 0; m < MF * NF; ++m) {
                            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);      // 1 MFMA
                            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);      // 1 DS read
                            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);      // 2 VALU
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
                loop_barrier();
            }
        }
        __builtin_amdgcn_s_setprio(0);
        stamp(2); stamp_wait();
        if (do_epi) {
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
// 3x3 s1: 4-row tiles stage 3 taps per barrier, 8-row tiles 1 tap (LDS); ConvTranspose parities (4 taps): 2 / 1.
template <typename T> static tile_fn_t pick_ws_t(int ntaps, int th, int bn)
{
    if (ntaps == 9) {
        if (th == 8) return bn == 128 ? conv_ws_kernel<T, 4, 2, 9, 1> : conv_ws_kernel<T, 4, 1, 9, 1>;
        return bn == 128 ? conv_ws_kernel<T, 2, 2, 9, 3> : conv_ws_kernel<T, 2, 1, 9, 3>;
    }
    if (th == 8) return bn == 128 ? conv_ws_kernel<T, 4, 2, 4, 1> : conv_ws_kernel<T, 4, 1, 4, 1>;
    return bn == 128 ? conv_ws_kernel<T, 2, 2, 4, 2> : conv_ws_kernel<T, 2, 1, 4, 2>;
}
// dtype: the storage type, or CCN_DTYPE_F16X3 = 2 for fp32 storage with split operand rows (ConvArgs::ops)
static tile_fn_t pick_ws(int dtype, int ntaps, int th, int bn)
{
    if (dtype == 2) return pick_ws_t<f16x3_t>(ntaps, th, bn);
    return dtype == 0 ? pick_ws_t<float>(ntaps, th, bn) : pick_ws_t<__bf16>(ntaps, th, bn);
}
static size_t ws_lds(int ntaps, int th, int bn)
{
    if (th == 8) return bn == 128 ? WsLds<8, 128, 1>::TOTAL : WsLds<8, 64, 1>::TOTAL;
    if (ntaps == 9) return bn == 128 ? WsLds<4, 128, 3>::TOTAL : WsLds<4, 64, 3>::TOTAL;
    return bn == 128 ? WsLds<4, 128, 2>::TOTAL : WsLds<4, 64, 2>::TOTAL;
}

bool conv_ws_supported(int kind, int bn) { return (kind == KIND_C3S1 || kind == KIND_CT4) && (bn == 128 || bn == 64); }

hipError_t conv_ws_prepare() { return tiled_prepare(pick_ws, ws_lds); }

static StampBuf g_stamps;
extern "C" int ccn_internal_dump_stamps(const char* path) { return g_stamps.dump(path); }

hipError_t launch_conv_ws(int dtype, int bn, const ConvArgs& a, hipStream_t s)
{
    const unsigned grid = (unsigned)(a.B * a.n_ty * a.n_tx * a.npar * a.n_nt);
    if (a.ops && dtype != 0) return hipErrorInvalidValue;       // split operand rows exist for fp32 storage only
    return launch_tiled(pick_ws(a.ops ? 2 : dtype, a.ntaps, a.th, bn), grid, ws_lds(a.ntaps, a.th, bn), a, s, g_stamps);
}

}  // namespace ccn
