// What the tiled conv kernels share.
//
// Compile-time geometry and the host side of the 8-wave kernels (ccn_conv_ws.hip, ccn_conv_fr.hip) are ordinary C++, below.
//
// The device code they share lives in tile/*.inc and is shared TEXTUALLY: each fragment is included inside the kernel body, reads
// the kernel's locals by name and defines more of them (its first lines say which).  That is deliberate.  The pieces are lambdas
// and straight-line code over a dozen kernel locals; written as structs and __forceinline__ functions they compute the same values,
// but hipcc optimises a function body before it inlines it, and register allocation and schedule of these 250-VGPR kernels then
// move (docs/EXPERIMENTS.md R4.1: the struct form changed instruction counts in all 16 conv_ws_kernel
// instantiations).  Included as text, the compiler sees the tokens it saw when each kernel carried its own copy, and the code
// objects do not change.
//
//   tile/decode.inc            blockIdx.x -> (sample, tile, parity, channel tile)                      ws, fr, 4-wave
//   tile/operands.inc          halo corner, buffer descriptors of input and weights                   ws, fr
//   tile/prologue_a_load.inc   Cin chunk 0 of the input halo by the whole workgroup: request ...      ws, fr
//   tile/prologue_a_write.inc  ... GroupNorm + SiLU, swizzled write                                   ws, fr
//   tile/epilogue.inc          fp32 tile -> bias / FiLM / residual -> NHWC rows, running sums          ws, fr
//   tile/acc_to_lds.inc        a consumer wave's accumulators -> fp32 tile                             ws, fr
//   tile/gn_part_tail.inc      running sums -> GroupNorm partials -> optional in-kernel finalize       ws, fr, 4-wave
//   tile/split_steps.inc       f16x3 operand form only: the consumers' MFMA steps over the staged taps   ws, fr
//
// What stays in each kernel file is what tells the kernels apart: the LDS ring layout of the main loop, the split of the waves
// into roles with their stamps, and the main loops.  The 4-wave kernel's epilogue is deliberately its own (tile/epilogue.inc
// says why), and so is everything in conv_pr_kernel (epilogue in the producer waves, bf16 staging tile, another thread mapping).
#pragma once
#include "ccn_device.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace ccn {

// input halo of a TH x 32 tile of a 3x3 s1 conv / ConvTranspose parity: one 128-byte LDS row per pixel and Cin chunk
template <int TH> struct TileGeom {
    static constexpr int HROWS = TH + 2, HPITCH = 34;
    static constexpr int A_BYTES = HROWS * HPITCH * 128;
    static constexpr int AU = HROWS * HPITCH * 8;            // 16-byte units per chunk
};
// what the epilogue of an NWAVES-wave kernel lays over the main loop's LDS
template <int TH, int BN, int NWAVES> struct EpiLds {
    static constexpr int CP = BN + 4;                        // fp32 tile pitch (floats)
    static constexpr int CS1_BYTES = 128 * CP * 4;           // fp32 epilogue tile of one 128-pixel pass
    static constexpr int CS_BYTES = (TH / 4) * CS1_BYTES;    // all passes at once: one barrier for the whole epilogue
    static constexpr int RED_BYTES = NWAVES * BN * 2 * 4 + BN * 2 * 4;      // tile/gn_part_tail.inc: red[NWAVES][BN][2], chs[BN][2]
    static constexpr int total(int loop) { return loop > CS_BYTES + RED_BYTES ? loop : CS_BYTES + RED_BYTES; }
};

// ---- host side of the 8-wave kernels ----------------------------------------------------------------------------------
typedef void (*tile_fn_t)(const ConvArgs);

// raise the dynamic-LDS limit of every instantiation a pick table can return: 3 operand forms (fp32, bf16, f16x3) x {4, 9} taps x {4, 8} rows x BN {64, 128}
template <class Pick, class Lds> hipError_t tiled_prepare(Pick pick, Lds lds)
{
    for (int dt = 0; dt < 3; ++dt)
        for (int ntaps = 4; ntaps <= 9; ntaps += 5)
            for (int th = 4; th <= 8; th += 4)
                for (int bn = 64; bn <= 128; bn += 64) {
                    hipError_t e = hipFuncSetAttribute((const void*)pick(dt, ntaps, th, bn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       (int)lds(ntaps, th, bn));
                    if (e != hipSuccess) return e;
                }
    return hipSuccess;
}

// Diagnostic: CCN_STAMPS=<grid>[:<ntaps>] records the in-kernel stamps of every launch with that grid (last one wins), STAMP_WORDS
// 64-bit words per workgroup = 3 role rows x 8 (each kernel's `stamp` lambda says what it writes where); dump() writes them
// out, one workgroup per line.  Never set in timed runs.
struct StampBuf {
    static constexpr unsigned MAX_GRID = 8192;
    static constexpr int STAMP_WORDS = 24;
    unsigned long long* dev = nullptr;
    unsigned grid = 0;          // of the last recorded launch
    int dump(const char* path) const
    {
        if (!dev || !grid) return 1;
        std::vector<unsigned long long> h((size_t)grid * STAMP_WORDS);
        if (hipMemcpy(h.data(), dev, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return 2;
        FILE* f = fopen(path, "w");
        if (!f) return 3;
        for (unsigned b = 0; b < grid; ++b)
            for (int k = 0; k < STAMP_WORDS; ++k) fprintf(f, "%llu%c", h[(size_t)b * STAMP_WORDS + k], k == STAMP_WORDS - 1 ? '\n' : ' ');
        fclose(f);
        return 0;
    }
};

inline hipError_t launch_tiled(tile_fn_t fn, unsigned grid, size_t lds, const ConvArgs& a, hipStream_t s, StampBuf& sb)
{
    static const char* env = diag_env("CCN_STAMPS");
    if (env) {
        const unsigned want = (unsigned)atoi(env), want_taps = strchr(env, ':') ? (unsigned)atoi(strchr(env, ':') + 1) : 9u;
        if (grid == want && (unsigned)a.ntaps == want_taps && grid <= StampBuf::MAX_GRID) {
            if (!sb.dev && hipMalloc((void**)&sb.dev, (size_t)StampBuf::MAX_GRID * StampBuf::STAMP_WORDS * 8) != hipSuccess) return hipErrorOutOfMemory;
            sb.grid = grid;
            ConvArgs d = a; d.stamps = sb.dev;
            hipLaunchKernelGGL(fn, dim3(grid), dim3(512), lds, s, d);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL(fn, dim3(grid), dim3(512), lds, s, a);
    return hipGetLastError();
}

}  // namespace ccn
