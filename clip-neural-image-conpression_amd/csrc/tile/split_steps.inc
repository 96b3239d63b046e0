// f16x3: a consumer wave's MFMA steps over NT staged taps of the current Cin chunk (ccn_device.h describes the split rows).
// Step j = tap * 2 + kk is the K = 16 slice kk of the tap's 32 channels: acc += a_lo b_hi; acc += a_hi b_lo; acc += a_hi b_hi, a term at a
// time over the wave's MF x NF accumulators.  Fragments are fetched a term ahead into the registers the previous term released --
// a_lo and b_hi of step j + 1 under the last term of step j, a_hi and b_lo of step j under its first -- so only b_hi is double
// buffered: 56 fragment registers, where two whole steps in flight would take 96 and spill the 8-row / BN 128 tile.
// Expects: MF, NF, NT, acc, smem, abase[MF], bbase[NF] and the kernel's lambdas
//   a_tap(tt)      abase[] <- tap tt            b_tap(tt)       byte offset of tap tt's weight rows of this wave
//   tap_begin(tt)  issued at the tap's first step (fr: refill the ring slot of the tap before)
//   tap_landed(tt) before the first fragment read of tap tt (fr: its LDS-DMA has landed)
//   DPM            VMEM instructions tap_begin() issues per MFMA shadow (0: none)
    {
        constexpr int NSTEP = NT * 2;
        u32x4 ah[MF], al[MF], bh[2][NF], bl[NF];
        auto ld_a = [&](u32x4* d, int unit) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < MF; ++i) d[i] = *(const u32x4*)(smem + (abase[i] ^ (unit << 5)));
        };
        auto ld_b = [&](u32x4* d, int tt, int unit) __attribute__((always_inline)) {
            const int bo = b_tap(tt);
#pragma unroll
            for (int jn = 0; jn < NF; ++jn) d[jn] = *(const u32x4*)(smem + bo + (bbase[jn] ^ (unit << 5)));
        };
        // unit = 16-byte pair (2 unit + h) of the row: units 0, 1 are the hi fragments of slices 0, 1; units 2, 3 their lo fragments
        tap_landed(0); a_tap(0);
        ld_b(bh[0], 0, 0); ld_a(al, 2);
#pragma unroll
        for (int j = 0; j < NSTEP; ++j) {
            const int tt = j >> 1, kk = j & 1;
            __builtin_amdgcn_sched_barrier(0);
            if (kk == 0) tap_begin(tt);
            ld_b(bl, tt, 2 + kk); ld_a(ah, kk);
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int jn = 0; jn < NF; ++jn) mfma_f16(acc[i][jn], al[i], bh[j & 1][jn]);
            // one MFMA, then in its shadow the tap's DMA pieces (first step), one LDS read and up to two VALU of the fetch
#pragma unroll
            for (int m = 0; m < MF * NF; ++m) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                if (kk == 0 && DPM > 0) __builtin_amdgcn_sched_group_barrier(0x020, DPM, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int jn = 0; jn < NF; ++jn) mfma_f16(acc[i][jn], ah[i], bl[jn]);
            __builtin_amdgcn_sched_barrier(0);
            if (j + 1 < NSTEP) {
                if (kk == 1) { tap_landed(tt + 1); a_tap(tt + 1); }
                ld_b(bh[(j + 1) & 1], (j + 1) >> 1, (j + 1) & 1); ld_a(al, 2 + ((j + 1) & 1));
            }
#pragma unroll
            for (int i = 0; i < MF; ++i)
#pragma unroll
                for (int jn = 0; jn < NF; ++jn) mfma_f16(acc[i][jn], ah[i], bh[j & 1][jn]);
#pragma unroll
            for (int m = 0; m < MF * NF; ++m) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
