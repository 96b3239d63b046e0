// Diagnostic stamps and the main loop's barrier.  CCN_STAMPS_PTR(a) is a constant null in the product build, where all of this
// folds to the bare barrier, and null outside profiling runs of the diagnostics build.
// A workgroup owns 3 rows of 8 words (StampBuf::STAMP_WORDS), written by lane 0 of the first wave of each role: row 0 consumers
// (wave 0), row 1 weight producers (wave STAMP_B0; -1: the kernel has none), row 2 input producers (wave A0).  Per row: words
// 0..3 s_memrealtime at entry, prologue done, loop done, exit; 4 shader cycles spent inside the loop's barriers; 5, 6 s_memtime
// around the loop (-> in-kernel clock).  tools/stamp_*.py and tools/prof_sample.py parse this layout.
// Expects: a, lane, wave, A0, STAMP_B0, LOOP_BARRIER_RAW (the loop's barrier is raw_barrier(), else __syncthreads()).
// Defines: stamp(slot), bar_wait, raw_barrier(), loop_barrier(), stamp_wait().
    auto stamp = [&](int slot) __attribute__((always_inline)) {
        if (CCN_STAMPS_PTR(a) && lane == 0 && (wave == 0 || wave == STAMP_B0 || wave == A0)) {
            unsigned long long* st = CCN_STAMPS_PTR(a) + ((size_t)blockIdx.x * 3 + (wave == 0 ? 0 : (wave == STAMP_B0 ? 1 : 2))) * 8;
            st[slot] = __builtin_amdgcn_s_memrealtime();
            if (slot == 1) st[5] = __builtin_amdgcn_s_memtime();
            if (slot == 2) st[6] = __builtin_amdgcn_s_memtime();
        }
    };
    unsigned long long bar_wait = 0;
    // raw barrier: drain only this wave's LDS operations; in-flight buffer loads (register prefetch, LDS-DMA) survive it
    [[maybe_unused]] auto raw_barrier = [&]() __attribute__((always_inline)) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    };
    auto loop_barrier = [&]() __attribute__((always_inline)) {
        auto barrier = [&]() __attribute__((always_inline)) { if constexpr (LOOP_BARRIER_RAW) raw_barrier(); else __syncthreads(); };
        if (CCN_STAMPS_PTR(a)) { const unsigned long long t0 = __builtin_amdgcn_s_memtime(); barrier(); bar_wait += __builtin_amdgcn_s_memtime() - t0; }
        else barrier();
    };
    auto stamp_wait = [&]() __attribute__((always_inline)) {
        if (CCN_STAMPS_PTR(a) && lane == 0 && (wave == 0 || wave == STAMP_B0 || wave == A0))
            CCN_STAMPS_PTR(a)[((size_t)blockIdx.x * 3 + (wave == 0 ? 0 : (wave == STAMP_B0 ? 1 : 2))) * 8 + 4] = bar_wait;
    };
    stamp(0);
