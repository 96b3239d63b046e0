// GroupNorm partial sums of the tile just stored: each thread's s1 / s2 (its pixels of 8 channels) -> one partial per (tile,
// group) -> the in-kernel finalize where the launch asks for it.  By all 64 * NWAVES threads, once no wave reads the fp32 tile.
// The summation order is part of the contract (outputs are compared bit for bit between builds): lanes sharing an octet by xor
// stride from NOCT up, then the waves in index order, then the channels of each group in index order.
// Expects: decode.inc, E = EpiLds<TH, BN, NWAVES>, NWAVES, NOCT, s1, s2, smem, tid, lane, wave; inside `if (a.part) { }`.
#pragma unroll
    for (int s = NOCT; s < 64; s <<= 1)
#pragma unroll
        for (int e = 0; e < 8; ++e) { s1[e] += __shfl_xor(s1[e], s); s2[e] += __shfl_xor(s2[e], s); }
    float* const red = (float*)(smem + E::CS_BYTES);        // [NWAVES][BN][2]
    float* const chs = red + NWAVES * BN * 2;               // [BN][2]
    if (lane < NOCT) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            red[(wave * BN + lane * 8 + e) * 2 + 0] = s1[e];
            red[(wave * BN + lane * 8 + e) * 2 + 1] = s2[e];
        }
    }
    __syncthreads();
    if (tid < BN) {
        float t1 = 0.f, t2 = 0.f;
#pragma unroll
        for (int w = 0; w < NWAVES; ++w) { t1 += red[(w * BN + tid) * 2]; t2 += red[(w * BN + tid) * 2 + 1]; }
        chs[tid * 2] = t1; chs[tid * 2 + 1] = t2;
    }
    __syncthreads();
    if (n0 < a.Cout) {
        const int nend = min(n0 + BN, a.Cout);
        const int g = n0 / a.cpg + tid;
        if (g <= (nend - 1) / a.cpg) {
            const int clo = max(g * a.cpg, n0), chi = min((g + 1) * a.cpg, nend);
            float t1 = 0.f, t2 = 0.f;
            for (int c = clo; c < chi; ++c) { t1 += chs[(c - n0) * 2]; t2 += chs[(c - n0) * 2 + 1]; }
            const int slot = (((ty * a.n_tx + tx) * a.npar + par) * a.n_nt) + nt;
            part_store(a.part + (size_t)(b * a.G + g) * a.nslot + slot, t1, t2);
        }
    }
    if (a.fin_counter) gn_fused_finalize<64 * NWAVES>(a, b, (unsigned*)red, tid);
