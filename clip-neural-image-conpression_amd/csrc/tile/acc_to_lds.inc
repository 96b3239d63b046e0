// A consumer wave's accumulators (fragment rows wm * MF + i, fragment columns wn * NF + j) into the epilogue's fp32 tile.
// Expects: epilogue.inc, acc[MF][NF], wm, wn, r, h.
#pragma unroll
    for (int i = 0; i < MF; ++i) {
        const int row = wm * MF + i;                        // tile row of this fragment -> pass row/4, rows (row&3)*32..
        float* const cst = Cs + (row / 4) * (E::CS1_BYTES / 4);
#pragma unroll
        for (int j = 0; j < NF; ++j)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int m = (row & 3) * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
                cst[m * CP + (wn * NF + j) * 32 + r] = acc[i][j][q];
            }
    }
