// Epilogue of the 8-wave kernels, run by all 512 threads after their loops: fp32 tile in LDS -> bias / FiLM / residual -> 16-byte
// NHWC rows, with the running sums for the next GroupNorm.  Thread (o, ps) owns the 8 output channels nb .. nb + 7 of the pixels
// ps, ps + PSL, ... of every 128-pixel pass.  Expects: decode.inc, E = EpiLds<TH, BN, 8>, T, EPC, SPLIT, smem, tid.
// Defines: Cs, CP, NOCT, PSL, NIT, NPASS, o, ps, nb, nvalid, f1, f2, s1, s2, outb, resb, epi_init(), epi_all().
//
// NOT for the 4-wave kernel (ccn_kernels.hip): that one computes fmaf(v + bias, f1, f2), this one folds the bias into the shift
// first and computes fmaf(v, f1, fmaf(bias, f1, shift)).  The two round differently, and the goldens and replay bounds of the
// tests are fitted to each kernel's bits.
    float* const Cs = (float*)smem;
    constexpr int CP = E::CP;
    constexpr int NOCT = BN / 8, PSL = 512 / NOCT, NIT = 128 / PSL;
    constexpr int NPASS = TH / 4;
    const int o = tid % NOCT, ps = tid / NOCT;
    const int nb = n0 + o * 8;
    const bool nvalid = nb < a.Cout;
    float f1[8], f2[8], s1[8], s2[8];           // v = acc * f1 + f2 with f2 = bias * f1 + shift; running sum / sum of squares
    unsigned char* const outb = (unsigned char*)a.out;
    const unsigned char* const resb = (const unsigned char*)a.res;
    auto epi_init = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { f1[e] = 1.f; f2[e] = 0.f; s1[e] = 0.f; s2[e] = 0.f; }
        if (nvalid) {
#pragma unroll
            for (int e = 0; e < 8; ++e) f2[e] = a.bias[nb + e];
            if (a.film) {
                const float* fp = a.film + (size_t)b * a.film_bstride;
#pragma unroll
                for (int e = 0; e < 8; ++e) { f1[e] = 1.0f + fp[nb + e]; f2[e] = fmaf(f2[e], f1[e], fp[a.Cout + nb + e]); }
            }
        }
    };
    // Whole tile at once: every residual / skip row is requested before the single barrier that publishes the fp32
    // tiles (one 128-pixel tile per 4 tile rows), so the HBM latency of the residual overlaps the accumulator hand-off.
    auto epi_all = [&]() __attribute__((always_inline)) {
        u32x4 rres[NPASS * NIT][EPC == 8 ? 1 : 2];
        size_t eoff[NPASS * NIT];
        unsigned vmask = 0;
#pragma unroll
        for (int q = 0; q < NPASS * NIT; ++q) {
            const int pass = q / NIT, itp = q - pass * NIT;
            const int m = itp * PSL + ps;
            const int my = my0 + pass * 4 + (m >> 5), mx = mx0 + (m & 31);
            const bool v = nvalid && my < a.MH && mx < a.MW;
            const int oy = my * a.OS + py, ox = mx * a.OS + px_;
            eoff[q] = (((size_t)(b * a.Hout + oy) * a.Wout + ox) * a.Cout + nb) * sizeof(T);
            if (v) vmask |= 1u << q;
#pragma unroll
            for (int w = 0; w < (EPC == 8 ? 1 : 2); ++w) {
                rres[q][w] = u32x4{0u, 0u, 0u, 0u};
                if (v && resb) rres[q][w] = *(const u32x4*)(resb + eoff[q] + 16 * w);
            }
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < NPASS * NIT; ++q) {
            if ((vmask >> q) & 1u) {
                const int pass = q / NIT, itp = q - pass * NIT;
                const int m = itp * PSL + ps;
                const float* cs = Cs + pass * (E::CS1_BYTES / 4) + m * CP + o * 8;
                float v[8];
                const f32x4 c0 = *(const f32x4*)cs, c1 = *(const f32x4*)(cs + 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[e] = c0[e]; v[4 + e] = c1[e]; }
                if constexpr (SPLIT) {                    // f16x3: undo the weights' power-of-two scale (exact), before the bias
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] *= a.wscale_inv;
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = fmaf(v[e], f1[e], f2[e]);
                if (resb) {
                    float rv[8];
                    Vec16<T>::unpack(rres[q][0], rv);
                    if constexpr (EPC == 4) Vec16<T>::unpack(rres[q][1], rv + 4);
#pragma unroll
                    for (int e = 0; e < 8; ++e) v[e] += rv[e];
                }
                *(u32x4*)(outb + eoff[q]) = Vec16<T>::pack(v);
                if constexpr (EPC == 4) *(u32x4*)(outb + eoff[q] + 16) = Vec16<T>::pack(v + 4);
#pragma unroll
                for (int e = 0; e < 8; ++e) { s1[e] += v[e]; s2[e] = fmaf(v[e], v[e], s2[e]); }
            }
        }
    };
