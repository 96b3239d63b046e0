// Prologue, first half: Cin chunk 0 of the input halo requested by all 512 threads (prologue_a_write.inc is the second half; a
// kernel puts its other prologue loads between the two).  Expects: operands.inc, G = TileGeom<TH>, HPITCH, EPC, tid, inside a
// block of its own.  Defines: ck, gk, cv, PIT, raw[], okm (bit i: unit i is a real pixel), srd0.
    const int ck = tid & 7;
    GnCoef<T> gk;
    const bool cv = ck * EPC < a.Cin;
    gk.load(a.gn_ab + (size_t)b * a.Cin + (cv ? ck * EPC : 0), gn && cv);
    constexpr int PIT = (G::AU + 511) / 512;
    u32x4 raw[PIT];
    unsigned okm = 0;
    const auto srd0 = in_srd(0);
#pragma unroll
    for (int i = 0; i < PIT; ++i) {
        const int px = (tid >> 3) + 64 * i;
        const int hy = px / HPITCH, hx = px - hy * HPITCH;
        const int iy = iy0 + hy, ix = ix0 + hx;
        const bool ok = px < G::HROWS * HPITCH && cv && iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win;
        const unsigned off = ok ? (unsigned)((((size_t)(b * a.Hin + iy) * a.Win + ix) * a.Cin + ck * EPC) * sizeof(T)) : OOB;
        raw[i] = __builtin_amdgcn_raw_buffer_load_b128(srd0, off, 0, 0);
        if (ok) okm |= 1u << i;
    }
