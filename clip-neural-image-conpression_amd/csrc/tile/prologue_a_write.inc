// Prologue, second half: GroupNorm + SiLU on the real pixels (padding and overhang stay zero), swizzled write into As.
// Expects: prologue_a_load.inc in the same block, As; SPLIT and ovf (f16x3 form: the unit goes out as fp16 hi + lo halves).
#pragma unroll
    for (int i = 0; i < PIT; ++i) {
        const int px = (tid >> 3) + 64 * i;
        if (px < G::HROWS * HPITCH) {
            u32x4 o = raw[i];
            if (((okm >> i) & 1u) && gn) o = gk.template apply<true>(raw[i]);
            if constexpr (SPLIT) split_put(As + px * 128, px >> 1, ck, o, ovf);
            else *(u32x4*)(As + px * 128 + (((ck ^ (px >> 1)) & 7) << 4)) = o;
        }
    }
