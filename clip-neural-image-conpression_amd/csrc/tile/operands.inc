// The two operands of a 3x3 s1 / ConvTranspose-parity tile.  Expects: decode.inc, T, CKE.  Defines: wbase, inb, gn, iy0, ix0 (input
// pixel of the halo's corner), wtap_bytes, OOB, in_bytes, in_srd(chunk), w_srd(tap, chunk).
    const unsigned char* const wbase = (const unsigned char*)a.w;
    const unsigned char* const inb = (const unsigned char*)a.in;
    const bool gn = a.gn_ab != nullptr;
    const int iy0 = my0 - 1, ix0 = mx0 - 1;
    const size_t wtap_bytes = (size_t)a.Cout_pad * a.Cin_pad * sizeof(T);      // one tap of the packed weights
    // Buffer descriptors: a wave-uniform base in SGPRs + a 32-bit per-lane byte offset, and hardware range checking --
    // an offset past num_records returns zeros without touching memory, which implements the conv zero padding, the
    // tile overhang and the Cin tail with no branch around any load (loads issue back to back).
    constexpr unsigned OOB = 0x7FFFFFF0u;
    const unsigned in_bytes = (unsigned)((size_t)a.B * a.Hin * a.Win * a.Cin * sizeof(T));
    auto in_srd = [&](int chunk) __attribute__((always_inline)) {
        const unsigned off = (unsigned)((size_t)chunk * CKE * sizeof(T));
        return __builtin_amdgcn_make_buffer_rsrc((void*)(inb + off), 0, in_bytes - off, 0x00020000);
    };
    auto w_srd = [&](int tap, int chunk) __attribute__((always_inline)) {
        return __builtin_amdgcn_make_buffer_rsrc((void*)(wbase + (size_t)a.tapinfo_w(par_off + tap) * wtap_bytes + (size_t)chunk * CKE * sizeof(T)),
                                                 0, (unsigned)wtap_bytes, 0x00020000);
    };
