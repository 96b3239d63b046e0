// The network, once: what models/unet.py:45-79 registers, as plain host data.  Included by ccn_api.hip (inference handle) and
// ccn_train.hip (training handle) and by nothing else; each handle keeps this description plus its own per-conv device state.
//
// Everything both handles -- and their callers -- must agree on is decided here: parameter names, shapes and order (the key order
// of CLIPCondUNet.state_dict(), which is also the order of the training step's flat buffers and of the DDP buckets), the conv
// list, the ResBlock / stride-2 / ConvTranspose channel arithmetic, the layer list and the rows of the concatenated FiLM linear.
#pragma once
#include "../../include/ccn_hip.h"
#include "ccn_internal.h"

#include <string>
#include <vector>

namespace ccn {

struct ArchParam {
    std::string name;
    std::vector<int64_t> shape;
    size_t off = 0;             // floats from the start of the training step's flat buffers; every parameter starts 16-byte aligned
    size_t numel() const { size_t n = 1; for (auto d : shape) n *= (size_t)d; return n; }
};
// Conv2d weights are (Cout, Cin, 3, 3), ConvTranspose2d (KIND_CT4) weights (Cin, Cout, 4, 4)
struct ArchConv {
    int kind = KIND_C3S1, Cin = 0, Cout = 0;
    std::string name;           // in_conv, <block>.conv1, <block>.conv2, down.N, up.N, out
    int pw = -1, pb = -1;       // parameter indices (weight, bias)
};
struct ArchNorm { int C = 0, pg = -1, pb = -1; };
struct ArchLin { int pw = -1, pb = -1, N = 0, K = 0; };
struct ArchRes {
    std::string prefix;
    int C = 0;
    ArchNorm n1, n2;
    int c1 = -1, c2 = -1;       // indices into Arch::convs
    ArchLin fs, fh;             // film.to_scale, film.to_shift
    int film_off = 0;           // row offset into the concatenated FiLM linear: [off, off+C) scale, [off+C, off+2C) shift
};
enum LType { L_STEM, L_RES, L_DOWN, L_UP, L_HEAD };
struct ArchLayer { LType type; std::string name; int idx; };   // name: the activation the layer writes; idx: into res (L_RES), else convs

struct Arch {
    std::vector<ArchParam> params;      // registration order
    size_t total = 0;                   // floats of the flat layout
    std::vector<ArchConv> convs;        // registration order
    std::vector<ArchRes> res;
    std::vector<ArchLayer> layers;
    ArchNorm out_norm;
    ArchLin tp0, tp2, zp;               // time_proj.0, time_proj.2, z_proj.0
    int F = 0;                          // rows of the concatenated FiLM linear
};

inline Arch build_arch(const ccn_config_t& c)
{
    Arch a;
    const int td = c.time_dim;
    auto param = [&](const std::string& name, std::vector<int64_t> shape) {
        ArchParam p; p.name = name; p.shape = std::move(shape); p.off = a.total;
        a.total += (p.numel() + 3) / 4 * 4;
        a.params.push_back(p);
        return (int)a.params.size() - 1;
    };
    auto lin = [&](const std::string& n, int N, int K) { ArchLin l; l.N = N; l.K = K; l.pw = param(n + ".weight", {N, K}); l.pb = param(n + ".bias", {N}); return l; };
    auto norm = [&](const std::string& n, int C) { ArchNorm g; g.C = C; g.pg = param(n + ".weight", {C}); g.pb = param(n + ".bias", {C}); return g; };
    auto conv = [&](const std::string& n, int kind, int Cin, int Cout) {
        ArchConv w; w.kind = kind; w.Cin = Cin; w.Cout = Cout; w.name = n;
        if (kind == KIND_CT4) w.pw = param(n + ".weight", {Cin, Cout, 4, 4});
        else w.pw = param(n + ".weight", {Cout, Cin, 3, 3});
        w.pb = param(n + ".bias", {Cout});
        a.convs.push_back(w);
        return (int)a.convs.size() - 1;
    };
    auto res = [&](const std::string& name, int cc) {
        ArchRes r; r.prefix = name; r.C = cc;
        r.n1 = norm(name + ".norm1", cc); r.c1 = conv(name + ".conv1", KIND_C3S1, cc, cc);
        r.n2 = norm(name + ".norm2", cc); r.c2 = conv(name + ".conv2", KIND_C3S1, cc, cc);
        r.fs = lin(name + ".film.to_scale", cc, td); r.fh = lin(name + ".film.to_shift", cc, td);
        r.film_off = a.F; a.F += 2 * cc;
        a.res.push_back(r);
        a.layers.push_back({L_RES, name, (int)a.res.size() - 1});
    };
    auto conv_layer = [&](LType type, const std::string& name, int kind, int Cin, int Cout) { a.layers.push_back({type, name, conv(name, kind, Cin, Cout)}); };
    a.tp0 = lin("time_proj.0", td * 4, td);
    a.tp2 = lin("time_proj.2", td, td * 4);
    a.zp = lin("z_proj.0", td, c.z_dim);
    conv_layer(L_STEM, "in_conv", KIND_STEM, c.img_ch, c.base);
    int ch = c.base;
    for (int i = 0; i < c.n_mult; ++i) {
        const int m = c.ch_mult[i];
        res("down." + std::to_string(3 * i), ch);
        res("down." + std::to_string(3 * i + 1), ch);
        conv_layer(L_DOWN, "down." + std::to_string(3 * i + 2), KIND_C3S2, ch, ch * m);
        ch *= m;
    }
    res("mid1", ch);
    res("mid2", ch);
    for (int i = 0; i < c.n_mult; ++i) {
        const int m = c.ch_mult[c.n_mult - 1 - i];
        res("up." + std::to_string(3 * i), ch);
        res("up." + std::to_string(3 * i + 1), ch);
        conv_layer(L_UP, "up." + std::to_string(3 * i + 2), KIND_CT4, ch, ch / m);
        ch /= m;
    }
    a.out_norm = norm("out_norm", ch);
    conv_layer(L_HEAD, "out", KIND_HEAD, ch, c.img_ch);
    return a;
}

}  // namespace ccn
