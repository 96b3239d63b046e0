// Host side of the training step: ccn_train_* of include/ccn_hip.h, everything that works on a ccn_trainer_t.  (The loss, the step
// guard, AdamW and the EMA take raw buffers and no handle: ccn_optim.hip.)
//
// Reference: the loop body of train/diffusion_train.py:119-124,137-140 -- eps_hat = net(x_t, z, t); loss = mse(eps_hat, noise);
// loss.backward(); opt.step().  ccn_train_forward is CLIPCondUNet.forward (models/unet.py:81-106) with every tensor the
// backward needs kept in the caller's workspace; ccn_train_backward takes d loss / d eps_hat and ACCUMULATES the gradient of
// every parameter into a flat fp32 buffer laid out like the flat parameter buffer (the order of CLIPCondUNet.state_dict()).
// The network itself -- parameters with their flat offsets, convs, ResBlocks, layer list -- is build_arch's description
// (ccn_arch.h), shared with the inference handle; this file adds the per-conv operands and repack descriptors (TConvW).
//
// Parameters are read from the caller's flat fp32 buffer on every call (they change with every optimiser step) and repacked on
// the device into the operand layouts of the convolution kernels.  Activations and activation gradients are NHWC in the
// handle's arithmetic type (fp32 parity mode / bf16); GroupNorm statistics, FiLM, the conditioning MLP, all parameter
// gradients and the optimiser state are fp32.
//
// The workspace is planned once per shape (StepPlan: a byte offset for every tensor, table and scratch region, no two of them
// overlapping, and the geometry of every launch) and cached in the handle; forward and backward calls launch from that plan, so the
// backward reads the forward's tensors at the offsets the plan names.
#include "../../include/ccn_hip.h"
#include "ccn_train.h"
#include "ccn_arch.h"

#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace ccn;

namespace {

#define THIP(expr)                                                                                       \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) { err = std::string(#expr) + ": " + hipGetErrorString(e_); return false; } \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// a conv of the description (ccn_arch.h) and the training step's operands for it
struct TConvW : ArchConv {
    TConvW(const ArchConv& c) : ArchConv(c) {}
    int BN = 0, Cin_pad = 0, Cout_pad = 0;      // forward operand
    int dkind = KIND_C3S1, dBN = 0, dCin_pad = 0, dCout_pad = 0, dtaps = 9;   // data-gradient operand (roles of Cin / Cout swapped)
    void* wf = nullptr; void* wd = nullptr;
    void* wf_frag = nullptr; void* wd_frag = nullptr;   // 3x3 s1, bf16: fragment-ordered operands for the persistent kernel, else null
    PackDesc pd_f{}, pd_d{}, pf_f{}, pf_d{};             // repack descriptors: plain / fragment, forward / data gradient
};

enum { TF_PACK = 0, TF_COND, TF_CONV_FWD, TF_GN_STATS, TF_PREACT, TF_CONV_DGRAD, TF_WGRAD, TF_WGRAD_REDUCE, TF_BIAS, TF_GN_BWD, TF_SMALL, TF_COUNT };
const char* kTrainFamilies[TF_COUNT] = {"weight_repack", "conditioning_fwd_bwd", "conv_forward", "gn_stats", "gn_silu_prepass", "conv_data_grad", "conv_weight_grad",
                                        "weight_grad_reduce", "bias_grad", "groupnorm_silu_film_bwd", "stem_head_weight_grad"};
struct Mark { int fam; hipEvent_t ev; double flops, bytes; };

// one launch decision of a forward / backward call, kept for the test hook ccn_internal_train_routes (formatted there, not here)
enum { RN_CONV = 0, RN_NORM, RN_GNBWD, RN_WGRAD, RN_COLSUM };
struct RouteNote { int what, kind; const char* name; int v[5]; };

// ---- the step plan: everything that is a function of (configuration, B, H, W, kernel choice) ------------------------------------------
// Built once per shape by Planner, which sees no stream, parameter or workspace pointer; Step (below) launches from it and computes no
// size or geometry of its own.  Every `size_t` that names a tensor or a table is a byte offset from the workspace base.
struct Region { std::string name; size_t off, bytes; };
struct Tensor {                                 // an NHWC activation and the partial sums of the GroupNorm that reads it
    size_t off = 0; int C = 0, H = 0, W = 0;
    size_t part = 0; int n_sp = 0, n_nt = 0, bn = 0;
};
struct ConvPlan { ConvRoute r; ConvArgs a; int fam; double flops; };   // a: what ConvRoute::fill sets, and the operand(s) the route consumes
struct NormPlan {                               // a forward GroupNorm: its tables and the shape's part of the choice between its launch forms
    int G = 0, cpg = 0, HW = 0, slots = 0;
    double count = 0, inv_count = 0, act_bytes = 0;
    size_t ab = 0, st = 0;                      // scale / shift per (sample, channel); (mean, rstd) per (sample, group)
    bool separate_stats = false;                // more than 128 partial-sum slots: statistics as a launch of their own
    bool in_conv = false;                       // side form: the consuming conv forms the statistics itself
};
struct WgPlan { WgArgs a; int kind, nsplit[2], tiles, Cov, Civ; double flops; };   // nsplit: alone / beside the main stream's kernels
struct GnBwdPlan { GnBwdGeom gg; int silu; double bytes; size_t gstat; };
struct BiasPlan { GnBwdGeom gg; int HW, C, rows; bool pairs; };   // pairs: from the GroupNorm backward's per-block channel sums (`rows` of them)
struct LayerPlan {
    // forward.  x: the layer's input; ResBlock: xa = SiLU(GN1(x)), y = FiLM(conv1), ya = SiLU(GN2(y)); o: the layer's output
    Tensor x, xa, y, ya, o;
    size_t skip = 0;                            // ConvTranspose: the skip tensor its epilogue adds
    NormPlan n1, n2;                            // ResBlock; head: n1 = out_norm
    ConvPlan c1{}, c2{};                        // c2: ResBlock only
    bool pre = false;                           // ResBlock: the pre-pass kernel takes its channels (activated tensors are written and kept)
    bool both_pr = false;                       // ... and both convs run on the persistent kernel: the side form may be chosen at run time
    bool head2 = false; size_t head2_scratch = 0;
    // backward.  g: gradient w.r.t. o (head: the caller's d eps); ResBlock: g1 w.r.t. y, g2 w.r.t. x; the others: g2 w.r.t. x
    size_t g = 0, g1 = 0, g2 = 0;
    size_t dskip = 0;                           // stride-2 conv: the gradient that waits at its skip connection
    size_t de = 0, col = 0;                     // head: d eps as NHWC; stem: im2col of the image
    WgPlan w1{}, w2{};
    BiasPlan bias{};
    ConvPlan d1{}, d2{};
    GnBwdPlan gb1{}, gb2{};
};
struct StepPlan {
    int B = 0, H = 0, W = 0; int64_t HW = 0;
    std::vector<Region> regions; size_t total = 0;
    size_t scr_wg = 0, scr_gn = 0, scr_film = 0, scr_col = 0;                       // shared scratch, sized for the largest user
    size_t temb = 0, u0 = 0, t1 = 0, tp = 0, uz = 0, zpv = 0, hv = 0, film = 0;     // conditioning
    size_t dfilm = 0, dh = 0, dt1 = 0, du0 = 0, duz = 0, dh_bytes = 0;
    std::vector<LayerPlan> layers;              // one per arch.layers entry
    std::vector<PackDesc> pack_list;            // one per conv launch, the forward's first
    PackDesc* packs = nullptr; int n_packs = 0, n_packs_fwd = 0;                    // the same on the device
};

}  // namespace

struct ccn_trainer_s {
    ccn_config_t cfg{};
    int elem = 4, G = 8;
    Arch arch;                            // parameters (with the flat layout's offsets), convs, ResBlocks, layer list: build_arch, ccn_arch.h
    std::vector<TConvW> convs;            // one per arch.convs entry
    float* zero_bias = nullptr;
    // captured hipGraphs of one forward / one backward, keyed by every pointer argument (ccn_train_set_graph)
    struct TGraph { std::vector<const void*> key; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; };
    bool use_graph = false;
    hipStream_t cap_stream = nullptr;
    std::vector<TGraph> graphs;
    hipStream_t side = nullptr;           // weight gradients run here, beside the data-gradient chain (nothing downstream reads them)
    hipEvent_t pack_dg_done = nullptr;    // the data-gradient operands' repack, enqueued on `side` by the last forward
    bool pack_dg_pending = false;
    hipEvent_t fwd_fork = nullptr;
    std::vector<hipEvent_t> sync_pool; size_t sync_used = 0;
    LinDesc* lin_descs = nullptr; int n_lin = 0, max_lin_n = 0;
    std::vector<void*> allocs;
    std::map<std::string, StepPlan> shapes;     // shape_key -> the plan of that shape
    // profiling (ccn_train_profile_*): an event before every group of launches; the time up to the next event is the group's
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool; size_t ev_used = 0;
    std::vector<Mark> marks;
    // state of the last forward (checked by backward)
    int fB = 0, fH = 0, fW = 0; void* fws = nullptr;
    // launch decisions of the last forward call and of the backward calls since (a graph replay leaves the captured call's)
    std::vector<RouteNote> route_log;
};

namespace {

bool alloc_dev(ccn_trainer_s* tr, size_t bytes, void** out, std::string& err)
{
    void* p = nullptr;
    THIP(hipMalloc(&p, bytes ? bytes : 4));
    tr->allocs.push_back(p);
    *out = p;
    return true;
}

// operand geometry and device buffers of one convolution (forward and data-gradient operands)
bool setup_conv(ccn_trainer_s* tr, TConvW& w, std::string& err)
{
    const int cke = conv_cin_chunk(tr->cfg.dtype);
    const int fkind = w.kind;
    w.BN = conv_bn_for(w.Cout, fkind);
    w.Cout_pad = (int)align_up(w.Cout, w.BN);
    w.Cin_pad = fkind == KIND_STEM ? cke : (int)align_up(w.Cin, cke);
    const int ftaps = fkind == KIND_CT4 ? 16 : (fkind == KIND_STEM ? 1 : 9);
    if (!alloc_dev(tr, (size_t)ftaps * w.Cout_pad * w.Cin_pad * tr->elem, &w.wf, err)) return false;
    const long long src = (long long)tr->arch.params[w.pw].off;
    switch (fkind) {
        case KIND_CT4: w.pd_f = {src, w.wf, PK_CONVT, w.Cout, w.Cin, 16, w.Cout_pad, w.Cin_pad}; break;
        case KIND_STEM: w.pd_f = {src, w.wf, PK_STEM, w.Cout, w.Cin, 1, w.Cout_pad, w.Cin_pad}; break;
        default: w.pd_f = {src, w.wf, PK_CONV3, w.Cout, w.Cin, 9, w.Cout_pad, w.Cin_pad}; break;
    }
    if (fkind == KIND_STEM) {
        // bf16: the register-weight stem kernel (ccn_stem.hip) instead of the generic one on an im2col tile
        if (stem2_supported(tr->cfg.dtype, w.Cin, w.Cout, tr->G)) {
            if (!alloc_dev(tr, (size_t)w.Cout * 32 * 2, &w.wf_frag, err)) return false;
            w.pf_f = {src, w.wf_frag, PK_FRAG_STEM, w.Cout, w.Cin, 1, w.Cout, 32, (long long)tr->arch.params[w.pb].off};
        }
        return true;                                         // the image needs no gradient
    }
    // data gradient: a convolution from Cout back to Cin
    switch (fkind) {
        case KIND_C3S1: w.dkind = KIND_C3S1; w.dtaps = 9; break;
        case KIND_C3S2: w.dkind = KIND_CT4; w.dtaps = 16; break;
        case KIND_CT4: w.dkind = KIND_C3S2; w.dtaps = 16; break;
        case KIND_HEAD: w.dkind = KIND_STEM; w.dtaps = 1; break;
    }
    w.dBN = conv_bn_for(w.Cin, w.dkind);
    w.dCout_pad = (int)align_up(w.Cin, w.dBN);
    w.dCin_pad = w.dkind == KIND_STEM ? cke : (int)align_up(w.Cout, cke);
    if (!alloc_dev(tr, (size_t)w.dtaps * w.dCout_pad * w.dCin_pad * tr->elem, &w.wd, err)) return false;
    switch (fkind) {
        case KIND_C3S1: w.pd_d = {src, w.wd, PK_DG3S1, w.Cout, w.Cin, 9, w.dCout_pad, w.dCin_pad}; break;
        case KIND_C3S2: w.pd_d = {src, w.wd, PK_DG3S2, w.Cout, w.Cin, 16, w.dCout_pad, w.dCin_pad}; break;
        case KIND_CT4: w.pd_d = {src, w.wd, PK_DGT, w.Cout, w.Cin, 16, w.dCout_pad, w.dCin_pad}; break;
        case KIND_HEAD: w.pd_d = {src, w.wd, PK_HEAD_DG, w.Cout, w.Cin, 1, w.dCout_pad, w.dCin_pad}; break;
    }
    if (fkind == KIND_HEAD && stem2_supported(tr->cfg.dtype, w.Cout, w.Cin, tr->G)) {
        // the head's data gradient is a stem conv (img_ch -> C, taps flipped) on d eps, which arrives as NCHW fp32 like the image
        if (!alloc_dev(tr, (size_t)w.Cin * 32 * 2, &w.wd_frag, err)) return false;
        w.pf_d = {src, w.wd_frag, PK_FRAG_STEM_HEAD_DG, w.Cout, w.Cin, 1, w.Cin, 32, 0};
    }
    if (fkind == KIND_C3S1 && tr->elem == 2) {
        if (w.BN == 128 && w.Cin_pad >= 128) {
            if (!alloc_dev(tr, (size_t)9 * w.Cout_pad * w.Cin_pad * 2, &w.wf_frag, err)) return false;
            w.pf_f = {src, w.wf_frag, PK_FRAG3, w.Cout, w.Cin, 9, w.Cout_pad, w.Cin_pad};
        }
        if (w.dBN == 128 && w.dCin_pad >= 128) {
            if (!alloc_dev(tr, (size_t)9 * w.dCout_pad * w.dCin_pad * 2, &w.wd_frag, err)) return false;
            w.pf_d = {src, w.wd_frag, PK_FRAG3_DG, w.Cout, w.Cin, 9, w.dCout_pad, w.dCin_pad};
        }
    }
    // stride-2 conv / ConvTranspose on the persistent kernel's plane-pass / parity forms (bf16, 128-wide N tiles, >= 2 Cin chunks):
    // the forward operands, and the stride-2 conv's data gradient (a ConvTranspose with the 3x3 kernel zero-padded to 4x4)
    if (tr->elem == 2 && (fkind == KIND_C3S2 || fkind == KIND_CT4) && w.BN == 128 && w.Cin_pad >= 128) {
        const int slots = fkind == KIND_C3S2 ? 10 : 16;
        if (!alloc_dev(tr, (size_t)slots * w.Cout_pad * w.Cin_pad * 2, &w.wf_frag, err)) return false;
        w.pf_f = {src, w.wf_frag, fkind == KIND_C3S2 ? PK_FRAG_S2 : PK_FRAG_CT, w.Cout, w.Cin, slots, w.Cout_pad, w.Cin_pad};
    }
    if (tr->elem == 2 && (fkind == KIND_C3S2 || fkind == KIND_CT4) && w.dBN == 128 && w.dCin_pad >= 128) {
        // (the ConvTranspose's data gradient: a 4x4 stride-2 conv, run as four plane passes of 2x2 taps)
        if (!alloc_dev(tr, (size_t)16 * w.dCout_pad * w.dCin_pad * 2, &w.wd_frag, err)) return false;
        w.pf_d = {src, w.wd_frag, fkind == KIND_C3S2 ? PK_FRAG_CT_DG : PK_FRAG_P4_DG, w.Cout, w.Cin, 16, w.dCout_pad, w.dCin_pad};
    }
    return true;
}

// geometry, taps and split counts of one weight-gradient launch: the planner's (Planner::wgrad) and the test hook's (ccn_internal_wgrad)
WgPlan wgrad_plan(int dtype, int kind, int B, int Hin, int Win, int Cin, int Civ, int silu, int Cout, int Cov)
{
    const ConvGeom g = conv_geom(kind, false, Hin, Win, 4);
    WgPlan w{};
    WgArgs& a = w.a;
    a.silu = silu;
    a.B = B; a.Hin = Hin; a.Win = Win; a.Cin = Cin; a.Hout = g.Hout; a.Wout = g.Wout; a.Cout = Cout;
    a.MH = g.MH; a.MW = g.MW; a.OS = g.OS; a.npar = g.npar; a.ntaps = g.ntaps; a.taps_w = kind == KIND_CT4 ? 16 : (kind == KIND_STEM ? 1 : 9);
    a.n_ty = g.n_ty; a.n_tx = g.n_tx;
    fill_taps(a.tapinfo, kind, false);
    w.kind = kind; w.Cov = Cov; w.Civ = Civ; w.tiles = B * g.n_ty * g.n_tx;
    w.nsplit[0] = wgrad_nsplit(dtype, kind, B, g.MH, g.MW, Cin, Cout, false);
    w.nsplit[1] = wgrad_nsplit(dtype, kind, B, g.MH, g.MW, Cin, Cout, true);
    w.flops = 2.0 * B * g.Hout * g.Wout * (double)Cov * (kind == KIND_CT4 ? 4 : (kind == KIND_STEM ? 1 : 9)) * Civ;
    return w;
}

// ---- planner: one pass over the layer list, forward then backward, that places every region and fixes every launch's geometry ---------
struct Planner {
    const ccn_trainer_s* tr;
    const int B, H, W;
    StepPlan& pl;
    size_t off = 0;

    Planner(const ccn_trainer_s* t, StepPlan& p) : tr(t), B(p.B), H(p.H), W(p.W), pl(p) {}

    size_t take(const std::string& name, size_t bytes)
    {
        off = align_up(off, 256);
        pl.regions.push_back({name, off, bytes});
        off += bytes;
        return off - bytes;
    }
    Tensor tensor(const std::string& name, int C, int h, int w)
    {
        Tensor t; t.C = C; t.H = h; t.W = w; t.off = take(name, (size_t)B * h * w * C * tr->elem);
        return t;
    }
    static void want(size_t& slot, size_t bytes) { if (bytes > slot) slot = bytes; }
    int groups_for(int C) const { return C < tr->G ? C : tr->G; }

    // The training step's policy for conv_route: the stride-2 conv, the ConvTranspose and the 4x4 data-gradient form on the persistent
    // kernel from CCN_TRAIN_PR2_MIN (64) eight-row tiles, no split-K.  `four`: the 4x4 form of KIND_C3S2.
    ConvRoute route(int kind, bool four, const PackDesc& frag, int BN, int K, int Kpad, int N, int Npad, int Hin, int Win, bool gn_ab, bool film, bool res) const
    {
        static const char* pr2_min = diag_env("CCN_TRAIN_PR2_MIN");         // A/B switches
        static const ConvPolicy policy{!diag_env("CCN_TRAIN_NO_PR"), diag_env("CCN_TRAIN_NO_PR_S2CT") ? LONG_MAX : (pr2_min ? atol(pr2_min) : 64), true,
                                       false, false, !diag_env("CCN_TRAIN_NO_STEM2")};
        return conv_route({tr->cfg.dtype, kind, four, BN, K, Kpad, N, Npad, B, Hin, Win, tr->G, frag.dst != nullptr, gn_ab, res, film}, policy);
    }
    // one conv launch on route `r`; `out`: the tensor whose consuming GroupNorm wants the epilogue's partial sums, or null
    ConvPlan conv(int fam, const ConvRoute& r, const PackDesc& plain, const PackDesc& frag, Tensor* out, const std::string& name)
    {
        ConvPlan c{};
        c.r = r; c.fam = fam;
        r.fill(c.a);
        c.a.w = plain.dst; c.a.wfrag = r.uses_frag() ? frag.dst : nullptr;
        pl.pack_list.push_back(r.uses_frag() ? frag : plain);
        if (out) {
            out->part = take(name + ".part", (size_t)B * c.a.G * c.a.nslot * sizeof(float2));
            out->n_sp = r.part_nsp; out->n_nt = r.part_nnt; out->bn = r.part_bn;
        }
        const int kind = r.q.kind;
        c.flops = 2.0 * B * r.g.Hout * r.g.Wout * (double)r.q.Cout * (kind == KIND_CT4 ? 4 : (kind == KIND_STEM ? 1 : r.g.ntaps)) * (kind == KIND_STEM ? 9.0 * r.q.Cin : (double)r.q.Cin);
        return c;
    }
    ConvPlan conv_fwd(const TConvW& w, const Tensor& in, Tensor* out, bool gn_ab, bool film, bool res, const std::string& name)
    {
        return conv(TF_CONV_FWD, route(w.kind, false, w.pf_f, w.BN, w.Cin, w.Cin_pad, w.Cout, w.Cout_pad, in.H, in.W, gn_ab, film, res), w.pd_f, w.pf_f, out, name);
    }
    // dX = conv'(dY): N = the forward conv's Cin
    ConvPlan conv_dgrad(const TConvW& w, int Hdy, int Wdy, bool res)
    {
        pair_rows = 0;                                          // the gradient tensor that follows comes out of a conv: no channel sums
        return conv(TF_CONV_DGRAD, route(w.dkind, w.kind == KIND_CT4, w.pf_d, w.dBN, w.kind == KIND_HEAD ? tr->cfg.img_ch : w.Cout, w.dCin_pad, w.Cin, w.dCout_pad, Hdy, Wdy,
                                         false, false, res), w.pd_d, w.pf_d, nullptr, "");
    }
    // the GroupNorm reading `t`, whose consumer is `c` (null: none that could form the statistics itself)
    NormPlan norm(const Tensor& t, const ConvPlan* c, const std::string& name)
    {
        NormPlan n;
        n.G = groups_for(t.C); n.cpg = t.C / n.G; n.HW = t.H * t.W; n.slots = t.n_sp * t.n_nt;
        n.count = (double)n.cpg * t.H * t.W; n.inv_count = 1.0 / n.count;
        n.act_bytes = 2.0 * B * t.H * t.W * t.C * tr->elem;
        n.ab = take(name + ".ab", (size_t)B * t.C * sizeof(float2));
        n.st = take(name + ".st", (size_t)B * n.G * sizeof(float2));
        // every workgroup of the fused pass redoes the reduction of G x slots partial sums: worth it while that is a few KB (below the
        // 256-pixel level); at 256 px (256+ slots per group, 1024 workgroups per sample) the separate 5-us statistics launch stays
        n.separate_stats = (long)t.n_sp * t.n_nt > 128;
        n.in_conv = c && c->r.gs_ok && conv_in_kernel_stats(tr->cfg.dtype, t.C, n.G, t.n_sp, t.bn);
        return n;
    }
    // kind: the forward conv's family (KIND_STEM = 1x1 on an im2col'ed input); Cin / Cout as stored (multiples of 8), Civ / Cov the
    // channels that exist in the parameter
    WgPlan wgrad(int kind, int Hin, int Win, int Cin, int Civ, int silu, int Cout, int Cov)
    {
        const WgPlan w = wgrad_plan(tr->cfg.dtype, kind, B, Hin, Win, Cin, Civ, silu, Cout, Cov);
        want(pl.scr_wg, (size_t)(w.nsplit[0] > w.nsplit[1] ? w.nsplit[0] : w.nsplit[1]) * w.a.taps_w * Cout * Cin * 4);
        return w;
    }
    // > 0: scr_film holds per-block channel sums of the current gradient tensor (rows = B * blocks); a conv's output has none
    int pair_rows = 0;
    // bias gradient of a conv from its output gradient (C channels, HW pixels)
    BiasPlan bias(int HW, int C)
    {
        BiasPlan b{gn_bwd_geom(tr->cfg.dtype, B, HW, C), HW, C, 0, pair_rows > 0};
        b.rows = b.pairs ? pair_rows : B * b.gg.nblk;
        want(pl.scr_col, (size_t)B * b.gg.nblk * C * 4);
        return b;
    }
    // GroupNorm(+SiLU) backward of the norm reading `x`; without FiLM its apply pass leaves the channel sums of its output
    GnBwdPlan gn_bwd(const Tensor& x, const NormPlan& n, bool silu, bool addend, bool film, const std::string& name)
    {
        GnBwdPlan g{};
        g.gg = gn_bwd_geom(tr->cfg.dtype, B, x.H * x.W, x.C);
        g.silu = silu ? 1 : 0;
        want(pl.scr_gn, (size_t)B * g.gg.nblk * x.C * sizeof(float2));
        want(pl.scr_film, (size_t)B * g.gg.nblk * x.C * sizeof(float2));
        pair_rows = film ? 0 : B * g.gg.nblk;
        g.gstat = take(name + ".gstat", (size_t)B * n.G * sizeof(float2));
        // algorithmic HBM bytes: pass 1 reads x and dA, pass 2 reads them again (+ the residual gradient) and writes dx
        g.bytes = (double)B * x.H * x.W * x.C * tr->elem * (addend ? 6.0 : 5.0);
        return g;
    }

    void forward()
    {
        const int td = tr->cfg.time_dim;
        pl.temb = take("temb", (size_t)B * td * 4); pl.u0 = take("u0", (size_t)B * td * 16); pl.t1 = take("t1", (size_t)B * td * 16);
        pl.tp = take("tp", (size_t)B * td * 4); pl.uz = take("uz", (size_t)B * td * 4); pl.zpv = take("zpv", (size_t)B * td * 4);
        pl.hv = take("h", (size_t)B * td * 4); pl.film = take("film", (size_t)B * tr->arch.F * 4);
        Tensor x; std::vector<Tensor> skips;
        Tensor img; img.C = tr->cfg.img_ch; img.H = H; img.W = W;
        for (size_t li = 0; li < tr->arch.layers.size(); ++li) {
            const ArchLayer& L = tr->arch.layers[li];
            LayerPlan& lp = pl.layers[li];
            const std::string n = L.name + ".";
            lp.x = x;
            switch (L.type) {
                case L_STEM: case L_DOWN: case L_UP: {
                    const Tensor& in = L.type == L_STEM ? img : x;
                    if (L.type == L_DOWN) skips.push_back(x);
                    if (L.type == L_UP) { lp.skip = skips.back().off; skips.pop_back(); }
                    lp.o = tensor(n + "o", tr->convs[L.idx].Cout, L.type == L_DOWN ? in.H / 2 : (L.type == L_UP ? in.H * 2 : in.H),
                                  L.type == L_DOWN ? in.W / 2 : (L.type == L_UP ? in.W * 2 : in.W));
                    lp.c1 = conv_fwd(tr->convs[L.idx], in, &lp.o, false, false, L.type == L_UP, n + "o");
                    break;
                }
                case L_RES: {
                    const ArchRes& r = tr->arch.res[L.idx];
                    const TConvW &c1 = tr->convs[r.c1], &c2 = tr->convs[r.c2];
                    // The activated tensors SiLU(GN(.)) are written once by a pre-pass and kept: the forward conv AND the weight-gradient
                    // kernel then stage plain copies.  Redoing the transform while staging costs both of them VALU issue slots next to
                    // their MFMAs (per pixel tile the weight-gradient kernel spent more cycles in exp/rcp than in MFMAs); the pre-pass is
                    // one HBM-bound read + write per norm.  Layers the pre-pass kernel cannot take keep the fused prologue.
                    static const bool no_pre = diag_env("CCN_TRAIN_NO_PREACT") != nullptr;       // A/B switch
                    lp.pre = !no_pre && r.C / (tr->elem == 2 ? 8 : 4) <= 256;
                    // (a 3x3 s1 conv's route does not depend on whether its input GroupNorm comes as a table, so one route serves the
                    // prologue, the pre-pass and the side form)
                    if (lp.pre) lp.xa = tensor(n + "xa", r.C, x.H, x.W);
                    lp.y = tensor(n + "y", r.C, x.H, x.W);
                    lp.c1 = conv_fwd(c1, x, &lp.y, true, true, false, n + "y");
                    lp.n1 = norm(x, &lp.c1, n + "n1");
                    if (lp.pre) lp.ya = tensor(n + "ya", r.C, x.H, x.W);
                    lp.o = tensor(n + "o", r.C, x.H, x.W);
                    lp.c2 = conv_fwd(c2, lp.y, &lp.o, true, false, true, n + "o");
                    lp.n2 = norm(lp.y, &lp.c2, n + "n2");
                    lp.both_pr = lp.c1.r.pr && lp.c2.r.pr;
                    break;
                }
                case L_HEAD: {
                    const TConvW& hd = tr->convs[L.idx];
                    lp.n1 = norm(x, nullptr, "out_norm");
                    // bf16: the inference plan's head kernels (out_norm folded into per-sample weights, nine taps in the N dimension) instead
                    // of the generic kernel: 20 instead of 45 us
                    static const bool no_head2 = diag_env("CCN_TRAIN_NO_HEAD2") != nullptr;      // A/B switch
                    lp.head2 = !no_head2 && head2_supported(tr->cfg.dtype, hd.Cin, hd.Cout, tr->G) && (double)B * H * W * x.C * 2 < 2.0e9;
                    if (lp.head2) {
                        lp.head2_scratch = take(n + "head2", head2_scratch_bytes(B, x.C));
                        lp.c1.a.B = B; lp.c1.a.Hin = H; lp.c1.a.Win = W; lp.c1.a.Cin = hd.Cin; lp.c1.a.Cout = hd.Cout; lp.c1.a.Hout = H; lp.c1.a.Wout = W;
                        lp.c1.fam = TF_CONV_FWD; lp.c1.flops = 2.0 * B * H * W * (double)hd.Cout * 9.0 * hd.Cin;
                    } else lp.c1 = conv_fwd(hd, x, nullptr, true, false, false, "");
                    break;
                }
            }
            x = lp.o;
        }
    }

    void backward()
    {
        const ccn_config_t& c = tr->cfg;
        const int td = c.time_dim;
        pl.dh_bytes = (size_t)B * td * 4;
        pl.dfilm = take("dfilm", (size_t)B * tr->arch.F * 4); pl.dh = take("dh", pl.dh_bytes);
        pl.dt1 = take("dt1", (size_t)B * td * 16); pl.du0 = take("du0", (size_t)B * td * 16); pl.duz = take("duz", (size_t)B * td * 4);
        Tensor g;                                              // gradient w.r.t. the current tensor
        std::vector<size_t> dskip;                             // gradients waiting at the skip connections (pushed by the up path)
        for (int li = (int)tr->arch.layers.size() - 1; li >= 0; --li) {
            const ArchLayer& L = tr->arch.layers[li];
            LayerPlan& lp = pl.layers[li];
            const std::string n = L.name + ".";
            const Tensor& x = lp.x;
            lp.g = g.off;
            switch (L.type) {
                case L_HEAD: {
                    // out.weight: the generic kernel on d eps as an NHWC tensor (channels padded to 8), A = out_norm(u) without SiLU
                    lp.de = take(n + "de", (size_t)B * H * W * 8 * tr->elem);
                    lp.w1 = wgrad(KIND_C3S1, H, W, x.C, x.C, 0, 8, c.img_ch);
                    g = tensor(n + "g", x.C, H, W);
                    lp.d1 = conv_dgrad(tr->convs[L.idx], H, W, false);
                    lp.gb1 = gn_bwd(x, lp.n1, false, false, false, "out_norm");
                    break;
                }
                case L_UP: case L_DOWN: {
                    const TConvW& w = tr->convs[L.idx];
                    if (L.type == L_UP) dskip.push_back(g.off);                     // x = convT(xin) + skip
                    lp.w1 = wgrad(w.kind, x.H, x.W, w.Cin, w.Cin, 1, w.Cout, w.Cout);
                    lp.bias = bias(g.H * g.W, w.Cout);
                    if (L.type == L_DOWN) { lp.dskip = dskip.back(); dskip.pop_back(); }
                    lp.d1 = conv_dgrad(w, g.H, g.W, L.type == L_DOWN);
                    g = tensor(n + "g", x.C, x.H, x.W);
                    break;
                }
                case L_RES: {
                    const ArchRes& r = tr->arch.res[L.idx];
                    const TConvW &c1 = tr->convs[r.c1], &c2 = tr->convs[r.c2];
                    // out = x + conv2(A2), A2 = silu(gn2(F)), F = film(conv1(A1)), A1 = silu(gn1(x))
                    lp.w2 = wgrad(c2.kind, x.H, x.W, c2.Cin, c2.Cin, 1, c2.Cout, c2.Cout);
                    lp.bias = bias(g.H * g.W, c2.Cout);
                    lp.g1 = take(n + "g1", (size_t)B * g.H * g.W * r.C * tr->elem);
                    lp.d2 = conv_dgrad(c2, g.H, g.W, false);
                    lp.gb2 = gn_bwd(lp.y, lp.n2, true, false, true, n + "n2");
                    // (conv1's bias gradient comes out of the FiLM finalize of that pass)
                    lp.w1 = wgrad(c1.kind, x.H, x.W, c1.Cin, c1.Cin, 1, c1.Cout, c1.Cout);
                    want(pl.scr_col, (size_t)B * gn_bwd_geom(c.dtype, B, g.H * g.W, c1.Cout).nblk * c1.Cout * 4);
                    lp.g2 = take(n + "g2", (size_t)B * g.H * g.W * r.C * tr->elem);
                    lp.d1 = conv_dgrad(c1, g.H, g.W, false);
                    lp.gb1 = gn_bwd(x, lp.n1, true, true, false, n + "n1");
                    g.off = lp.g2;
                    break;
                }
                case L_STEM: {
                    const TConvW& w = tr->convs[L.idx];
                    // in_conv.weight: 1x1 weight gradient against the im2col of the image (27 of 32 columns)
                    lp.bias = bias(H * W, w.Cout);
                    lp.col = take(n + "col", (size_t)B * H * W * 32 * tr->elem);
                    lp.w1 = wgrad(KIND_STEM, H, W, 32, c.img_ch * 9, 0, w.Cout, w.Cout);
                    break;
                }
            }
            if (L.type != L_RES && L.type != L_STEM) lp.g2 = g.off;
        }
    }

    void run()
    {
        pl.layers.assign(tr->arch.layers.size(), LayerPlan{});
        pl.HW = (int64_t)H * W;
        forward();
        pl.n_packs_fwd = (int)pl.pack_list.size();               // the forward convs' operands come first in the list
        backward();
        pl.scr_wg = take("scr_wg", pl.scr_wg); pl.scr_gn = take("scr_gn", pl.scr_gn);
        pl.scr_film = take("scr_film", pl.scr_film); pl.scr_col = take("scr_col", pl.scr_col);
        pl.total = align_up(off, 256) + 5 * 256;
    }
};

// ---- launcher: one forward or backward call, enqueued from the plan -----------------------------------------------------------------------
// Adds pointers (workspace base + planned offset, parameters, gradients), the stream, film_bstride and eps_out; the choices it makes are
// the run-time ones: side stream or not, side or pre-pass form of a ResBlock, the pack split, the bucket callback.
struct Step {
    ccn_trainer_s* tr;
    const StepPlan& pl;
    char* ws;
    hipStream_t st;
    const float* P; float* Gd;            // flat parameters / gradients
    const int B;
    std::string err;
    hipStream_t wg_stream = nullptr;      // where the weight gradients go: the side stream after fork_side, else `st`
    // bucketed backward: cb(user, lo, hi) as soon as the gradients of flat range [lo, hi) are complete in stream order on `st`
    ccn_grad_ready_cb bucket_cb = nullptr; void* bucket_user = nullptr; long long bucket_floats = 0, hi_pending = 0;
    bool fwd_side_used = false;

    Step(ccn_trainer_s* t, const StepPlan& p, void* w, hipStream_t s, const float* par_, float* g)
        : tr(t), pl(p), ws((char*)w), st(s), P(par_), Gd(g), B(p.B) {}

    template <typename T = void> T* at(size_t off) const { return (T*)(ws + off); }
    const float* par(int i) const { return P + tr->arch.params[i].off; }
    float* grad(int i) const { return Gd + tr->arch.params[i].off; }
    float* grad_or_null(int i) const { return Gd ? grad(i) : nullptr; }
    bool ok(hipError_t e, const char* what) { if (e != hipSuccess) { err = std::string(what) + ": " + hipGetErrorString(e); return false; } return true; }
    bool ok(hipError_t e, const ArchLin& l) { const std::string& n = tr->arch.params[l.pw].name; return ok(e, n.substr(0, n.rfind('.')).c_str()); }

    // profiling: the launches that follow belong to family `fam` (flops: their algorithmic work); fam < 0 closes the sequence
    void mark(int fam, double flops = 0.0, double bytes = 0.0)
    {
        if (!tr->profiling) return;
        if (tr->ev_used == tr->ev_pool.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return; tr->ev_pool.push_back(e); }
        hipEvent_t e = tr->ev_pool[tr->ev_used++];
        if (hipEventRecord(e, st) != hipSuccess) return;
        tr->marks.push_back({fam, e, flops, bytes});
    }
    void note(int what, int kind, const char* name, int v0 = 0, int v1 = 0, int v2 = 0, int v3 = 0, int v4 = 0)
    {
        tr->route_log.push_back({what, kind, name, {v0, v1, v2, v3, v4}});
    }

    // ---- streams ---------------------------------------------------------------------------------------------------------------------------
    // `to` continues from this point of `from`: an event (`own`, else the next of the pool, which every backward call and every forward
    // call that returns eps starts over) recorded on `from` and waited for on `to`
    enum { ORD_OK = 0, ORD_NO_EVENT, ORD_FAILED };
    int order(hipStream_t from, hipStream_t to, hipEvent_t own = nullptr)
    {
        hipEvent_t e = own;
        if (!e) {
            if (tr->sync_used == tr->sync_pool.size()) {
                if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return ORD_NO_EVENT;
                tr->sync_pool.push_back(e);
            }
            e = tr->sync_pool[tr->sync_used++];
        }
        return hipEventRecord(e, from) == hipSuccess && hipStreamWaitEvent(to, e, 0) == hipSuccess ? ORD_OK : ORD_FAILED;
    }
    bool side_active() const
    {
        static const bool off_ = diag_env("CCN_TRAIN_NO_SIDE_STREAM") != nullptr;
        return !off_ && !tr->profiling && tr->side != nullptr;
    }
    // fork: the side stream continues from this point of the main stream; join: the main stream waits for everything on the side
    bool fork_side()
    {
        wg_stream = st;
        if (!side_active()) return true;
        const int o = order(st, tr->side);
        if (o == ORD_NO_EVENT) return true;
        if (o == ORD_FAILED) { err = "stream fork failed"; return false; }
        wg_stream = tr->side;
        return true;
    }
    bool join_side()
    {
        if (!tr->side || tr->sync_used == 0) return true;
        const int o = order(tr->side, st);
        if (o != ORD_OK) { err = o == ORD_NO_EVENT ? "event create failed" : "stream join failed"; return false; }
        return true;
    }

    // ---- forward pieces --------------------------------------------------------------------------------------------------
    // input GroupNorm formed inside the persistent kernel from the producer's partial sums (its GS = 1; only where n.in_conv)
    bool run_conv(const ConvPlan& c, const float* bias, const void* in, void* out, float2* part, const float2* gn_ab, const float* film, const void* res,
                  float* eps_out, const Tensor* gs_x = nullptr, const NormPlan* gs_n = nullptr, const ArchNorm* gs_p = nullptr)
    {
        ConvArgs a = c.a;
        a.in = in; a.bias = bias; a.out = out; a.part = part;
        a.gn_ab = gn_ab; a.film = film; a.res = res;
        if (gs_x) {
            a.gn_ab = nullptr;
            a.gs_part = at<float2>(gs_x->part); a.gs_gamma = par(gs_p->pg); a.gs_beta = par(gs_p->pb); a.gs_inv_count = gs_n->inv_count;
            a.gs_nsp = gs_x->n_sp; a.gs_nnt = gs_x->n_nt; a.gs_bn = gs_x->bn; a.gs_cpg = gs_n->cpg;
        }
        a.film_bstride = tr->arch.F;
        a.eps_out = eps_out;
        // (measured and dropped: capping the data-gradient convs' persistent grid to the CUs the side stream's weight-gradient kernel
        // leaves free -- 192 / 160 / 128 workgroups: 652-658 vs 663 images/s uncapped; docs/EXPERIMENTS.md R3.12)
        const ConvQuery& q = c.r.q;
        mark(c.fam, c.flops);
        note(RN_CONV, q.kind, conv_kernel_name(conv_kernel_for(q.kind, q.BN, a)), c.fam == TF_CONV_FWD ? 1 : 0, a.th, q.BN, a.n_nt, q.four ? 1 : 0);
        return ok(launch_conv(tr->cfg.dtype, q.kind, q.BN, a, st), "conv");
    }
    bool conv_fwd(const TConvW& w, const ConvPlan& c, const void* in, const Tensor& out, const float2* gn_ab, const float* film, const void* res)
    {
        return run_conv(c, par(w.pb), in, at(out.off), at<float2>(out.part), gn_ab, film, res, nullptr);
    }
    // ---- forward ResBlock conv with its GroupNorm + SiLU, side-stream form (bf16, plain stream launches) --------------------------------
    // The conv transforms its raw input in its producer waves (the inference kernels' prologue: statistics formed in-kernel from the
    // partial sums where they are few, else from the table of a 5-us statistics launch), so the pass that WRITES the activated tensor
    // -- which only the weight-gradient kernel reads, in the backward pass -- leaves the forward's critical path: it runs on the side
    // stream beside the convs (HBM-bound next to MFMA-bound).  The backward pass waits for pack_dg_done, recorded after the last of them.
    bool side_pre_ok() const
    {
        static const bool off_ = diag_env("CCN_TRAIN_NO_SIDE_PRE") != nullptr;       // A/B switch
        return !off_ && side_active() && !tr->use_graph && tr->pack_dg_done && tr->elem == 2;
    }
    bool fork_fwd_side()
    {
        if (order(st, tr->side) != ORD_OK) { err = "stream fork failed"; return false; }
        fwd_side_used = true;
        return true;
    }
    bool norm_conv_fwd_side(const Tensor& x, const ArchNorm& an, const NormPlan& n, const TConvW& w, const ConvPlan& c, const Tensor& xa, const Tensor& y,
                            const float* film_r, const void* res)
    {
        const int dt = tr->cfg.dtype, HW = n.HW;
        float2 *ab = at<float2>(n.ab), *stats = at<float2>(n.st), *part = at<float2>(x.part);
        if (n.in_conv) {
            // statistics in the conv itself; the side stream's pass writes the activated tensor AND the tables the backward pass reads
            if (!fork_fwd_side()) return false;
            note(RN_NORM, 0, "side-fused", n.slots);
            if (!ok(launch_gn_act_fused(dt, at(x.off), at(xa.off), B, HW, x.C, part, n.G, x.n_sp, x.n_nt, x.bn, n.cpg, n.count, par(an.pg), par(an.pb), 1e-5f, tr->side, ab, stats),
                    "gn_act_fused")) return false;
            return run_conv(c, par(w.pb), at(x.off), at(y.off), at<float2>(y.part), nullptr, film_r, res, nullptr, &x, &n, &an);
        }
        note(RN_NORM, 0, "side-stats+act", n.slots);
        if (!ok(launch_gn_stats(part, B, n.G, x.n_sp, x.n_nt, x.bn, n.cpg, x.C, n.count, par(an.pg), par(an.pb), 1e-5f, ab, stats, st), "gn_stats")) return false;
        if (!fork_fwd_side()) return false;
        if (!ok(launch_gn_act(dt, at(x.off), ab, at(xa.off), B, HW, x.C, tr->side), "gn_act")) return false;
        return run_conv(c, par(w.pb), at(x.off), at(y.off), at<float2>(y.part), ab, film_r, res, nullptr);
    }
    // The GroupNorm reading `t` on the main stream.  With `out`: statistics AND the pre-activated tensor SiLU(GN(t)) in one launch (round 3:
    // 29 gn_stats launches of a step gone) -- every workgroup of the pass reduces the producer's partial sums itself, the first one of
    // each sample also writes the scale / shift table and (mean, rstd) for the backward pass -- or, with many slots, as two.  Without:
    // the tables only, for the consuming conv's prologue.
    bool norm_fwd(const Tensor& t, const ArchNorm& an, const NormPlan& n, const Tensor* out)
    {
        const int dt = tr->cfg.dtype, HW = n.HW;
        float2 *ab = at<float2>(n.ab), *stats = at<float2>(n.st), *part = at<float2>(t.part);
        if (out && !n.separate_stats) {
            note(RN_NORM, 0, "fused", n.slots);
            mark(TF_PREACT, 0.0, n.act_bytes);
            return ok(launch_gn_act_fused(dt, at(t.off), at(out->off), B, HW, t.C, part, n.G, t.n_sp, t.n_nt, t.bn, n.cpg, n.count, par(an.pg), par(an.pb), 1e-5f, st, ab, stats),
                      "gn_act_fused");
        }
        note(RN_NORM, 0, out ? "stats+act" : "prologue", n.slots);
        mark(TF_GN_STATS);
        if (!ok(launch_gn_stats(part, B, n.G, t.n_sp, t.n_nt, t.bn, n.cpg, t.C, n.count, par(an.pg), par(an.pb), 1e-5f, ab, stats, st), "gn_stats")) return false;
        if (!out) return true;
        mark(TF_PREACT, 0.0, n.act_bytes);
        return ok(launch_gn_act(dt, at(t.off), ab, at(out->off), B, HW, t.C, st), "gn_act");
    }

    bool conditioning(const float* z, const int64_t* t)
    {
        const ccn_config_t& c = tr->cfg;
        const Arch& A = tr->arch;
        const int td = c.time_dim;
        float *temb = at<float>(pl.temb), *t1 = at<float>(pl.t1), *tp = at<float>(pl.tp), *zpv = at<float>(pl.zpv), *hv = at<float>(pl.hv);
        mark(TF_COND);
        if (!ok(launch_temb_i64(t, temb, B, td, st), "temb")) return false;
        if (!ok(launch_tlinear_fwd(temb, td, par(A.tp0.pw), par(A.tp0.pb), t1, 4 * td, at<float>(pl.u0), B, td, 4 * td, 1, st), A.tp0)) return false;
        if (!ok(launch_tlinear_fwd(t1, 4 * td, par(A.tp2.pw), par(A.tp2.pb), tp, td, nullptr, B, 4 * td, td, 0, st), A.tp2)) return false;
        if (!ok(launch_tlinear_fwd(z, c.z_dim, par(A.zp.pw), par(A.zp.pb), zpv, td, at<float>(pl.uz), B, c.z_dim, td, 1, st), A.zp)) return false;
        if (!ok(launch_add2(hv, tp, zpv, (int64_t)B * td, st), "h")) return false;
        return ok(launch_film_group_fwd(P, tr->lin_descs, tr->n_lin, tr->max_lin_n, hv, at<float>(pl.film), B, td, A.F, st), "film");
    }

    bool forward(const float* x_t, const float* z, const int64_t* t, float* eps)
    {
        tr->route_log.clear();
        tr->sync_used = 0;                                       // (fork events of this call; a wait keeps the record it saw when it was enqueued)
        mark(TF_PACK);
        // The forward convs' operands now, on this stream; the data-gradient convs' operands (the other half of the 0.18 ms repack)
        // on the side stream beside the forward pass -- the backward pass waits for them (pack_dg_done).  One launch under a graph
        // capture (the side branch would have to rejoin inside the forward's graph) and while profiling.
        static const bool no_split = diag_env("CCN_TRAIN_NO_PACK_SPLIT") != nullptr;     // A/B switch
        const bool split = !no_split && side_active() && tr->pack_dg_done && !tr->use_graph && pl.n_packs_fwd > 0 && pl.n_packs_fwd < pl.n_packs;
        if (!ok(launch_pack_group(tr->cfg.dtype, P, pl.packs, split ? pl.n_packs_fwd : pl.n_packs, st), "pack")) return false;
        tr->pack_dg_pending = false;
        if (split) {
            // (the forward call's own fork event: the pool starts over with every backward call, after this event has done its work)
            if (!tr->fwd_fork && hipEventCreateWithFlags(&tr->fwd_fork, hipEventDisableTiming) != hipSuccess) tr->fwd_fork = nullptr;
            if (!tr->fwd_fork || order(st, tr->side, tr->fwd_fork) != ORD_OK) { err = "stream fork failed"; return false; }
            if (!ok(launch_pack_group(tr->cfg.dtype, P, pl.packs + pl.n_packs_fwd, pl.n_packs - pl.n_packs_fwd, tr->side), "pack")) return false;
            if (hipEventRecord(tr->pack_dg_done, tr->side) != hipSuccess) { err = "event record failed"; return false; }
            tr->pack_dg_pending = true;
        }
        if (!conditioning(z, t)) return false;
        const float* film = at<float>(pl.film);
        for (size_t li = 0; li < tr->arch.layers.size(); ++li) {
            const ArchLayer& L = tr->arch.layers[li];
            const LayerPlan& lp = pl.layers[li];
            switch (L.type) {
                case L_STEM: case L_DOWN: case L_UP:             // one conv: of the image; into the next level; back up, plus the skip
                    if (!conv_fwd(tr->convs[L.idx], lp.c1, L.type == L_STEM ? (const void*)x_t : at(lp.x.off), lp.o, nullptr, nullptr,
                                  L.type == L_UP ? at(lp.skip) : nullptr)) return false;
                    break;
                case L_RES: {
                    const ArchRes& r = tr->arch.res[L.idx];
                    const TConvW &c1 = tr->convs[r.c1], &c2 = tr->convs[r.c2];
                    const float* film_r = film + r.film_off;
                    // Side form where both convs run on the persistent kernel (their input GroupNorm in the prologue either way), over the
                    // same planned tensors and tables as the pre-pass form
                    if (lp.pre && lp.both_pr && side_pre_ok()) {
                        if (!norm_conv_fwd_side(lp.x, r.n1, lp.n1, c1, lp.c1, lp.xa, lp.y, film_r, nullptr)) return false;
                        if (!norm_conv_fwd_side(lp.y, r.n2, lp.n2, c2, lp.c2, lp.ya, lp.o, nullptr, at(lp.x.off))) return false;
                        break;
                    }
                    if (!norm_fwd(lp.x, r.n1, lp.n1, lp.pre ? &lp.xa : nullptr)) return false;
                    if (!conv_fwd(c1, lp.c1, at(lp.pre ? lp.xa.off : lp.x.off), lp.y, lp.pre ? nullptr : at<float2>(lp.n1.ab), film_r, nullptr)) return false;
                    if (!norm_fwd(lp.y, r.n2, lp.n2, lp.pre ? &lp.ya : nullptr)) return false;
                    if (!conv_fwd(c2, lp.c2, at(lp.pre ? lp.ya.off : lp.y.off), lp.o, lp.pre ? nullptr : at<float2>(lp.n2.ab), nullptr, at(lp.x.off))) return false;
                    break;
                }
                case L_HEAD: {
                    const TConvW& hd = tr->convs[L.idx];
                    if (!norm_fwd(lp.x, tr->arch.out_norm, lp.n1, nullptr)) return false;
                    if (lp.head2) {
                        ConvArgs a = lp.c1.a;
                        a.in = at(lp.x.off); a.bias = par(hd.pb); a.eps_out = eps;
                        mark(lp.c1.fam, lp.c1.flops);
                        note(RN_CONV, KIND_HEAD, "head2", 1);
                        if (!ok(launch_head2(a, at<float2>(lp.n1.ab), par(hd.pw), at(lp.head2_scratch), 0, st), "head")) return false;
                    } else if (!run_conv(lp.c1, par(hd.pb), at(lp.x.off), nullptr, nullptr, at<float2>(lp.n1.ab), nullptr, nullptr, eps)) return false;
                    break;
                }
            }
        }
        if (fwd_side_used || tr->pack_dg_pending) {
            // Everything this forward put on the side stream -- the data-gradient operands' repack (reads the parameters), the activated-
            // tensor passes (write into the workspace) -- is joined HERE, on the caller's stream: the side work ended long before the
            // last convs of the main chain do, so the wait is free, and whatever the caller does next with the parameters or the
            // workspace (an optimizer step without a backward pass, freeing the workspace) is ordered behind it.
            if (order(tr->side, st, tr->pack_dg_done) != ORD_OK) { err = "stream join failed"; return false; }
            tr->pack_dg_pending = false;
        }
        return true;
    }

    // ---- backward pieces ---------------------------------------------------------------------------------------------------
    // dW of a conv from A (`gn_ab`: act(GN(x)) redone on the fly) and dY; weight gradients run on the side stream where there is one
    bool wgrad(const WgPlan& w, const void* x, const float2* gn_ab, const void* dy, float* gdst)
    {
        WgArgs a = w.a;
        float* scr_wg = at<float>(pl.scr_wg);
        a.x = x; a.gn_ab = gn_ab; a.dy = dy; a.part = scr_wg;
        a.nsplit = w.nsplit[side_active() ? 1 : 0];
        if (!fork_side()) return false;
        mark(TF_WGRAD, w.flops);
        note(RN_WGRAD, w.kind, "", a.nsplit, w.tiles, a.Cin, a.Cout);
        if (!ok(launch_wgrad(tr->cfg.dtype, w.kind, a, wg_stream), "wgrad")) return false;
        mark(TF_WGRAD_REDUCE);
        return ok(launch_wgrad_reduce(scr_wg, a.nsplit, a.taps_w, a.Cout, a.Cin, w.Cov, w.Civ, w.kind == KIND_CT4 ? 1 : 0, gdst, wg_stream), "wgrad_reduce");
    }
    // db of a conv: from the GroupNorm backward's pairs where its output gradient came out of one, else launch_colsum on that gradient
    bool bias_grad(const BiasPlan& b, const void* dy, float* gdst, const char* what)
    {
        mark(TF_BIAS);
        note(RN_COLSUM, 0, b.pairs ? "pairs" : "dy", b.rows, colsum_finalize_ygrid(b.rows));
        if (b.pairs) return ok(launch_colsum_from_pairs(at<float2>(pl.scr_film), b.rows, b.C, gdst, st), what);
        return ok(launch_colsum(tr->cfg.dtype, dy, at<float>(pl.scr_col), gdst, B, b.HW, b.C, st), what);
    }
    bool conv_dgrad(const ConvPlan& c, const void* dy, void* dx, const void* res)
    {
        return run_conv(c, tr->zero_bias, dy, dx, nullptr, nullptr, nullptr, res, nullptr);
    }
    // GroupNorm(+SiLU) backward of the norm reading tensor `x`: dA -> out (may alias dA); film_off >= 0: the FiLM behind the norm
    bool gn_bwd(const Tensor& x, const ArchNorm& an, const NormPlan& n, const GnBwdPlan& g, const void* dA, void* out, const void* addend, int film_off,
                float* film_bias = nullptr)
    {
        const int dt = tr->cfg.dtype, HW = n.HW;
        const float2 *ab = at<float2>(n.ab), *stats = at<float2>(n.st);
        float2 *scr_gn = at<float2>(pl.scr_gn), *scr_film = at<float2>(pl.scr_film), *gstat = at<float2>(g.gstat);
        const float* film_r = film_off >= 0 ? at<float>(pl.film) + film_off : nullptr;
        mark(TF_GN_BWD, 0.0, g.bytes);
        note(RN_GNBWD, 0, "", x.C, HW, g.gg.ppb / g.gg.pstep, g.gg.nblk, HW % g.gg.ppb);
        // (round 3: the three passes as ONE launch with one 1024-thread workgroup per (sample, group) for the levels below 256 px was
        // built, parity-green, and 0.95 ms SLOWER per step (2.47 vs 1.53 ms for the family): a group's channels are 32-128 contiguous
        // bytes per pixel, so 32 workgroups pull uncoalesced 32-byte segments at a few tens of GB/s each; docs/EXPERIMENTS.md R3.5)
        if (!ok(launch_gn_bwd_reduce(dt, at(x.off), dA, ab, stats, scr_gn, B, HW, x.C, n.cpg, n.G, g.silu, st), "gn_bwd_reduce")) return false;
        if (!ok(launch_gn_bwd_finalize(scr_gn, g.gg.nblk, B, x.C, n.cpg, n.G, n.count, par(an.pg), gstat, grad(an.pg), grad(an.pb), st), "gn_bwd_finalize")) return false;
        if (!ok(launch_gn_bwd_apply(dt, at(x.off), dA, ab, stats, gstat, addend, out, film_r, tr->arch.F, scr_film, B, HW, x.C, n.cpg, n.G, g.silu, st), "gn_bwd_apply"))
            return false;
        if (film_r) return ok(launch_film_bwd_finalize(scr_film, g.gg.nblk, film_r, tr->arch.F, at<float>(pl.dfilm) + film_off, film_bias, B, x.C, st), "film_bwd");
        return true;
    }
    bool flush_bucket(long long lo, bool force)
    {
        if (!bucket_cb) return true;
        if (!force && hi_pending - lo < bucket_floats) return true;
        if (lo >= hi_pending) return true;
        if (!join_side()) return false;
        bucket_cb(bucket_user, lo, hi_pending);
        hi_pending = lo;
        return true;
    }
    bool lin_bwd(const ArchLin& l, const float* dy, int lddy, const float* x, int ldx, float* dx, int lddx, int accumulate)
    {
        if (!ok(launch_tlinear_dw(dy, lddy, x, ldx, grad(l.pw), grad(l.pb), B, l.K, l.N, st), "linear_dw")) return false;
        if (dx) return ok(launch_tlinear_dx(dy, lddy, par(l.pw), dx, lddx, B, l.K, l.N, accumulate, st), "linear_dx");
        return true;
    }

    bool backward(const float* x_t, const float* z, const float* d_eps)
    {
        const ccn_config_t& c = tr->cfg;
        const int td = c.time_dim, dt = c.dtype, H = pl.H, W = pl.W;
        float *dfilm = at<float>(pl.dfilm), *dh = at<float>(pl.dh), *dt1 = at<float>(pl.dt1), *du0 = at<float>(pl.du0), *duz = at<float>(pl.duz);
        float* hv = at<float>(pl.hv);
        tr->sync_used = 0;
        hi_pending = (long long)tr->arch.total;
        if (tr->pack_dg_pending) {                              // the data-gradient operands repacked beside the forward pass
            if (hipStreamWaitEvent(st, tr->pack_dg_done, 0) != hipSuccess) { err = "stream wait failed"; return false; }
            tr->pack_dg_pending = false;
        }
        if (bucket_cb && hipMemsetAsync(dh, 0, pl.dh_bytes, st) != hipSuccess) { err = "hipMemsetAsync failed"; return false; }
        for (int li = (int)tr->arch.layers.size() - 1; li >= 0; --li) {
            const ArchLayer& L = tr->arch.layers[li];
            const LayerPlan& lp = pl.layers[li];
            switch (L.type) {
                case L_HEAD: {
                    const TConvW& w = tr->convs[L.idx];
                    // out.weight: the generic kernel on d eps as an NHWC tensor (channels padded to 8), A = out_norm(u) without SiLU
                    mark(TF_SMALL);
                    if (!ok(launch_nchw_to_nhwc_pad(dt, d_eps, at(lp.de), B, c.img_ch, 8, pl.HW, st), "head_deps_layout")) return false;
                    if (!ok(launch_nchw_chansum(d_eps, grad(w.pb), B, c.img_ch, pl.HW, st), "head_bias")) return false;
                    if (!wgrad(lp.w1, at(lp.x.off), at<float2>(lp.n1.ab), at(lp.de), grad_or_null(w.pw))) return false;
                    if (!conv_dgrad(lp.d1, d_eps, at(lp.g2), nullptr)) return false;
                    if (!gn_bwd(lp.x, tr->arch.out_norm, lp.n1, lp.gb1, at(lp.g2), at(lp.g2), nullptr, -1)) return false;
                    break;
                }
                case L_UP: case L_DOWN: {
                    const TConvW& w = tr->convs[L.idx];
                    if (!wgrad(lp.w1, at(lp.x.off), nullptr, at(lp.g), grad_or_null(w.pw))) return false;
                    if (!bias_grad(lp.bias, at(lp.g), grad(w.pb), "bias_grad")) return false;
                    if (!conv_dgrad(lp.d1, at(lp.g), at(lp.g2), L.type == L_DOWN ? at(lp.dskip) : nullptr)) return false;
                    break;
                }
                case L_RES: {
                    const ArchRes& r = tr->arch.res[L.idx];
                    const TConvW &c1 = tr->convs[r.c1], &c2 = tr->convs[r.c2];
                    // out = x + conv2(A2), A2 = silu(gn2(F)), F = film(conv1(A1)), A1 = silu(gn1(x))
                    if (!wgrad(lp.w2, at(lp.pre ? lp.ya.off : lp.y.off), lp.pre ? nullptr : at<float2>(lp.n2.ab), at(lp.g), grad_or_null(c2.pw))) return false;
                    if (!bias_grad(lp.bias, at(lp.g), grad(c2.pb), "bias_grad")) return false;
                    if (!conv_dgrad(lp.d2, at(lp.g), at(lp.g1), nullptr)) return false;
                    if (!gn_bwd(lp.y, r.n2, lp.n2, lp.gb2, at(lp.g1), at(lp.g1), nullptr, r.film_off, grad(c1.pb))) return false;
                    if (bucket_cb) {
                        // bucketed mode: this block's FiLM linears now (side stream) instead of one grouped launch at the end, so that the
                        // block's whole parameter range is complete when its bucket is handed out
                        if (!fork_side()) return false;
                        const LinDesc* d2 = tr->lin_descs + 2 * L.idx;
                        if (!ok(launch_film_group_dw(Gd, d2, 2, r.C, dfilm, hv, B, td, tr->arch.F, wg_stream), "film_dw")) return false;
                        if (!ok(launch_film_group_dx(P, d2, 2, dfilm, dh, B, td, tr->arch.F, wg_stream), "film_dx")) return false;
                    }
                    if (!wgrad(lp.w1, at(lp.pre ? lp.xa.off : lp.x.off), lp.pre ? nullptr : at<float2>(lp.n1.ab), at(lp.g1), grad_or_null(c1.pw))) return false;
                    if (!conv_dgrad(lp.d1, at(lp.g1), at(lp.g2), nullptr)) return false;
                    if (!gn_bwd(lp.x, r.n1, lp.n1, lp.gb1, at(lp.g2), at(lp.g2), at(lp.g), -1)) return false;
                    break;
                }
                case L_STEM: {
                    const TConvW& w = tr->convs[L.idx];
                    // in_conv.weight: 1x1 weight gradient against the im2col of the image (27 of 32 columns)
                    mark(TF_SMALL);
                    if (!ok(launch_im2col27(dt, x_t, at(lp.col), B, c.img_ch, H, W, st), "stem_im2col")) return false;
                    if (!bias_grad(lp.bias, at(lp.g), grad(w.pb), "stem_bias")) return false;
                    if (!wgrad(lp.w1, at(lp.col), nullptr, at(lp.g), grad_or_null(w.pw))) return false;
                    break;
                }
            }
            if (bucket_cb) {
                // first parameter of this layer: everything from its offset up is complete
                const int first = L.type == L_HEAD ? tr->arch.out_norm.pg : (L.type == L_RES ? tr->arch.res[L.idx].n1.pg : tr->convs[L.idx].pw);
                if (L.type != L_STEM && !flush_bucket((long long)tr->arch.params[first].off, false)) return false;
            }
        }
        // conditioning: film_r = h W_r^T + b_r for every block; h = time_proj(temb(t)) + z_proj(z)
        mark(TF_COND);
        if (bucket_cb) {
            if (!join_side()) return false;                      // dh was accumulated block by block on the side stream
        } else {
            if (hipMemsetAsync(dh, 0, pl.dh_bytes, st) != hipSuccess) { err = "hipMemsetAsync failed"; return false; }
            if (!ok(launch_film_group_dw(Gd, tr->lin_descs, tr->n_lin, tr->max_lin_n, dfilm, hv, B, td, tr->arch.F, st), "film_dw")) return false;
            if (!ok(launch_film_group_dx(P, tr->lin_descs, tr->n_lin, dfilm, dh, B, td, tr->arch.F, st), "film_dx")) return false;
        }
        if (!lin_bwd(tr->arch.tp2, dh, td, at<float>(pl.t1), 4 * td, dt1, 4 * td, 0)) return false;
        if (!ok(launch_silu_bwd(du0, dt1, at<float>(pl.u0), (int64_t)B * 4 * td, st), "silu_bwd")) return false;
        if (!lin_bwd(tr->arch.tp0, du0, 4 * td, at<float>(pl.temb), td, nullptr, 0, 0)) return false;
        if (!ok(launch_silu_bwd(duz, dh, at<float>(pl.uz), (int64_t)B * td, st), "silu_bwd")) return false;
        if (!lin_bwd(tr->arch.zp, duz, td, z, c.z_dim, nullptr, 0, 0)) return false;
        return flush_bucket(0, true) && join_side();
    }
};

// the kernel choice (tests switch it between handles) decides which repacks a shape needs, so it is part of the key
std::string shape_key(int B, int H, int W)
{
    return std::to_string(B) + "x" + std::to_string(H) + "x" + std::to_string(W) + (conv_pr_selected(1, KIND_C3S1, 128, 8) ? "p" : "n");
}

// the cached plan of a shape, built (and its repack list uploaded) on first use
int step_plan(ccn_trainer_s* tr, int B, int H, int W, const StepPlan** out)
{
    if (B <= 0 || H <= 0 || W <= 0) return fail(CCN_EINVAL, "B, H, W must be positive");
    const int div = 1 << tr->cfg.n_mult;
    if (H % div || W % div) return fail(CCN_EINVAL, "H and W must be divisible by 2^len(ch_mult)");
    const std::string key = shape_key(B, H, W);
    auto it = tr->shapes.find(key);
    if (it == tr->shapes.end()) {
        StepPlan pl;
        pl.B = B; pl.H = H; pl.W = W;
        Planner(tr, pl).run();
        std::string err;
        void* dev = nullptr;
        if (!alloc_dev(tr, pl.pack_list.size() * sizeof(PackDesc), &dev, err)) return fail(CCN_EHIP, err);
        if (hipMemcpy(dev, pl.pack_list.data(), pl.pack_list.size() * sizeof(PackDesc), hipMemcpyHostToDevice) != hipSuccess) return fail(CCN_EHIP, "descriptor upload failed");
        pl.packs = (PackDesc*)dev; pl.n_packs = (int)pl.pack_list.size();
        it = tr->shapes.emplace(key, std::move(pl)).first;
    }
    *out = &it->second;
    return CCN_OK;
}

// snprintf-like end of the report hooks: at most cap bytes (NUL-terminated) into buf, returns the length of the whole text
int copy_report(const std::string& text, char* buf, size_t cap)
{
    if (buf && cap) {
        const size_t n = text.size() < cap - 1 ? text.size() : cap - 1;
        std::memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return (int)text.size();
}

// replay the cached graph for `key`, or capture `body` (which enqueues on the capture stream) and replay it
template <typename F>
int run_graphed(ccn_trainer_s* tr, const std::vector<const void*>& key, hipStream_t user, F&& body)
{
    for (auto& g : tr->graphs)
        if (g.key == key) {
            if (hipGraphLaunch(g.exec, user) != hipSuccess) return fail(CCN_EHIP, "hipGraphLaunch failed");
            return CCN_OK;
        }
    if (!tr->cap_stream && hipStreamCreateWithFlags(&tr->cap_stream, hipStreamNonBlocking) != hipSuccess) return fail(CCN_EHIP, "capture stream");
    if (hipStreamBeginCapture(tr->cap_stream, hipStreamCaptureModeRelaxed) != hipSuccess) return fail(CCN_EHIP, "hipStreamBeginCapture failed");
    std::string err;
    const bool good = body(tr->cap_stream, err);
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(tr->cap_stream, &graph);
    if (!good) { if (graph) (void)hipGraphDestroy(graph); return fail(CCN_EHIP, err); }
    if (ce != hipSuccess) return fail(CCN_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
    ccn_trainer_s::TGraph g; g.key = key; g.graph = graph;
    if (hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0) != hipSuccess) { (void)hipGraphDestroy(graph); return fail(CCN_EHIP, "hipGraphInstantiate failed"); }
    if (tr->graphs.size() >= 8) {
        (void)hipGraphExecDestroy(tr->graphs.front().exec); (void)hipGraphDestroy(tr->graphs.front().graph);
        tr->graphs.erase(tr->graphs.begin());
    }
    tr->graphs.push_back(g);
    if (hipGraphLaunch(g.exec, user) != hipSuccess) return fail(CCN_EHIP, "hipGraphLaunch failed");
    return CCN_OK;
}

}  // namespace

extern "C" {

int ccn_train_set_graph(ccn_trainer_t tr, int32_t on)
{
    if (!tr) return fail(CCN_EINVAL, "null handle");
    tr->use_graph = on != 0;
    return CCN_OK;
}

int ccn_train_create(const ccn_config_t* cfg, ccn_trainer_t* out)
{
    if (!cfg || !out) return fail(CCN_EINVAL, "null argument");
    if (cfg->n_mult <= 0 || cfg->n_mult > CCN_MAX_MULT || cfg->base <= 0 || cfg->time_dim <= 0 || cfg->z_dim <= 0 || cfg->img_ch <= 0 || cfg->img_ch > 3)
        return fail(CCN_EINVAL, "bad config");
    if (cfg->dtype == CCN_DTYPE_F16X3) return fail(CCN_EINVAL, "training supports CCN_DTYPE_F32 (fp32) and CCN_DTYPE_BF16 (bf16); f16x3 is an inference mode");
    if (cfg->dtype != CCN_DTYPE_F32 && cfg->dtype != CCN_DTYPE_BF16) return fail(CCN_EINVAL, "bad dtype");
    if (cfg->base % 8) return fail(CCN_EINVAL, "training path needs base % 8 == 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(CCN_EHIP, "no HIP device: libccn_hip.so has no CPU fallback");
    ccn_trainer_s* tr = new ccn_trainer_s();
    tr->cfg = *cfg;
    tr->elem = cfg->dtype == CCN_DTYPE_BF16 ? 2 : 4;
    tr->G = cfg->groups > 0 ? cfg->groups : 8;
    tr->arch = build_arch(tr->cfg);
    tr->convs.assign(tr->arch.convs.begin(), tr->arch.convs.end());
    std::string err;
    bool good = true;
    for (TConvW& w : tr->convs) good = good && setup_conv(tr, w, err);
    int maxc = cfg->base;
    for (const ArchRes& r : tr->arch.res) if (r.C > maxc) maxc = r.C;
    void* zb = nullptr;
    good = good && alloc_dev(tr, (size_t)(maxc + 256) * 4, &zb, err);
    if (good && hipMemset(zb, 0, (size_t)(maxc + 256) * 4) != hipSuccess) { good = false; err = "hipMemset failed"; }
    if (good && (conv_prepare() != hipSuccess || wgrad_prepare() != hipSuccess)) { good = false; err = "kernel attribute setup failed"; }
    if (good && hipStreamCreateWithFlags(&tr->side, hipStreamNonBlocking) != hipSuccess) { tr->side = nullptr; }
    if (good && tr->side && hipEventCreateWithFlags(&tr->pack_dg_done, hipEventDisableTiming) != hipSuccess) { tr->pack_dg_done = nullptr; }
    if (good) {
        // descriptor tables of the grouped launches (offsets into the caller's flat buffers are fixed by the architecture)
        std::vector<LinDesc> ld;
        for (const ArchRes& r : tr->arch.res) {
            ld.push_back({(long long)tr->arch.params[r.fs.pw].off, (long long)tr->arch.params[r.fs.pb].off, r.C, r.film_off});
            ld.push_back({(long long)tr->arch.params[r.fh.pw].off, (long long)tr->arch.params[r.fh.pb].off, r.C, r.film_off + r.C});
            if (r.C > tr->max_lin_n) tr->max_lin_n = r.C;
        }
        void* ldd = nullptr;
        good = alloc_dev(tr, ld.size() * sizeof(LinDesc), &ldd, err);
        if (good && hipMemcpy(ldd, ld.data(), ld.size() * sizeof(LinDesc), hipMemcpyHostToDevice) != hipSuccess) { good = false; err = "descriptor upload failed"; }
        tr->lin_descs = (LinDesc*)ldd; tr->n_lin = (int)ld.size();
    }
    if (!good) { ccn_train_destroy(tr); return fail(CCN_EHIP, err); }
    tr->zero_bias = (float*)zb;
    *out = tr;
    return CCN_OK;
}

int ccn_train_destroy(ccn_trainer_t tr)
{
    if (!tr) return CCN_OK;
    for (void* p : tr->allocs) (void)hipFree(p);
    for (hipEvent_t e : tr->ev_pool) (void)hipEventDestroy(e);
    for (auto& g : tr->graphs) { if (g.exec) (void)hipGraphExecDestroy(g.exec); if (g.graph) (void)hipGraphDestroy(g.graph); }
    if (tr->cap_stream) (void)hipStreamDestroy(tr->cap_stream);
    for (hipEvent_t e : tr->sync_pool) (void)hipEventDestroy(e);
    if (tr->side) (void)hipStreamDestroy(tr->side);
    if (tr->pack_dg_done) (void)hipEventDestroy(tr->pack_dg_done);
    if (tr->fwd_fork) (void)hipEventDestroy(tr->fwd_fork);
    delete tr;
    return CCN_OK;
}

int ccn_train_num_params(ccn_trainer_t tr, int32_t* n, int64_t* total_floats)
{
    if (!tr || !n) return fail(CCN_EINVAL, "null argument");
    *n = (int32_t)tr->arch.params.size();
    if (total_floats) *total_floats = (int64_t)tr->arch.total;
    return CCN_OK;
}

int ccn_train_param_info(ccn_trainer_t tr, int32_t i, const char** name, int64_t shape[4], int32_t* ndim, int64_t* offset)
{
    if (!tr || i < 0 || i >= (int32_t)tr->arch.params.size()) return fail(CCN_EINVAL, "parameter index out of range");
    const ArchParam& p = tr->arch.params[i];
    if (name) *name = p.name.c_str();
    if (ndim) *ndim = (int32_t)p.shape.size();
    if (shape) for (size_t k = 0; k < p.shape.size() && k < 4; ++k) shape[k] = p.shape[k];
    if (offset) *offset = (int64_t)p.off;
    return CCN_OK;
}

int ccn_train_workspace_bytes(ccn_trainer_t tr, int32_t B, int32_t H, int32_t W, size_t* bytes)
{
    if (!tr || !bytes) return fail(CCN_EINVAL, "null argument");
    const StepPlan* pl;
    const int rc = step_plan(tr, B, H, W, &pl);
    if (rc) return rc;
    *bytes = pl->total;
    return CCN_OK;
}

int ccn_train_forward(ccn_trainer_t tr, const float* params_dev, const float* x_t_dev, const float* z_dev, const int64_t* t_dev, float* eps_dev,
                      int32_t B, int32_t H, int32_t W, void* workspace_dev, size_t workspace_bytes, void* stream)
{
    if (!tr || !params_dev || !x_t_dev || !z_dev || !t_dev || !eps_dev) return fail(CCN_EINVAL, "null argument");
    const StepPlan* pl;
    int rc = step_plan(tr, B, H, W, &pl);
    if (rc) return rc;
    if (!workspace_dev || ((uintptr_t)workspace_dev & 255)) return fail(CCN_EWORKSPACE, "workspace must be non-null and 256-byte aligned");
    if (workspace_bytes < pl->total) return fail(CCN_EWORKSPACE, "workspace too small: need " + std::to_string(pl->total));
    auto body = [&](hipStream_t st, std::string& err) {
        Step s(tr, *pl, workspace_dev, st, params_dev, nullptr);
        if (!s.forward(x_t_dev, z_dev, t_dev, eps_dev)) { err = s.err; return false; }
        s.mark(-1);
        return true;
    };
    if (tr->use_graph && !tr->profiling) {
        const std::vector<const void*> key = {(const void*)1, params_dev, x_t_dev, z_dev, t_dev, eps_dev, workspace_dev, (const void*)(uintptr_t)B,
                                              (const void*)(uintptr_t)H, (const void*)(uintptr_t)W};
        rc = run_graphed(tr, key, (hipStream_t)stream, body);
        if (rc) return rc;
    } else {
        std::string err;
        if (!body((hipStream_t)stream, err)) return fail(CCN_EHIP, err);
    }
    tr->fB = B; tr->fH = H; tr->fW = W; tr->fws = workspace_dev;
    return CCN_OK;
}

}  // extern "C"

namespace {

// both backward entry points; cb: the bucketed form, which never runs under a graph
int train_backward(const char* who, ccn_trainer_t tr, const float* params_dev, float* grads_dev, const float* x_t_dev, const float* z_dev, const float* d_eps_dev,
                   int32_t B, int32_t H, int32_t W, void* workspace_dev, size_t workspace_bytes, void* stream, int64_t bucket_floats, ccn_grad_ready_cb cb, void* user)
{
    if (tr->fB != B || tr->fH != H || tr->fW != W || tr->fws != workspace_dev)
        return fail(CCN_ESTATE, std::string(who) + " must follow ccn_train_forward with the same shape and workspace");
    const StepPlan* pl;
    const int rc = step_plan(tr, B, H, W, &pl);
    if (rc) return rc;
    if (workspace_bytes < pl->total) return fail(CCN_EWORKSPACE, "workspace too small");
    auto body = [&](hipStream_t st, std::string& err) {
        Step s(tr, *pl, workspace_dev, st, params_dev, grads_dev);
        s.bucket_cb = cb; s.bucket_user = user; s.bucket_floats = bucket_floats > 0 ? bucket_floats : 1;
        if (!s.backward(x_t_dev, z_dev, d_eps_dev)) { err = s.err; return false; }
        if (!cb) s.mark(-1);
        return true;
    };
    if (!cb && tr->use_graph && !tr->profiling) {
        const std::vector<const void*> key = {(const void*)2, params_dev, grads_dev, x_t_dev, z_dev, d_eps_dev, workspace_dev, (const void*)(uintptr_t)B,
                                              (const void*)(uintptr_t)H, (const void*)(uintptr_t)W};
        return run_graphed(tr, key, (hipStream_t)stream, body);
    }
    std::string err;
    if (!body((hipStream_t)stream, err)) return fail(CCN_EHIP, err);
    return CCN_OK;
}

// one launch decision as its report line (ccn_internal_train_routes; ccn_internal_conv_dgrad for the launch it made)
std::string route_line(const RouteNote& r)
{
    static const char* kinds[] = {"C3S1", "C3S2", "CT4", "STEM", "HEAD"};
    char line[192];
    const char* kind = r.kind >= 0 && r.kind < 5 ? kinds[r.kind] : "?";
    switch (r.what) {
        case RN_CONV: std::snprintf(line, sizeof(line), "conv %s %s %s th=%d bn=%d n_nt=%d four=%d\n", r.v[0] ? "fwd" : "dgrad", kind, r.name, r.v[1], r.v[2], r.v[3], r.v[4]); break;
        case RN_NORM: std::snprintf(line, sizeof(line), "norm %s slots=%d\n", r.name, r.v[0]); break;
        case RN_GNBWD: std::snprintf(line, sizeof(line), "gnbwd C=%d HW=%d iters=%d nblk=%d tail=%d\n", r.v[0], r.v[1], r.v[2], r.v[3], r.v[4]); break;
        case RN_WGRAD: std::snprintf(line, sizeof(line), "wgrad %s nsplit=%d tiles=%d cin=%d cout=%d\n", kind, r.v[0], r.v[1], r.v[2], r.v[3]); break;
        default: std::snprintf(line, sizeof(line), "colsum src=%s rows=%d ygrid=%d\n", r.name, r.v[0], r.v[1]); break;
    }
    return line;
}

}  // namespace

extern "C" {

int ccn_train_backward(ccn_trainer_t tr, const float* params_dev, float* grads_dev, const float* x_t_dev, const float* z_dev, const float* d_eps_dev,
                       int32_t B, int32_t H, int32_t W, void* workspace_dev, size_t workspace_bytes, void* stream)
{
    if (!tr || !params_dev || !grads_dev || !x_t_dev || !z_dev || !d_eps_dev) return fail(CCN_EINVAL, "null argument");
    return train_backward("ccn_train_backward", tr, params_dev, grads_dev, x_t_dev, z_dev, d_eps_dev, B, H, W, workspace_dev, workspace_bytes, stream, 0, nullptr, nullptr);
}

int ccn_train_backward_bucketed(ccn_trainer_t tr, const float* params_dev, float* grads_dev, const float* x_t_dev, const float* z_dev, const float* d_eps_dev,
                                int32_t B, int32_t H, int32_t W, void* workspace_dev, size_t workspace_bytes, void* stream, int64_t bucket_floats,
                                ccn_grad_ready_cb cb, void* user)
{
    if (!tr || !params_dev || !grads_dev || !x_t_dev || !z_dev || !d_eps_dev || !cb) return fail(CCN_EINVAL, "null argument");
    return train_backward("ccn_train_backward_bucketed", tr, params_dev, grads_dev, x_t_dev, z_dev, d_eps_dev, B, H, W, workspace_dev, workspace_bytes, stream, bucket_floats,
                          cb, user);
}

// Test hook, not part of include/ccn_hip.h (ccn_internal_plan_routes' counterpart for the training step): one line per launch decision
// of the last forward call and the backward calls since, in launch order, taken where the launch is made:
//   conv fwd|dgrad <KIND> <kernel> th= bn= n_nt= four=     (kernel: conv_kernel_name(conv_kernel_for(..)), or head2)
//   norm fused|stats+act|prologue|side-fused|side-stats+act slots=
//   gnbwd C= HW= iters= nblk= tail=                        (pixel passes per workgroup; pixels of the partial last block)
//   wgrad <KIND> nsplit= tiles= cin= cout=
//   colsum src=dy|pairs rows= ygrid=
// A graph replay leaves the captured call's lines.  snprintf-like: writes at most cap bytes (NUL-terminated) and returns the length of the
// whole report, or -1.
int ccn_internal_train_routes(ccn_trainer_t tr, char* buf, size_t cap)
{
    if (!tr) return -1;
    std::string text;
    for (const RouteNote& r : tr->route_log) text += route_line(r);
    return copy_report(text, buf, cap);
}

// Test hook, not part of include/ccn_hip.h: the planned workspace of a shape (built if absent, otherwise only read), one line per region
// in planning order
//   <name> off= bytes=
// and a last line total=, the value of ccn_train_workspace_bytes.  snprintf-like, as ccn_internal_train_routes.
int ccn_internal_train_layout(ccn_trainer_t tr, int32_t B, int32_t H, int32_t W, char* buf, size_t cap)
{
    const StepPlan* pl;
    if (!tr || step_plan(tr, B, H, W, &pl)) return -1;
    std::string text;
    for (const Region& r : pl->regions) text += r.name + " off=" + std::to_string(r.off) + " bytes=" + std::to_string(r.bytes) + "\n";
    text += "total=" + std::to_string(pl->total) + "\n";
    return copy_report(text, buf, cap);
}

// Test hooks, not part of include/ccn_hip.h: one training-backward kernel family alone, on operands the caller supplies, through the same
// launch_* functions and in the same order as Step::wgrad, Step::gn_bwd / bias_grad and launch_colsum.  Device pointers, the caller's
// stream, CCN error codes; every argument is checked before anything is launched.  With scratch == NULL nothing is launched and *need
// receives the scratch bytes of the call (the geometry outputs are filled too).  tests/test_gpu_train_kernels.py.

// dW of one conv.  kind: KIND_C3S1 / C3S2 / CT4 / STEM (0..3); x [B][Hin][Win][Cin], dy [B][Hout][Wout][Cout] in `dtype`; gn_ab: the
// pair-interleaved scale / shift table [B][Cin] or NULL; grad (fp32, parameter layout with Cov x Civ channels) is added to.
// split: 0 the planner's count for a lone launch, -1 its count beside the main stream's kernels, n > 0 that many (at most the tile count).
int ccn_internal_wgrad(int32_t dtype, int32_t kind, const void* x, const void* gn_ab, int32_t silu, const void* dy, int32_t B, int32_t Hin, int32_t Win,
                       int32_t Cin, int32_t Civ, int32_t Cout, int32_t Cov, int32_t split, void* scratch, size_t scratch_bytes, float* grad, void* stream,
                       int32_t* nsplit_out, int32_t* tiles_out, size_t* need)
{
    if (dtype != CCN_DTYPE_F32 && dtype != CCN_DTYPE_BF16) return fail(CCN_EINVAL, "ccn_internal_wgrad: dtype must be fp32 or bf16");
    if (kind != KIND_C3S1 && kind != KIND_C3S2 && kind != KIND_CT4 && kind != KIND_STEM) return fail(CCN_EINVAL, "ccn_internal_wgrad: bad kind");
    if (B <= 0 || Hin <= 0 || Win <= 0 || Cin <= 0 || Cout <= 0) return fail(CCN_EINVAL, "ccn_internal_wgrad: sizes must be positive");
    const int epc = dtype == CCN_DTYPE_F32 ? 4 : 8;
    if (Cin % epc || Cout % epc) return fail(CCN_EINVAL, "ccn_internal_wgrad: Cin and Cout must be multiples of " + std::to_string(epc));
    if (Civ <= 0 || Civ > Cin || Cov <= 0 || Cov > Cout) return fail(CCN_EINVAL, "ccn_internal_wgrad: Civ / Cov must lie in 1..Cin / 1..Cout");
    if (kind == KIND_C3S2 && (Hin % 2 || Win % 2)) return fail(CCN_EINVAL, "ccn_internal_wgrad: the stride-2 conv needs even Hin and Win");
    if (gn_ab && !silu && kind != KIND_C3S1) return fail(CCN_EINVAL, "ccn_internal_wgrad: GroupNorm without SiLU only exists in front of a 3x3 s1 conv");
    if (split < -1) return fail(CCN_EINVAL, "ccn_internal_wgrad: split must be -1, 0 or a count");
    const WgPlan w = wgrad_plan(dtype, kind, B, Hin, Win, Cin, Civ, silu ? 1 : 0, Cout, Cov);
    const int nsplit = split == 0 ? w.nsplit[0] : (split < 0 ? w.nsplit[1] : (split > w.tiles ? w.tiles : split));
    const size_t bytes = (size_t)nsplit * w.a.taps_w * Cout * Cin * 4;
    if (nsplit_out) *nsplit_out = nsplit;
    if (tiles_out) *tiles_out = w.tiles;
    if (need) *need = bytes;
    if (!scratch) return need ? CCN_OK : fail(CCN_EINVAL, "ccn_internal_wgrad: null scratch and nowhere to report its size");
    if (!x || !dy || !grad) return fail(CCN_EINVAL, "ccn_internal_wgrad: null argument");
    if (scratch_bytes < bytes) return fail(CCN_EINVAL, "ccn_internal_wgrad: scratch too small: need " + std::to_string(bytes));
    if (wgrad_prepare() != hipSuccess) return fail(CCN_EHIP, "kernel attribute setup failed");
    WgArgs a = w.a;
    a.x = x; a.gn_ab = (const float2*)gn_ab; a.dy = dy; a.part = (float*)scratch; a.nsplit = nsplit;
    hipError_t e = launch_wgrad(dtype, kind, a, (hipStream_t)stream);
    if (e != hipSuccess) return fail(CCN_EHIP, std::string("wgrad: ") + hipGetErrorString(e));
    e = launch_wgrad_reduce(a.part, nsplit, a.taps_w, Cout, Cin, Cov, Civ, kind == KIND_CT4 ? 1 : 0, grad, (hipStream_t)stream);
    if (e != hipSuccess) return fail(CCN_EHIP, std::string("wgrad_reduce: ") + hipGetErrorString(e));
    return CCN_OK;
}

// GroupNorm(+SiLU) backward of the norm reading x [B][HW][C]: reduce, finalize, apply, then the FiLM finalize (film != NULL: the
// sample's row of `film_bstride` floats holds C scales then C shifts, `dfilm` has the same layout; dbias, when given, is added to) or,
// without FiLM and with dbias, the column sum of `out` from the apply pass's pairs.  out may alias dA; dgamma / dbeta are added to.
// geom: {nslb, pstep, ppb, nblk, zblocks} of gn_bwd_geom.
int ccn_internal_gn_bwd(int32_t dtype, const void* x, const void* dA, const void* ab, const void* stats, const float* gamma, const void* addend,
                        const float* film, int32_t film_bstride, int32_t silu, int32_t B, int32_t HW, int32_t C, int32_t G, void* out, void* gstat,
                        float* dgamma, float* dbeta, float* dfilm, float* dbias, void* scratch, size_t scratch_bytes, void* stream, int32_t* geom,
                        size_t* need)
{
    if (dtype != CCN_DTYPE_F32 && dtype != CCN_DTYPE_BF16) return fail(CCN_EINVAL, "ccn_internal_gn_bwd: dtype must be fp32 or bf16");
    if (B <= 0 || HW <= 0 || C <= 0 || G <= 0) return fail(CCN_EINVAL, "ccn_internal_gn_bwd: sizes must be positive");
    if (C % 8) return fail(CCN_EINVAL, "ccn_internal_gn_bwd: C must be a multiple of 8");
    if (C % G) return fail(CCN_EINVAL, "ccn_internal_gn_bwd: C must be a multiple of G");
    if (film && film_bstride < 2 * C) return fail(CCN_EINVAL, "ccn_internal_gn_bwd: a FiLM row holds C scales and C shifts");
    if (film && !dfilm) return fail(CCN_EINVAL, "ccn_internal_gn_bwd: FiLM needs dfilm");
    const GnBwdGeom gg = gn_bwd_geom(dtype, B, HW, C);
    const size_t half = align_up((size_t)B * gg.nblk * C * sizeof(float2), 256), bytes = 2 * half;
    if (geom) { geom[0] = gg.nslb; geom[1] = gg.pstep; geom[2] = gg.ppb; geom[3] = gg.nblk; geom[4] = gg.zblocks; }
    if (need) *need = bytes;
    if (!scratch) return need ? CCN_OK : fail(CCN_EINVAL, "ccn_internal_gn_bwd: null scratch and nowhere to report its size");
    if (!x || !dA || !ab || !stats || !gamma || !out || !gstat || !dgamma || !dbeta) return fail(CCN_EINVAL, "ccn_internal_gn_bwd: null argument");
    if (scratch_bytes < bytes) return fail(CCN_EINVAL, "ccn_internal_gn_bwd: scratch too small: need " + std::to_string(bytes));
    hipStream_t st = (hipStream_t)stream;
    float2 *scr_gn = (float2*)scratch, *scr_film = (float2*)((char*)scratch + half);
    const int cpg = C / G;
    const double count = (double)cpg * HW;
    const float2 *abt = (const float2*)ab, *stt = (const float2*)stats;
    hipError_t e = launch_gn_bwd_reduce(dtype, x, dA, abt, stt, scr_gn, B, HW, C, cpg, G, silu ? 1 : 0, st);
    if (e != hipSuccess) return fail(CCN_EHIP, std::string("gn_bwd_reduce: ") + hipGetErrorString(e));
    e = launch_gn_bwd_finalize(scr_gn, gg.nblk, B, C, cpg, G, count, gamma, (float2*)gstat, dgamma, dbeta, st);
    if (e != hipSuccess) return fail(CCN_EHIP, std::string("gn_bwd_finalize: ") + hipGetErrorString(e));
    e = launch_gn_bwd_apply(dtype, x, dA, abt, stt, (const float2*)gstat, addend, out, film, film_bstride, scr_film, B, HW, C, cpg, G, silu ? 1 : 0, st);
    if (e != hipSuccess) return fail(CCN_EHIP, std::string("gn_bwd_apply: ") + hipGetErrorString(e));
    if (film) e = launch_film_bwd_finalize(scr_film, gg.nblk, film, film_bstride, dfilm, dbias, B, C, st);
    else if (dbias) e = launch_colsum_from_pairs(scr_film, B * gg.nblk, C, dbias, st);
    if (e != hipSuccess) return fail(CCN_EHIP, std::string(film ? "film_bwd: " : "colsum_from_pairs: ") + hipGetErrorString(e));
    return CCN_OK;
}

// db += the per-channel sum over (B, HW) of dy [B][HW][C]
int ccn_internal_colsum(int32_t dtype, const void* dy, int32_t B, int32_t HW, int32_t C, void* scratch, size_t scratch_bytes, float* db, void* stream,
                        size_t* need)
{
    if (dtype != CCN_DTYPE_F32 && dtype != CCN_DTYPE_BF16) return fail(CCN_EINVAL, "ccn_internal_colsum: dtype must be fp32 or bf16");
    if (B <= 0 || HW <= 0 || C <= 0) return fail(CCN_EINVAL, "ccn_internal_colsum: sizes must be positive");
    if (C % 8) return fail(CCN_EINVAL, "ccn_internal_colsum: C must be a multiple of 8");
    const size_t bytes = (size_t)B * gn_bwd_geom(dtype, B, HW, C).nblk * C * 4;
    if (need) *need = bytes;
    if (!scratch) return need ? CCN_OK : fail(CCN_EINVAL, "ccn_internal_colsum: null scratch and nowhere to report its size");
    if (!dy || !db) return fail(CCN_EINVAL, "ccn_internal_colsum: null argument");
    if (scratch_bytes < bytes) return fail(CCN_EINVAL, "ccn_internal_colsum: scratch too small: need " + std::to_string(bytes));
    const hipError_t e = launch_colsum(dtype, dy, (float*)scratch, db, B, HW, C, (hipStream_t)stream);
    if (e != hipSuccess) return fail(CCN_EHIP, std::string("colsum: ") + hipGetErrorString(e));
    return CCN_OK;
}

// Test hook, not part of include/ccn_hip.h: the data-gradient conv of one conv weight alone, as the step launches it.  weight_name: a conv
// weight as ccn_train_param_info names it (the stem's is CCN_EINVAL: the image needs no gradient).  The conv's data-gradient operand is
// repacked from params_dev by launch_pack_group on the descriptor the route consumes (the one Planner::conv puts on the step's pack
// list), the route and the ConvArgs are Planner::conv_dgrad's and the launch is Step::conv_dgrad's, so no launch comes out of here that
// a step could not make.  dy [B][Hdy][Wdy][Cout] NHWC in the trainer's type (the head: fp32 NCHW [B][img_ch][Hdy][Wdy], as d eps);
// res: NULL, or -- the stride-2 conv only, whose launch adds dskip in the step -- a tensor like dx that the epilogue adds; dx
// [B][Hdx][Wdx][Cin] NHWC is overwritten (3x3 / head: Hdy x Wdy; stride-2 conv: 2 Hdy x 2 Wdy; ConvTranspose: Hdy / 2 x Wdy / 2, both
// even).  route: the launch's line of ccn_internal_train_routes, without the newline (snprintf-like truncation); the handle's own route
// log is left as it was.  Every argument is checked before anything is launched; returns after the stream has drained.
// tests/test_gpu_dgrad.py.
int ccn_internal_conv_dgrad(ccn_trainer_t tr, const char* weight_name, const float* params_dev, const void* dy, const void* res, void* dx, int32_t B,
                            int32_t Hdy, int32_t Wdy, void* stream, char* route, size_t route_cap)
{
    if (!tr || !weight_name || !params_dev || !dy || !dx) return fail(CCN_EINVAL, "ccn_internal_conv_dgrad: null argument");
    if (B <= 0 || Hdy <= 0 || Wdy <= 0) return fail(CCN_EINVAL, "ccn_internal_conv_dgrad: sizes must be positive");
    const TConvW* w = nullptr;
    for (const TConvW& c : tr->convs)
        if (tr->arch.params[c.pw].name == weight_name) w = &c;
    if (!w) return fail(CCN_EINVAL, std::string("ccn_internal_conv_dgrad: no conv weight named ") + weight_name);
    if (w->kind == KIND_STEM) return fail(CCN_EINVAL, "ccn_internal_conv_dgrad: the stem has no data gradient");
    if (w->kind == KIND_CT4 && (Hdy % 2 || Wdy % 2)) return fail(CCN_EINVAL, "ccn_internal_conv_dgrad: the ConvTranspose's gradient needs even Hdy and Wdy");
    if (res && w->kind != KIND_C3S2) return fail(CCN_EINVAL, "ccn_internal_conv_dgrad: only the stride-2 conv's gradient adds a residual in the step");
    StepPlan pl;
    pl.B = B; pl.H = Hdy; pl.W = Wdy;
    const ConvPlan c = Planner(tr, pl).conv_dgrad(*w, Hdy, Wdy, res != nullptr);   // (leaves the operand's descriptor on pl.pack_list)
    hipStream_t st = (hipStream_t)stream;
    PackDesc* desc = nullptr;
    if (hipMalloc((void**)&desc, sizeof(PackDesc)) != hipSuccess) return fail(CCN_EHIP, "ccn_internal_conv_dgrad: hipMalloc failed");
    std::string err;
    if (hipMemcpy(desc, &pl.pack_list.back(), sizeof(PackDesc), hipMemcpyHostToDevice) != hipSuccess) err = "descriptor upload failed";
    if (err.empty()) {
        const hipError_t e = launch_pack_group(tr->cfg.dtype, params_dev, desc, 1, st);
        if (e != hipSuccess) err = std::string("pack: ") + hipGetErrorString(e);
    }
    if (err.empty()) {
        Step s(tr, pl, nullptr, st, params_dev, nullptr);
        const size_t logged = tr->route_log.size();
        if (!s.conv_dgrad(c, dy, dx, res)) err = s.err;
        if (tr->route_log.size() > logged) {
            std::string line = route_line(tr->route_log.back());
            if (!line.empty() && line.back() == '\n') line.pop_back();
            copy_report(line, route, route_cap);
            tr->route_log.resize(logged);
        }
    }
    const hipError_t se = hipStreamSynchronize(st);                       // the descriptor is read by the pack kernel
    (void)hipFree(desc);
    if (!err.empty()) return fail(CCN_EHIP, "ccn_internal_conv_dgrad: " + err);
    if (se != hipSuccess) return fail(CCN_EHIP, std::string("ccn_internal_conv_dgrad: ") + hipGetErrorString(se));
    return CCN_OK;
}

int ccn_train_profile_enable(ccn_trainer_t tr, int32_t on)
{
    if (!tr) return fail(CCN_EINVAL, "null handle");
    tr->profiling = on != 0;
    tr->marks.clear(); tr->ev_used = 0;
    return CCN_OK;
}

int ccn_train_profile_read(ccn_trainer_t tr, const char** names, float* ms, int32_t* calls, double* flops, double* bytes, int32_t cap, int32_t* n)
{
    if (!tr || !names || !ms || !calls || !flops || !bytes || !n) return fail(CCN_EINVAL, "null argument");
    if (cap < TF_COUNT) return fail(CCN_EINVAL, "cap too small");
    if (hipDeviceSynchronize() != hipSuccess) return fail(CCN_EHIP, "hipDeviceSynchronize failed");
    for (int f = 0; f < TF_COUNT; ++f) { names[f] = kTrainFamilies[f]; ms[f] = 0.f; calls[f] = 0; flops[f] = 0.0; bytes[f] = 0.0; }
    for (size_t i = 0; i + 1 < tr->marks.size(); ++i) {
        const Mark& m = tr->marks[i];
        if (m.fam < 0) continue;
        float t = 0.f;
        if (hipEventElapsedTime(&t, m.ev, tr->marks[i + 1].ev) != hipSuccess) return fail(CCN_EHIP, "hipEventElapsedTime failed");
        ms[m.fam] += t; calls[m.fam] += 1; flops[m.fam] += m.flops; bytes[m.fam] += m.bytes;
    }
    *n = TF_COUNT;
    tr->marks.clear(); tr->ev_used = 0;
    return CCN_OK;
}

}  // extern "C"
