// Host side of libccn_hip.so: the C ABI of include/ccn_hip.h.
//
// A handle owns the repacked weights of one CLIPCondUNet: build_arch's description of the network (ccn_arch.h, shared with the
// training handle) plus, per conv, the committed operands in every weight version (ConvW).  ccn_commit_params walks the conv list
// once, one weight version at a time.  ccn_forward / ccn_sample plan (once per shape: ShapePlan) the fixed list
// of kernel launches of one UNet evaluation, every activation, GroupNorm partial-sum and scale/shift buffer an
// offset into the caller's workspace; a Binding ties a plan to one workspace address and owns what depends on it.
// ccn_sample replays the plan `steps` times -- conditioning (timestep MLP, z projection, all FiLM
// linears) is hoisted in front of the loop for all steps, because t is batch-uniform and known ahead
// (diffusion/ddim.py:25,32) -- either launch by launch or as one captured hipGraph.
#include "../../include/ccn_hip.h"
#include "ccn_internal.h"
#include "ccn_arch.h"
#include "ccn_philox.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

using namespace ccn;

namespace {

thread_local std::string g_err;             // behind ccn_last_error(); written by ccn::fail (ccn_internal.h) from every file
#define HIPCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            return fail(CCN_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));                    \
    } while (0)

}  // namespace
extern "C" void ccn_internal_set_error(const char* msg) { g_err = msg ? msg : ""; }

// the one argument check of the launches that take an X0Operands record (ccn_internal.h)
int ccn::check_x0_operands(const X0Operands& o, bool for_rescale, bool pointers)
{
    if (pointers && (!o.out_c || (for_rescale ? !o.out_u : !o.x))) return fail(CCN_EINVAL, "a tensor pointer is NULL");
    if (o.pred != CCN_PRED_EPS && o.pred != CCN_PRED_V) return fail(CCN_EINVAL, "unknown prediction (CCN_PRED_EPS or CCN_PRED_V)");
    if (o.records <= 0 || o.records > 65535) return fail(CCN_EINVAL, "the number of records must be in [1, 65535]: one grid row per record");
    if (for_rescale && (o.per_record < 2 || o.per_record >= kThrMaxPerRecord))
        return fail(CCN_EINVAL, "per_record must be in [2, 2^34): an unbiased std needs two elements");
    if (o.per_record <= 0 || o.per_record >= kThrMaxPerRecord) return fail(CCN_EINVAL, "per_record must be in [1, 2^34)");
    return CCN_OK;
}
namespace {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

uint16_t f2bf_host(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// a conv of the description (ccn_arch.h) and its committed operands
struct ConvW : ArchConv {
    ConvW() {}
    ConvW(const ArchConv& c) : ArchConv(c) {}
    int Cin_pad = 0, Cout_pad = 0, BN = 0, ntaps_w = 0;
    void* w = nullptr;
    void* wfrag = nullptr;      // MFMA-fragment-ordered copy for the persistent 3x3 kernel (Cout_pad % 128 == 0), else null
    float* bias = nullptr;
    bool split = false;         // f16x3 mode, layers on the ws / fr kernels: `w` holds fp16 hi + lo rows of the weights times 1 / inv_scale
    float inv_scale = 1.f;
    // bf16 mode, CCN_ROUND_DIFFUSED_PHASES: further roundings of the same weights, used by DDIM step i as version i % nphase
    // (version 0 = w / wfrag above); see round_version()
    int nphase = 1;
    void* w_ph[7] = {};
    void* wfrag_ph[7] = {};
};
struct NormW { int C = 0; float* gamma = nullptr; float* beta = nullptr; };
struct ResW { NormW n1, n2; };

constexpr size_t kNone = ~(size_t)0;     // workspace offset of an operand the launch does not have
// an NHWC activation of a plan: offsets into the workspace
struct TensorRef {
    std::string name;            // of its workspace region; the conv that writes it is reported under it (RouteRec)
    size_t off = kNone;
    int C = 0, H = 0, W = 0;
    size_t part = kNone;         // GroupNorm partial sums written by the producer
    int n_sp = 0, n_nt = 0, bn = 0;
    bool pr = false;             // partial sums laid out per consumer wave (persistent kernel)
    int prod = -1;               // index in ShapePlan::ops of the producing conv (patched when its GroupNorm finalize is fused in)
};

// what a launch takes from the call instead of the plan
struct StepCtx {
    int step = 0;
    const float* x_in = nullptr;   // NCHW fp32 image entering the stem
    float* x_state = nullptr;      // DDIM state updated by the head (== x_in inside the loop)
    float* eps_out = nullptr;
    int do_ddim = 0;
    float c[4] = {0, 0, 0, 0};
    const float* noise = nullptr;  // eta > 0: this step's noise tensor (sigma > 0), else null
    float sigma = 0.f;
    float* x0_hist = nullptr;      // multistep sampler: the previous step's x0 (caller-owned, outside the workspace), else null
    float c4 = 0.f;                // ... and its coefficient in this step's update
    int pred = CCN_PRED_EPS;       // the run's parameterisation (SamplerRun::pred), read by the head's update
};

const char* kFamilies[] = {"conv3x3_s1_igemm", "conv3x3_s2_igemm", "convT4x4_s2_igemm", "stem_conv_igemm",
                           "head_conv_ddim", "gn_finalize", "conditioning", "gn_silu_prepass"};
enum { F_C3S1 = 0, F_C3S2, F_CT4, F_STEM, F_HEAD, F_GNF, F_COND, F_LAYOUT, F_COUNT };

// One launch of a plan, as plain data: the arguments that depend on the shape and the committed model, and the workspace offsets
// of its operands.  launch() adds the workspace address, the stream and the StepCtx.
enum Op { OP_CONV = 0, OP_HEAD2, OP_GN_FINALIZE, OP_GN_ACT, OP_GN_ACT_FUSED };
struct Launch {
    Op op = OP_CONV; int family = 0; double flops = 0, bytes = 0;     // (profiling family, algorithmic work)
    int conv = -1;               // OP_CONV, OP_HEAD2: index in h->convs (weights: version step % nphase; stem and head by its kind)
    bool frag = false;           // OP_CONV: the route reads the fragment-ordered weights
    int film_off = -1;           // OP_CONV: offset of this conv's [scale | shift] in a FiLM row, or -1
    ConvArgs a{};                // OP_CONV, OP_HEAD2: every field that is not a workspace address or a per-call value
    size_t in = kNone, out = kNone, res = kNone, part = kNone, kpart = kNone, kflag = kNone, gs_part = kNone, gn_ab = kNone,
           fin_ab = kNone, fin_counter = kNone, scratch = kNone;
    // the GroupNorm kinds: finalize of `part` into `gn_ab`; GroupNorm + SiLU pass in -> out from `gn_ab`, or (fused) from `part`
    int C = 0, HW = 0, G = 0, cpg = 0, n_sp = 0, n_nt = 0, bn = 0;
    double count = 0; const float* gamma = nullptr; const float* beta = nullptr;
};

constexpr int kMaxNorms = 128;

// one conv-family launch of a plan as decided at plan build (ccn_internal_plan_routes)
struct RouteRec {
    std::string name;          // the activation it writes: <block>.film (conv1), <block> (conv2), down.N, up.N, in_conv; out = head
    int kind = 0;
    const char* kernel = "";   // conv_kernel_name(conv_kernel_for(...)), or head2
    const char* geom = nullptr; // persistent kernel: the fixed-geometry instantiation launch_conv_pr picks (conv_pr_geom_name), or null
    int th = 0, ksplit = 1, n_nt = 1;
    const char* gn = "none";   // input GroupNorm: none, prologue (finalize launch + conv prologue), instat (in-kernel statistics),
                               // preact / preact_fused (GroupNorm + SiLU pass in front), weights (head2: folded into the weights)
    bool film = false, res = false;
    int ops = -1;              // f16x3 plans only: 1 = split fp16 operands, 0 = the fp32 kernel; -1: not reported
};

// The plan of one (B, H, W, steps) on the committed model: every buffer an offset, every launch a record.  No address, no stream.
struct Region { std::string name; size_t off, bytes; };
struct ShapePlan {
    int B = 0, H = 0, W = 0, steps = 0;
    std::vector<Region> regions; size_t total = 0;
    std::vector<std::pair<size_t, size_t>> zero;        // (offset, bytes) zeroed when a workspace is bound: split-K hand-off flags, counters
    size_t ts_dev = 0, temb = 0, t1 = 0, tp = 0, zp = 0, film = 0, zbuf = 0, xstate = 0;   // conditioning buffers, DDIM state
    int film_stride = 0;                 // floats between consecutive samples' FiLM rows
    size_t counters = 0;                 // arrival counters of the fused GroupNorm finalizes, [max_counters][B], zero at rest
    int n_counters = 0, max_counters = 0;
    std::vector<Launch> ops;             // one UNet evaluation (+ DDIM update in the head)
    std::map<std::string, TensorRef> named;
    std::vector<RouteRec> routes;        // every conv-family launch of `ops`, in order
};

// One run of a sampler loop: what the step loop is a function of besides the handle, the shape and the tensors.  build_run makes it
// from a ccn_sampler_run_t and the handle's state, checked and NORMALISED: a field the run does not use holds the fixed value named
// below, whatever the caller passed.  The host tables are copies, so the record of a captured run outlives the call (GraphEntry).
struct SamplerRun {
    int steps = 0;
    std::vector<int32_t> ts;
    std::vector<float> coef;             // [steps][4]
    std::vector<float> sigma;            // eta > 0 (empty: eta = 0)
    const float* noise = nullptr;        // ... and the caller's noise tensor, [steps] x one state
    // ... or, instead of `noise`, one seed per record of the state: step i's noise is draw 1 + i of each record, generated by the
    // updating launch.  The address is captured, the contents are read at run time.  Unguided, the head then writes the raw output
    // of the B rows into `out_scratch` on the steps with sigma > 0 and one sampler-step launch follows it, as in the guided loop.
    const uint64_t* seeds = nullptr;     // (null without sigma: nothing would be drawn)
    // Classifier-free guidance: the plan's batch is 2B rows -- [0, B) carry z, [B, 2B) the null embedding, both the same state -- the
    // head writes the raw network output of all 2B rows into `out_scratch` (whatever it predicts: the combine launch applies `pred`),
    // and one combine launch per step updates both halves of the state.
    bool guided = false;
    const float* z_null = nullptr;       // one row (null: zeros), copied into the workspace on every call: not part of a capture
    float w = 0.f;                       // the by-value guidance scale of the combine launch (0 unless guided)
    // The raw network output of the steps that update in a launch of their own (the split route: guided, seeded on a step with
    // sigma > 0, every step when thresholded): the caller's scratch in a guided or seeded run (2B / B states), else the head of the
    // handle's threshold scratch in a thresholded one, else null.
    float* out_scratch = nullptr;
    // The multistep sampler: per step the coefficient c4 of (x0 - previous x0) (empty: none), and the caller's history tensor of one
    // state (B rows, also when guided; null without c4), which the updating launch of every step reads (c4 != 0) and rewrites.
    std::vector<float> c4;
    float* hist = nullptr;
    int pred = CCN_PRED_EPS;             // the handle's ccn_set_prediction when the run was built: the update form of every launch
    // Dynamic thresholding (the handle's ccn_set_dynamic_threshold when the run was built; thr_p == 0: off, and the three fields
    // below are zero).  EVERY step then takes the split route: the threshold launches leave one float per record in `thr`, and the
    // sampler-step launch clamps to it.  `thr` and `thr_sel` are parts of the handle's scratch: captured by address.
    double thr_p = 0.0;
    float thr_max = 0.f;
    float* thr = nullptr;
    void* thr_sel = nullptr;
    // Guidance rescale (the handle's ccn_set_guidance_rescale when the run was built; rs_phi == 0: off or unguided, and the two
    // fields below are null).  Every step then runs the two rescale launches after the network: they leave one factor per record in
    // `gscale`, which the threshold launches (if any) and the sampler-step launch multiply the combined output by.  `gscale` and
    // `rs_part` are parts of the handle's rescale scratch: captured by address.
    double rs_phi = 0.0;
    float* gscale = nullptr;
    void* rs_part = nullptr;
    // The low-resolution guide (the handle's ccn_set_lowres_guide when the run was built; lr_N == 0: off, and the fields below are
    // zero).  A step with ts[i] >= lr_tmin takes the split route: after the rescale and threshold launches one delta launch leaves
    // the correction of every block in `lr_delta`, which the sampler-step launch adds to the clamped x0.  `lr_guide` (the caller's
    // thumbnails, contents read at run time) and `lr_delta` (part of the handle's guide scratch) are captured by address.
    const float* lr_guide = nullptr;
    int lr_N = 0;
    float lr_strength = 0.f;
    int lr_tmin = 0;
    float* lr_delta = nullptr;

    // Does a graph captured for `o` replay this run?  Every member a captured launch holds by value or by address, that is all but
    // z_null, the tables bit for bit.  No feature decides which members count: the ones a run does not use are normalised above.
    bool same_graph(const SamplerRun& o) const
    {
        auto same = [](const std::vector<float>& a, const std::vector<float>& b) {
            return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(float)));
        };
        return steps == o.steps && ts == o.ts && same(coef, o.coef) && same(sigma, o.sigma) && noise == o.noise && seeds == o.seeds &&
               guided == o.guided && w == o.w && out_scratch == o.out_scratch && same(c4, o.c4) && hist == o.hist && pred == o.pred &&
               thr_p == o.thr_p && thr_max == o.thr_max && thr == o.thr && thr_sel == o.thr_sel && rs_phi == o.rs_phi &&
               gscale == o.gscale && rs_part == o.rs_part && lr_guide == o.lr_guide && lr_N == o.lr_N && lr_strength == o.lr_strength &&
               lr_tmin == o.lr_tmin && lr_delta == o.lr_delta;
    }
};

struct GraphEntry {
    SamplerRun run;                      // the run it was captured for
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    void destroy() { if (exec) (void)hipGraphExecDestroy(exec); if (graph) (void)hipGraphDestroy(graph); }   // (after draining the device)
};

// A plan bound to one workspace address: what lives IN that workspace (the uploaded timestep table, the zeroed flags) and the graphs
// captured with its addresses.
constexpr size_t kMaxGraphsPerBinding = 4;
struct Binding {
    const ShapePlan* plan = nullptr;
    char* ws = nullptr;
    std::vector<int32_t> ts_keep;        // the timestep table currently in ts_dev (uploaded synchronously, only when it changes)
    std::vector<GraphEntry> graphs;
    ~Binding() { for (auto& g : graphs) g.destroy(); }
};

}  // namespace

struct ccn_handle_s {
    ccn_config_t cfg{};                 // (dtype: the STORAGE type; CCN_DTYPE_F16X3 is fp32 storage with `split` set)
    bool split = false;                 // CCN_DTYPE_F16X3: the ws / fr layers multiply fp16 hi + lo operand rows
    int elem = 4;                       // bytes per activation / weight element
    Arch arch;                          // parameters, convs, ResBlocks, layer list: build_arch, ccn_arch.h
    std::map<std::string, std::vector<float>> host;   // loaded fp32 copies until commit (ccn_commit_params only reads them)
    bool committed = false;
    std::vector<void*> dev_allocs;
    // model: device state per arch.convs / arch.res entry
    std::vector<ConvW> convs;
    std::vector<ResW> res;
    NormW out_norm;
    float *tp0_w = nullptr, *tp0_b = nullptr, *tp2_w = nullptr, *tp2_b = nullptr, *zp_w = nullptr, *zp_b = nullptr;
    float *film_w = nullptr, *film_b = nullptr;
    float* head_w_f32 = nullptr;       // (img_ch, C, 3, 3) fp32 copy of out.weight for the dedicated head kernel
    int G = 8;
    int weight_rounding = CCN_ROUND_DIFFUSED_PHASES;   // how bf16 mode rounds the conv weights in ccn_commit_params (ccn_set_weight_rounding)
    int nphase = 1;                                     // versions per conv weight of the committed model (round_version)
    int pred = CCN_PRED_EPS;                            // what the network output is to the ccn_sample* loops (ccn_set_prediction)
    double thr_p = 0.0;                                 // dynamic thresholding of x0 in the ccn_sample* loops (ccn_set_dynamic_threshold);
    float thr_max = 0.f;                                // 0: off
    char* thr_scratch = nullptr;                        // caller-owned: [raw output of one state | B thresholds | select state]
    size_t thr_scratch_bytes = 0;
    double rs_phi = 0.0;                                // guidance rescale in the guided ccn_sample* loops (ccn_set_guidance_rescale); 0: off
    char* rs_scratch = nullptr;                         // caller-owned: [B factors | the partial sums]
    size_t rs_scratch_bytes = 0;
    const float* lr_guide = nullptr;                    // the low-resolution guide in the ccn_sample* loops (ccn_set_lowres_guide); lr_N == 0: off
    int lr_N = 0;
    float lr_strength = 0.f;
    int lr_tmin = 0;
    char* lr_scratch = nullptr;                         // caller-owned: [delta table | raw output of one state]
    size_t lr_scratch_bytes = 0;
    std::vector<std::unique_ptr<ShapePlan>> shape_plans;   // of the committed model, one per (B, H, W, steps)
    std::vector<std::unique_ptr<Binding>> bindings;         // plan x workspace address, least recently used first
    hipStream_t cap_stream = nullptr;
    int captures = 0;                   // sampler graphs captured so far (ccn_internal_graph_captures)
    unsigned* err_host = nullptr;       // pinned, device-mapped error word the kernels OR into (ConvArgs::err)
    unsigned* err_dev = nullptr;
    // profiling
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;
    struct Rec { int family; double flops, bytes; int e0, e1; };
    std::vector<Rec> recs;
    size_t ev_used = 0;
    std::vector<std::string> fam_names;
};

namespace {

// ---- weight repacking ------------------------------------------------------------------------------------
int upload(ccn_handle_s* h, const void* src, size_t bytes, void** dst)
{
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, bytes ? bytes : 4));
    h->dev_allocs.push_back(p);
    if (bytes) HIPCHK(hipMemcpy(p, src, bytes, hipMemcpyHostToDevice));
    *dst = p;
    return CCN_OK;
}
const std::vector<float>& host_param(const ccn_handle_s* h, int i) { return h->host.at(h->arch.params[i].name); }
int upload_f32(ccn_handle_s* h, int param, float** dst)
{
    const auto& v = host_param(h, param);
    return upload(h, v.data(), v.size() * 4, (void**)dst);
}

float bf16_value(float f)
{
    const uint32_t u = (uint32_t)f2bf_host(f) << 16;
    float r;
    std::memcpy(&r, &u, 4);
    return r;
}

// bf16 mode, CCN_ROUND_DIFFUSED: the conv weights are rounded to bf16 with ERROR DIFFUSION along the contraction of every output
// channel instead of independently (round-to-nearest-even): walking (cin, ky, kx) with kx fastest, each element is rounded after
// the accumulated rounding error of its predecessors has been added to it, so that every partial sum of an output channel's
// weights -- over the taps of one input channel, over input channels -- stays within half an ulp of the fp32 sum.  Independent
// rounding perturbs the model statically: the response of each conv to the smooth / mean part of its input shifts by a random
// walk over K = 9 Cin roundings, the same way in all 50 steps, and the reconstructions lose 0.33 % contrast (+0.11 % PSNR against
// the fp32 mode, above north_star's 0.1 % gate; tools/weight_rounding_probe.py, profiles/r03_weight_rounding_probe.txt).  With
// diffusion the same bf16 kernels land within 0.04 % mean / 0.075 % max.  Costs nothing at run time: the values are ordinary bf16.
// `w` is replaced by bf16-representable fp32 values, so every packer below rounds them exactly.
// ConvTranspose2d (Cin, Cout, 4, 4): an output pixel of parity (py, px) sees only 4 of the 16 taps (ky in {1,3} or {0,2}), so the
// diffusion runs per (output channel, parity) over (cin, those 4 taps).
void diffuse_round_conv(float* w, int O, int I, int taps)                     // Conv2d (O, I, k, k)
{
    for (int o = 0; o < O; ++o) {
        double err = 0.0;
        float* row = w + (size_t)o * I * taps;
        for (size_t k = 0; k < (size_t)I * taps; ++k) {
            const double t = (double)row[k] + err;
            const float r = bf16_value((float)t);
            err = t - (double)r;
            row[k] = r;
        }
    }
}
void diffuse_round_convT(float* w, int I, int O)                              // ConvTranspose2d (I, O, 4, 4), stride 2, padding 1
{
    static const int kk2[2][2] = {{1, 3}, {0, 2}};                            // kernel indices feeding even / odd outputs (fill_taps)
    for (int o = 0; o < O; ++o)
        for (int par = 0; par < 4; ++par) {
            double err = 0.0;
            for (int i = 0; i < I; ++i)
                for (int t = 0; t < 4; ++t) {
                    const int wt = kk2[par >> 1][t >> 1] * 4 + kk2[par & 1][t & 1];
                    float& v = w[((size_t)i * O + o) * 16 + wt];
                    const double tt = (double)v + err;
                    const float r = bf16_value((float)tt);
                    err = tt - (double)r;
                    v = r;
                }
        }
}

// CCN_ROUND_DIFFUSED_PHASES: error diffusion ALSO ALONG THE DDIM STEPS.  A rounded weight is a static perturbation of the model:
// the same error acts in each of the 50 evaluations of one trajectory, and because x changes slowly from step to step its effect
// adds up coherently -- that, not the size of one forward's error, is what moved the PSNR (zero-mean noise of twice the size drawn
// afresh every step moves it 30x less; tools/bf16_bias_probe.py).  So the sampler uses n roundings W_0 .. W_{n-1} of every conv
// weight in turn (step i takes version i % n), built with the rounding error fed forward from version to version:
//     W_k = round( (k + 1) W - (W_0 + ... + W_{k-1}) )      (each `round` = the spatial diffusion above)
// Every partial sum W_0 + ... + W_k stays within half a bf16 ulp of (k + 1) W: the MEAN weight over a period is accurate to
// ulp / (2n) instead of ulp / 2, and what remains alternates in sign from step to step with period <= n steps, which the sampler
// averages out.  Costs n copies of the bf16 weights in HBM (65 MB each at C2) and nothing at run time: each step reads one version.
// n = 8 (bench workload, mean / max PSNR delta per record: 1 version 5.2e-4 / 8.6e-4, 4 versions 4.5e-4 / 9.4e-4, 8 versions
// 3.9e-4 / 8.5e-4); 4 for models above 100 M conv weights (C4: 816 M -- commit time and 1.6 GB per version).
int phases_for(const ccn_handle_s* h)
{
    size_t total = 0;
    for (auto& p : h->arch.params) if (p.shape.size() == 4) total += p.numel();
    return total > (size_t)100000000 ? 4 : 8;
}
// Version k of one conv weight, the one implementation of the recurrence above: out = round((k + 1) w - sum), then sum += out.
// `sum` is the float64 running sum W_0 + ... + W_{k-1} (zeros for k = 0, where the operand is w itself: the plain CCN_ROUND_DIFFUSED
// rounding).  `w` is a Conv2d (O, I, taps) or -- convT -- a ConvTranspose2d (I, O, 4, 4) weight of n elements and is only read.
void round_version(const float* w, size_t n, bool convT, int O, int I, int taps, int k, double* sum, float* out)
{
    for (size_t i = 0; i < n; ++i) out[i] = (float)((double)(k + 1) * (double)w[i] - sum[i]);
    if (convT) diffuse_round_convT(out, I, O); else diffuse_round_conv(out, O, I, taps);
    for (size_t i = 0; i < n; ++i) sum[i] += (double)out[i];
}

}  // namespace
// Host-only arithmetic of the bf16 weight rounding, exported for tests/test_host_logic.py (not part of include/ccn_hip.h; no GPU
// involved): `w` is a Conv2d (O, I, taps) or -- convT != 0 -- a ConvTranspose2d (I, O, 4, 4) weight; out[p] receives version p of
// `phases` versions (phases == 1: the plain error-diffused rounding), each bf16-representable fp32.  The versions come from
// round_version, the routine ccn_commit_params packs from.
extern "C" int ccn_internal_round_weights(const float* w, int O, int I, int taps, int convT, int phases, float* out)
{
    if (!w || !out || O <= 0 || I <= 0 || phases < 1 || phases > 8 || (convT && taps != 16)) return 1;
    const size_t n = (size_t)O * I * taps;
    std::vector<double> sum(n, 0.0);
    for (int k = 0; k < phases; ++k) round_version(w, n, convT != 0, O, I, taps, k, sum.data(), out + (size_t)k * n);
    return 0;
}
// f16x3: the commit-time split of one weight tensor, exported for tests/test_split_host.py (not part of include/ccn_hip.h; no GPU
// involved).  *scale = the power of two s with max|w| s in [2^13, 2^14) (1 for an all-zero tensor): it lifts the low halves of
// all but the smallest weights out of fp16's subnormal range while hi stays 4x below its largest finite value.  hi = RNE_fp16(w s),
// lo = RNE_fp16(w s - hi), as fp16 bit patterns: hi + lo = w s to 2^-22 relative (2^-25 absolute where lo is subnormal).
extern "C" int ccn_internal_split_weights(const float* w, size_t n, float* scale, uint16_t* hi, uint16_t* lo)
{
    if ((!w && n) || !scale || ((!hi || !lo) && n)) return 1;
    float mx = 0.f;
    for (size_t i = 0; i < n; ++i) { const float v = std::fabs(w[i]); if (v > mx) mx = v; }
    int e = 0;
    float s = 1.f;
    if (mx > 0.f && std::isfinite(mx)) { (void)std::frexp(mx, &e); s = std::ldexp(1.f, std::min(14 - e, 126)); }   // mx in [2^(e-1), 2^e)
    *scale = s;
    for (size_t i = 0; i < n; ++i) {
        const float ws = w[i] * s;                              // exact
        const _Float16 h = (_Float16)ws;
        const _Float16 l = (_Float16)(ws - (float)h);           // the subtraction is exact
        std::memcpy(hi + i, &h, 2);
        std::memcpy(lo + i, &l, 2);
    }
    return 0;
}
namespace {

// The packers: one version of a conv's weights `w` (fp32, the layout of its parameter) into the operand layouts of its kernels.
// The device pointers go to *dw (every kernel's [taps][Cout_pad][Cin_pad] operand) and *dfrag (fragment order of the persistent /
// register-weight kernels, where the layer has one); the operand geometry goes into `cw`, the same for every version.
// element (tap, o, i) of the packed [taps][Cout_pad][Cin_pad] tensor
template <typename F>
int pack_and_upload(ccn_handle_s* h, ConvW& cw, int taps, F&& at, void** dw)
{
    cw.BN = conv_bn_for(cw.Cout, cw.kind);
    cw.Cout_pad = (int)align_up(cw.Cout, cw.BN);
    cw.ntaps_w = taps;
    const size_t n = (size_t)taps * cw.Cout_pad * cw.Cin_pad;
    if (h->cfg.dtype == CCN_DTYPE_BF16) {
        std::vector<uint16_t> buf(n, 0);
        for (int t = 0; t < taps; ++t)
            for (int o = 0; o < cw.Cout; ++o)
                for (int i = 0; i < cw.Cin_pad; ++i) buf[((size_t)t * cw.Cout_pad + o) * cw.Cin_pad + i] = f2bf_host(at(t, o, i));
        return upload(h, buf.data(), n * 2, dw);
    }
    std::vector<float> buf(n, 0.f);
    for (int t = 0; t < taps; ++t)
        for (int o = 0; o < cw.Cout; ++o)
            for (int i = 0; i < cw.Cin_pad; ++i) buf[((size_t)t * cw.Cout_pad + o) * cw.Cin_pad + i] = at(t, o, i);
    // f16x3: the layers conv_kernel_for sends to the ws / fr kernels (fp32 storage never takes the persistent one) get the same
    // [tap][Cout_pad][Cin_pad] geometry in 128-byte rows of 32 fp16 hi + 32 fp16 lo per 32-channel chunk, scaled per layer
    cw.split = h->split && conv_ws_enabled() && conv_ws_supported(cw.kind, cw.BN);
    cw.inv_scale = 1.f;
    if (cw.split) {
        std::vector<uint16_t> hi(n), lo(n), rows(2 * n);
        float s = 1.f;
        if (ccn_internal_split_weights(buf.data(), n, &s, hi.data(), lo.data())) return fail(CCN_EINVAL, "weight split failed");
        cw.inv_scale = 1.f / s;
        for (size_t i = 0; i < n; ++i) {
            const size_t row = i / 32, c = i % 32;
            rows[row * 64 + c] = hi[i];
            rows[row * 64 + 32 + c] = lo[i];
        }
        return upload(h, rows.data(), n * 4, dw);
    }
    return upload(h, buf.data(), n * 4, dw);
}

int pack_conv3(ccn_handle_s* h, ConvW& cw, const float* w, void** dw, void** dfrag)     // Conv2d weight (O, I, 3, 3)
{
    const int cke = conv_cin_chunk(h->cfg.dtype);
    cw.Cin_pad = (int)align_up(cw.Cin, cke);
    const int I = cw.Cin;
    int rc = pack_and_upload(h, cw, 9, [&](int t, int o, int i) { return i < I ? w[((size_t)o * I + i) * 9 + t] : 0.f; }, dw);
    if (rc) return rc;
    if (cw.kind == KIND_C3S2 && cw.BN == 128 && h->cfg.dtype == CCN_DTYPE_BF16) {
        // plane-pass order for the persistent kernel (ccn_conv_pr.hip, NTAPS == 2): prs2_frag_index / prs2_tap (ccn_internal.h), the tenth
        // tap slot stays zero; the training step's device-side packer (PK_FRAG_S2) goes through the same functions
        const int nch = cw.Cin_pad / cke, n32 = cw.Cout_pad / 32, O = cw.Cout;
        std::vector<uint16_t> fr((size_t)nch * 5 * n32 * 2 * 4 * 64 * 8, 0);
        for (int o = 0; o < O; ++o)
            for (int i = 0; i < I; ++i)
                for (int ps = 0; ps < 10; ++ps) {
                    const int tp = prs2_tap(ps >> 1, ps & 1);
                    if (tp >= 0) fr[prs2_frag_index(ps >> 1, ps & 1, o, i, cw.Cout_pad)] = f2bf_host(w[((size_t)o * I + i) * 9 + tp]);
                }
        return upload(h, fr.data(), fr.size() * 2, dfrag);
    }
    if (cw.kind == KIND_C3S1 && cw.BN == 128 && h->cfg.dtype == CCN_DTYPE_BF16) {
        // fragment order of the persistent kernel's 3x3 form (pr3_frag_index, ccn_internal.h): one wave load = 1 KiB contiguous
        const int nch = cw.Cin_pad / cke, n32 = cw.Cout_pad / 32, O = cw.Cout;
        std::vector<uint16_t> fr((size_t)nch * n32 * 36 * 64 * 8, 0);
        for (int o = 0; o < O; ++o)
            for (int i = 0; i < I; ++i)
                for (int t = 0; t < 9; ++t) fr[pr3_frag_index(o, i, t, cw.Cout_pad)] = f2bf_host(w[((size_t)o * I + i) * 9 + t]);
        return upload(h, fr.data(), fr.size() * 2, dfrag);
    }
    return CCN_OK;
}
int pack_convT(ccn_handle_s* h, ConvW& cw, const float* w, void** dw, void** dfrag)     // ConvTranspose2d weight (I, O, 4, 4)
{
    const int cke = conv_cin_chunk(h->cfg.dtype);
    cw.Cin_pad = (int)align_up(cw.Cin, cke);
    const int I = cw.Cin, O = cw.Cout;
    int rc = pack_and_upload(h, cw, 16, [&](int t, int o, int i) { return i < I ? w[((size_t)i * O + o) * 16 + t] : 0.f; }, dw);
    if (rc) return rc;
    if (cw.BN == 128 && h->cfg.dtype == CCN_DTYPE_BF16) {
        // fragment order for ccn_conv_pr.hip: [parity][chunk][Cout_pad/32][tap 0..3][kk][lane][8] = prct_frag_index, tap -> kernel
        // element prct_tap (ccn_internal.h; the same order as fill_taps: even outputs <- k in {1, 3}, odd <- {0, 2}); the training
        // step's device-side packer (PK_FRAG_CT) goes through the same functions
        const int nch = cw.Cin_pad / cke, n32 = cw.Cout_pad / 32;
        std::vector<uint16_t> fr((size_t)4 * nch * n32 * 4 * 4 * 64 * 8, 0);
        for (int o = 0; o < O; ++o)
            for (int i = 0; i < I; ++i)
                for (int pt = 0; pt < 16; ++pt)
                    fr[prct_frag_index(pt >> 2, pt & 3, o, i, cw.Cout_pad, nch)] = f2bf_host(w[((size_t)i * O + o) * 16 + prct_tap(pt >> 2, pt & 3)]);
        return upload(h, fr.data(), fr.size() * 2, dfrag);
    }
    return CCN_OK;
}
int pack_stem(ccn_handle_s* h, ConvW& cw, const float* w, const float* bias, void** dw, void** dfrag)     // Conv2d weight (O, img_ch, 3, 3) as K = I*9
{
    const int cke = conv_cin_chunk(h->cfg.dtype);
    cw.Cin_pad = cke;
    const int K = cw.Cin * 9;
    int rc = pack_and_upload(h, cw, 1, [&](int, int o, int k) { return k < K ? w[(size_t)o * K + k] : 0.f; }, dw);
    if (rc) return rc;
    if (stem2_supported(h->cfg.dtype, cw.Cin, cw.Cout, h->G)) {
        // fragment order for ccn_stem.hip: [Cout/32][k-step 2][lane = h*32 + r][8 bf16]; lane (r, h) holds output channel
        // j*32 + r, k = 16 s + 8 h + e; k = K is the bias (multiplied by a constant-one im2col element)
        const int nt = cw.Cout / 32;
        std::vector<uint16_t> fr((size_t)nt * 2 * 64 * 8, 0);
        for (int j = 0; j < nt; ++j)
            for (int s = 0; s < 2; ++s)
                for (int ln = 0; ln < 64; ++ln)
                    for (int e = 0; e < 8; ++e) {
                        const int o = j * 32 + (ln & 31), k = 16 * s + 8 * (ln >> 5) + e;
                        const float v = k < K ? w[(size_t)o * K + k] : (k == K ? bias[o] : 0.f);
                        fr[(((size_t)j * 2 + s) * 64 + ln) * 8 + e] = f2bf_host(v);
                    }
        return upload(h, fr.data(), fr.size() * 2, dfrag);
    }
    return CCN_OK;
}
int pack_conv(ccn_handle_s* h, ConvW& cw, const float* w, const float* bias, void** dw, void** dfrag)
{
    if (cw.kind == KIND_STEM) return pack_stem(h, cw, w, bias, dw, dfrag);
    return cw.kind == KIND_CT4 ? pack_convT(h, cw, w, dw, dfrag) : pack_conv3(h, cw, w, dw, dfrag);
}

// ---- plan -------------------------------------------------------------------------------------------------
struct ConvOpts {
    int film_off = -1;                  // epilogue FiLM: offset of this conv's [scale | shift] in a FiLM row
    const TensorRef* res = nullptr;     // epilogue residual / skip
    bool want_part = false;             // also emit the partial sums of the output's GroupNorm
    size_t gn_ab = kNone;               // prologue GroupNorm from this finalized scale/shift table, or
    const NormW* in_norm = nullptr;     // the input goes through this GroupNorm (+ SiLU) first; its finalize either becomes part of the
                                        // conv launch itself (persistent kernel, conv_in_kernel_stats) or a gn_finalize launch in front of it
    const char* pre_pass = nullptr;     // the input was made by a GroupNorm + SiLU pass: its form, for the route report
};

struct PlanBuilder {
    ccn_handle_s* h; ShapePlan& pl; const int B;
    size_t off = 0;
    PlanBuilder(ccn_handle_s* h_, ShapePlan& p) : h(h_), pl(p), B(p.B) {}

    size_t take(const std::string& name, size_t bytes)     // a named region of the workspace, 256-byte aligned: its offset
    {
        pl.regions.push_back({name, align_up(off, 256), bytes});
        off = pl.regions.back().off + bytes;
        return off - bytes;
    }
    TensorRef new_tensor(const std::string& name, int C, int H, int W)
    {
        TensorRef t; t.name = name; t.C = C; t.H = H; t.W = W;
        t.off = take(name, (size_t)B * H * W * C * h->elem);
        return t;
    }
    int groups_for(int C) const { return C < h->G ? C : h->G; }
    // arrival counters of the fused GroupNorm finalizes: they start (and are left) at zero
    void take_counters(int n) { pl.max_counters = n; pl.counters = take("counters", (size_t)n * B * 4); pl.zero.push_back({pl.counters, (size_t)n * B * 4}); }

    // the inference plan's policy for conv_route: the stride-2 conv on the persistent kernel from 128 eight-row tiles (half the CUs),
    // the ConvTranspose only where conv_tile_rows gives 8 rows; split-K on the stride-2 layers (CCN_SPLITK_S1=1: the 3x3 s1 layers too)
    ConvRoute route(const ConvW& cw, int Hin, int Win, bool gn_ab, bool res, bool film) const
    {
        static const ConvPolicy policy{true, 128, false, !diag_env("CCN_NO_SPLITK"), diag_env("CCN_SPLITK_S1") != nullptr, true};
        return conv_route({h->cfg.dtype, cw.kind, false, cw.BN, cw.Cin, cw.Cin_pad, cw.Cout, cw.Cout_pad, B, Hin, Win, h->G, cw.wfrag != nullptr,
                           gn_ab, res, film}, policy);
    }

    // conv launch of h->convs[ci]; the stem reads the call's image and the head writes the call's outputs (by the conv's kind)
    void conv(int ci, const TensorRef& in, TensorRef& out, const ConvOpts& o)
    {
        const ConvW& cw = h->convs[ci];
        size_t gn_ab = o.gn_ab;
        const ConvRoute r = route(cw, in.H, in.W, gn_ab != kNone, o.res != nullptr, o.film_off >= 0);
        const ConvGeom& g = r.g;
        Launch L;
        static_assert(F_C3S1 == KIND_C3S1 && F_C3S2 == KIND_C3S2 && F_CT4 == KIND_CT4 && F_STEM == KIND_STEM && F_HEAD == KIND_HEAD, "family = kind");
        L.family = cw.kind; L.conv = ci; L.film_off = o.film_off; L.frag = r.uses_frag() && cw.wfrag;
        L.in = in.off; L.out = out.off; L.res = o.res ? o.res->off : kNone;
        ConvArgs& a = L.a;
        r.fill(a);
        a.bias = cw.bias; a.ops = cw.split ? 1 : 0; a.wscale_inv = cw.inv_scale;
        RouteRec rec;
        if (h->split) rec.ops = a.ops;
        rec.name = out.name; rec.kind = cw.kind; rec.th = r.th; rec.ksplit = r.ksplit; rec.n_nt = r.n_nt;
        rec.film = o.film_off >= 0; rec.res = o.res != nullptr;
        rec.gn = gn_ab != kNone ? "prologue" : "none";
        static const bool no_instat = diag_env("CCN_NO_INSTAT") != nullptr;       // diagnostics build only
        if (o.in_norm) {
            const int G_in = groups_for(cw.Cin), cpg_in = cw.Cin / G_in;
            if (r.gs_ok && !no_instat && in.C == cw.Cin && conv_in_kernel_stats(h->cfg.dtype, in.C, G_in, in.n_sp, in.bn)) {
                L.gs_part = in.part; a.gs_gamma = o.in_norm->gamma; a.gs_beta = o.in_norm->beta;
                a.gs_inv_count = 1.0 / ((double)cpg_in * in.H * in.W);
                a.gs_nsp = in.n_sp; a.gs_nnt = in.n_nt; a.gs_bn = in.bn; a.gs_cpg = cpg_in;
                rec.gn = "instat";
            } else { gn_ab = gn(in, *o.in_norm); rec.gn = "prologue"; }     // (pushes the finalize launch in front of this conv)
        }
        if (o.pre_pass) rec.gn = o.pre_pass;
        L.gn_ab = gn_ab;
        rec.kernel = conv_kernel_name(conv_kernel_for(cw.kind, cw.BN, a));
        pl.routes.push_back(rec);
        if (r.ksplit == 2) {
            L.kpart = take(out.name + ".kpart", (size_t)B * g.Hout * g.Wout * cw.Cout * h->elem);
            const size_t fbytes = (size_t)B * r.fin_blocks * 4 * sizeof(unsigned);
            L.kflag = take(out.name + ".kflag", fbytes);
            pl.zero.push_back({L.kflag, fbytes});
        }
        a.film_bstride = pl.film_stride; a.err = h->err_dev;
        if (o.want_part) {
            out.part = take(out.name + ".part", (size_t)B * a.G * a.nslot * sizeof(float2));
            out.n_sp = r.part_nsp; out.n_nt = r.part_nnt; out.bn = r.part_bn;
            if (r.pr || r.stem2) out.pr = true;
            out.prod = (int)pl.ops.size();
        }
        L.part = out.part;
        if (conv_kernel_for(cw.kind, cw.BN, a) == CK_PR)
            pl.routes.back().geom = conv_pr_geom_name(a, o.res != nullptr, o.film_off >= 0, L.gs_part != kNone ? 1 : (gn_ab != kNone ? 0 : 2));
        const double macs = (double)B * g.Hout * g.Wout * cw.Cout * (double)(cw.kind == KIND_CT4 ? 4 : 9) * cw.Cin;
        L.flops = 2.0 * macs;
        L.bytes = ((double)B * in.H * in.W * cw.Cin + (double)B * g.Hout * g.Wout * cw.Cout + (o.res ? (double)B * g.Hout * g.Wout * cw.Cout : 0.0)
                   + (double)(cw.kind == KIND_CT4 ? 16 : 9) * cw.Cin * cw.Cout) * h->elem;
        if (cw.kind == KIND_STEM) L.bytes = (double)B * in.H * in.W * cw.Cin * 4 + ((double)B * g.Hout * g.Wout * cw.Cout + 9.0 * cw.Cin * cw.Cout) * h->elem;
        if (cw.kind == KIND_HEAD) L.bytes = ((double)B * in.H * in.W * cw.Cin + 9.0 * cw.Cin * cw.Cout) * h->elem + 3.0 * (double)B * g.Hout * g.Wout * cw.Cout * 4;
        pl.ops.push_back(L);
    }
    // a GroupNorm launch over tensor `t` for the norm (gamma, beta)
    Launch norm_launch(Op op, int family, double bytes, const TensorRef& t, const NormW& n) const
    {
        Launch L;
        L.op = op; L.family = family; L.bytes = bytes;
        L.C = t.C; L.HW = t.H * t.W; L.G = groups_for(t.C); L.cpg = t.C / L.G; L.count = (double)L.cpg * t.H * t.W;
        L.in = t.off; L.part = t.part; L.n_sp = t.n_sp; L.n_nt = t.n_nt; L.bn = t.bn; L.gamma = n.gamma; L.beta = n.beta;
        return L;
    }

    // GroupNorm finalize of tensor `t` for the norm (gamma, beta): returns the scale/shift table
    size_t gn(const TensorRef& t, const NormW& n)
    {
        const size_t ab = take(t.name + ".ab", (size_t)B * t.C * sizeof(float2));
        Launch L = norm_launch(OP_GN_FINALIZE, F_GNF, (double)B * groups_for(t.C) * t.n_sp * t.n_nt * 8.0 + (double)B * t.C * 8.0, t, n);
        // measured slower than the 5 us finalize launch it removes (every workgroup drains its stores and pays an atomic
        // round trip before exiting): 50.4 vs 52.1 img/s at C2, so opt-in only
        static const bool fuse = diag_env("CCN_FUSED_FINALIZE") != nullptr;
        if (fuse && t.prod >= 0 && !t.pr && pl.n_counters < pl.max_counters) {
            // the producing conv's last workgroup per sample does the finalize (no launch, no kernel boundary)
            Launch& p = pl.ops[t.prod];
            p.fin_counter = pl.counters + (size_t)pl.n_counters * B * sizeof(unsigned);
            pl.n_counters++;
            p.a.fin_gamma = n.gamma; p.a.fin_beta = n.beta; p.fin_ab = ab; p.a.fin_count = L.count;
            return ab;
        }
        L.gn_ab = ab;
        pl.ops.push_back(L);
        return ab;
    }

    // GroupNorm-apply + SiLU as a separate pass when the consuming conv would redo it per N tile (C >= 256): from the finalized table
    // `ab`, or (kNone) with the finalize of `t`'s GroupNorm folded in (no gn() launch, no scale/shift table)
    TensorRef preact(const TensorRef& t, const NormW& n, size_t ab)
    {
        TensorRef o = new_tensor(t.name + ".act", t.C, t.H, t.W);
        Launch L = norm_launch(ab == kNone ? OP_GN_ACT_FUSED : OP_GN_ACT, F_LAYOUT, 2.0 * B * t.H * t.W * (double)t.C * h->elem, t, n);
        L.out = o.off; L.gn_ab = ab;
        pl.ops.push_back(L);
        return o;
    }

    // x + conv2(SiLU(GN2(FiLM(conv1(SiLU(GN1(x))))))) -- models/blocks.py:40-44
    TensorRef resblock(int ri, const TensorRef& x, bool out_feeds_gn, int film_off)
    {
        const ArchRes& r = h->arch.res[ri];
        const ConvW& c1 = h->convs[r.c1];
        const NormW &n1 = h->res[ri].n1, &n2 = h->res[ri].n2;
        // pre-pass only where the conv kernel would redo the transform per N tile AND has no idle VALU for it: the persistent
        // kernel's producers absorb it up to 4 N tiles (measured at the 512-channel level of C2, 4-row tiles: 69.5 vs 68.8
        // images/s against pre-pass + finalize-free conv; CCN_PREACT_PR=1 restores the pre-pass in front of it for A/B runs)
        static const bool preact_pr = diag_env("CCN_PREACT_PR") != nullptr;
        const bool pre = conv_wants_preact(c1.kind, c1.BN, c1.Cout_pad / c1.BN) && r.C / (h->elem == 2 ? 8 : 4) <= 256 &&
                         (preact_pr || c1.Cout_pad / c1.BN >= 6 || !route(c1, x.H, x.W, false, false, false).pr);
        static const bool fuse_act = !diag_env("CCN_NO_FUSED_GNACT");       // finalize folded into the pre-pass (A/B switch)
        const bool f1 = pre && fuse_act && x.n_sp > 0, f2 = pre && fuse_act;     // (an input without partial sums: table first)
        ConvOpts o1, o2;
        o1.film_off = film_off; o1.want_part = true; o1.pre_pass = f1 ? "preact_fused" : (pre ? "preact" : nullptr);
        o2.res = &x; o2.want_part = out_feeds_gn; o2.pre_pass = f2 ? "preact_fused" : (pre ? "preact" : nullptr);
        TensorRef y = new_tensor(r.prefix + ".film", r.C, x.H, x.W);
        if (pre) conv(r.c1, preact(x, n1, f1 ? kNone : gn(x, n1)), y, o1);
        else { o1.in_norm = &n1; conv(r.c1, x, y, o1); }
        pl.named[y.name] = y;
        TensorRef o = new_tensor(r.prefix, r.C, x.H, x.W);
        if (pre) conv(r.c2, preact(y, n2, f2 ? kNone : gn(y, n2)), o, o2);
        else { o2.in_norm = &n2; conv(r.c2, y, o, o2); }
        pl.named[o.name] = o;
        return o;
    }
};

int build_plan(ccn_handle_s* h, ShapePlan& pl)
{
    const ccn_config_t& c = h->cfg;
    PlanBuilder pb(h, pl);
    const int B = pl.B, H = pl.H, W = pl.W, S = pl.steps;
    const int TR = B > S ? B : S, FR = S * B > B ? S * B : B;
    pl.film_stride = h->arch.F;
    pl.ts_dev = pb.take("ts", (size_t)S * 4);
    pl.temb = pb.take("temb", (size_t)TR * c.time_dim * 4);
    pl.t1 = pb.take("t1", (size_t)TR * c.time_dim * 4 * 4);
    pl.tp = pb.take("tp", (size_t)TR * c.time_dim * 4);
    pl.zp = pb.take("zp", (size_t)B * c.time_dim * 4);
    pl.film = pb.take("film", (size_t)FR * h->arch.F * 4);
    pl.zbuf = pb.take("z", (size_t)B * c.z_dim * 4);
    pl.xstate = pb.take("x_state", (size_t)B * c.img_ch * H * W * 4);
    pb.take_counters(kMaxNorms);

    TensorRef x, img; img.C = c.img_ch; img.H = H; img.W = W;     // img: NCHW fp32, pointer supplied per call
    std::vector<TensorRef> skips;
    const std::vector<ArchLayer>& layers = h->arch.layers; const size_t nl = layers.size();
    for (size_t li = 0; li < nl; ++li) {
        const ArchLayer& L = layers[li];
        ConvOpts o;
        o.want_part = li + 1 < nl && (layers[li + 1].type == L_RES || layers[li + 1].type == L_HEAD);   // a GroupNorm reads the output
        if (L.type == L_RES) { x = pb.resblock(L.idx, x, o.want_part, h->arch.res[L.idx].film_off); continue; }
        const ConvW& cw = h->convs[L.idx];
        if (L.type == L_HEAD) {
            o.gn_ab = pb.gn(x, h->out_norm); o.want_part = false;
            static const bool no_head2 = diag_env("CCN_NO_HEAD2") != nullptr;
            if (no_head2 || !head2_supported(c.dtype, cw.Cin, cw.Cout, h->G)) {
                TensorRef none; none.name = L.name;
                pb.conv(L.idx, x, none, o);
                continue;
            }
            // dedicated kernel pair: out_norm's finalize folded into per-sample head weights, taps in the N dimension
            Launch Lh;
            Lh.op = OP_HEAD2; Lh.family = F_HEAD; Lh.conv = L.idx; Lh.in = x.off; Lh.gn_ab = o.gn_ab;
            ConvArgs& a = Lh.a;
            a.bias = cw.bias; a.B = B; a.Hin = H; a.Win = W; a.Cin = cw.Cin; a.Cout = cw.Cout; a.Hout = H; a.Wout = W;
            Lh.scratch = pb.take(L.name + ".scratch", head2_scratch_bytes(B, x.C));
            const double macs = (double)B * H * W * cw.Cout * 9.0 * cw.Cin;
            Lh.flops = 2.0 * macs;
            Lh.bytes = ((double)B * H * W * x.C + 9.0 * x.C * cw.Cout) * h->elem + 3.0 * (double)B * H * W * cw.Cout * 4;
            pl.ops.push_back(Lh);
            RouteRec rec;
            rec.name = L.name; rec.kind = KIND_HEAD; rec.kernel = "head2"; rec.th = 8; rec.gn = "weights";
            if (h->split) rec.ops = 0;
            pl.routes.push_back(rec);
            continue;
        }
        TensorRef sk;
        if (L.type == L_DOWN) skips.push_back(x);                   // (check_shape: H and W halve evenly at every level)
        if (L.type == L_UP) { sk = skips.back(); skips.pop_back(); o.res = &sk; }
        const TensorRef& in = L.type == L_STEM ? img : x;
        const int up = L.type == L_UP ? 2 : 1, down = L.type == L_DOWN ? 2 : 1;
        TensorRef out = pb.new_tensor(L.name, cw.Cout, in.H * up / down, in.W * up / down);
        if (o.res && (sk.C != cw.Cout || sk.H != out.H || sk.W != out.W)) return fail(CCN_EINVAL, "skip shape mismatch");
        pb.conv(L.idx, in, out, o);
        pl.named[L.name] = x = out;
    }
    pl.total = align_up(pb.off, 256);
    return CCN_OK;
}

// ---- launching --------------------------------------------------------------------------------------------
// The one place where a record meets a workspace, a stream and a call: offsets become pointers, DDIM step i takes weight version
// i % nphase (round_version) and its FiLM row, the stem the call's image, the head (both forms) the call's per-step fields.
hipError_t launch(const ccn_handle_s* h, const ShapePlan& pl, const Launch& L, char* ws, hipStream_t s, const StepCtx& c)
{
    auto at = [ws](size_t o) -> char* { return o == kNone ? nullptr : ws + o; };
    const int dtype = h->cfg.dtype;
    switch (L.op) {
        case OP_GN_FINALIZE:
            return launch_gn_finalize((const float2*)at(L.part), pl.B, L.G, L.n_sp, L.n_nt, L.bn, L.cpg, L.C, L.count, L.gamma, L.beta, 1e-5f,
                                      (float2*)at(L.gn_ab), s);
        case OP_GN_ACT: return launch_gn_act(dtype, at(L.in), (const float2*)at(L.gn_ab), at(L.out), pl.B, L.HW, L.C, s);
        case OP_GN_ACT_FUSED:
            return launch_gn_act_fused(dtype, at(L.in), at(L.out), pl.B, L.HW, L.C, (const float2*)at(L.part), L.G, L.n_sp, L.n_nt, L.bn, L.cpg,
                                       L.count, L.gamma, L.beta, 1e-5f, s);
        default: break;
    }
    const ConvW& cw = h->convs[L.conv];
    ConvArgs k = L.a;
    k.in = cw.kind == KIND_STEM ? (const void*)c.x_in : at(L.in);
    if (cw.kind == KIND_HEAD) {
        k.x_state = c.x_state; k.eps_out = c.eps_out; k.do_ddim = c.do_ddim;
        k.c0 = c.c[0]; k.c1 = c.c[1]; k.c2 = c.c[2]; k.c3 = c.c[3]; k.noise = c.noise; k.sigma = c.sigma;
        k.x0_hist = c.x0_hist; k.c4 = c.c4; k.pred = c.pred;
    }
    if (L.op == OP_HEAD2) return launch_head2(k, (const float2*)at(L.gn_ab), h->head_w_f32, at(L.scratch), c.step, s);
    const int v = c.step % cw.nphase;
    k.w = v ? cw.w_ph[v - 1] : cw.w;
    k.wfrag = !L.frag ? nullptr : (v ? cw.wfrag_ph[v - 1] : cw.wfrag);
    k.out = at(L.out); k.res = at(L.res); k.part = (float2*)at(L.part); k.gn_ab = (const float2*)at(L.gn_ab);
    k.gs_part = (const float2*)at(L.gs_part); k.kpart = at(L.kpart); k.kflag = (unsigned*)at(L.kflag);
    k.fin_ab = (float2*)at(L.fin_ab); k.fin_counter = (unsigned*)at(L.fin_counter);
    if (L.film_off >= 0) k.film = (const float*)at(pl.film) + (size_t)c.step * pl.B * k.film_bstride + L.film_off;
    return launch_conv(dtype, cw.kind, cw.BN, k, s);
}

// ---- plan and binding caches ------------------------------------------------------------------------------
int check_shape(const ccn_handle_s* h, int B, int H, int W, int steps)
{
    if (B <= 0 || H <= 0 || W <= 0 || steps <= 0) return fail(CCN_EINVAL, "B, H, W, steps must be positive");
    const int div = 1 << h->cfg.n_mult;
    if (H % div || W % div) return fail(CCN_EINVAL, "H and W must be divisible by 2^len(ch_mult)");
    return CCN_OK;
}

// A Binding owns hipGraphExec objects whose replays may still be running on caller streams (two batches in flight in cli.eval /
// bench.py): drain the device before destroying any of them.
void drop_bindings(ccn_handle_s* h, size_t keep_newest)
{
    if (h->bindings.size() <= keep_newest) return;
    (void)hipDeviceSynchronize();
    while (h->bindings.size() > keep_newest) h->bindings.erase(h->bindings.begin());
}

// the plan of a shape on the committed model, built on first use (ccn_commit_params drops them all)
int shape_plan(ccn_handle_s* h, int B, int H, int W, int steps, const ShapePlan** out)
{
    if (int rc = check_shape(h, B, H, W, steps)) return rc;
    for (auto& p : h->shape_plans)
        if (p->B == B && p->H == H && p->W == W && p->steps == steps) { *out = p.get(); return CCN_OK; }
    std::unique_ptr<ShapePlan> p(new ShapePlan);
    p->B = B; p->H = H; p->W = W; p->steps = steps;
    if (int rc = build_plan(h, *p)) return rc;
    if (h->shape_plans.size() >= 64) { drop_bindings(h, 0); h->shape_plans.clear(); }    // a caller walking through shapes: start over
    *out = p.get();
    h->shape_plans.push_back(std::move(p));
    return CCN_OK;
}

int get_binding(ccn_handle_s* h, int B, int H, int W, int steps, void* ws, size_t ws_bytes, Binding** out)
{
    const ShapePlan* pl = nullptr;
    if (int rc = shape_plan(h, B, H, W, steps, &pl)) return rc;
    if (!ws || ((uintptr_t)ws & 255)) return fail(CCN_EWORKSPACE, "workspace must be non-null and 256-byte aligned");
    if (ws_bytes < pl->total) return fail(CCN_EWORKSPACE, "workspace too small: need " + std::to_string(pl->total));
    for (size_t i = 0; i < h->bindings.size(); ++i) {
        Binding* b = h->bindings[i].get();
        if (b->plan == pl && b->ws == ws) {
            // least recently used first: a hit moves the binding to the back, eviction (below) takes the front
            std::rotate(h->bindings.begin() + (long)i, h->bindings.begin() + (long)i + 1, h->bindings.end());
            *out = b;
            return CCN_OK;
        }
    }
    std::unique_ptr<Binding> b(new Binding);
    b->plan = pl; b->ws = (char*)ws;
    for (auto& z : pl->zero) HIPCHK(hipMemset(b->ws + z.first, 0, z.second));
    if (h->bindings.size() >= 8) drop_bindings(h, 7);
    *out = b.get();
    h->bindings.push_back(std::move(b));
    return CCN_OK;
}

}  // namespace
int ccn_release_workspace(ccn_handle_t h, void* workspace_dev)
{
    if (!h) return fail(CCN_EINVAL, "null handle");
    auto lives_there = [&](const std::unique_ptr<Binding>& b) { return b->ws == workspace_dev; };
    if (std::none_of(h->bindings.begin(), h->bindings.end(), lives_there)) return CCN_OK;
    HIPCHK(hipDeviceSynchronize());                                 // replays on caller streams may still be using it
    h->bindings.erase(std::remove_if(h->bindings.begin(), h->bindings.end(), lives_there), h->bindings.end());
    return CCN_OK;
}
namespace {

// ---- running a plan -------------------------------------------------------------------------------------------
// `go` enqueues one launch on `s`; while profiling it is bracketed by two events and booked under `family`
template <typename F>
int timed(ccn_handle_s* h, int family, double flops, double bytes, hipStream_t s, F&& go)
{
    if (!h->profiling) { HIPCHK(go()); return CCN_OK; }
    for (hipEvent_t e; h->ev_pool.size() < h->ev_used + 2; h->ev_pool.push_back(e)) HIPCHK(hipEventCreate(&e));
    const int e0 = (int)h->ev_used, e1 = e0 + 1;
    h->ev_used += 2;
    HIPCHK(hipEventRecord(h->ev_pool[e0], s));
    HIPCHK(go());
    HIPCHK(hipEventRecord(h->ev_pool[e1], s));
    h->recs.push_back({family, flops, bytes, e0, e1});
    return CCN_OK;
}

// one UNet evaluation (+ DDIM update in the head)
int run_ops(ccn_handle_s* h, const Binding* b, hipStream_t s, const StepCtx& c)
{
    for (const Launch& L : b->plan->ops) {
        if (int rc = timed(h, L.family, L.flops, L.bytes, s, [&] { return launch(h, *b->plan, L, b->ws, s, c); })) return rc;
    }
    return CCN_OK;
}

// conditioning for `TR` time rows and `FR` FiLM rows; sample: FR = S*B rows (s,b); forward: FR = B rows
int run_conditioning(ccn_handle_s* h, const Binding* b, hipStream_t s, const int64_t* t_i64, int TR, int FR, int a_div)
{
    const ccn_config_t& c = h->cfg; const ShapePlan& p = *b->plan;
    const int td = c.time_dim, B = p.B, F = h->arch.F;
    auto f32 = [b](size_t off) { return (float*)(b->ws + off); };
    float *temb = f32(p.temb), *t1 = f32(p.t1), *tp = f32(p.tp), *zp = f32(p.zp);
    int rc;
    if ((rc = timed(h, F_COND, 0, 0, s, [&] {
            return t_i64 ? launch_temb_i64(t_i64, temb, TR, td, s) : launch_temb_i32((const int32_t*)(b->ws + p.ts_dev), temb, TR, td, s); }))) return rc;
    if ((rc = timed(h, F_COND, 2.0 * TR * td * 4.0 * td, 0, s, [&] { return launch_linear(temb, nullptr, 1, TR, h->tp0_w, h->tp0_b, t1, TR, td, 4 * td, 1, s); }))) return rc;
    if ((rc = timed(h, F_COND, 2.0 * TR * td * 4.0 * td, 0, s, [&] { return launch_linear(t1, nullptr, 1, TR, h->tp2_w, h->tp2_b, tp, TR, 4 * td, td, 0, s); }))) return rc;
    if ((rc = timed(h, F_COND, 2.0 * B * c.z_dim * td, 0, s, [&] { return launch_linear(f32(p.zbuf), nullptr, 1, B, h->zp_w, h->zp_b, zp, B, c.z_dim, td, 1, s); }))) return rc;
    return timed(h, F_COND, 2.0 * FR * td * (double)F, 0, s, [&] { return launch_linear(tp, zp, a_div, B, h->film_w, h->film_b, f32(p.film), FR, td, F, 0, s); });
}

int run_steps(ccn_handle_s* h, const Binding* b, hipStream_t s, const SamplerRun& r)
{
    const ShapePlan& p = *b->plan;
    const size_t img = (size_t)(r.guided ? p.B / 2 : p.B) * h->cfg.img_ch * p.H * p.W;     // one state (and one step's draws)
    const bool ms = !r.c4.empty();
    float* xstate = (float*)(b->ws + p.xstate);
    for (int i = 0; i < r.steps; ++i) {
        const float* cf = r.coef.data() + i * 4;
        const float c4 = ms ? r.c4[i] : 0.f;
        const bool noisy = !r.sigma.empty() && (r.noise || r.seeds) && r.sigma[i] > 0.f;
        const float* nz = noisy && r.noise ? r.noise + (size_t)i * img : nullptr;
        const float sigma = noisy ? r.sigma[i] : 0.f;
        const uint64_t* seeds = noisy ? r.seeds : nullptr;          // this step's update generates draw 1 + i
        const bool thresholded = r.thr_p > 0.0;
        const bool lowres = r.lr_N > 0 && r.ts[i] >= r.lr_tmin;     // this step holds x0 to the guide
        const bool split = r.guided || seeds || thresholded || lowres;   // the head writes the raw output, a sampler-step launch updates
        StepCtx c;
        c.step = i; c.x_in = xstate; c.pred = r.pred;
        if (split) { c.x_state = nullptr; c.eps_out = r.out_scratch; c.do_ddim = 0; }
        else {
            c.x_state = xstate; c.eps_out = nullptr; c.do_ddim = 1;
            for (int k = 0; k < 4; ++k) c.c[k] = cf[k];
            if (noisy) { c.noise = nz; c.sigma = sigma; }
            if (ms) { c.x0_hist = r.hist; c.c4 = c4; }
        }
        if (int rc = run_ops(h, b, s, c)) return rc;
        if (!split) continue;
        // guided: the combine and the update of both halves (unguided, the update is the head kernel's epilogue)
        // (unguided with seeds, a noisy step: the same launch without the second half -- 3 passes over one state)
        // (thresholded: the same launch with the record's threshold; the noise tensor and the history enter as in the head's epilogue)
        const double passes = r.guided ? 5 + (nz ? 1 : 0) + (ms ? (c4 != 0.f ? 2 : 1) : 0)
                                       : 3 + (thresholded || lowres ? (nz ? 1 : 0) + (ms ? (c4 != 0.f ? 2 : 1) : 0) : 0);
        // the operands of this step's x0, named once for the (up to) four launches that form it
        SamplerStep u;
        X0Operands& o = u.o;
        o.x = xstate; o.out_c = r.out_scratch; o.gscale = r.gscale; o.thr = r.thr; o.pred = r.pred; o.w = r.w; o.c0 = cf[0]; o.c1 = cf[1];
        o.per_record = (int64_t)h->cfg.img_ch * p.H * p.W; o.records = (int64_t)img / o.per_record;
        u.hist = r.hist; u.noise = nz;
        if (r.guided) { u.x_dup = xstate + img; o.out_u = r.out_scratch + img; }
        u.c2 = cf[2]; u.c3 = cf[3]; u.c4 = c4; u.sigma = sigma;
        u.seeds = seeds; u.draw = 1u + (uint32_t)i;
        // guidance rescale: the factor of every record, one read of both halves of the output scratch
        if (r.rs_phi > 0.0)
            if (int rc = timed(h, F_HEAD, 0, (double)img * 4 * 2, s, [&] { return launch_guidance_rescale(o, r.rs_phi, r.gscale, r.rs_part, s); }))
                return rc;
        // the quantile of |x0| per record, on the combined output when guided: three select passes over the state and the output(s)
        if (thresholded)
            if (int rc = timed(h, F_HEAD, 0, (double)img * 4 * 3 * (r.guided ? 3 : 2), s, [&] {
                    return launch_x0_threshold(o, r.thr_p, r.thr_max, r.thr, r.thr_sel, s); })) return rc;
        // the low-resolution guide: the correction of every block, one read of the state and the output(s)
        if (lowres) {
            u.delta = r.lr_delta; u.lr_W = p.W; u.lr_N = r.lr_N;
            if (int rc = timed(h, F_HEAD, 0, (double)img * 4 * (r.guided ? 3 : 2), s, [&] {
                    return launch_lowres_delta(o, h->cfg.img_ch, p.H, p.W, r.lr_N, r.lr_guide, r.lr_strength, r.lr_delta, s); })) return rc;
        }
        if (int rc = timed(h, F_HEAD, 0, (double)img * 4 * passes, s, [&] { return launch_sampler_step(u, s); })) return rc;
    }
    return CCN_OK;
}

// sticky device-side failure (a kernel ORed into the error word since the last check): report once, then clear
int check_device_errors(ccn_handle_s* h)
{
    if (!h->err_host) return CCN_OK;
    const unsigned e = __atomic_exchange_n(h->err_host, 0u, __ATOMIC_RELAXED);
    if (e & 1u)
        return fail(CCN_EHIP, "device-side hand-off timeout: a split-K partial tile never arrived; the results of the launches enqueued "
                              "since the last successful check are invalid");
    if (e & 2u)
        return fail(CCN_EHIP, "split-K partners ran on different XCDs (the hand-off took the agent-scope path: results are valid, but the "
                              "placement assumption of launch_conv_pr does not hold on this device / partition mode)");
    if (e & 4u)
        return fail(CCN_EHIP, "f16x3: an activation left the fp16 operand range (|x| >= 65520) and was saturated; the results of the "
                              "launches enqueued since the last successful check are not fp32-grade: use dtype fp32 for this model");
    if (e) return fail(CCN_EHIP, "device-side error word " + std::to_string(e));
    return CCN_OK;
}

// a report of a test hook, snprintf-like: writes at most cap bytes (NUL-terminated) and returns the length of the whole text
int copy_report(const std::string& text, char* buf, size_t cap)
{
    if (buf && cap) {
        const size_t n = std::min(text.size(), cap - 1);
        std::memcpy(buf, text.data(), n);
        buf[n] = 0;
    }
    return (int)text.size();
}

// instantiations = true: the kernel word of a launch that runs a fixed-geometry instantiation is that instantiation's name ("pr:...")
std::string routes_text(const ShapePlan& pl, bool instantiations = false)
{
    static const char* kinds[] = {"C3S1", "C3S2", "CT4", "STEM", "HEAD"};
    std::string text;
    for (const RouteRec& r : pl.routes) {
        char line[256];
        std::snprintf(line, sizeof(line), "%s %s %s th=%d ksplit=%d n_nt=%d gn=%s film=%d res=%d", r.name.c_str(), kinds[r.kind], instantiations && r.geom ? r.geom : r.kernel,
                      r.th, r.ksplit, r.n_nt, r.gn, r.film ? 1 : 0, r.res ? 1 : 0);
        text += std::string(line) + (r.ops < 0 ? "" : r.ops ? " ops=f16x3" : " ops=f32") + "\n";
    }
    return text;
}

int check_ready(ccn_handle_s* h)
{
    if (!h) return fail(CCN_EINVAL, "null handle");
    if (!h->committed) return fail(CCN_ESTATE, "ccn_commit_params has not succeeded on this handle");
    return check_device_errors(h);
}

}  // namespace

// =================================================================================================================
extern "C" {

const char* ccn_last_error(void) { return g_err.c_str(); }
#ifdef CCN_DIAG
const char* ccn_version(void) { return "ccn_hip 0.3 (gfx950, diagnostics build)"; }
#else
const char* ccn_version(void) { return "ccn_hip 0.3 (gfx950)"; }
#endif

int ccn_create(const ccn_config_t* cfg, ccn_handle_t* out)
{
    if (!cfg || !out) return fail(CCN_EINVAL, "null argument");
    if (cfg->n_mult < 1 || cfg->n_mult > CCN_MAX_MULT) return fail(CCN_EINVAL, "n_mult out of range");
    if (cfg->dtype != CCN_DTYPE_F32 && cfg->dtype != CCN_DTYPE_BF16 && cfg->dtype != CCN_DTYPE_F16X3) return fail(CCN_EINVAL, "unknown dtype");
    if (cfg->base <= 0 || cfg->base % 8) return fail(CCN_EINVAL, "base must be a positive multiple of 8");
    if (cfg->img_ch < 1 || cfg->img_ch * 9 > 32) return fail(CCN_EINVAL, "img_ch must be 1..3");
    if (cfg->time_dim <= 0 || cfg->z_dim <= 0 || cfg->groups <= 0) return fail(CCN_EINVAL, "bad dims");
    int ch = cfg->base;
    for (int i = 0; i < cfg->n_mult; ++i) {
        if (cfg->ch_mult[i] < 1) return fail(CCN_EINVAL, "ch_mult entries must be >= 1");
        if ((long)ch * cfg->ch_mult[i] > (1 << 16)) return fail(CCN_EINVAL, "channel width (running product of ch_mult, models/unet.py:64) above 65536");
        ch *= cfg->ch_mult[i];
    }
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev <= 0) return fail(CCN_EHIP, "no HIP device");
    std::unique_ptr<ccn_handle_s> h(new ccn_handle_s);
    h->cfg = *cfg;
    // f16x3 is the fp32 mode in every respect but the operands of the ws / fr kernels: the plan, the workspace and every other
    // kernel are chosen by the storage type
    h->split = cfg->dtype == CCN_DTYPE_F16X3;
    if (h->split) h->cfg.dtype = CCN_DTYPE_F32;
    h->elem = cfg->dtype == CCN_DTYPE_BF16 ? 2 : 4;
    h->G = cfg->groups;
    h->arch = build_arch(h->cfg);
    h->convs.assign(h->arch.convs.begin(), h->arch.convs.end());
    h->res.resize(h->arch.res.size());
    for (auto& r : h->arch.res)
        if (r.C % (r.C < h->G ? r.C : h->G)) return fail(CCN_EINVAL, "channel count not divisible by GroupNorm groups");
    HIPCHK(conv_prepare());
    HIPCHK(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
    HIPCHK(hipHostMalloc((void**)&h->err_host, 64, hipHostMallocMapped));
    *h->err_host = 0u;
    HIPCHK(hipHostGetDevicePointer((void**)&h->err_dev, h->err_host, 0));
    for (int i = 0; i < F_COUNT; ++i) h->fam_names.push_back(kFamilies[i]);
    *out = h.release();
    return CCN_OK;
}

int ccn_destroy(ccn_handle_t h)
{
    if (!h) return CCN_OK;
    (void)hipDeviceSynchronize();
    h->bindings.clear();
    for (void* p : h->dev_allocs) (void)hipFree(p);
    for (auto e : h->ev_pool) (void)hipEventDestroy(e);
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    if (h->err_host) (void)hipHostFree(h->err_host);
    delete h;
    return CCN_OK;
}

int ccn_num_params(ccn_handle_t h, int32_t* n)
{
    if (!h || !n) return fail(CCN_EINVAL, "null argument");
    *n = (int32_t)h->arch.params.size();
    return CCN_OK;
}

int ccn_param_info(ccn_handle_t h, int32_t i, const char** name, int64_t shape[4], int32_t* ndim)
{
    if (!h || !name || !shape || !ndim) return fail(CCN_EINVAL, "null argument");
    if (i < 0 || i >= (int32_t)h->arch.params.size()) return fail(CCN_EINVAL, "parameter index out of range");
    const ArchParam& p = h->arch.params[i];
    *name = p.name.c_str();
    *ndim = (int32_t)p.shape.size();
    for (size_t k = 0; k < 4; ++k) shape[k] = k < p.shape.size() ? p.shape[k] : 1;
    return CCN_OK;
}

int ccn_load_param(ccn_handle_t h, const char* name, const float* data, const int64_t* shape, int32_t ndim)
{
    if (!h || !name || !data || !shape) return fail(CCN_EINVAL, "null argument");
    const ArchParam* pi = nullptr;
    for (auto& p : h->arch.params) if (p.name == name) { pi = &p; break; }
    if (!pi) return fail(CCN_EWEIGHTS, std::string("Unexpected key in state_dict: ") + name);
    if ((size_t)ndim != pi->shape.size()) return fail(CCN_EWEIGHTS, std::string("size mismatch for ") + name);
    for (int k = 0; k < ndim; ++k)
        if (shape[k] != pi->shape[k]) return fail(CCN_EWEIGHTS, std::string("size mismatch for ") + name);
    std::vector<float> buf(pi->numel());
    hipPointerAttribute_t attr;
    const hipError_t pe = hipPointerGetAttributes(&attr, data);
    if (pe == hipSuccess && attr.type == hipMemoryTypeDevice) {
        HIPCHK(hipMemcpy(buf.data(), data, buf.size() * 4, hipMemcpyDeviceToHost));
    } else {
        (void)hipGetLastError();
        std::memcpy(buf.data(), data, buf.size() * 4);
    }
    h->host[name] = std::move(buf);
    h->committed = false;
    return CCN_OK;
}

int ccn_set_weight_rounding(ccn_handle_t h, int32_t mode)
{
    if (!h) return fail(CCN_EINVAL, "null handle");
    if (mode != CCN_ROUND_NEAREST && mode != CCN_ROUND_DIFFUSED && mode != CCN_ROUND_DIFFUSED_PHASES) return fail(CCN_EINVAL, "unknown weight rounding mode");
    h->weight_rounding = mode;
    return CCN_OK;
}

int ccn_set_prediction(ccn_handle_t h, int32_t pred)
{
    if (!h) return fail(CCN_EINVAL, "null handle");
    if (pred != CCN_PRED_EPS && pred != CCN_PRED_V) return fail(CCN_EINVAL, "unknown prediction (CCN_PRED_EPS or CCN_PRED_V)");
    h->pred = pred;
    return CCN_OK;
}

// what the three handle features below need of a run's state, B records of img_ch x H x W: check_x0_operands without the pointers
static int check_state_shape(const ccn_handle_s* h, int32_t B, int32_t H, int32_t W, bool for_rescale, int64_t& per)
{
    if (H <= 0 || W <= 0) return fail(CCN_EINVAL, "B, H, W must be positive");
    X0Operands o;
    o.records = B; o.per_record = per = (int64_t)h->cfg.img_ch * H * W;
    return check_x0_operands(o, for_rescale, false);
}

// Dynamic thresholding is handle state: every ccn_sample* entry picks it up here.  The scratch of ccn_set_dynamic_threshold is cut
// into [raw output of one state | B thresholds | select state], each part 16-byte aligned (threshold_scratch_layout).
struct ThrLayout { size_t thr, sel, total; };
static int threshold_scratch_layout(const ccn_handle_s* h, int32_t B, int32_t H, int32_t W, ThrLayout& l)
{
    int64_t per;
    if (int rc = check_state_shape(h, B, H, W, false, per)) return rc;
    l.thr = ((size_t)B * (size_t)per * 4 + 15) / 16 * 16;
    l.sel = l.thr + ((size_t)B * 4 + 15) / 16 * 16;
    l.total = l.sel + x0_threshold_scratch_bytes(B);
    return CCN_OK;
}

int ccn_set_dynamic_threshold(ccn_handle_t h, double p, float max_value, void* scratch_dev, size_t scratch_bytes)
{
    // the arguments first (they can be judged without a handle), then the handle
    if (!(p >= 0.0 && p <= 1.0)) return fail(CCN_EINVAL, "the quantile p must be in [0, 1] (0: off)");
    if (p > 0.0) {
        if (!(max_value >= 1.0f)) return fail(CCN_EINVAL, "max_value must be at least 1 (+inf: no upper bound)");
        if (!scratch_dev || ((uintptr_t)scratch_dev & 15)) return fail(CCN_EINVAL, "the dynamic-threshold scratch must be non-null and 16-byte aligned");
        // the smallest shape there is (one record of one element): a scratch below that fits no call
        if (scratch_bytes < 32 + x0_threshold_scratch_bytes(1))
            return fail(CCN_EINVAL, "the dynamic-threshold scratch is too small (ccn_dynamic_threshold_scratch_bytes)");
    }
    if (!h) return fail(CCN_EINVAL, "null handle");
    if (p == 0.0) { h->thr_p = 0.0; h->thr_max = 0.f; h->thr_scratch = nullptr; h->thr_scratch_bytes = 0; return CCN_OK; }
    h->thr_p = p; h->thr_max = max_value; h->thr_scratch = (char*)scratch_dev; h->thr_scratch_bytes = scratch_bytes;
    return CCN_OK;
}

int ccn_dynamic_threshold_scratch_bytes(ccn_handle_t h, int32_t B, int32_t H, int32_t W, size_t* bytes)
{
    if (!h) return fail(CCN_EINVAL, "null handle");
    if (!bytes) return fail(CCN_EINVAL, "null argument");
    ThrLayout l;
    if (int rc = threshold_scratch_layout(h, B, H, W, l)) return rc;
    *bytes = l.total;
    return CCN_OK;
}

// Guidance rescale is handle state likewise.  The scratch of ccn_set_guidance_rescale is the one of ccn_guidance_rescale: the B
// factors first, then the partial sums.
int ccn_set_guidance_rescale(ccn_handle_t h, double phi, void* scratch_dev, size_t scratch_bytes)
{
    // the arguments first (they can be judged without a handle), then the handle
    if (!(phi >= 0.0 && phi <= 1.0)) return fail(CCN_EINVAL, "the rescale factor phi must be in [0, 1] (0: off)");
    if (phi > 0.0) {
        if (!scratch_dev || ((uintptr_t)scratch_dev & 15)) return fail(CCN_EINVAL, "the guidance-rescale scratch must be non-null and 16-byte aligned");
        // the smallest shape there is (one record of two elements): a scratch below that fits no call
        if (scratch_bytes < guidance_rescale_scratch_bytes(1, 2))
            return fail(CCN_EINVAL, "the guidance-rescale scratch is too small (ccn_guidance_rescale_scratch_bytes)");
    }
    if (!h) return fail(CCN_EINVAL, "null handle");
    if (phi == 0.0) { h->rs_phi = 0.0; h->rs_scratch = nullptr; h->rs_scratch_bytes = 0; return CCN_OK; }
    h->rs_phi = phi; h->rs_scratch = (char*)scratch_dev; h->rs_scratch_bytes = scratch_bytes;
    return CCN_OK;
}

// The low-resolution guide is handle state likewise.  The scratch of ccn_set_lowres_guide is cut into [delta table | raw output of one
// state], each part 16-byte aligned (lowres_scratch_layout).
struct LrLayout { size_t raw, total; };
static int lowres_scratch_layout(const ccn_handle_s* h, int32_t B, int32_t H, int32_t W, int32_t N, LrLayout& l)
{
    if (int rc = guide_check(H, W, N)) return rc;
    int64_t per;
    if (int rc = check_state_shape(h, B, H, W, false, per)) return rc;
    l.raw = ((size_t)B * (size_t)(per / N / N) * 4 + 15) / 16 * 16;
    l.total = l.raw + ((size_t)B * (size_t)per * 4 + 15) / 16 * 16;
    return CCN_OK;
}

int ccn_set_lowres_guide(ccn_handle_t h, const float* guide_dev, int32_t N, float strength, int32_t t_min, void* scratch_dev, size_t scratch_bytes)
{
    // the arguments first (they can be judged without a handle), then the handle
    if (N != 0) {
        if (N < 2 || N > 64 || (N & (N - 1))) return fail(CCN_EINVAL, "N must be a power of two in 2..64 (0: off)");
        if (!guide_dev) return fail(CCN_EINVAL, "the guide is NULL");
        if (!(strength > 0.0f && strength <= 1.0f)) return fail(CCN_EINVAL, "the guide strength must be in (0, 1]");
        if (t_min < 0) return fail(CCN_EINVAL, "t_min must not be negative");
        if (!scratch_dev || ((uintptr_t)scratch_dev & 15)) return fail(CCN_EINVAL, "the low-resolution-guide scratch must be non-null and 16-byte aligned");
        // the smallest shape there is (one record of one block of one channel): a scratch below that fits no call
        if (scratch_bytes < 16 + (size_t)N * N * 4)
            return fail(CCN_EINVAL, "the low-resolution-guide scratch is too small (ccn_lowres_guide_scratch_bytes)");
    }
    if (!h) return fail(CCN_EINVAL, "null handle");
    if (N == 0) { h->lr_guide = nullptr; h->lr_N = 0; h->lr_strength = 0.f; h->lr_tmin = 0; h->lr_scratch = nullptr; h->lr_scratch_bytes = 0; return CCN_OK; }
    h->lr_guide = guide_dev; h->lr_N = N; h->lr_strength = strength; h->lr_tmin = t_min;
    h->lr_scratch = (char*)scratch_dev; h->lr_scratch_bytes = scratch_bytes;
    return CCN_OK;
}

int ccn_lowres_guide_scratch_bytes(ccn_handle_t h, int32_t B, int32_t H, int32_t W, int32_t N, size_t* bytes)
{
    if (!h) return fail(CCN_EINVAL, "null handle");
    if (!bytes) return fail(CCN_EINVAL, "null argument");
    LrLayout l;
    if (int rc = lowres_scratch_layout(h, B, H, W, N, l)) return rc;
    *bytes = l.total;
    return CCN_OK;
}

int ccn_commit_params(ccn_handle_t h)
{
    if (!h) return fail(CCN_EINVAL, "null handle");
    const Arch& a = h->arch;
    std::string missing;
    for (auto& p : a.params)
        if (!h->host.count(p.name)) missing += (missing.empty() ? "" : ", ") + p.name;
    if (!missing.empty()) return fail(CCN_EWEIGHTS, "Missing key(s) in state_dict: " + missing);
    drop_bindings(h, 0);                                          // drains the device first: replays may still read the old weights
    h->shape_plans.clear();                                       // they hold what this commit decides: BN, fragment operands, split rows
    for (void* p : h->dev_allocs) (void)hipFree(p);
    h->dev_allocs.clear();
    const ccn_config_t& c = h->cfg;
    int rc;
    // bf16 mode rounds the conv weights with error diffusion (round_version) unless CCN_ROUND_NEAREST asks for the packers' own
    // independent rounding; CCN_ROUND_DIFFUSED is one version.  h->host is only read: a commit that fails half-way leaves the loaded
    // weights as they were.  Per conv, one version at a time is formed, packed, uploaded and dropped again.
    const bool diffuse = c.dtype == CCN_DTYPE_BF16 && h->weight_rounding != CCN_ROUND_NEAREST;
    h->nphase = diffuse && h->weight_rounding == CCN_ROUND_DIFFUSED_PHASES ? phases_for(h) : 1;
    for (size_t ci = 0; ci < a.convs.size(); ++ci) {
        ConvW& cw = h->convs[ci] = ConvW(a.convs[ci]);
        const std::vector<float>&w = host_param(h, cw.pw), &b = host_param(h, cw.pb);
        if ((rc = upload_f32(h, cw.pb, &cw.bias))) return rc;
        // (the head keeps fp32 weights: head_prep_kernel scales them per sample and rounds them with a carry along the steps)
        const bool dif = diffuse && cw.kind != KIND_HEAD;
        cw.nphase = dif ? h->nphase : 1;
        std::vector<double> sum(dif ? w.size() : 0, 0.0);
        std::vector<float> wk(dif ? w.size() : 0);
        for (int k = 0; k < cw.nphase; ++k) {
            if (dif) round_version(w.data(), w.size(), cw.kind == KIND_CT4, cw.Cout, cw.Cin, cw.kind == KIND_CT4 ? 16 : 9, k, sum.data(), wk.data());
            if ((rc = pack_conv(h, cw, dif ? wk.data() : w.data(), b.data(), k ? &cw.w_ph[k - 1] : &cw.w, k ? &cw.wfrag_ph[k - 1] : &cw.wfrag))) return rc;
        }
        if (cw.kind == KIND_HEAD && (rc = upload_f32(h, cw.pw, &h->head_w_f32))) return rc;
    }
    for (size_t ri = 0; ri < a.res.size(); ++ri) {
        const ArchRes& r = a.res[ri];
        ResW& rw = h->res[ri];
        rw.n1.C = rw.n2.C = r.C;
        if ((rc = upload_f32(h, r.n1.pg, &rw.n1.gamma))) return rc;
        if ((rc = upload_f32(h, r.n1.pb, &rw.n1.beta))) return rc;
        if ((rc = upload_f32(h, r.n2.pg, &rw.n2.gamma))) return rc;
        if ((rc = upload_f32(h, r.n2.pb, &rw.n2.beta))) return rc;
    }
    h->out_norm.C = a.out_norm.C;
    if ((rc = upload_f32(h, a.out_norm.pg, &h->out_norm.gamma))) return rc;
    if ((rc = upload_f32(h, a.out_norm.pb, &h->out_norm.beta))) return rc;
    if ((rc = upload_f32(h, a.tp0.pw, &h->tp0_w))) return rc;
    if ((rc = upload_f32(h, a.tp0.pb, &h->tp0_b))) return rc;
    if ((rc = upload_f32(h, a.tp2.pw, &h->tp2_w))) return rc;
    if ((rc = upload_f32(h, a.tp2.pb, &h->tp2_b))) return rc;
    if ((rc = upload_f32(h, a.zp.pw, &h->zp_w))) return rc;
    if ((rc = upload_f32(h, a.zp.pb, &h->zp_b))) return rc;
    // all FiLM linears as one (F x time_dim) matrix: per block [to_scale rows | to_shift rows]
    std::vector<float> fw((size_t)a.F * c.time_dim), fb((size_t)a.F);
    for (auto& r : a.res) {
        const ArchLin* parts[2] = {&r.fs, &r.fh};
        for (int q = 0; q < 2; ++q) {
            const auto& w = host_param(h, parts[q]->pw);
            const auto& b = host_param(h, parts[q]->pb);
            std::memcpy(&fw[(size_t)(r.film_off + q * r.C) * c.time_dim], w.data(), w.size() * 4);
            std::memcpy(&fb[(size_t)(r.film_off + q * r.C)], b.data(), b.size() * 4);
        }
    }
    if ((rc = upload(h, fw.data(), fw.size() * 4, (void**)&h->film_w))) return rc;
    if ((rc = upload(h, fb.data(), fb.size() * 4, (void**)&h->film_b))) return rc;
    HIPCHK(hipDeviceSynchronize());
    h->host.clear();
    h->committed = true;
    return CCN_OK;
}

int ccn_workspace_bytes(ccn_handle_t h, int32_t B, int32_t H, int32_t W, int32_t steps, size_t* bytes)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!bytes) return fail(CCN_EINVAL, "null argument");
    const ShapePlan* pl = nullptr;
    if ((rc = shape_plan(h, B, H, W, steps, &pl))) return rc;
    *bytes = pl->total;
    return CCN_OK;
}

int ccn_forward(ccn_handle_t h, const float* x_dev, const float* z_dev, const int64_t* t_dev, float* eps_dev,
                int32_t B, int32_t H, int32_t W, void* workspace_dev, size_t workspace_bytes, void* stream)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!x_dev || !z_dev || !t_dev || !eps_dev) return fail(CCN_EINVAL, "null tensor pointer");
    Binding* b = nullptr;
    if ((rc = get_binding(h, B, H, W, 1, workspace_dev, workspace_bytes, &b))) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(hipMemcpyAsync(b->ws + b->plan->zbuf, z_dev, (size_t)B * h->cfg.z_dim * 4, hipMemcpyDeviceToDevice, s));
    if ((rc = run_conditioning(h, b, s, t_dev, B, B, 1))) return rc;
    StepCtx c;
    c.step = 0; c.x_in = x_dev; c.x_state = nullptr; c.eps_out = eps_dev; c.do_ddim = 0;
    return run_ops(h, b, s, c);
}

// (handle, descriptor, shape) -> the run: every check of the descriptor, the host tables copied, the handle's prediction, dynamic
// threshold, guidance rescale and low-resolution guide read -- here and nowhere else -- and every unused field at its fixed value
// (SamplerRun)
static int build_run(ccn_handle_t h, const ccn_sampler_run_t* d, int32_t B, int32_t H, int32_t W, SamplerRun& r)
{
    if (!d) return fail(CCN_EINVAL, "null sampler run descriptor");
    if (d->size != sizeof(ccn_sampler_run_t))
        return fail(CCN_EINVAL, "ccn_sampler_run_t: size " + std::to_string(d->size) + ", this library's is " + std::to_string(sizeof(ccn_sampler_run_t)));
    const bool ms = d->coef_cols == 5, guided = d->guided != 0;
    if (d->coef_cols != 4 && !ms) return fail(CCN_EINVAL, "coef_cols must be 4 or 5");
    if (d->steps <= 0) return fail(CCN_EINVAL, "B, H, W, steps must be positive");
    if (!d->ts_host || !d->coef_host) return fail(CCN_EINVAL, "null pointer");
    if (ms && (d->sigma_host || d->noise_dev || d->seeds_dev))
        return fail(CCN_EINVAL, "a fifth coefficient column with sigma, noise or seeds: no ccn_sample* entry expresses this run");
    if (d->noise_dev && d->seeds_dev) return fail(CCN_EINVAL, "noise_dev with seeds_dev: no ccn_sample* entry expresses this run");
    if (d->sigma_host ? !d->noise_dev && !d->seeds_dev : d->noise_dev != nullptr) return fail(CCN_EINVAL, "sigma and noise must be given together");
    if ((uintptr_t)d->seeds_dev & 7) return fail(CCN_EINVAL, "the seeds must be 8-byte aligned");
    const uint64_t* seeds = d->sigma_host ? d->seeds_dev : nullptr;
    if (guided && !std::isfinite(d->w)) return fail(CCN_EINVAL, "the guidance scale must be finite");
    if (guided && (B <= 0 || B > INT32_MAX / 2)) return fail(CCN_EINVAL, "B, H, W, steps must be positive");
    if ((guided || seeds) && (!d->out_scratch_dev || ((uintptr_t)d->out_scratch_dev & 15)))
        return fail(CCN_EINVAL, "the output scratch (guided: eps scratch) must be non-null and 16-byte aligned");
    if (ms && (!d->x0_hist_dev || ((uintptr_t)d->x0_hist_dev & 15))) return fail(CCN_EINVAL, "the x0 history must be non-null and 16-byte aligned");
    const size_t n = (size_t)d->steps, cols = (size_t)d->coef_cols;
    for (size_t i = 0; ms && i < n * 5; ++i)
        if (!std::isfinite(d->coef_host[i])) return fail(CCN_EINVAL, "non-finite sampler coefficient");
    if (ms && d->coef_host[4] != 0.f) return fail(CCN_EINVAL, "c4 must be 0 on step 0: there is no x0 history yet");
    if (int rc = check_ready(h)) return rc;
    if (d->seeds_dev && H > 0 && W > 0 && (int64_t)h->cfg.img_ch * H * W >= kDrawMaxPerRecord)
        return fail(CCN_EINVAL, "a record of 2^34 elements or more cannot be drawn");

    r.steps = d->steps; r.pred = h->pred;
    r.ts.assign(d->ts_host, d->ts_host + n);
    r.coef.resize(n * 4);
    for (size_t i = 0; i < n; ++i) std::copy_n(d->coef_host + i * cols, 4, r.coef.begin() + i * 4);
    for (size_t i = 0; ms && i < n; ++i) r.c4.push_back(d->coef_host[i * 5 + 4]);
    if (d->sigma_host) { r.sigma.assign(d->sigma_host, d->sigma_host + n); r.noise = d->noise_dev; r.seeds = seeds; }
    if (guided) { r.guided = true; r.w = d->w; r.z_null = d->z_null_dev; }
    if (ms) r.hist = d->x0_hist_dev;
    if (guided || seeds) r.out_scratch = d->out_scratch_dev;
    if (h->thr_p > 0.0) {
        ThrLayout l;
        if (int rc = threshold_scratch_layout(h, B, H, W, l)) return rc;
        if (h->thr_scratch_bytes < l.total)
            return fail(CCN_EINVAL, "the dynamic-threshold scratch is too small for this shape: need " + std::to_string(l.total) + " bytes");
        r.thr_p = h->thr_p; r.thr_max = h->thr_max;
        r.thr = (float*)(h->thr_scratch + l.thr); r.thr_sel = h->thr_scratch + l.sel;
        if (!r.out_scratch) r.out_scratch = (float*)h->thr_scratch;   // a run without a scratch of its own: the head of the handle's
    }
    if (h->rs_phi > 0.0 && guided) {                                // (an unguided run ignores it: there is nothing to match)
        int64_t per;
        if (int rc = check_state_shape(h, B, H, W, true, per)) return rc;
        const size_t need = guidance_rescale_scratch_bytes(B, per);
        if (h->rs_scratch_bytes < need)
            return fail(CCN_EINVAL, "the guidance-rescale scratch is too small for this shape: need " + std::to_string(need) + " bytes");
        r.rs_phi = h->rs_phi; r.gscale = (float*)h->rs_scratch; r.rs_part = guidance_rescale_partials(h->rs_scratch, B);
    }
    if (h->lr_N > 0) {
        LrLayout l;
        if (int rc = lowres_scratch_layout(h, B, H, W, h->lr_N, l)) return rc;
        if (h->lr_scratch_bytes < l.total)
            return fail(CCN_EINVAL, "the low-resolution-guide scratch is too small for this shape: need " + std::to_string(l.total) + " bytes");
        r.lr_guide = h->lr_guide; r.lr_N = h->lr_N; r.lr_strength = h->lr_strength; r.lr_tmin = h->lr_tmin;
        r.lr_delta = (float*)h->lr_scratch;
        if (!r.out_scratch) r.out_scratch = (float*)(h->lr_scratch + l.raw);   // no guided, seeded or threshold scratch owns the raw output
    }
    return CCN_OK;
}

int ccn_sample_run(ccn_handle_t h, const ccn_sampler_run_t* run, const float* z_dev, const float* x_T_dev, float* x_out_dev, int32_t B, int32_t H,
                   int32_t W, void* workspace_dev, size_t workspace_bytes, void* stream, int32_t use_graph)
{
    int rc;
    SamplerRun r;
    if ((rc = build_run(h, run, B, H, W, r))) return rc;
    if (!z_dev || !x_T_dev || !x_out_dev) return fail(CCN_EINVAL, "null pointer");
    const int PB = r.guided ? 2 * B : B;                            // the plan's batch: guided, the two halves
    const int steps = r.steps;
    Binding* p = nullptr;
    if ((rc = get_binding(h, PB, H, W, steps, workspace_dev, workspace_bytes, &p))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t img_bytes = (size_t)B * h->cfg.img_ch * H * W * 4, z_row = (size_t)h->cfg.z_dim * 4;
    float* xstate = (float*)(p->ws + p->plan->xstate);
    char* zbuf = p->ws + p->plan->zbuf;
    HIPCHK(hipMemcpyAsync(zbuf, z_dev, (size_t)B * z_row, hipMemcpyDeviceToDevice, s));
    if (r.guided && !r.z_null) HIPCHK(hipMemsetAsync(zbuf + (size_t)B * z_row, 0, (size_t)B * z_row, s));
    if (r.guided && r.z_null) {
        // the null row B times: once from the caller, then doubling from the rows already there
        char* zn = zbuf + (size_t)B * z_row;
        HIPCHK(hipMemcpyAsync(zn, r.z_null, z_row, hipMemcpyDeviceToDevice, s));
        for (int have = 1; have < B; have *= 2)
            HIPCHK(hipMemcpyAsync(zn + (size_t)have * z_row, zn, (size_t)std::min(have, B - have) * z_row, hipMemcpyDeviceToDevice, s));
    }
    if (x_T_dev != xstate) HIPCHK(hipMemcpyAsync(xstate, x_T_dev, img_bytes, hipMemcpyDeviceToDevice, s));
    if (r.guided) HIPCHK(hipMemcpyAsync((char*)xstate + img_bytes, xstate, img_bytes, hipMemcpyDeviceToDevice, s));

    // the timestep table of a binding almost never changes: upload it only when it does, and then synchronously after draining
    // the stream (an async copy out of a host vector that the next call rewrites could still be pending)
    if (p->ts_keep != r.ts) {
        HIPCHK(hipStreamSynchronize(s));
        p->ts_keep = r.ts;
        HIPCHK(hipMemcpy(p->ws + p->plan->ts_dev, p->ts_keep.data(), (size_t)steps * 4, hipMemcpyHostToDevice));
    }
    if (use_graph && !h->profiling) {
        GraphEntry* ge = nullptr;
        for (auto& g : p->graphs)
            if (g.run.same_graph(r)) { ge = &g; break; }
        if (!ge) {
            GraphEntry g;
            g.run = r;
            HIPCHK(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeRelaxed));
            rc = run_conditioning(h, p, h->cap_stream, nullptr, steps, steps * PB, PB);
            if (!rc) rc = run_steps(h, p, h->cap_stream, r);
            hipGraph_t graph = nullptr;
            const hipError_t ce = hipStreamEndCapture(h->cap_stream, &graph);
            if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
            if (ce != hipSuccess) return fail(CCN_EHIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
            g.graph = graph;
            HIPCHK(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
            ++h->captures;
            // at most kMaxGraphsPerBinding captured graphs per binding, least recently used first (a caller that passes a fresh noise
            // tensor / coefficient table every call would otherwise grow the list without bound); an exec may still be replaying
            // on a caller stream, so the device is drained before one is destroyed
            if (p->graphs.size() >= kMaxGraphsPerBinding) {
                HIPCHK(hipDeviceSynchronize());
                p->graphs.front().destroy();
                p->graphs.erase(p->graphs.begin());
            }
            p->graphs.push_back(g);
            ge = &p->graphs.back();
        } else if (ge != &p->graphs.back()) {
            std::rotate(p->graphs.begin() + (ge - p->graphs.data()), p->graphs.begin() + (ge - p->graphs.data()) + 1, p->graphs.end());
            ge = &p->graphs.back();
        }
        HIPCHK(hipGraphLaunch(ge->exec, s));
    } else {
        if ((rc = run_conditioning(h, p, s, nullptr, steps, steps * PB, PB))) return rc;
        if ((rc = run_steps(h, p, s, r))) return rc;
    }
    if (x_out_dev != xstate) HIPCHK(hipMemcpyAsync(x_out_dev, xstate, img_bytes, hipMemcpyDeviceToDevice, s));
    return CCN_OK;
}

// The seven fixed-shape entries: each fills a descriptor from its arguments, keeps the checks the descriptor cannot express (an entry
// that insists on a pointer its run may not use), and calls ccn_sample_run.
static ccn_sampler_run_t run_of(int32_t steps, const int32_t* ts_host, const float* coef_host, int32_t coef_cols)
{
    ccn_sampler_run_t d{};
    d.size = sizeof(d); d.steps = steps; d.ts_host = ts_host; d.coef_host = coef_host; d.coef_cols = coef_cols;
    return d;
}

int ccn_sample(ccn_handle_t h, const float* z_dev, const float* x_T_dev, float* x_out_dev, int32_t B, int32_t H, int32_t W,
               int32_t steps, const int32_t* ts_host, const float* coef_host, void* workspace_dev, size_t workspace_bytes,
               void* stream, int32_t use_graph)
{
    const ccn_sampler_run_t d = run_of(steps, ts_host, coef_host, 4);
    return ccn_sample_run(h, &d, z_dev, x_T_dev, x_out_dev, B, H, W, workspace_dev, workspace_bytes, stream, use_graph);
}

int ccn_sample_eta(ccn_handle_t h, const float* z_dev, const float* x_T_dev, float* x_out_dev, int32_t B, int32_t H, int32_t W,
                   int32_t steps, const int32_t* ts_host, const float* coef_host, const float* sigma_host, const float* noise_dev,
                   void* workspace_dev, size_t workspace_bytes, void* stream, int32_t use_graph)
{
    if (!sigma_host || !noise_dev) return fail(CCN_EINVAL, "null sigma / noise");
    ccn_sampler_run_t d = run_of(steps, ts_host, coef_host, 4);
    d.sigma_host = sigma_host; d.noise_dev = noise_dev;
    return ccn_sample_run(h, &d, z_dev, x_T_dev, x_out_dev, B, H, W, workspace_dev, workspace_bytes, stream, use_graph);
}

int ccn_sample_guided(ccn_handle_t h, const float* z_dev, const float* z_null_dev, const float* x_T_dev, float* x_out_dev, int32_t B,
                      int32_t H, int32_t W, int32_t steps, const int32_t* ts_host, const float* coef_host, const float* sigma_host,
                      const float* noise_dev, float w, float* eps_scratch_dev, void* workspace_dev, size_t workspace_bytes, void* stream,
                      int32_t use_graph)
{
    ccn_sampler_run_t d = run_of(steps, ts_host, coef_host, 4);
    d.sigma_host = sigma_host; d.noise_dev = noise_dev;
    d.guided = 1; d.w = w; d.z_null_dev = z_null_dev; d.out_scratch_dev = eps_scratch_dev;
    return ccn_sample_run(h, &d, z_dev, x_T_dev, x_out_dev, B, H, W, workspace_dev, workspace_bytes, stream, use_graph);
}

int ccn_sample_seeded(ccn_handle_t h, const float* z_dev, const float* x_T_dev, float* x_out_dev, int32_t B, int32_t H, int32_t W,
                      int32_t steps, const int32_t* ts_host, const float* coef_host, const float* sigma_host, const uint64_t* seeds_dev,
                      float* out_scratch_dev, void* workspace_dev, size_t workspace_bytes, void* stream, int32_t use_graph)
{
    // (also with sigma_host NULL, where the run uses neither)
    if (!out_scratch_dev || ((uintptr_t)out_scratch_dev & 15)) return fail(CCN_EINVAL, "the output scratch must be non-null and 16-byte aligned");
    if (!seeds_dev) return fail(CCN_EINVAL, "the seeds must be non-null and 8-byte aligned");
    ccn_sampler_run_t d = run_of(steps, ts_host, coef_host, 4);
    d.sigma_host = sigma_host; d.seeds_dev = seeds_dev; d.out_scratch_dev = out_scratch_dev;
    return ccn_sample_run(h, &d, z_dev, x_T_dev, x_out_dev, B, H, W, workspace_dev, workspace_bytes, stream, use_graph);
}

int ccn_sample_guided_seeded(ccn_handle_t h, const float* z_dev, const float* z_null_dev, const float* x_T_dev, float* x_out_dev, int32_t B,
                             int32_t H, int32_t W, int32_t steps, const int32_t* ts_host, const float* coef_host, const float* sigma_host,
                             const uint64_t* seeds_dev, float w, float* eps_scratch_dev, void* workspace_dev, size_t workspace_bytes,
                             void* stream, int32_t use_graph)
{
    if (!seeds_dev) return fail(CCN_EINVAL, "the seeds must be non-null and 8-byte aligned");
    ccn_sampler_run_t d = run_of(steps, ts_host, coef_host, 4);
    d.sigma_host = sigma_host; d.seeds_dev = seeds_dev;
    d.guided = 1; d.w = w; d.z_null_dev = z_null_dev; d.out_scratch_dev = eps_scratch_dev;
    return ccn_sample_run(h, &d, z_dev, x_T_dev, x_out_dev, B, H, W, workspace_dev, workspace_bytes, stream, use_graph);
}

int ccn_sample_ms(ccn_handle_t h, const float* z_dev, const float* x_T_dev, float* x_out_dev, int32_t B, int32_t H, int32_t W, int32_t steps,
                  const int32_t* ts_host, const float* coef_host, float* x0_hist_dev, void* workspace_dev, size_t workspace_bytes,
                  void* stream, int32_t use_graph)
{
    ccn_sampler_run_t d = run_of(steps, ts_host, coef_host, 5);
    d.x0_hist_dev = x0_hist_dev;
    return ccn_sample_run(h, &d, z_dev, x_T_dev, x_out_dev, B, H, W, workspace_dev, workspace_bytes, stream, use_graph);
}

int ccn_sample_guided_ms(ccn_handle_t h, const float* z_dev, const float* z_null_dev, const float* x_T_dev, float* x_out_dev, int32_t B,
                         int32_t H, int32_t W, int32_t steps, const int32_t* ts_host, const float* coef_host, float w, float* eps_scratch_dev,
                         float* x0_hist_dev, void* workspace_dev, size_t workspace_bytes, void* stream, int32_t use_graph)
{
    ccn_sampler_run_t d = run_of(steps, ts_host, coef_host, 5);
    d.guided = 1; d.w = w; d.z_null_dev = z_null_dev; d.out_scratch_dev = eps_scratch_dev; d.x0_hist_dev = x0_hist_dev;
    return ccn_sample_run(h, &d, z_dev, x_T_dev, x_out_dev, B, H, W, workspace_dev, workspace_bytes, stream, use_graph);
}

// ---- the stand-alone updates: their own argument checks, then the one kernel ----------------------------------------------------
static int enqueue_step(const SamplerStep& a, void* stream)
{
    if (a.o.records * a.o.per_record == 0) return CCN_OK;
    HIPCHK(launch_sampler_step(a, (hipStream_t)stream));
    return CCN_OK;
}
// the four older entries: the eps form on by-value coefficients
static SamplerStep eps_step(float* x, const float* eps_c, float c0, float c1, float c2, float c3, int64_t n)
{
    SamplerStep a;
    a.o.x = x; a.o.out_c = eps_c; a.o.c0 = c0; a.o.c1 = c1; a.c2 = c2; a.c3 = c3;
    a.o.records = 1; a.o.per_record = n;                           // one run of n elements
    return a;
}

int ccn_ms_step(float* x_dev, float* x0_hist_dev, const float* eps_dev, float c0, float c1, float c2, float c3, float c4, int64_t n, void* stream)
{
    if (!x_dev || !x0_hist_dev || !eps_dev || n < 0) return fail(CCN_EINVAL, "bad argument");
    SamplerStep a = eps_step(x_dev, eps_dev, c0, c1, c2, c3, n);
    a.hist = x0_hist_dev; a.c4 = c4;
    return enqueue_step(a, stream);
}

int ccn_cfg_ms_step(float* x_dev, float* x_dup_dev, float* x0_hist_dev, const float* eps_c_dev, const float* eps_u_dev, float w,
                    float c0, float c1, float c2, float c3, float c4, int64_t n, void* stream)
{
    if (!x_dev || !x0_hist_dev || !eps_c_dev || !eps_u_dev || n < 0) return fail(CCN_EINVAL, "bad argument");
    SamplerStep a = eps_step(x_dev, eps_c_dev, c0, c1, c2, c3, n);
    a.x_dup = x_dup_dev; a.o.out_u = eps_u_dev; a.o.w = w; a.hist = x0_hist_dev; a.c4 = c4;
    return enqueue_step(a, stream);
}

int ccn_cfg_ddim_step(float* x_dev, float* x_dup_dev, const float* eps_c_dev, const float* eps_u_dev, const float* noise_dev, float w,
                      float c0, float c1, float c2, float c3, float sigma, int64_t n, void* stream)
{
    if (!x_dev || !eps_c_dev || !eps_u_dev || n < 0) return fail(CCN_EINVAL, "bad argument");
    SamplerStep a = eps_step(x_dev, eps_c_dev, c0, c1, c2, c3, n);
    a.x_dup = x_dup_dev; a.o.out_u = eps_u_dev; a.o.w = w; a.noise = noise_dev; a.sigma = sigma;
    return enqueue_step(a, stream);
}

int ccn_ddim_step(float* x_dev, const float* eps_dev, const float* noise_dev, float c0, float c1, float c2, float c3,
                  float sigma, int64_t n, void* stream)
{
    if (!x_dev || !eps_dev || n < 0) return fail(CCN_EINVAL, "bad argument");
    SamplerStep a = eps_step(x_dev, eps_dev, c0, c1, c2, c3, n);
    a.noise = noise_dev; a.sigma = sigma;
    return enqueue_step(a, stream);
}

// the three general entries: the checks of ccn_sampler_step and what all three take, into `a`
static int general_step(float* x_dev, float* x_dup_dev, float* x0_hist_dev, const float* out_c_dev, const float* out_u_dev, int32_t pred, float w,
                        const float* coef_host, float sigma, int64_t n, SamplerStep& a)
{
    if (!x_dev || !out_c_dev || !coef_host || n < 0) return fail(CCN_EINVAL, "bad argument");
    if (pred != CCN_PRED_EPS && pred != CCN_PRED_V) return fail(CCN_EINVAL, "unknown prediction (CCN_PRED_EPS or CCN_PRED_V)");
    a = eps_step(x_dev, out_c_dev, coef_host[0], coef_host[1], coef_host[2], coef_host[3], n);
    a.x_dup = x_dup_dev; a.hist = x0_hist_dev; a.o.out_u = out_u_dev; a.o.pred = pred; a.o.w = w; a.sigma = sigma;
    if (x0_hist_dev) a.c4 = coef_host[4];
    return CCN_OK;
}
// ... and of the two that walk the state record by record: n elements as records of per_record, into `a`, checked
static_assert(kDrawMaxPerRecord == kThrMaxPerRecord, "one per_record limit for the draws and the select");
static int set_records(SamplerStep& a, int64_t per_record, int64_t n)
{
    if (per_record <= 0 || per_record >= kDrawMaxPerRecord || n % per_record) return fail(CCN_EINVAL, "per_record must be in [1, 2^34) and divide n");
    a.o.per_record = per_record; a.o.records = n / per_record;
    return n == 0 ? CCN_OK : check_x0_operands(a.o, false);         // (n == 0: nothing is launched)
}

int ccn_sampler_step(float* x_dev, float* x_dup_dev, float* x0_hist_dev, const float* out_c_dev, const float* out_u_dev,
                     const float* noise_dev, int32_t pred, float w, const float* coef_host, float sigma, int64_t n, void* stream)
{
    SamplerStep a;
    if (int rc = general_step(x_dev, x_dup_dev, x0_hist_dev, out_c_dev, out_u_dev, pred, w, coef_host, sigma, n, a)) return rc;
    a.noise = noise_dev;
    return enqueue_step(a, stream);
}

int ccn_sampler_step_seeded(float* x_dev, float* x_dup_dev, float* x0_hist_dev, const float* out_c_dev, const float* out_u_dev,
                            const uint64_t* seeds_dev, uint32_t draw, int64_t per_record, int32_t pred, float w, const float* coef_host,
                            float sigma, int64_t n, void* stream)
{
    SamplerStep a;
    if (int rc = general_step(x_dev, x_dup_dev, x0_hist_dev, out_c_dev, out_u_dev, pred, w, coef_host, sigma, n, a)) return rc;
    if (!seeds_dev || ((uintptr_t)seeds_dev & 7)) return fail(CCN_EINVAL, "the seeds must be non-null and 8-byte aligned");
    if (int rc = set_records(a, per_record, n)) return rc;
    a.seeds = seeds_dev; a.draw = draw;
    return enqueue_step(a, stream);
}

int ccn_sampler_step_thr(float* x_dev, float* x_dup_dev, float* x0_hist_dev, const float* out_c_dev, const float* out_u_dev,
                         const float* noise_dev, const uint64_t* seeds_dev, uint32_t draw, int64_t per_record, int32_t pred, float w,
                         const float* coef_host, float sigma, int64_t n, const float* thr_dev, void* stream)
{
    return ccn_sampler_step_rs(x_dev, x_dup_dev, x0_hist_dev, out_c_dev, out_u_dev, noise_dev, seeds_dev, draw, per_record, pred, w, coef_host,
                               sigma, n, thr_dev, nullptr, stream);
}

int ccn_sampler_step_rs(float* x_dev, float* x_dup_dev, float* x0_hist_dev, const float* out_c_dev, const float* out_u_dev,
                        const float* noise_dev, const uint64_t* seeds_dev, uint32_t draw, int64_t per_record, int32_t pred, float w,
                        const float* coef_host, float sigma, int64_t n, const float* thr_dev, const float* gscale_dev, void* stream)
{
    return ccn_sampler_step_lr(x_dev, x_dup_dev, x0_hist_dev, out_c_dev, out_u_dev, noise_dev, seeds_dev, draw, per_record, pred, w, coef_host,
                               sigma, n, thr_dev, gscale_dev, 0, 0, 0, 0, nullptr, stream);
}

int ccn_sampler_step_lr(float* x_dev, float* x_dup_dev, float* x0_hist_dev, const float* out_c_dev, const float* out_u_dev,
                        const float* noise_dev, const uint64_t* seeds_dev, uint32_t draw, int64_t per_record, int32_t pred, float w,
                        const float* coef_host, float sigma, int64_t n, const float* thr_dev, const float* gscale_dev, int32_t C, int32_t H,
                        int32_t W, int32_t N, const float* delta_dev, void* stream)
{
    SamplerStep a;
    if (int rc = general_step(x_dev, x_dup_dev, x0_hist_dev, out_c_dev, out_u_dev, pred, w, coef_host, sigma, n, a)) return rc;
    if (noise_dev && seeds_dev) return fail(CCN_EINVAL, "noise_dev and seeds_dev exclude each other");
    if (seeds_dev && ((uintptr_t)seeds_dev & 7)) return fail(CCN_EINVAL, "the seeds must be 8-byte aligned");
    if (int rc = set_records(a, per_record, n)) return rc;
    a.noise = noise_dev; a.seeds = seeds_dev; a.draw = draw; a.o.thr = thr_dev; a.o.gscale = gscale_dev;
    if (delta_dev) {
        if (int rc = guide_check(H, W, N)) return rc;
        if (C <= 0 || (int64_t)C * H * W != per_record) return fail(CCN_EINVAL, "per_record must equal C*H*W");
        a.delta = delta_dev; a.lr_W = W; a.lr_N = N;
    }
    return enqueue_step(a, stream);
}

int ccn_q_sample(float* out_dev, const float* x0_dev, const float* noise_dev, const float* a_dev, const float* s_dev,
                 int32_t B, int64_t per_sample, void* stream)
{
    if (!out_dev || !x0_dev || !noise_dev || !a_dev || !s_dev || B <= 0 || per_sample <= 0) return fail(CCN_EINVAL, "bad argument");
    HIPCHK(launch_q_sample(out_dev, x0_dev, noise_dev, a_dev, s_dev, B, per_sample, (hipStream_t)stream));
    return CCN_OK;
}

int ccn_predict_x0(float* out_dev, const float* x_t_dev, const float* eps_dev, const float* a_dev, const float* s_dev,
                   int32_t B, int64_t per_sample, void* stream)
{
    if (!out_dev || !x_t_dev || !eps_dev || !a_dev || !s_dev || B <= 0 || per_sample <= 0) return fail(CCN_EINVAL, "bad argument");
    HIPCHK(launch_predict_x0(out_dev, x_t_dev, eps_dev, a_dev, s_dev, B, per_sample, (hipStream_t)stream));
    return CCN_OK;
}

int ccn_timestep_embedding(const int64_t* t_dev, float* out_dev, int32_t n, int32_t dim, void* stream)
{
    if (!t_dev || !out_dev || n <= 0 || dim <= 0) return fail(CCN_EINVAL, "bad argument");
    HIPCHK(launch_temb_i64(t_dev, out_dev, n, dim, (hipStream_t)stream));
    return CCN_OK;
}

int ccn_film_forward(const float* x_dev, const float* h_dev, const float* ws_dev, const float* bs_dev, const float* wh_dev,
                     const float* bh_dev, float* y_dev, int32_t B, int32_t C, int32_t H, int32_t W, int32_t D,
                     float* scratch_dev, void* stream)
{
    if (!x_dev || !h_dev || !ws_dev || !bs_dev || !wh_dev || !bh_dev || !y_dev || !scratch_dev) return fail(CCN_EINVAL, "null pointer");
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || D <= 0) return fail(CCN_EINVAL, "bad shape");
    hipStream_t s = (hipStream_t)stream;
    float* sc = scratch_dev; float* sh = scratch_dev + (size_t)B * C;
    HIPCHK(launch_linear(h_dev, nullptr, 1, B, ws_dev, bs_dev, sc, B, D, C, 0, s));
    HIPCHK(launch_linear(h_dev, nullptr, 1, B, wh_dev, bh_dev, sh, B, D, C, 0, s));
    HIPCHK(launch_film_nchw(x_dev, sc, sh, y_dev, B, C, (int64_t)H * W, s));
    return CCN_OK;
}

int ccn_resblock_forward(ccn_handle_t h, const char* prefix, const float* x_dev, const float* cond_dev, float* y_dev,
                         int32_t B, int32_t H, int32_t W, void* workspace_dev, size_t workspace_bytes, void* stream)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!prefix || !x_dev || !cond_dev || !y_dev || !workspace_dev) return fail(CCN_EINVAL, "null pointer");
    if (B <= 0 || H <= 0 || W <= 0) return fail(CCN_EINVAL, "bad shape");
    const ArchRes* r = nullptr;
    for (auto& q : h->arch.res) if (q.prefix == prefix) { r = &q; break; }
    if (!r) return fail(CCN_EINVAL, std::string("no ResBlock with prefix ") + prefix);
    if ((uintptr_t)workspace_dev & 255) return fail(CCN_EWORKSPACE, "workspace must be 256-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int G = (r->C < h->G ? r->C : h->G), cpg = r->C / G;
    int nslot = (H * W + 1023) / 1024; if (nslot < 1) nslot = 1;
    // the block's own plan (not cached): offsets first, nothing is written before the size is known to fit
    ShapePlan pl; pl.B = B; pl.H = H; pl.W = W; pl.steps = 1;
    PlanBuilder pb(h, pl);
    pl.film_stride = 2 * r->C;                                    // dense (B, 2C) table: [scale | shift] of this block only
    pl.film = pb.take("film", (size_t)B * 2 * r->C * 4);
    pb.take_counters(8);
    TensorRef x = pb.new_tensor("x", r->C, H, W);
    x.part = pb.take("x.part", (size_t)B * G * nslot * sizeof(float2));
    x.n_sp = nslot; x.n_nt = 1; x.bn = 1 << 30;
    const TensorRef o = pb.resblock((int)(r - h->arch.res.data()), x, false, 0);
    if (pb.off > workspace_bytes) return fail(CCN_EWORKSPACE, "workspace too small: need " + std::to_string(pb.off));
    char* ws = (char*)workspace_dev;
    for (auto& z : pl.zero) HIPCHK(hipMemsetAsync(ws + z.first, 0, z.second, s));   // counters, split-K hand-off flags of a fresh workspace
    HIPCHK(launch_nchw_to_nhwc(h->cfg.dtype, x_dev, ws + x.off, B, r->C, H, W, s));
    HIPCHK(launch_gn_partials(h->cfg.dtype, ws + x.off, (float2*)(ws + x.part), B, H * W, r->C, cpg, G, nslot, s));
    HIPCHK(launch_linear(cond_dev, nullptr, 1, B, h->film_w + (size_t)r->film_off * h->cfg.time_dim, h->film_b + r->film_off,
                         (float*)(ws + pl.film), B, h->cfg.time_dim, 2 * r->C, 0, s));
    StepCtx c;
    for (const Launch& L : pl.ops) HIPCHK(launch(h, pl, L, ws, s, c));
    HIPCHK(launch_nhwc_to_nchw(h->cfg.dtype, ws + o.off, y_dev, B, r->C, H, W, s));
    return CCN_OK;
}

int ccn_read_activation(ccn_handle_t h, const char* name, float* out_dev, size_t out_elems, void* stream)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!name || !out_dev) return fail(CCN_EINVAL, "null pointer");
    if (h->bindings.empty()) return fail(CCN_ESTATE, "no forward has run yet");
    const Binding* b = h->bindings.back().get();                    // the most recently used one
    auto it = b->plan->named.find(name);
    if (it == b->plan->named.end()) return fail(CCN_EINVAL, std::string("unknown activation ") + name);
    const TensorRef& t = it->second;
    if (out_elems < (size_t)b->plan->B * t.C * t.H * t.W) return fail(CCN_EINVAL, "output buffer too small");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(launch_nhwc_to_nchw(h->cfg.dtype, b->ws + t.off, out_dev, b->plan->B, t.C, t.H, t.W, s));
    HIPCHK(hipStreamSynchronize(s));
    return CCN_OK;
}

// Test hook, not part of include/ccn_hip.h: one line per conv-family launch of the plan that ccn_read_activation reads (the one the
// last ccn_forward / ccn_sample used), "<activation> <kind> <kernel> th=.. ksplit=.. n_nt=.. gn=.. film=0|1 res=0|1", as decided when
// that plan was built; lines of an f16x3 plan end in " ops=f16x3" (split fp16 operands) or " ops=f32".  snprintf-like: writes at most cap bytes (NUL-terminated) and returns the length of the whole report, or -1.
extern "C" int ccn_internal_plan_routes(ccn_handle_t h, char* buf, size_t cap)
{
    if (!h || h->bindings.empty()) return -1;
    return copy_report(routes_text(*h->bindings.back()->plan), buf, cap);
}
// Test hooks, not part of include/ccn_hip.h, on the cached plan of a shape (built if need be; nothing is bound to a workspace, launched,
// or made "the last used"): the same report, and the workspace layout -- "<name> off=<bytes> bytes=<bytes>" per region, "total=<bytes>".
extern "C" int ccn_internal_plan_routes_of(ccn_handle_t h, int32_t B, int32_t H, int32_t W, int32_t steps, char* buf, size_t cap)
{
    const ShapePlan* pl;
    if (!h || !h->committed || shape_plan(h, B, H, W, steps, &pl)) return -1;
    return copy_report(routes_text(*pl), buf, cap);
}
// The route report with the kernel word of every launch that runs a fixed-geometry instantiation of the persistent kernel replaced by
// that instantiation's name ("pr:c3.128x128.film", ...; plain "pr" = the run-time instantiation).  A report of its own: the lines of
// ccn_internal_plan_routes are compared with the parent commit's (tests/golden/infer_plan_parent.json) and stay what they were.
extern "C" int ccn_internal_plan_kernels(ccn_handle_t h, char* buf, size_t cap)
{
    if (!h || h->bindings.empty()) return -1;
    return copy_report(routes_text(*h->bindings.back()->plan, true), buf, cap);
}
extern "C" int ccn_internal_plan_kernels_of(ccn_handle_t h, int32_t B, int32_t H, int32_t W, int32_t steps, char* buf, size_t cap)
{
    const ShapePlan* pl;
    if (!h || !h->committed || shape_plan(h, B, H, W, steps, &pl)) return -1;
    return copy_report(routes_text(*pl, true), buf, cap);
}
// How many sampler-loop graphs the handle has captured so far: a call that replays a cached graph leaves it unchanged.
extern "C" int ccn_internal_graph_captures(ccn_handle_t h) { return h ? h->captures : -1; }
extern "C" int ccn_internal_plan_layout(ccn_handle_t h, int32_t B, int32_t H, int32_t W, int32_t steps, char* buf, size_t cap)
{
    const ShapePlan* pl;
    if (!h || !h->committed || shape_plan(h, B, H, W, steps, &pl)) return -1;
    std::string text;
    for (const Region& r : pl->regions) text += r.name + " off=" + std::to_string(r.off) + " bytes=" + std::to_string(r.bytes) + "\n";
    text += "total=" + std::to_string(pl->total) + "\n";
    return copy_report(text, buf, cap);
}

int ccn_poll_errors(ccn_handle_t h)
{
    if (!h) return fail(CCN_EINVAL, "null handle");
    return check_device_errors(h);
}

int ccn_profile_enable(ccn_handle_t h, int32_t on)
{
    if (!h) return fail(CCN_EINVAL, "null handle");
    h->profiling = on != 0;
    h->recs.clear();
    h->ev_used = 0;
    return CCN_OK;
}

int ccn_profile_read(ccn_handle_t h, const char** names, float* ms, int32_t* calls, double* flops, double* bytes,
                     int32_t cap, int32_t* n)
{
    if (!h || !names || !ms || !calls || !flops || !bytes || !n) return fail(CCN_EINVAL, "null pointer");
    HIPCHK(hipDeviceSynchronize());
    std::vector<double> t(F_COUNT, 0.0), fl(F_COUNT, 0.0), by(F_COUNT, 0.0);
    std::vector<int> cnt(F_COUNT, 0);
    for (auto& r : h->recs) {
        float e = 0.f;
        HIPCHK(hipEventElapsedTime(&e, h->ev_pool[r.e0], h->ev_pool[r.e1]));
        t[r.family] += e; fl[r.family] += r.flops; by[r.family] += r.bytes; cnt[r.family]++;
    }
    int k = 0;
    for (int f = 0; f < F_COUNT && k < cap; ++f) {
        if (!cnt[f]) continue;
        names[k] = h->fam_names[f].c_str(); ms[k] = (float)t[f]; calls[k] = cnt[f]; flops[k] = fl[f]; bytes[k] = by[f];
        ++k;
    }
    *n = k;
    h->recs.clear();
    h->ev_used = 0;
    return CCN_OK;
}

int ccn_algorithmic_work(ccn_handle_t h, int32_t B, int32_t H, int32_t W, double* flops, double* bytes)
{
    int rc = check_ready(h);
    if (rc) return rc;
    if (!flops || !bytes) return fail(CCN_EINVAL, "null pointer");
    const ShapePlan* pl = nullptr;
    if ((rc = shape_plan(h, B, H, W, 1, &pl))) return rc;
    double f = 0, b = 0;
    for (auto& L : pl->ops) if (L.family <= F_HEAD) { f += L.flops; b += L.bytes; }
    const ccn_config_t& c = h->cfg;
    f += 2.0 * B * ((double)c.time_dim * 4 * c.time_dim * 2 + (double)c.z_dim * c.time_dim + (double)c.time_dim * h->arch.F);
    *flops = f; *bytes = b;
    return CCN_OK;
}

}  // extern "C"
