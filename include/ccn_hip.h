/*
 * ccn_hip.h -- C ABI of libccn_hip.so: the MI355X (gfx950) DDIM reconstruction path of
 * clip-feature-codec (CLIPCondUNet epsilon-prediction forward + DDIM update).
 *
 * The reference (lionl1106/Clip-Neural-image-conpression) is pure Python on torch.nn and has no
 * FFI of its own; every entry point below names the reference interface it stands in for
 * (paths relative to src/clip_feature_codec/).  A reference maintainer binds them with ctypes
 * (see INTEGRATION.md); nothing here carries a torch type.
 *
 * Conventions
 *   - every function returns 0 on success, a CCN_E* code otherwise; ccn_last_error() returns a
 *     thread-local message for the last failure.  No C++ exception crosses the boundary.
 *   - pointers named *_dev are device (HBM) pointers owned by the caller; *_host are host pointers.
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream).  Calls enqueue work and return;
 *     they never synchronise the device, except where stated.
 *   - image tensors at the boundary are NCHW fp32 contiguous, exactly what the reference passes to
 *     CLIPCondUNet.forward; NHWC and (in bf16 mode) bf16 are internal.
 *   - one handle per process per device; handles are not thread-safe.
 */
#ifndef CCN_HIP_H
#define CCN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCN_OK            0
#define CCN_EINVAL        1   /* bad argument / unsupported shape            */
#define CCN_EHIP          2   /* a HIP runtime call failed                   */
#define CCN_EWEIGHTS      3   /* missing / unexpected / mis-shaped parameter */
#define CCN_EWORKSPACE    4   /* workspace too small or misaligned           */
#define CCN_ESTATE        5   /* call order violated                         */

#define CCN_DTYPE_F32     0   /* fp32 storage, fp32 MFMA (v_mfma_f32_32x32x2_f32): parity mode        */
#define CCN_DTYPE_BF16    1   /* bf16 storage, bf16 MFMA (v_mfma_f32_16x16x32_bf16 / 32x32x16), fp32 accumulate */
#define CCN_DTYPE_F16X3   2   /* fp32 storage; conv operands split into fp16 hi + lo, three v_mfma_f32_32x32x16_f16 per product,
                                 fp32 accumulate: fp32-grade results from the fast MFMAs.  Inference only (ccn_train_create rejects
                                 it); ccn_set_weight_rounding has no effect.  Activations must stay below 65520 in magnitude where a
                                 ResBlock conv or ConvTranspose reads them: beyond that the operand saturates and the next call /
                                 ccn_poll_errors fails once, naming fp32 as the mode to use. */

#define CCN_MAX_MULT      8

typedef struct ccn_handle_s* ccn_handle_t;

/* Constructor arguments of CLIPCondUNet (models/unet.py:45) plus the arithmetic mode. */
typedef struct ccn_config {
    int32_t z_dim;                 /* 512                                         */
    int32_t base;                  /* 128                                         */
    int32_t n_mult;                /* len(ch_mult)                                */
    int32_t ch_mult[CCN_MAX_MULT]; /* (1,2,2); widths are a running product       */
    int32_t time_dim;              /* 256                                         */
    int32_t img_ch;                /* 3                                           */
    int32_t groups;                /* GroupNorm groups, 8 (models/blocks.py:31)   */
    int32_t dtype;                 /* CCN_DTYPE_*                                 */
} ccn_config_t;

/* ---- lifetime ------------------------------------------------------------------------------- */

/* CLIPCondUNet.__init__ + .to(device) (models/unet.py:45-79; cli/eval.py:50). Uses the current HIP device. */
int ccn_create(const ccn_config_t* cfg, ccn_handle_t* out);
int ccn_destroy(ccn_handle_t h);

/* Number of state-dict entries the handle expects, and the i-th key / shape: the key set of
 * CLIPCondUNet.state_dict() (192 entries at base=128, ch_mult=(1,2,2)). */
int ccn_num_params(ccn_handle_t h, int32_t* n);
int ccn_param_info(ccn_handle_t h, int32_t i, const char** name, int64_t shape[4], int32_t* ndim);

/* One entry of load_state_dict (cli/eval.py:51, cli/reconstruct_diffusion.py:48).  `data` is fp32,
 * contiguous, in the reference's own layout (Conv2d OIHW, ConvTranspose2d (Cin,Cout,4,4), Linear
 * (out,in)); host or device pointer.  The library copies; the caller keeps ownership. */
int ccn_load_param(ccn_handle_t h, const char* name, const float* data, const int64_t* shape, int32_t ndim);

/* How CCN_DTYPE_BF16 rounds the conv weights to bf16 when they are repacked (call before ccn_commit_params; no effect in fp32
 * mode).  A rounded weight is a static perturbation of the model that acts the same way in every one of the sampler's steps, and
 * that coherent accumulation is what moves the 50-step reconstructions: independent rounding loses 0.33 % contrast, 0.165 % PSNR
 * (max per record) against the fp32 reference path -- above north_star's 0.1 % gate (eval/metrics.py:22-29).
 *   CCN_ROUND_NEAREST          independent round-to-nearest-even, what `.to(torch.bfloat16)` of the checkpoint gives;
 *   CCN_ROUND_DIFFUSED         error diffusion along (cin, ky, kx) of every output channel: partial sums of an output channel's
 *                              weights stay within half an ulp of the fp32 sums;
 *   CCN_ROUND_DIFFUSED_PHASES  (default) the same, plus error diffusion ALONG THE DDIM STEPS: n such roundings of every weight whose
 *                              running sums track the fp32 weight, step i of ccn_sample uses version i % n (ccn_forward: version 0).
 *                              n = 8 (4 for models above 100 M conv weights): the mean weight over a period is accurate to 1/16 ulp;
 *                              costs n copies of the bf16 weights in HBM and nothing at run time. */
#define CCN_ROUND_NEAREST         0
#define CCN_ROUND_DIFFUSED        1
#define CCN_ROUND_DIFFUSED_PHASES 2
int ccn_set_weight_rounding(ccn_handle_t h, int32_t mode);

/* strict=True check (every key loaded exactly once with the right shape), then repack to the kernel
 * layouts ([tap][Cout][Cin], bf16 copies in bf16 mode) and upload.  Synchronises the device. */
int ccn_commit_params(ccn_handle_t h);

/* ---- the hot path --------------------------------------------------------------------------- */

/* Scratch needed by ccn_forward / ccn_sample for this shape; the caller allocates it (e.g. through
 * torch's caching allocator), 256-byte aligned, and keeps it alive and at the same address while a
 * captured graph for it is cached. `steps` = 1 for ccn_forward. */
int ccn_workspace_bytes(ccn_handle_t h, int32_t B, int32_t H, int32_t W, int32_t steps, size_t* bytes);

/* The caller is about to free (or reuse for something else) a workspace it handed to ccn_forward / ccn_sample: drains the
 * device, then drops every cached plan and captured graph that lives in it.  The plan cache is keyed by (B, H, W, steps,
 * workspace address) and a plan keeps state in its workspace between calls (the uploaded timestep table, the zeroed split-K
 * hand-off flags and arrival counters), so a LATER allocation that lands on the same address must not find the old plan.
 * Without this call a freed workspace must never be reused at the same address with the same shape.  (No reference
 * counterpart: torch owns all memory there; this is the ownership rule of SURVEY.md section 8b, "Python owns the workspace".) */
int ccn_release_workspace(ccn_handle_t h, void* workspace_dev);

/* CLIPCondUNet.forward(x_t, z_clip, t) (models/unet.py:81-106).
 * x_dev (B,img_ch,H,W) fp32 NCHW; z_dev (B,z_dim) fp32; t_dev (B,) int64; eps_dev (B,img_ch,H,W) fp32 NCHW. */
int ccn_forward(ccn_handle_t h, const float* x_dev, const float* z_dev, const int64_t* t_dev,
                float* eps_dev, int32_t B, int32_t H, int32_t W,
                void* workspace_dev, size_t workspace_bytes, void* stream);

/* DDIMSampler.sample(model, z_clip, shape, steps, x_T=...) for eta = 0 (diffusion/ddim.py:21-45).
 * ts_host[steps]: the timestep table (linspace(T-1,0,steps).long());
 * coef_host[steps][4]: fp32 (sqrt(1-ab_t), sqrt(ab_t), sqrt(ab_s), sqrt(ab_s - sigma^2)) per step, so that
 *     x0 = clamp((x - c0*eps)/c1, -1, 1);  x = c2*x0 + c3*eps      -- every op rounded to fp32
 * x_T_dev -> x_out_dev (may alias), (B,img_ch,H,W) fp32 NCHW, unclamped like the reference.
 * use_graph != 0: the whole steps-long loop is captured once into a hipGraph (cached per
 * shape/steps/table/workspace address) and replayed with one launch. */
int ccn_sample(ccn_handle_t h, const float* z_dev, const float* x_T_dev, float* x_out_dev,
               int32_t B, int32_t H, int32_t W, int32_t steps,
               const int32_t* ts_host, const float* coef_host,
               void* workspace_dev, size_t workspace_bytes, void* stream, int32_t use_graph);

/* The same loop for eta > 0 (diffusion/ddim.py:41-45): sigma_host[steps] fp32 per-step sigma (0 on steps without noise, e.g. the
 * last one), coef_host as above with c3 = sqrt(ab_s - sigma^2); noise_dev (steps,B,img_ch,H,W) fp32 holds the N(0,1) draws of every
 * step, made by the caller (the reference draws torch.randn_like per step: a torch caller fills slice i with its i-th draw so that
 * the fused loop consumes the generator exactly like the step-by-step loop); the update adds sigma*noise, rounded like the torch ops.
 * The captured graph is cached per (table, sigma, noise address). */
int ccn_sample_eta(ccn_handle_t h, const float* z_dev, const float* x_T_dev, float* x_out_dev,
                   int32_t B, int32_t H, int32_t W, int32_t steps,
                   const int32_t* ts_host, const float* coef_host, const float* sigma_host, const float* noise_dev,
                   void* workspace_dev, size_t workspace_bytes, void* stream, int32_t use_graph);

/* One DDIM update outside the fused loop (eta > 0, or a caller-driven loop; diffusion/ddim.py:34-45):
 * x = c2*clamp((x - c0*eps)/c1) + c3*eps [+ sigma*noise]; noise_dev may be NULL. In place on x_dev. */
int ccn_ddim_step(float* x_dev, const float* eps_dev, const float* noise_dev,
                  float c0, float c1, float c2, float c3, float sigma, int64_t n, void* stream);

/* The DDIM loop under classifier-free guidance: per step eps = eps_u + w*(eps_c - eps_u), eps_c the prediction with z, eps_u the one
 * with the null embedding, then the update of ccn_sample / ccn_sample_eta on that eps.  (No reference counterpart: the reference's
 * sampler accepts cfg_scale and never reads it, diffusion/ddim.py:22.)
 * The loop is the plan of batch 2B: rows [0, B) carry z_dev (B,z_dim), rows [B, 2B) carry z_null_dev (z_dim,) (NULL: zeros), both
 * halves the same state.  Each step evaluates the UNet on the 2B rows, the head writing eps, and one ccn_sampler_step launch
 * writes the new state into both halves.  Conditioning of all steps is hoisted in front of the loop as in ccn_sample.
 * workspace_dev: the one of ccn_workspace_bytes(h, 2*B, H, W, steps).  eps_scratch_dev: 2*B*img_ch*H*W floats, 16-byte aligned,
 * owned by the caller like the workspace, and to be kept at the same address while a captured graph for it is cached.
 * sigma_host / noise_dev: both NULL (eta = 0) or both given as for ccn_sample_eta, noise_dev (steps,B,img_ch,H,W): one set of draws,
 * shared by the two halves.  w must be finite.  x_T_dev -> x_out_dev (may alias), (B,img_ch,H,W).
 * The captured graph is cached with those of ccn_sample at batch 2B on the same workspace, per (table, sigma, noise address, w,
 * eps scratch address): w is a by-value kernel argument, so a new w is a new capture. */
int ccn_sample_guided(ccn_handle_t h, const float* z_dev, const float* z_null_dev, const float* x_T_dev, float* x_out_dev,
                      int32_t B, int32_t H, int32_t W, int32_t steps,
                      const int32_t* ts_host, const float* coef_host, const float* sigma_host, const float* noise_dev,
                      float w, float* eps_scratch_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream, int32_t use_graph);

/* One guided DDIM update, combine and update in one pass, every op rounded to fp32 on its own like the torch ops:
 *     e = eps_u + w*(eps_c - eps_u);  x0 = clamp((x - c0*e)/c1, -1, 1);  x = c2*x0 + c3*e [+ sigma*noise]
 * In place on x_dev; x_dup_dev (may be NULL) receives the same values (the second half of ccn_sample_guided's state); noise_dev may
 * be NULL.  n elements each.  Four elements per lane when every pointer is 16-byte aligned, one otherwise. */
int ccn_cfg_ddim_step(float* x_dev, float* x_dup_dev, const float* eps_c_dev, const float* eps_u_dev, const float* noise_dev,
                      float w, float c0, float c1, float c2, float c3, float sigma, int64_t n, void* stream);

/* A second-order multistep sampler, DPM-Solver++ 2M in its data-prediction form, deterministic, on the loop of ccn_sample.  (No
 * reference counterpart: the reference ships first-order DDIM only.)
 * coef_host[steps][5]: fp32 (c0..c3 as for ccn_sample, c4) per step; the head's update becomes
 *     x0 = clamp((x - c0*eps)/c1, -1, 1);  x = c2*x0 + c3*eps;  c4 != 0:  x = x + c4*(x0 - hist);  hist = x0    -- every op rounded to fp32
 * With a = sqrt(ab), s = sqrt(1 - ab), lambda = log(a/s), a step from t = ts[i] to u = ts[i+1], h_i = lambda_u - lambda_t and
 * r_i = h_(i-1)/h_i:  c0 = s_t, c1 = a_t, c2 = a_u, c3 = s_u (1, 0 on the last step), c4 = a_u (1 - exp(-h_i)) / (2 r_i) on the
 * steps 0 < i < steps-1, else 0.  Unlike DDIMSampler's table, ab_u is the noise level of the NEXT table entry.  With c4 == 0 on every
 * step the loop computes what ccn_sample computes on coef_host[:, :4], bit for bit.
 * x0_hist_dev: B*img_ch*H*W floats, 16-byte aligned, owned by the caller like the workspace (and outside it: ccn_workspace_bytes is
 * unchanged), to be kept at the same address while a captured graph for it is cached; its contents on entry do not matter (it is
 * not read while c4 == 0, and every step rewrites it).
 * CCN_EINVAL: x0_hist_dev NULL or misaligned, a non-finite coefficient, c4 != 0 on step 0 (there is no history yet).
 * The captured graph is cached with those of ccn_sample on the same workspace, per (table, c4 column, history address). */
int ccn_sample_ms(ccn_handle_t h, const float* z_dev, const float* x_T_dev, float* x_out_dev,
                  int32_t B, int32_t H, int32_t W, int32_t steps,
                  const int32_t* ts_host, const float* coef_host, float* x0_hist_dev,
                  void* workspace_dev, size_t workspace_bytes, void* stream, int32_t use_graph);

/* The same sampler under classifier-free guidance: ccn_sample_guided's loop at batch 2B (eta = 0 only: no sigma, no noise), each step
 * ending in one ccn_sampler_step launch that writes the new state into both halves.  coef_host[steps][5] and the CCN_EINVAL cases as for
 * ccn_sample_ms; x0_hist_dev holds ONE state, B*img_ch*H*W floats; workspace_dev and eps_scratch_dev as for ccn_sample_guided.
 * The captured graph is cached per (table, c4 column, w, eps scratch address, history address). */
int ccn_sample_guided_ms(ccn_handle_t h, const float* z_dev, const float* z_null_dev, const float* x_T_dev, float* x_out_dev,
                         int32_t B, int32_t H, int32_t W, int32_t steps,
                         const int32_t* ts_host, const float* coef_host,
                         float w, float* eps_scratch_dev, float* x0_hist_dev,
                         void* workspace_dev, size_t workspace_bytes, void* stream, int32_t use_graph);

/* One multistep update outside the fused loop, the sequence above: in place on x_dev; x0_hist_dev is read only when c4 != 0 and
 * then receives this step's clamped x0.  n elements each.  Four elements per lane when every pointer is 16-byte aligned, one otherwise. */
int ccn_ms_step(float* x_dev, float* x0_hist_dev, const float* eps_dev,
                float c0, float c1, float c2, float c3, float c4, int64_t n, void* stream);

/* ... and its guided form: e = eps_u + w*(eps_c - eps_u), then the update on e; x_dup_dev (may be NULL) receives a copy of the new x
 * (the second half of ccn_sample_guided_ms's state).  The eps inputs are not written. */
int ccn_cfg_ms_step(float* x_dev, float* x_dup_dev, float* x0_hist_dev, const float* eps_c_dev, const float* eps_u_dev,
                    float w, float c0, float c1, float c2, float c3, float c4, int64_t n, void* stream);

/* ---- parameterisation: what the network output is ------------------------------------------------------------------------------ *
 * (No reference counterpart: the reference trains and samples eps only.)  With a = sqrt(ab_t), s = sqrt(1 - ab_t):
 *   CCN_PRED_EPS  (default) the network predicts the noise, every formula above as written;
 *   CCN_PRED_V    the network predicts v = a*noise - s*x0 (Salimans & Ho 2022).  On the SAME coefficient tables (c0 = s_t, c1 = a_t)
 *                 the first line of every update becomes
 *                     x0 = clamp(c1*x - c0*y, -1, 1);  e = c0*x + c1*y        -- every op rounded to fp32, y the network output
 *                 and the rest (c2*x0 + c3*e, the c4 term, sigma*noise, x_dup) is unchanged.  Under guidance y = y_u + w*(y_c - y_u)
 *                 is combined first.  x0 is formed directly and not through e: at t = 999 of the cosine table 1/a = 6.4e4 and s
 *                 rounds to 1.0f, so the eps form applied to e returns x0 = 0 whatever the network said. */
enum { CCN_PRED_EPS = 0, CCN_PRED_V = 1 };

/* Handle state read by ccn_sample, ccn_sample_eta, ccn_sample_guided, ccn_sample_ms and ccn_sample_guided_ms when they enqueue or
 * capture; part of every captured graph's cache key, so toggling finds each mode's own graph on a shared workspace.  ccn_forward
 * is unaffected (it returns the raw network output).  Any other value: CCN_EINVAL, the state is unchanged. */
int ccn_set_prediction(ccn_handle_t h, int32_t pred);

/* One sampler update outside the fused loop, for either parameterisation: the general form of ccn_ddim_step, ccn_cfg_ddim_step,
 * ccn_ms_step and ccn_cfg_ms_step.  In place on x_dev; coef_host[5] = c0..c4 (a HOST pointer, read before the call returns).
 *   out_c_dev   the network output (eps or v, by `pred`);
 *   out_u_dev   NULL, or the unconditional output: y = out_u + w*(out_c - out_u) is used (w is ignored when NULL);
 *   x0_hist_dev NULL (c4 is not applied, nothing is stored), or the x0 history: read only when c4 != 0, then receives this step's x0;
 *   noise_dev   NULL, or N(0,1) draws added as sigma*noise;   x_dup_dev  NULL, or receives a copy of the new x.
 * The four older entry points are this one with pred = CCN_PRED_EPS, bit for bit.  The output tensors are not written.
 * n elements each.  Four elements per lane when every non-NULL pointer is 16-byte aligned, one otherwise.
 * CCN_EINVAL: x_dev, out_c_dev or coef_host NULL, n < 0, an unknown pred. */
int ccn_sampler_step(float* x_dev, float* x_dup_dev, float* x0_hist_dev, const float* out_c_dev, const float* out_u_dev,
                     const float* noise_dev, int32_t pred, float w, const float* coef_host /* [5] */, float sigma, int64_t n,
                     void* stream);

/* ---- seeded device noise: a record's draws are a function of its seed ------------------------------------------------------------ *
 * (No reference counterpart: the reference draws torch.randn / randn_like from whatever generator is current.)  A counter-based
 * generator, Philox4x32-10 with the Random123 constants, through Box-Muller.  Element j (NCHW index inside the record, j < C*H*W) of
 * draw d of the record with 64-bit seed s:
 *   key      (s & 0xffffffff, s >> 32);
 *   counter  (q, d, 0, 0) with q = j >> 2; d = 0 is the start noise, d = 1 + i the noise of loop step i; words 2 and 3 are reserved;
 *   normals  the output words r0..r3 give elements 4q..4q+3: pair p = (j & 3) >> 1 has u1 = ((r[2p] >> 9) + 0.5) * 2^-23 and
 *            u2 = ((r[2p+1] >> 9) + 0.5) * 2^-23 (exact in fp32, inside (0, 1)), rad = sqrtf(-2 logf(u1)); an even j is
 *            rad * cospif(2 u2), an odd j rad * sinpif(2 u2), the precise library functions; |n| <= 5.77.
 * Batch position, batch size, rank and call history do not enter, and neither does how a kernel walks the record (a quad per lane
 * or an element per lane).  per_record >= 2^34 is CCN_EINVAL (q is one counter word).
 *
 * ccn_normal_fill: out_dev (B, per_record) fp32, row b the draw `draw` of the record with seed seeds_dev[b] (B x uint64 on the
 * device, read when the kernel runs).  16-byte stores in the rows that start 16-byte aligned, 4-byte stores in the others
 * (per_record % 4 != 0 puts later rows off alignment).  CCN_EINVAL: a NULL pointer, out_dev not 4-byte or seeds_dev not 8-byte
 * aligned, B outside [1, 65535], per_record <= 0 or >= 2^34. */
int ccn_normal_fill(float* out_dev, const uint64_t* seeds_dev, int32_t B, int64_t per_record, uint32_t draw, void* stream);

/* ccn_sampler_step whose noise is generated where it is consumed: x_dev holds n / per_record records of per_record elements (one
 * state; x_dup_dev receives the same values), record b drawing from seeds_dev[b].  With sigma > 0 the update adds sigma * n with
 * n the element's value of draw `draw`, by the same two separately rounded ops as sigma * noise_dev[i]: the result equals
 * ccn_sampler_step on a noise tensor filled by ccn_normal_fill, bit for bit.  sigma <= 0: no noise, seeds_dev is not read.
 * CCN_EINVAL: as for ccn_sampler_step, and seeds_dev NULL or not 8-byte aligned, per_record <= 0 or >= 2^34, n % per_record != 0, more than
 * 65535 records. */
int ccn_sampler_step_seeded(float* x_dev, float* x_dup_dev, float* x0_hist_dev, const float* out_c_dev, const float* out_u_dev,
                            const uint64_t* seeds_dev, uint32_t draw, int64_t per_record, int32_t pred, float w,
                            const float* coef_host /* [5] */, float sigma, int64_t n, void* stream);

/* ccn_sample_eta with the noise of step i generated as draw 1 + i of each record: no noise tensor exists.  seeds_dev: B x uint64 on
 * the device, owned by the caller and kept at the same address while a captured graph for it is cached; its CONTENTS are read when
 * the loop runs, so a replay after the caller rewrote them gives the new records' draws.  sigma_host NULL: eta = 0, the loop is
 * ccn_sample's and the seeds only matter to the caller's start noise (ccn_normal_fill, draw 0).  out_scratch_dev: B*img_ch*H*W
 * floats, 16-byte aligned, owned by the caller like the workspace: on a step with sigma > 0 the head writes the raw network output
 * there and one ccn_sampler_step_seeded launch applies the update; the other steps update in the head as in ccn_sample.  The result
 * equals ccn_sample_eta on the materialised draws, bit for bit.  The captured graph is cached per (table, sigma, seeds address,
 * scratch address); the draw index of a step is a by-value kernel argument. */
int ccn_sample_seeded(ccn_handle_t h, const float* z_dev, const float* x_T_dev, float* x_out_dev,
                      int32_t B, int32_t H, int32_t W, int32_t steps,
                      const int32_t* ts_host, const float* coef_host, const float* sigma_host, const uint64_t* seeds_dev,
                      float* out_scratch_dev,
                      void* workspace_dev, size_t workspace_bytes, void* stream, int32_t use_graph);

/* ccn_sample_guided likewise: the combine launch of a step with sigma > 0 generates the draws, one set for both halves.
 * eps_scratch_dev as for ccn_sample_guided (2*B*img_ch*H*W floats). */
int ccn_sample_guided_seeded(ccn_handle_t h, const float* z_dev, const float* z_null_dev, const float* x_T_dev, float* x_out_dev,
                             int32_t B, int32_t H, int32_t W, int32_t steps,
                             const int32_t* ts_host, const float* coef_host, const float* sigma_host, const uint64_t* seeds_dev,
                             float w, float* eps_scratch_dev,
                             void* workspace_dev, size_t workspace_bytes, void* stream, int32_t use_graph);

/* ---- dynamic thresholding of x0 -------------------------------------------------------------------------------------------------- *
 * (No reference counterpart: the reference clamps x0 to [-1, 1].  Saharia et al. 2022, Imagen section 2.3.)  Per record b and step,
 *     s = min(max(Q_p(|x0_b|), 1), max_value);   x0 = clamp(x0, -s, s) / s
 * replaces the static clamp of every update above; the rest of the update is unchanged, and s == 1 is the static clamp bit for bit.
 * Q_p is the linearly interpolated quantile over the per_record elements of the record: with v the ascending |x0| (the raw x0 as the
 * update forms it, after the guidance combine, each op rounded to fp32), pos = p*(per_record - 1) and k = floor(pos) in double,
 * frac = (float)(pos - k):  q = v[k] + frac * (v[min(k+1, per_record-1)] - v[k]),  three separately rounded fp32 ops.  v[k] and
 * v[k+1] are exact order statistics (a radix select on the bit patterns; integer counting only), so the threshold is reproducible
 * bit for bit and does not depend on B, on the record's position in the batch, on the launch shape or on pointer alignment (16-byte
 * loads when every pointer is 16-byte aligned and per_record % 4 == 0, 4-byte loads otherwise).
 * Non-finite input is not looked for: in the order of the bit patterns NaNs sort last, so a record whose rank-k or rank-(k+1) element
 * is a NaN gets s = NaN and with it a NaN update, other records are unaffected; +inf is an ordinary largest value (an interpolation
 * that meets inf - inf or 0 * inf is NaN like any other).
 *
 * ccn_x0_threshold: thr_dev[b] = s of record b, b < B, for x0 formed from x_dev / out_c_dev / out_u_dev (NULL: w ignored) / pred /
 * c0, c1 exactly as ccn_sampler_step forms it.  scratch_dev: ccn_x0_threshold_scratch_bytes bytes, 16-byte aligned, caller-owned, any
 * contents (every call zeroes what it uses, on the stream; two calls in flight need two scratches).  Five small launches on `stream`;
 * never synchronises, allocates nothing, capturable.  p = 0 is the minimum, p = 1 the maximum.
 * CCN_EINVAL: a NULL tensor, an unknown pred, p outside [0, 1] or NaN, max_value below 1 or NaN (+inf: no upper bound), B outside
 * [1, 65535], per_record <= 0 or >= 2^34, a NULL, misaligned or short scratch. */
int ccn_x0_threshold_scratch_bytes(int32_t B, int64_t per_record, size_t* bytes);
int ccn_x0_threshold(const float* x_dev, const float* out_c_dev, const float* out_u_dev,
                     int32_t pred, float w, float c0, float c1,
                     int32_t B, int64_t per_record, double p, float max_value,
                     float* thr_dev, void* scratch_dev, size_t scratch_bytes, void* stream);

/* The superset of ccn_sampler_step and ccn_sampler_step_seeded plus thr_dev: n / per_record records, record b clamping its x0 to
 * thr_dev[b] (one float per record, read when the kernel runs) as above.  noise_dev / seeds_dev exclude each other (both NULL: no
 * noise).  thr_dev NULL: those two entries, bit for bit.
 * CCN_EINVAL: as for those entries, and both noise_dev and seeds_dev given, per_record <= 0 or >= 2^34, n % per_record != 0, more than
 * 65535 records. */
int ccn_sampler_step_thr(float* x_dev, float* x_dup_dev, float* x0_hist_dev,
                         const float* out_c_dev, const float* out_u_dev,
                         const float* noise_dev, const uint64_t* seeds_dev, uint32_t draw,
                         int64_t per_record, int32_t pred, float w,
                         const float* coef_host /* [5] */, float sigma, int64_t n,
                         const float* thr_dev, void* stream);

/* Handle state, like ccn_set_prediction: read by every ccn_sample* entry when it enqueues or captures, and part of every captured
 * graph's cache key (p, max_value, the scratch address), so toggling finds each mode's own graph on a shared workspace and a run with
 * p == 0 replays the graph it had.  p == 0: off (the default; scratch_dev may be NULL).  With p in (0, 1] EVERY step of every loop --
 * plain, eta, seeded, guided, multistep, guided multistep, either parameterisation -- runs as: the head writes the raw network
 * output, ccn_x0_threshold's launches take the quantile (on the combined output when guided: one threshold per image, both halves of
 * the state get the same update), one ccn_sampler_step_thr launch updates; the multistep history receives the thresholded x0.
 * scratch_dev: ccn_dynamic_threshold_scratch_bytes(h, B, H, W) bytes for the largest shape sampled with it (B images, also when
 * guided), 16-byte aligned, owned by the caller and kept at its address while a graph captured with it is cached, like the workspace.
 * It holds the raw output of one state (runs with an eps / output scratch of their own keep using theirs), the B thresholds and the
 * select state.  ccn_workspace_bytes is unchanged.
 * CCN_EINVAL: p outside [0, 1] or NaN; with p > 0: max_value below 1 or NaN, a NULL, misaligned or short scratch (a scratch too
 * small for the shape of a later ccn_sample* call is that call's CCN_EINVAL), more than 65535 images, C*H*W >= 2^34. */
int ccn_set_dynamic_threshold(ccn_handle_t h, double p, float max_value, void* scratch_dev, size_t scratch_bytes);
int ccn_dynamic_threshold_scratch_bytes(ccn_handle_t h, int32_t B, int32_t H, int32_t W, size_t* bytes);

/* ---- guidance rescale -------------------------------------------------------------------------------------------------------------- *
 * (No reference counterpart.  Lin et al. 2023, Common Diffusion Noise Schedules and Sample Steps are Flawed, section 3.4; diffusers'
 * guidance_rescale.)  Under guidance the combined output has a much larger per-image standard deviation than anything the network
 * emits; the rescale matches it to the conditional output's.  Per record b of per_record elements and per step, with y_c the
 * conditional output, y = y_u + w (y_c - y_u) the combined one (the three separately rounded fp32 ops of ccn_sampler_step) and phi
 * in (0, 1]:
 *     std_c = std(y_c[b]),  std_cfg = std(y[b])          unbiased (n - 1), over the whole record
 *     k_b   = phi * std_c / std_cfg + (1 - phi)           double arithmetic, rounded ONCE to fp32
 *     y'    = k_b * y                                      one fp32 multiplication per element
 * and y' replaces y everywhere downstream: in the raw x0 of either parameterisation, in e (eps form: e = y'), in the dynamic
 * threshold's quantile and, through x0, in the multistep history.  (diffusers' phi (y r) + (1 - phi) y up to rounding; the single
 * factor is the format here.)  The sums S(y_c), S(y_c^2), S(y), S(y^2) are accumulated in double -- the square of an fp32 value is exact
 * there -- and the variance is (S(v^2) - S(v)^2 / n) / (n - 1), clamped at 0.  std_cfg == 0 gives k_b = 1 (nothing to rescale: a
 * zero-initialised head).  A NaN or an inf anywhere in a record makes that record's k_b NaN and with it its update; other records
 * are unaffected.
 * The order of summation is a function of (j, per_record) only -- not of B, of the record's position, of pointer alignment or of the
 * load width: with gx = clamp(ceil(per_record / 4096), 1, 64), quad q = j >> 2 of the record belongs to thread q mod (256 gx) of the
 * record's gx workgroups of 256, which adds its quads in increasing q and a quad's elements in increasing j; the 64 lanes of a wave
 * combine by an xor-shuffle tree (32, 16, .., 1), the 4 waves of a workgroup in index order, the gx workgroups in index order.  So k_b
 * is reproducible bit for bit (16-byte loads when both pointers are 16-byte aligned and per_record % 4 == 0, 4-byte loads otherwise).
 *
 * ccn_guidance_rescale: k_dev[b] = k_b, b < B.  scratch_dev: ccn_guidance_rescale_scratch_bytes bytes -- room for B factors first
 * (16-byte aligned; the handle state below keeps its factors there), then the workgroups' partial sums -- 16-byte aligned,
 * caller-owned, any contents (every slot read is written by the same call; two calls in flight need two scratches).  Two small launches
 * on `stream`: no floating-point atomics, no memset, never synchronises, allocates nothing, capturable.
 * CCN_EINVAL: a NULL tensor (out_u_dev included), a non-finite w, phi outside [0, 1] or NaN, B outside [1, 65535], per_record outside
 * [2, 2^34), a NULL, misaligned or short scratch. */
int ccn_guidance_rescale_scratch_bytes(int32_t B, int64_t per_record, size_t* bytes);
int ccn_guidance_rescale(const float* out_c_dev, const float* out_u_dev, float w, double phi,
                         int32_t B, int64_t per_record, float* k_dev,
                         void* scratch_dev, size_t scratch_bytes, void* stream);

/* ccn_x0_threshold plus gscale_dev (B floats, read when the kernels run): the quantile is taken on the x0 formed from k_b * y, the
 * bits the rescaled update clamps.  gscale_dev NULL: ccn_x0_threshold, bit for bit. */
int ccn_x0_threshold_rs(const float* x_dev, const float* out_c_dev, const float* out_u_dev,
                        int32_t pred, float w, float c0, float c1,
                        int32_t B, int64_t per_record, double p, float max_value,
                        float* thr_dev, void* scratch_dev, size_t scratch_bytes,
                        const float* gscale_dev, void* stream);

/* ccn_sampler_step_thr plus gscale_dev (one float per record): record b multiplies its (combined) output by gscale_dev[b] right
 * after the combine, and the state is walked record by record like the seeded and threshold forms.  gscale_dev NULL:
 * ccn_sampler_step_thr, bit for bit.  CCN_EINVAL: as for that entry. */
int ccn_sampler_step_rs(float* x_dev, float* x_dup_dev, float* x0_hist_dev,
                        const float* out_c_dev, const float* out_u_dev,
                        const float* noise_dev, const uint64_t* seeds_dev, uint32_t draw,
                        int64_t per_record, int32_t pred, float w,
                        const float* coef_host /* [5] */, float sigma, int64_t n,
                        const float* thr_dev, const float* gscale_dev, void* stream);

/* Handle state, exactly like ccn_set_dynamic_threshold: read by every ccn_sample* entry when it enqueues or captures, and part of
 * every captured graph's cache key (phi and the two scratch addresses), so toggling finds each mode's own graph on a shared workspace
 * and a run with phi == 0 replays the graph it had.  phi == 0: off (the default; scratch_dev may be NULL).  With phi in (0, 1] every
 * step of every GUIDED loop runs, after the network: ccn_guidance_rescale's two launches, the threshold launches (if a dynamic
 * threshold is set) with the factors, one ccn_sampler_step_rs launch.  An unguided run ignores it.  scratch_dev:
 * ccn_guidance_rescale_scratch_bytes(B, img_ch*H*W) bytes for the largest shape sampled with it (B images), 16-byte aligned, owned by
 * the caller and kept at its address while a graph captured with it is cached.  ccn_workspace_bytes is unchanged.
 * CCN_EINVAL: phi outside [0, 1] or NaN; with phi > 0 a NULL, misaligned or short scratch (a scratch too small for the shape of a
 * later guided ccn_sample* call is that call's CCN_EINVAL, as are more than 65535 images or C*H*W outside [2, 2^34)). */
int ccn_set_guidance_rescale(ccn_handle_t h, double phi, void* scratch_dev, size_t scratch_bytes);

/* ---- low-resolution guide ---------------------------------------------------------------------------------------------------------- *
 * (No reference counterpart.  ILVR, Choi et al. 2021; in x0 space the super-resolution case of DDNM, Wang et al. 2022:
 * x0' = x0 - A+(A x0 - g) with A the N x N block mean and A+ the replication of a block's value over its pixels.)  The decoder holds a
 * thumbnail g of the image, (B, C, H/N, W/N) fp32 with values expected in [-1, 1], and keeps every step's x0 prediction consistent
 * with it.  N: a power of two in 2..64 that divides H and W.  lambda = strength in (0, 1].  Per record, channel and N x N block:
 *   1. x0 is the prediction exactly as ccn_sampler_step_rs forms it: the guidance combine, the multiplication by gscale[b], the raw x0
 *      of either parameterisation, then the static clamp or clamp(., -thr[b], thr[b]) / thr[b].  |x0| <= 1 in every case.
 *   2. q(v) = the int64 nearest to v * 2^30, ties to even (the product is exact in fp32).  S = the int64 sum of q(x0) over the block;
 *      |S| <= 2^42 and integer addition is exact in any order, so S -- and with it everything below -- is reproducible bit for bit and
 *      independent of B, of the record's position, of pointer alignment and of the load width.
 *   3. m = (double)S / (N^2 2^30);  d = (float)((double)lambda * ((double)g - m)), rounded to fp32 once.
 *   4. x0' = x0 + d (one fp32 addition) for every pixel of the block, NOT clamped again; x0' replaces x0 in the update and in the
 *      multistep history; e is untouched, as with the clamp and the threshold.
 * Non-finite values are not looked for: the static clamp maps a NaN to -1 and +-inf to +-1; under a NaN threshold the record's x0 is
 * NaN, its d is unspecified and its update is NaN, as without a guide.
 *
 * ccn_block_mean: out_dev[p][i][j] = (float)m of clamp(x, -1, 1) for each of `planes` planes of H x W: the guide of an original, or the
 * thumbnail of a result.  ccn_lowres_delta: delta_dev, (B, C, H/N, W/N), = d above; out_u_dev (with w), thr_dev and gscale_dev are
 * nullable and mean what they mean to ccn_sampler_step_rs.  One launch each on `stream`: 64-bit integer LDS atomics only, no memset,
 * no scratch, never synchronises, allocates nothing, capturable; 16-byte loads when every tensor is 16-byte aligned, else 4-byte
 * loads, the same bits.
 * CCN_EINVAL: a NULL tensor, N not a power of two in 2..64, H or W not a multiple of N, strength outside (0, 1] or NaN, B outside
 * [1, 65535], C*H*W >= 2^34, an unknown pred. */
int ccn_block_mean(const float* x_dev, int64_t planes, int32_t H, int32_t W, int32_t N, float* out_dev, void* stream);
int ccn_lowres_delta(const float* x_dev, const float* out_c_dev, const float* out_u_dev,
                     int32_t pred, float w, float c0, float c1,
                     int32_t B, int32_t C, int32_t H, int32_t W, int32_t N,
                     const float* guide_dev, float strength,
                     const float* thr_dev, const float* gscale_dev,
                     float* delta_dev, void* stream);

/* ccn_sampler_step_rs plus the image's geometry and delta_dev (ccn_lowres_delta's table of the same state): element j of record b adds
 * the d of its block right after the clamp, and the state is walked record by record.  per_record must equal C*H*W.  delta_dev NULL:
 * ccn_sampler_step_rs, bit for bit (C, H, W, N are then not read).  CCN_EINVAL: as for that entry, and with delta_dev the N, H, W
 * rules above. */
int ccn_sampler_step_lr(float* x_dev, float* x_dup_dev, float* x0_hist_dev,
                        const float* out_c_dev, const float* out_u_dev,
                        const float* noise_dev, const uint64_t* seeds_dev, uint32_t draw,
                        int64_t per_record, int32_t pred, float w,
                        const float* coef_host /* [5] */, float sigma, int64_t n,
                        const float* thr_dev, const float* gscale_dev,
                        int32_t C, int32_t H, int32_t W, int32_t N, const float* delta_dev, void* stream);

/* Handle state, exactly like ccn_set_dynamic_threshold: read by every ccn_sample* entry when it enqueues or captures, and part of
 * every captured graph's cache key (the guide's address, N, strength, t_min and the scratch address; the guide's CONTENTS are read when
 * the kernels run, like seeds, so new contents at the same address replay the same graph).  N == 0: off (the default; the other
 * arguments are not read).  Otherwise guide_dev is (B, C, H/N, W/N) fp32 for the B images of the call, and every step i with
 * ts[i] >= t_min takes the split route: after the network the rescale launches (if set), the threshold launches (if set), one
 * ccn_lowres_delta launch, then one ccn_sampler_step_lr launch.  Guided, one d per image is formed from the combined output and both
 * halves of the state get the same update.  A step with ts[i] < t_min is exactly the step the run takes without a guide.
 * scratch_dev: ccn_lowres_guide_scratch_bytes(h, B, H, W, N) bytes for the largest shape sampled with it -- the delta table, then room
 * for the raw output of one state, which is used only by a run in which no guided, seeded or threshold scratch already holds it --
 * 16-byte aligned, owned by the caller and kept at its address while a graph captured with it is cached.  ccn_workspace_bytes is
 * unchanged.
 * CCN_EINVAL: N not 0 and not a power of two in 2..64; a NULL guide; strength outside (0, 1] or NaN; t_min < 0; a NULL, misaligned or
 * short scratch (a scratch too small for the shape of a later ccn_sample* call is that call's CCN_EINVAL, as are H or W not a
 * multiple of N and more than 65535 images). */
int ccn_set_lowres_guide(ccn_handle_t h, const float* guide_dev, int32_t N, float strength, int32_t t_min,
                         void* scratch_dev, size_t scratch_bytes);
int ccn_lowres_guide_scratch_bytes(ccn_handle_t h, int32_t B, int32_t H, int32_t W, int32_t N, size_t* bytes);

/* ---- the sampler loop, described by one record ------------------------------------------------------------------------------------ *
 * Everything a run of the loop is a function of besides the handle (its prediction and dynamic threshold are read like by every
 * other ccn_sample* entry), the tensors and the shape.  ccn_sample, ccn_sample_eta, ccn_sample_guided, ccn_sample_seeded,
 * ccn_sample_guided_seeded, ccn_sample_ms and ccn_sample_guided_ms above are fixed-shape conveniences: each fills this record from
 * its arguments and calls ccn_sample_run; their comments hold the formulas, the ownership rules and the graph keys, which are not
 * restated here.  A new caller binds this entry alone.  Plain C, natural alignment, no bit-fields: a ctypes.Structure with the same
 * fields in the same order mirrors it.  An absent feature is a NULL pointer or a 0; a field the run does not use is ignored.
 *   size             sizeof(ccn_sampler_run_t) as the caller compiled it; any other value is CCN_EINVAL;
 *   steps, ts_host   the timestep table, ts_host[steps] (ccn_sample);
 *   coef_host        [steps][coef_cols] fp32;  coef_cols  4: c0..c3 (ccn_sample), 5: the multistep table c0..c4 (ccn_sample_ms),
 *                    which needs x0_hist_dev and excludes sigma_host, noise_dev and seeds_dev;
 *   sigma_host       NULL: eta = 0.  Else [steps], together with ONE of
 *   noise_dev        the (steps,B,img_ch,H,W) draws made by the caller (ccn_sample_eta), or
 *   seeds_dev        B x uint64 on the device, 8-byte aligned: step i adds draw 1 + i of each record (ccn_sample_seeded); with
 *                    sigma_host NULL the seeds are not read and the run is the unseeded one;
 *   guided, w,       guided != 0: classifier-free guidance of finite scale w at plan batch 2B (ccn_sample_guided); z_null_dev
 *   z_null_dev       (z_dim,), NULL: zeros.  workspace_dev is then the one of ccn_workspace_bytes(h, 2*B, H, W, steps);
 *   out_scratch_dev  the raw network output of the steps that update in a launch of their own: 2*B*img_ch*H*W floats when guided
 *                    (the eps scratch of ccn_sample_guided), B*img_ch*H*W when seeds_dev draws (the output scratch of
 *                    ccn_sample_seeded), 16-byte aligned; not read by any other run -- under a dynamic threshold those keep the raw
 *                    output in the head of the handle's threshold scratch;
 *   x0_hist_dev      the multistep sampler's x0 history, B*img_ch*H*W floats, 16-byte aligned (ccn_sample_ms).
 * Every pointer with _dev is owned by the caller like the workspace and stays at its address while a captured graph is cached.
 * The captured graph is cached per workspace and per everything above that a launch holds by value or by address (the tables bit
 * for bit; not z_null_dev, which is copied on every call) plus the handle's prediction and dynamic threshold: the keys the seven
 * entries document, and a run reached through an entry and the same run described here share one graph.
 * CCN_EINVAL: what the entries refuse (a NULL table, sigma without noise or seeds or noise without sigma, a non-finite w, a missing
 * or misaligned scratch, history or seeds, a non-finite multistep coefficient, c4 != 0 on step 0, C*H*W >= 2^34 with seeds), a NULL
 * run or a wrong size, coef_cols other than 4 or 5, and the runs no entry expresses: a fifth coefficient column together with
 * sigma, noise or seeds, and noise_dev together with seeds_dev. */
typedef struct ccn_sampler_run {
    uint32_t size;
    int32_t steps;
    const int32_t* ts_host;
    const float* coef_host;
    int32_t coef_cols;
    const float* sigma_host;
    const float* noise_dev;
    const uint64_t* seeds_dev;
    int32_t guided;
    float w;
    const float* z_null_dev;
    float* out_scratch_dev;
    float* x0_hist_dev;
} ccn_sampler_run_t;

int ccn_sample_run(ccn_handle_t h, const ccn_sampler_run_t* run,
                   const float* z_dev, const float* x_T_dev, float* x_out_dev,
                   int32_t B, int32_t H, int32_t W,
                   void* workspace_dev, size_t workspace_bytes, void* stream, int32_t use_graph);

/* NoiseScheduler.q_sample (diffusion/scheduler.py:46-49): out[b] = a[b]*x0[b] + s[b]*noise[b];
 * a_dev/s_dev are the gathered per-sample coefficients, (B,) fp32; per_sample = C*H*W. */
int ccn_q_sample(float* out_dev, const float* x0_dev, const float* noise_dev,
                 const float* a_dev, const float* s_dev, int32_t B, int64_t per_sample, void* stream);

/* NoiseScheduler.predict_x0_from_eps (diffusion/scheduler.py:51-55): out[b] = (x_t[b] - s[b]*eps[b]) / a[b]. */
int ccn_predict_x0(float* out_dev, const float* x_t_dev, const float* eps_dev,
                   const float* a_dev, const float* s_dev, int32_t B, int64_t per_sample, void* stream);

/* ---- reconstruction scores on the device (eval/metrics.py: _to_uint8, psnr_u8, _ssim_plane) ---- */

/* Stateless like the optimiser tail: raw buffers, no handle, no allocation, never synchronises, capturable.
 * Per record b the two launches (partials per workgroup, then one wave per record that adds them in index order) write
 *     out_dev[b][0] = sum over C*H*W of (a - b)^2 on the two uint8 images, an exact integer (PSNR = 20 log10(255 / sqrt(sse / n)))
 *     out_dev[b][1] = SSIM with skimage's defaults: 7 x 7 uniform window, sample covariance (49/48), K1 = 0.01, K2 = 0.03,
 *                     data_range = 255, mean over the channels and over the (H-6) x (W-6) window positions inside the image
 * as float64.  The window sums are exact integers, the quotient and the sums over positions are fp64 in a fixed order without
 * atomics: results are bit-reproducible, do not depend on pointer alignment (16-byte accesses are used when W % 16 == 0 and the
 * image pointers are 16-byte aligned, single-pixel accesses otherwise) nor on what else is in the batch.  Identical images give
 * exactly 0 and 1.0.  H < 7 or W < 7: there is no window position, SSIM is NaN and the SSE is still produced.
 * The fp32 reconstruction (NCHW, nominally in [-1, 1]; the sampler's unclamped output is fine) is converted as _to_uint8 does:
 * (x + 1.0f) * 127.5f as two separately rounded fp32 operations, clipped to [0, 255], truncated -- byte for byte numpy's and
 * torch's result on finite input.  Non-finite input is this build's choice: +inf gives 255, -inf gives 0, NaN gives 0.
 * scratch_dev: at least ccn_score_scratch_bytes bytes (16 per workgroup; it depends on the tiling, hence the query), 8-byte aligned.
 * CCN_EINVAL: a NULL buffer (recon_u8_out_dev may be NULL), a non-positive dimension, scratch too small or not 8-byte aligned,
 * recon_dev not 4-byte aligned. */
int ccn_score_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W, size_t* bytes);

/* recon_dev (B,C,H,W) fp32; orig_u8_dev (B,C,H,W) uint8; recon_u8_out_dev: NULL, or (B,C,H,W) uint8 that receives the converted
 * reconstruction; out_dev (B,2) float64, 8-byte aligned. */
int ccn_psnr_ssim_f32(const float* recon_dev, const uint8_t* orig_u8_dev, uint8_t* recon_u8_out_dev, double* out_dev,
                      int32_t B, int32_t C, int32_t H, int32_t W, void* scratch_dev, size_t scratch_bytes, void* stream);

/* The same for a reconstruction that is already uint8 (two stored images, or the bytes ccn_psnr_ssim_f32 wrote): the same kernel
 * without the conversion, the same bits in out_dev. */
int ccn_psnr_ssim_u8(const uint8_t* recon_u8_dev, const uint8_t* orig_u8_dev, double* out_dev,
                     int32_t B, int32_t C, int32_t H, int32_t W, void* scratch_dev, size_t scratch_bytes, void* stream);

/* ---- operator-level entry points (what the reference's unit tests exercise) ------------------ */

/* FiLM.forward (models/blocks.py:22-25) with explicit parameters: y = x*(1 + Ws h + bs) + (Wh h + bh).
 * x/y (B,C,H,W) fp32 NCHW; h (B,D); Ws/Wh (C,D); bs/bh (C,). All device pointers.
 * scratch_dev: at least 2*B*C floats. */
int ccn_film_forward(const float* x_dev, const float* h_dev, const float* ws_dev, const float* bs_dev,
                     const float* wh_dev, const float* bh_dev, float* y_dev,
                     int32_t B, int32_t C, int32_t H, int32_t W, int32_t D,
                     float* scratch_dev, void* stream);

/* ResBlock.forward (models/blocks.py:40-44) of the block whose state-dict prefix is `prefix`
 * ("down.0", "mid1", "up.4", ...), using the handle's committed weights and arithmetic mode.
 * x/y (B,C,H,W) fp32 NCHW; h (B,time_dim) fp32.  Workspace: ccn_workspace_bytes(h,B,H,W,1) is enough
 * for any block at resolution HxW. */
int ccn_resblock_forward(ccn_handle_t h, const char* prefix, const float* x_dev, const float* cond_dev,
                         float* y_dev, int32_t B, int32_t H, int32_t W,
                         void* workspace_dev, size_t workspace_bytes, void* stream);

/* timestep_embedding(t, dim) (models/unet.py:22-39): (n,) int64 -> (n,dim) fp32, [cos | sin] order. */
int ccn_timestep_embedding(const int64_t* t_dev, float* out_dev, int32_t n, int32_t dim, void* stream);

/* ---- introspection (tests, profiling) -------------------------------------------------------- */

/* After ccn_forward / ccn_sample: copy an intermediate activation out as fp32 NCHW.  Names are the
 * reference module paths: "in_conv", "down.0" ... "mid2", "up.8" (after the skip add), and
 * "<block>.film" for the tensor entering norm2.  Synchronises `stream`. */
int ccn_read_activation(ccn_handle_t h, const char* name, float* out_dev, size_t out_elems, void* stream);

/* Device-side failures are sticky: a kernel that detects a broken hand-off (a split-K partial tile that never arrived) sets a
 * bit in the handle's error word and carries on; the NEXT call that takes the handle -- or this one, e.g. after the caller has
 * synchronised its stream -- returns CCN_EHIP once and clears it.  Results enqueued since the last successful check are then
 * invalid.  (The reference has no counterpart: torch raises asynchronous device errors the same way, at the next call.) */
int ccn_poll_errors(ccn_handle_t h);

/* Per-kernel-family device time of the next ccn_sample / ccn_forward calls, measured with HIP events
 * recorded on the launch stream around every kernel (the loop then runs launch by launch instead of
 * as one graph).  ccn_profile_read synchronises, then fills arrays of capacity `cap`: family name,
 * summed milliseconds, launch count, and the summed ALGORITHMIC flops (2*MAC) and HBM bytes of those
 * launches; *n receives the number of families. */
int ccn_profile_enable(ccn_handle_t h, int32_t on);
int ccn_profile_read(ccn_handle_t h, const char** names, float* ms, int32_t* calls,
                     double* flops, double* bytes, int32_t cap, int32_t* n);

/* Algorithmic work of one UNet forward for (B,H,W): conv/linear FLOPs (2*MAC) and minimal HBM bytes
 * under this handle's storage dtype. */
int ccn_algorithmic_work(ccn_handle_t h, int32_t B, int32_t H, int32_t W, double* flops, double* bytes);

/* ---- training step (train/diffusion_train.py:119-124,137-140) --------------------------------- *
 * The reference trains with `eps_hat = net(x_t, z, t); loss = F.mse_loss(eps_hat, noise); loss.backward(); opt.step()`.
 * A trainer handle reads the parameters from ONE flat fp32 device buffer owned by the caller (the entries of
 * CLIPCondUNet.state_dict(), in registration order, each at the offset ccn_train_param_info reports -- a torch caller makes
 * every nn.Parameter a view into it) and accumulates gradients into a second flat buffer of the same layout.
 * Arithmetic mode as for inference: CCN_DTYPE_F32 (parity) or CCN_DTYPE_BF16 (activations and conv operands in bf16,
 * fp32 accumulation, fp32 GroupNorm statistics, fp32 gradients and optimiser state: what torch.autocast(bfloat16) does
 * at train/diffusion_train.py:121). */
typedef struct ccn_trainer_s* ccn_trainer_t;

/* net = CLIPCondUNet(...).to(device); net.train() (train/diffusion_train.py:103,109) */
int ccn_train_create(const ccn_config_t* cfg, ccn_trainer_t* out);
int ccn_train_destroy(ccn_trainer_t tr);

/* Number of parameters, total floats of the flat buffer; i-th key / shape / offset (in floats) into the flat buffer. */
int ccn_train_num_params(ccn_trainer_t tr, int32_t* n, int64_t* total_floats);
int ccn_train_param_info(ccn_trainer_t tr, int32_t i, const char** name, int64_t shape[4], int32_t* ndim, int64_t* offset);

/* Scratch for one forward+backward at this shape (every activation of the forward is kept for the backward). */
int ccn_train_workspace_bytes(ccn_trainer_t tr, int32_t B, int32_t H, int32_t W, size_t* bytes);

/* eps_hat = net(x_t, z, t) (train/diffusion_train.py:123; models/unet.py:81-106), activations kept in the workspace.
 * x_t_dev (B,img_ch,H,W) fp32 NCHW; z_dev (B,z_dim); t_dev (B,) int64; eps_dev (B,img_ch,H,W) fp32 NCHW. */
int ccn_train_forward(ccn_trainer_t tr, const float* params_dev, const float* x_t_dev, const float* z_dev,
                      const int64_t* t_dev, float* eps_dev, int32_t B, int32_t H, int32_t W,
                      void* workspace_dev, size_t workspace_bytes, void* stream);

/* The backward pass of that forward (loss.backward(), train/diffusion_train.py:137) for a given d loss / d eps_hat
 * (B,img_ch,H,W) fp32 NCHW: grads_dev[offset_i ...] += d loss / d param_i for every parameter (the caller zeroes the
 * buffer when it wants plain gradients, as opt.zero_grad does at :140).  Must follow ccn_train_forward with the same
 * shape, workspace and x_t_dev / z_dev contents; the parameters must not have changed in between. */
int ccn_train_backward(ccn_trainer_t tr, const float* params_dev, float* grads_dev, const float* x_t_dev,
                       const float* z_dev, const float* d_eps_dev, int32_t B, int32_t H, int32_t W,
                       void* workspace_dev, size_t workspace_bytes, void* stream);

/* The same backward for a data-parallel caller that overlaps the gradient all-reduce with it (DistributedDataParallel's buckets):
 * cb(user, lo, hi) is called from the calling thread as soon as every gradient in the flat range [lo, hi) (floats) is complete
 * in stream order on `stream` -- the caller enqueues its collective on that range right there.  Ranges are disjoint, handed out
 * from the end of the buffer towards its start (the backward visits the layers in reverse registration order), each at least
 * bucket_floats long except the last, and together cover the whole buffer.  The FiLM linears are then differentiated block by
 * block instead of in one grouped launch at the end. */
typedef void (*ccn_grad_ready_cb)(void* user, int64_t lo_float, int64_t hi_float);
int ccn_train_backward_bucketed(ccn_trainer_t tr, const float* params_dev, float* grads_dev, const float* x_t_dev,
                                const float* z_dev, const float* d_eps_dev, int32_t B, int32_t H, int32_t W,
                                void* workspace_dev, size_t workspace_bytes, void* stream, int64_t bucket_floats,
                                ccn_grad_ready_cb cb, void* user);

/* on != 0: ccn_train_forward / ccn_train_backward capture their launch sequence into a hipGraph the first time they see a set of
 * pointer arguments (parameters, gradients, inputs, outputs, workspace) and replay it afterwards -- for callers that keep their
 * buffers at fixed addresses (a training loop with static input / output tensors).  Off by default. */
int ccn_train_set_graph(ccn_trainer_t tr, int32_t on);

/* Per-family timing of the training step (HIP events on the stream the launches go to): enable, run steps, read.
 * names/ms/calls/flops/bytes: arrays of `cap` (>= 16) entries; flops = algorithmic conv FLOPs of the family's launches,
 * bytes = algorithmic HBM bytes of the bandwidth-bound families (0 for the others).
 * Reading synchronises the device and resets the counters. */
int ccn_train_profile_enable(ccn_trainer_t tr, int32_t on);
int ccn_train_profile_read(ccn_trainer_t tr, const char** names, float* ms, int32_t* calls, double* flops,
                           double* bytes, int32_t cap, int32_t* n);

/* F.mse_loss(eps_hat, noise) (train/diffusion_train.py:124) and its gradient: *loss_dev = mean((eps - target)^2),
 * d_eps_dev = 2 (eps - target) / n (may be NULL).  scratch_dev: at least 1024 floats. */
int ccn_mse_loss_grad(const float* eps_dev, const float* target_dev, int64_t n, float* loss_dev, float* d_eps_dev,
                      float* scratch_dev, void* stream);

/* The reference's default training objective (train/diffusion_train.py:124-129 with diffusion/scheduler.py:51-55) and its
 * gradient in one pass, without storing x0_pred:
 *     x0_pred = predict_x0_from_eps(x_t, t, eps_hat).clamp(-1, 1)
 *     loss    = F.mse_loss(eps_hat, noise) + recon_w * F.l1_loss(x0_pred, x0) + tv_w * total_variation(x0_pred)
 * eps_dev / noise_dev / x_t_dev / x0_dev / d_eps_dev: (B,C,H,W) fp32 NCHW; a_dev / s_dev: (B,) fp32, sqrt_alphas_cumprod[t_b] and
 * sqrt_one_minus_alphas_cumprod[t_b] (what ccn_q_sample and ccn_predict_x0 take).  x0_pred is evaluated exactly as ccn_predict_x0
 * does, the clamp passes gradient on -1 <= raw <= 1 (bounds included) and sgn(0) = 0, as torch's backward of clamp and abs.
 * loss_dev[4] = total, mse, l1, tv; l1 and tv are reported UNWEIGHTED (total = mse + recon_w l1 + tv_w tv).  d_eps_dev = d total /
 * d eps_hat (may be NULL).  recon_w, tv_w >= 0; with both 0 the pass is ccn_mse_loss_grad's (bit-identical d_eps and mse; l1 and
 * tv are then not evaluated and read 0).  H, W >= 2 (CCN_EINVAL otherwise: torch's TV is NaN there).  scratch_dev: at least 8192
 * floats, 8-byte aligned.  Sums are accumulated in fp64 in a fixed order: results are bit-reproducible.  Never synchronises. */
int ccn_diffusion_loss_grad(const float* eps_dev, const float* noise_dev, const float* x_t_dev, const float* x0_dev,
                            const float* a_dev, const float* s_dev, int32_t B, int32_t C, int32_t H, int32_t W,
                            float recon_w, float tv_w, float* loss_dev /* [4]: total, mse, l1, tv */,
                            float* d_eps_dev /* may be NULL */, float* scratch_dev, void* stream);

/* The same objective for a network that predicts v (CCN_PRED_V; no reference counterpart).  Arguments, layout of loss_dev, the fixed
 * order fp64 sums, bit-reproducibility, the H, W >= 2 rule and the scratch contract are ccn_diffusion_loss_grad's; what differs:
 *     target  = a*noise - s*x0                       -- fp32: two products and one subtraction, each rounded
 *     mse     = mean((v_hat - target)^2)
 *     x0_pred = clamp(a*x_t - s*v_hat, -1, 1)        -- fp32, each op rounded; l1 and tv act on it as above
 *     d total / d v_hat = 2 (v_hat - target) / n + [-1 <= raw <= 1] dL/dx0_pred * (-s)
 * so the auxiliary gradient carries the factor s <= 1 where the eps form has s/a (up to 6.4e4).  With recon_w == tv_w == 0 d_v and
 * mse are bit-identical to ccn_mse_loss_grad(v_hat, target) on a target materialised by those three fp32 ops, and x_t_dev is not
 * read (it may then be NULL). */
int ccn_diffusion_loss_grad_v(const float* v_dev, const float* noise_dev, const float* x_t_dev, const float* x0_dev,
                              const float* a_dev, const float* s_dev, int32_t B, int32_t C, int32_t H, int32_t W,
                              float recon_w, float tv_w, float* loss_dev /* [4]: total, mse, l1, tv */,
                              float* d_v_dev /* may be NULL */, float* scratch_dev, void* stream);

/* One torch.optim.AdamW step over a flat buffer (train/diffusion_train.py:105,138): p *= 1 - lr*wd;
 * m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; p -= lr/(1-b1^step) * m / (sqrt(v)/sqrt(1-b2^step) + eps). step >= 1. */
int ccn_adamw_step(float* params_dev, const float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, void* stream);
/* The same step followed by opt.zero_grad() (train/diffusion_train.py:138-139) in the same pass: every gradient is read once and
 * its slot left at zero (one launch and one 4-byte write per parameter instead of a second pass over the buffer). */
int ccn_adamw_step_zero_grad(float* params_dev, float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t n,
                             float lr, float beta1, float beta2, float eps, float weight_decay, int32_t step, void* stream);

/* ---- step guard: loss scaling, the skipped step on non-finite gradients, gradient-norm clipping ---------------------------- *
 * The reference ends its loop body with `scaler.scale(loss).backward(); scaler.step(opt); scaler.update()`
 * (train/diffusion_train.py:137-139).  Here the whole decision lives in this 64-byte control block in DEVICE memory: nothing is read
 * back to the host, so the step stays asynchronous.  Semantics are torch's: torch.amp.GradScaler, then
 * torch.nn.utils.clip_grad_norm_(norm_type=2), then torch.optim.AdamW whose step count advances on APPLIED steps only.
 * A torch caller views the block as a tensor of 16 int32 words (words 0-5 reinterpreted as fp32). */
typedef struct ccn_step_guard_s {
    float scale;                /* the loss scale: d loss / d eps_hat is multiplied by it before the backward */
    float inv_scale;            /* (float)(1 / (double)scale) */
    float grad_norm;            /* last ccn_grad_guard: L2 norm of the UNSCALED gradient (inf / NaN on a skipped step) */
    float grad_mul;             /* last ccn_grad_guard: inv_scale * clip coefficient -- what ccn_adamw_step_guarded multiplies g by */
    float bc1;                  /* last ccn_grad_guard: 1 - beta1^step, step = good_steps (before the call) + 1 */
    float bc2_sqrt;             /*                      sqrt(1 - beta2^step) */
    int32_t apply;              /* last ccn_grad_guard: 1 = every gradient element finite, the step is applied; 0 = skipped */
    int32_t good_steps;         /* applied steps so far (AdamW's step count) */
    int32_t skipped_steps;      /* skipped steps so far */
    int32_t growth_tracker;     /* consecutive applied steps since the scale last changed (GradScaler's _growth_tracker) */
    int32_t reserved[6];
} ccn_step_guard_t;

/* scaler = GradScaler(init_scale) (train/diffusion_train.py:106), or its load_state_dict: writes the whole block (one small launch on
 * `stream`, no host memory is read later).  init_scale > 0 and finite; the three counters >= 0. */
int ccn_step_guard_init(void* guard_dev, float init_scale, int32_t growth_tracker0, int32_t good_steps0,
                        int32_t skipped_steps0, void* stream);

/* The decision of scaler.step + scaler.update (train/diffusion_train.py:138-139) for the n gradients of a flat buffer, which hold
 * d (scale * loss): one read of the buffer sums (g * inv_scale)^2 in fp64 (a fixed number of per-workgroup partials that depends on
 * n only, added in a fixed order, no atomics: bit-reproducible), then one wave writes into the block
 *     apply     = the sum is finite (fp64 cannot overflow here, so: no element is inf or NaN)
 *     grad_norm = sqrt(sum);  grad_mul = inv_scale * min(1, max_grad_norm / (grad_norm + 1e-6))   (max_grad_norm <= 0: no clipping)
 *     bc1, bc2_sqrt for step = good_steps + 1
 * and commits the state: good_steps += apply, skipped_steps += !apply, and GradScaler.update(): on a skip scale *= backoff_factor and
 * growth_tracker = 0, otherwise ++growth_tracker and, when it reaches growth_interval, scale *= growth_factor (if that is finite) and
 * growth_tracker = 0.  The gradients themselves are not touched.  scratch_dev: at least 4096 floats, 8-byte aligned.
 * 0 <= beta < 1, growth_factor and backoff_factor > 0, growth_interval >= 1.  Never synchronises, allocates nothing: capturable. */
int ccn_grad_guard(const float* grads_dev, int64_t n, void* guard_dev, float max_grad_norm, float beta1, float beta2,
                   float growth_factor, float backoff_factor, int32_t growth_interval, float* scratch_dev, void* stream);

/* opt.step() + opt.zero_grad() (train/diffusion_train.py:138,140) under the decision ccn_grad_guard left in the block, which this
 * call only reads: with apply == 1 it is ccn_adamw_step_zero_grad with g * grad_mul for g and the block's bias corrections; with
 * apply == 0 parameters and both moments stay bit for bit (no weight decay either) and the gradients are only zeroed.  16-byte
 * accesses when the four buffers share their alignment modulo 16 bytes, 4-byte accesses otherwise.  Never synchronises. */
int ccn_adamw_step_guarded(float* params_dev, float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t n,
                           float lr, float beta1, float beta2, float eps, float weight_decay, const void* guard_dev,
                           void* stream);

/* ---- weight EMA fused into the AdamW step ------------------------------------------------------------------------------------- *
 * A diffusion decoder is sampled from an exponential moving average of its parameters: in torch,
 *     ema = torch.optim.swa_utils.AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(decay))
 *     ... opt.step(); ema.update_parameters(net)
 * (swa_utils.py: the first update_parameters copies the parameters, every later one is `ema.lerp_(p, 1 - decay)`; n_averaged counts
 * them).  Under the step guard above the host does not know whether a step was applied, so the average is taken on the device, in
 * the AdamW pass itself, and this 32-byte block in DEVICE memory is its state.  A torch caller views it as 8 int32 words (word 0
 * reinterpreted as fp32). */
typedef struct ccn_ema_state_s {
    float weight;               /* last ccn_adamw_step_ema: the lerp weight of this update, 1 - decay_u */
    int32_t apply;              /* last ccn_adamw_step_ema: 1 = the step was applied and averaged; 0 = skipped (the guard's apply) */
    int32_t first;              /* last applied update was the first one: ema = p (AveragedModel's n_averaged == 0 branch) */
    int32_t updates;            /* EMA updates done so far (AveragedModel.n_averaged) */
    int32_t reserved[4];
} ccn_ema_state_t;

/* AveragedModel(...)'s n_averaged = 0, or its load_state_dict: writes the whole block with updates = updates0 >= 0 (one small
 * launch on `stream`).  The average itself is the caller's buffer: with updates0 == 0 its contents do not matter. */
int ccn_ema_init(void* ema_state_dev, int32_t updates0, void* stream);

/* opt.step() [+ opt.zero_grad()] (train/diffusion_train.py:138,140) followed by ema.update_parameters(net), as one pass over the five
 * flat buffers.  Two launches: a one-wave tick, the only writer of the block, sets
 *     apply  = guard_dev ? guard->apply : 1
 *     if apply:  first = (updates == 0);  weight = ema_warmup ? max(w, 9 / (10 + updates)) : w;  updates += 1
 * with w = (float)(1.0 - ema_decay), the fp32 weight get_ema_multi_avg_fn(decay) hands to lerp_ (ema_decay is a double so that
 * Python's 1 - decay is formed exactly as torch forms it); the warm-up is decay_u = min(decay, (1 + u) / (10 + u)), written as
 * its complement.  Then the fused kernel: guard_dev == NULL: ccn_adamw_step's (zero_grad == 0) or ccn_adamw_step_zero_grad's update
 * with bias corrections for `step`; guard_dev != NULL: ccn_adamw_step_guarded's under the block ccn_grad_guard has just written
 * (`step` ignored, zero_grad must be non-zero).  p, m, v (and g) end with the same bits as from those entries.  Per element then
 * ema = p_new on the first update, ema = fma(weight, p_new - ema, ema) afterwards.  With apply == 0 parameters, moments and average
 * stay bit for bit (the average is neither read nor written), the count of updates does not move, and the gradients are zeroed.
 * 16-byte accesses when the five buffers share their alignment modulo 16 bytes, 4-byte accesses otherwise.  n == 0 does nothing.
 * CCN_EINVAL: a NULL buffer or block, n < 0, ema_decay outside [0, 1), zero_grad == 0 with a guard, step < 1 without one.
 * Never synchronises, allocates nothing: capturable. */
int ccn_adamw_step_ema(float* params_dev, float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* ema_dev, int64_t n,
                       float lr, float beta1, float beta2, float eps, float weight_decay,
                       int32_t step,            /* used when guard_dev == NULL, as ccn_adamw_step's */
                       int32_t zero_grad,       /* must be non-zero when guard_dev != NULL */
                       double ema_decay, int32_t ema_warmup,
                       const void* guard_dev    /* NULL, or the block ccn_grad_guard has just written */,
                       void* ema_state_dev, void* stream);

const char* ccn_last_error(void);
const char* ccn_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CCN_HIP_H */
