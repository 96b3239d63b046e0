// The stateless tail of the training step (train/diffusion_train.py:124-129,137-139): the loss and its gradient, the step guard,
// AdamW and the weight EMA.  Kernels, their launchers and the extern "C" entry points of include/ccn_hip.h in one file: none of it
// touches a ccn_trainer_t, and nothing outside this file calls into it.
//   mse_*, objective_*   mean((eps - target)^2), and the reference's default objective MSE + L1 + TV in one pass, with d loss / d eps
//                        (objective_partial_kernel<VEC, VP>: VP = the same objective for a network that predicts v)
//   grad_guard_*         GradScaler's skipped step and scale update, clip_grad_norm_, decided on the device (ccn_step_guard_t)
//   ema_tick_kernel      the EMA's weight and count of updates for this step (ccn_ema_state_t)
//   adamw_kernel         torch.optim.AdamW over the flat buffers, <GUARDED, EMA, ZERO, VEC>: under the guard's decision, with the
//                        EMA of the updated parameters, zeroing the gradients, on 16-byte quads -- one pass whichever are set
#include "ccn_device.h"
#include "../../include/ccn_hip.h"

#include <cmath>
#include <cstdint>
#include <string>

namespace ccn {
namespace {

// ---- loss ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mse_partial_kernel(const float* __restrict__ eps, const float* __restrict__ target, int64_t n, float inv_n,
                                                           float* __restrict__ d_eps, float* __restrict__ scratch)
{
    __shared__ double red[4];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float d = eps[i] - target[i];
        s += (double)d * (double)d;
        if (d_eps) d_eps[i] = 2.0f * d * inv_n;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) scratch[blockIdx.x] = (float)((red[0] + red[1]) + (red[2] + red[3]));
}
__global__ void mse_final_kernel(const float* __restrict__ scratch, int nb, double inv_n, float* __restrict__ loss)
{
    // one wave, fixed order: lane l sums partials l, l + 64, ... in fp64, then a shuffle tree (a single thread walking the 1024 partials
    // took 46 us between the forward and the backward of the step)
    if (blockIdx.x) return;
    double s = 0.0;
    for (int i = (int)threadIdx.x; i < nb; i += 64) s += (double)scratch[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (threadIdx.x == 0) *loss = (float)(s * inv_n);
}
hipError_t launch_mse_loss_grad(const float* eps, const float* target, int64_t n, float* loss, float* d_eps, float* scratch, hipStream_t s)
{
    const int nb = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(mse_partial_kernel, dim3(nb), dim3(256), 0, s, eps, target, n, (float)(1.0 / (double)n), d_eps, scratch);
    hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(64), 0, s, scratch, nb, 1.0 / (double)n, loss);
    return hipGetLastError();
}

// ---- the reference's default objective: MSE + recon_w L1(x0_pred, x0) + tv_w TV(x0_pred) (train/diffusion_train.py:124-129) ------
// x0_pred = clamp((x_t - s eps) / a, -1, 1) is never stored: a workgroup takes OBJ_TY rows x OBJ_TX columns of one (b, c) plane,
// recomputes p = x0_pred for that tile plus a one-pixel halo into LDS (the same expression and op order as predict_x0_kernel, so the
// clamp mask is the one ccn_predict_x0 + torch.clamp would give) and differentiates the 4-neighbour stencil from LDS:
//   dL/dp = recon_w sgn(p - x0) / n + tv_w [ (sgn(p - p_up) - sgn(p_down - p)) / n_h + (sgn(p - p_left) - sgn(p_right - p)) / n_w ]
//   d_eps = 2 (eps - noise) / n + [-1 <= raw <= 1] dL/dp (-s / a)
// with sgn(0) = 0 (torch's abs backward), the clamp bounds inclusive (torch's clamp backward) and neighbours outside the image
// absent.  Each pixel owns its down and right difference in the TV sums.  The LDS row is laid out so that the tile's interior
// starts on a 16-byte boundary (columns 3 and OBJ_TX + 4 are the left / right halo): every interior access is a ds_*_b128.
// Sums: fp64 per thread -> wave shuffle tree -> 4 doubles per workgroup in scratch -> objective_final_kernel adds them in a fixed
// order: bit-reproducible from run to run, no atomics.
constexpr int OBJ_TX = 128, OBJ_TY = 16, OBJ_LD = OBJ_TX + 8, OBJ_MAX_WG = 1024;

__device__ __forceinline__ float sgnf(float v) { return (float)((v > 0.f) - (v < 0.f)); }

// VEC: W % 4 == 0 and every tensor 16-byte aligned, so that a quad of columns is inside the image as a whole and is one 16-byte access
template <bool VEC> __device__ __forceinline__ void obj_load4(const float* __restrict__ p, int cnt, float v[4])
{
    if (VEC) {
        const f32x4 t = *(const f32x4*)p;
        v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < cnt ? p[j] : 0.f;
    }
}

// VP: the v-parameterisation (ccn_diffusion_loss_grad_v): `eps` holds v_hat, raw x0_pred = a x_t - s v_hat, the MSE target is
// a noise - s x0 (three fp32 ops, formed in registers), and d raw / d v_hat = -s.  Everything else is shared.
template <bool VP> __device__ __forceinline__ float obj_raw_x0(float xt, float e, float ca, float cs)
{
    if (VP) return __fsub_rn(__fmul_rn(ca, xt), __fmul_rn(cs, e));
    return __fdiv_rn(__fsub_rn(xt, __fmul_rn(cs, e)), ca);
}
template <bool VEC, bool VP>
__global__ __launch_bounds__(256) void objective_partial_kernel(const float* __restrict__ eps, const float* __restrict__ noise,
                                                                 const float* __restrict__ xt, const float* __restrict__ x0,
                                                                 const float* __restrict__ a, const float* __restrict__ sg, int C, int H, int W,
                                                                 int nby, int nbx, int ntiles, float inv_n, float c_l1, float c_tvh, float c_tvw,
                                                                 float* __restrict__ d_eps, double* __restrict__ scratch)
{
    __shared__ __attribute__((aligned(16))) float tile[OBJ_TY + 2][OBJ_LD];
    __shared__ double red[4][4];
    const int tid = threadIdx.x, q = tid & 31, rr = tid >> 5;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};                      // sum (eps-noise)^2, sum |p-x0|, sum |p_down-p|, sum |p_right-p|
    for (int tix = blockIdx.x; tix < ntiles; tix += gridDim.x) {
        const int bx = tix % nbx, by = (tix / nbx) % nby, plane = tix / (nbx * nby);
        const int xs = bx * OBJ_TX, ys = by * OBJ_TY;
        const float ca = a[plane / C], cs = sg[plane / C];
        const size_t pbase = (size_t)plane * H * W;
        const int gx = xs + 4 * q;
        const int cw = gx >= W ? 0 : (W - gx < 4 ? W - gx : 4);                 // columns of this thread's quad inside the image
        float e[2][4];
        unsigned inside[2] = {0u, 0u};                                           // bit j: -1 <= raw <= 1 at column gx + j
        // ---- p of the tile's own rows (eps stays in registers for the second phase), then the halo rows and columns ---------
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int r = rr + 8 * k, gy = ys + r;
            if (gy < H && cw > 0) {
                const size_t o = pbase + (size_t)gy * W + gx;
                float v[4];
                obj_load4<VEC>(eps + o, cw, e[k]); obj_load4<VEC>(xt + o, cw, v);
                f32x4 p;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float raw = obj_raw_x0<VP>(v[j], e[k][j], ca, cs);
                    inside[k] |= (raw >= -1.0f && raw <= 1.0f) ? (1u << j) : 0u;
                    p[j] = fminf(fmaxf(raw, -1.0f), 1.0f);
                }
                *(f32x4*)&tile[r + 1][4 + 4 * q] = p;
            }
        }
        if (tid < 64) {                                                          // wave 0: the row above and the row below the band
            const int gy = rr ? ys + OBJ_TY : ys - 1;
            if (gy >= 0 && gy < H && cw > 0) {
                const size_t o = pbase + (size_t)gy * W + gx;
                float ev[4], v[4];
                obj_load4<VEC>(eps + o, cw, ev); obj_load4<VEC>(xt + o, cw, v);
                f32x4 p;
#pragma unroll
                for (int j = 0; j < 4; ++j) p[j] = fminf(fmaxf(obj_raw_x0<VP>(v[j], ev[j], ca, cs), -1.0f), 1.0f);
                *(f32x4*)&tile[rr ? OBJ_TY + 1 : 0][4 + 4 * q] = p;
            }
        } else if (tid < 64 + 2 * OBJ_TY) {                                      // wave 1: the column left and right of the tile
            const int i = tid - 64, r = i >> 1, right = i & 1;
            const int gy = ys + r, hx = right ? xs + OBJ_TX : xs - 1;
            if (gy < H && hx >= 0 && hx < W) {
                const size_t o = pbase + (size_t)gy * W + hx;
                tile[r + 1][right ? OBJ_TX + 4 : 3] = fminf(fmaxf(obj_raw_x0<VP>(xt[o], eps[o], ca, cs), -1.0f), 1.0f);
            }
        }
        __syncthreads();
        // ---- stencil from LDS --------------------------------------------------------------------------------------------------
        const float coef = VP ? -cs : -__fdiv_rn(cs, ca);                        // d raw / d eps (VP: d raw / d v_hat)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int r = rr + 8 * k, gy = ys + r;
            if (gy < H && cw > 0) {
                const size_t o = pbase + (size_t)gy * W + gx;
                float nz[4], xv[4];
                obj_load4<VEC>(noise + o, cw, nz); obj_load4<VEC>(x0 + o, cw, xv);
                const f32x4 cen = *(const f32x4*)&tile[r + 1][4 + 4 * q];
                const f32x4 up = *(const f32x4*)&tile[r][4 + 4 * q], dn = *(const f32x4*)&tile[r + 2][4 + 4 * q];
                const float row[6] = {tile[r + 1][3 + 4 * q], cen[0], cen[1], cen[2], cen[3], tile[r + 1][8 + 4 * q]};
                const bool has_up = gy > 0, has_dn = gy + 1 < H;
                f32x4 out;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (VP) nz[j] = __fsub_rn(__fmul_rn(ca, nz[j]), __fmul_rn(cs, xv[j]));   // the target: nz is only the MSE's from here on
                    const float d = e[k][j] - nz[j];
                    float g = 2.0f * d * inv_n;                                  // the op order of mse_partial_kernel
                    if (j < cw) {
                        const float p = row[j + 1];
                        const bool has_l = gx + j > 0, has_r = gx + j + 1 < W;
                        const float sv = (has_up ? sgnf(p - up[j]) : 0.f) - (has_dn ? sgnf(dn[j] - p) : 0.f);
                        const float sh = (has_l ? sgnf(p - row[j]) : 0.f) - (has_r ? sgnf(row[j + 2] - p) : 0.f);
                        const float dp = (c_l1 * sgnf(p - xv[j]) + c_tvh * sv) + c_tvw * sh;
                        if ((inside[k] >> j) & 1u) g += dp * coef;
                        const double dd = (double)e[k][j] - (double)nz[j];
                        acc[0] += dd * dd;
                        acc[1] += fabs((double)p - (double)xv[j]);
                        if (has_dn) acc[2] += fabs((double)dn[j] - (double)p);
                        if (has_r) acc[3] += fabs((double)row[j + 2] - (double)p);
                    }
                    out[j] = g;
                }
                if (d_eps) {
                    if (VEC) *(f32x4*)(d_eps + o) = out;
                    else {
#pragma unroll
                        for (int j = 0; j < 4; ++j) if (j < cw) d_eps[o + j] = out[j];
                    }
                }
            }
        }
        __syncthreads();                                                         // the next tile overwrites the LDS tile
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc[k] += __shfl_xor(acc[k], m);
        if ((tid & 63) == 0) red[k][tid >> 6] = acc[k];
    }
    __syncthreads();
    if (tid < 4) scratch[(size_t)blockIdx.x * 4 + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}
// one wave, fixed order (mse_final_kernel's scheme) over the 4 sums of every workgroup; loss[] = total, mse, l1, tv (l1, tv unweighted)
__global__ void objective_final_kernel(const double* __restrict__ scratch, int nb, double inv_n, double inv_nh, double inv_nw, double recon_w,
                                       double tv_w, float* __restrict__ loss)
{
    if (blockIdx.x) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = (int)threadIdx.x; i < nb; i += 64) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += scratch[(size_t)i * 4 + k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s[k] += __shfl_xor(s[k], m);
    }
    if (threadIdx.x == 0) {
        const double mse = s[0] * inv_n, l1 = s[1] * inv_n, tv = s[2] * inv_nh + s[3] * inv_nw;
        loss[0] = (float)(mse + recon_w * l1 + tv_w * tv); loss[1] = (float)mse; loss[2] = (float)l1; loss[3] = (float)tv;
    }
}
// recon_w == tv_w == 0: the terms next to what mse_final_kernel wrote (total == mse; l1 and tv are not evaluated and read 0)
__global__ void objective_mse_only_terms_kernel(float* __restrict__ loss)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) { loss[1] = loss[0]; loss[2] = 0.f; loss[3] = 0.f; }
}
// the v-MSE alone: mse_partial_kernel with the target a noise - s x0 formed in registers (the same three fp32 ops a caller would
// materialise it with), same grid, same sums: bit-identical to launch_mse_loss_grad on that target
__global__ __launch_bounds__(256) void mse_v_partial_kernel(const float* __restrict__ v, const float* __restrict__ noise, const float* __restrict__ x0,
                                                             const float* __restrict__ a, const float* __restrict__ sg, int64_t per, int64_t n,
                                                             float inv_n, float* __restrict__ d_v, float* __restrict__ scratch)
{
    __shared__ double red[4];
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / per;
        const float target = __fsub_rn(__fmul_rn(a[b], noise[i]), __fmul_rn(sg[b], x0[i]));
        const float d = v[i] - target;
        s += (double)d * (double)d;
        if (d_v) d_v[i] = 2.0f * d * inv_n;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) scratch[blockIdx.x] = (float)((red[0] + red[1]) + (red[2] + red[3]));
}
template <bool VP>
hipError_t launch_objective(const float* eps, const float* noise, const float* xt, const float* x0, const float* a, const float* sg,
                            int B, int C, int H, int W, float recon_w, float tv_w, float* loss, float* d_eps, float* scratch,
                            hipStream_t s)
{
    const int64_t n = (int64_t)B * C * H * W;
    if (recon_w == 0.f && tv_w == 0.f) {
        hipError_t e = hipSuccess;
        if (VP) {
            const int nb = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);     // launch_mse_loss_grad's grid
            hipLaunchKernelGGL(mse_v_partial_kernel, dim3(nb), dim3(256), 0, s, eps, noise, x0, a, sg, (int64_t)C * H * W, n,
                               (float)(1.0 / (double)n), d_eps, scratch);
            hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(64), 0, s, scratch, nb, 1.0 / (double)n, loss);
            e = hipGetLastError();
        } else e = launch_mse_loss_grad(eps, noise, n, loss, d_eps, scratch, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(objective_mse_only_terms_kernel, dim3(1), dim3(64), 0, s, loss);
        return hipGetLastError();
    }
    const int nbx = (W + OBJ_TX - 1) / OBJ_TX, nby = (H + OBJ_TY - 1) / OBJ_TY;
    const int64_t tiles = (int64_t)B * C * nby * nbx;
    if (tiles > INT32_MAX) return hipErrorInvalidValue;
    const int nb = (int)(tiles < OBJ_MAX_WG ? tiles : OBJ_MAX_WG);
    const double nh = (double)B * C * (H - 1) * W, nw = (double)B * C * H * (W - 1);
    const float inv_n = (float)(1.0 / (double)n);
    const float c_l1 = (float)((double)recon_w / (double)n), c_tvh = (float)((double)tv_w / nh), c_tvw = (float)((double)tv_w / nw);
    const uintptr_t bits = (uintptr_t)eps | (uintptr_t)noise | (uintptr_t)xt | (uintptr_t)x0 | (uintptr_t)d_eps;
    if (W % 4 == 0 && (bits & 15) == 0)
        hipLaunchKernelGGL((objective_partial_kernel<true, VP>), dim3(nb), dim3(256), 0, s, eps, noise, xt, x0, a, sg, C, H, W, nby, nbx, (int)tiles,
                           inv_n, c_l1, c_tvh, c_tvw, d_eps, (double*)scratch);
    else
        hipLaunchKernelGGL((objective_partial_kernel<false, VP>), dim3(nb), dim3(256), 0, s, eps, noise, xt, x0, a, sg, C, H, W, nby, nbx, (int)tiles,
                           inv_n, c_l1, c_tvh, c_tvw, d_eps, (double*)scratch);
    hipLaunchKernelGGL(objective_final_kernel, dim3(1), dim3(64), 0, s, (const double*)scratch, nb, 1.0 / (double)n, 1.0 / nh, 1.0 / nw,
                       (double)recon_w, (double)tv_w, loss);
    return hipGetLastError();
}

// ---- the flat range of an elementwise pass: [head scalars][nvec 16-byte quads][tail scalars] -------------------------------------
// head = floats up to the first 16-byte boundary.  Workgroup 0's first threads take the head and the tail (at most 3 + 3 elements),
// every thread strides over the quads.
struct QuadSplit { int head; int64_t nvec; };
QuadSplit quad_split(const void* base, int64_t n)
{
    int64_t head = (int64_t)(((16 - ((uintptr_t)base & 15)) & 15) >> 2);
    if (head > n) head = n;
    return {(int)head, (n - head) / 4};
}

// ---- the step guard: scaler.scale(loss).backward(); scaler.step(opt); scaler.update() (train/diffusion_train.py:137-139) ----------
// The gradient buffer holds d (scale * loss).  One extra read of it decides the step on the device: grad_guard_partial_kernel sums
// (g * inv_scale)^2 in fp64, grad_guard_final_kernel turns the sum into the decision and commits the scaler's state, and
// adamw_kernel<GUARDED> reads that decision.  fp64 cannot overflow on squares of fp32 values, so the sum is non-finite exactly when
// an element is: no separate flag.  scratch >= GUARD_MAX_WG doubles.
constexpr int GUARD_MAX_WG = 2048;

__global__ void step_guard_init_kernel(ccn_step_guard_t* __restrict__ guard, float scale, int tracker, int good, int skipped)
{
    if (blockIdx.x || threadIdx.x) return;
    ccn_step_guard_t b{};
    b.scale = scale; b.inv_scale = (float)(1.0 / (double)scale); b.grad_norm = 0.f; b.grad_mul = b.inv_scale; b.bc1 = 1.f; b.bc2_sqrt = 1.f;
    b.apply = 0; b.good_steps = good; b.skipped_steps = skipped; b.growth_tracker = tracker;
    *guard = b;
}

__device__ __forceinline__ double guard_sq(float g, float inv) { const float u = g * inv; return (double)u * (double)u; }

__global__ __launch_bounds__(256) void grad_guard_partial_kernel(const float* __restrict__ g, int64_t n, int head, int64_t nvec,
                                                                  const ccn_step_guard_t* __restrict__ guard, double* __restrict__ scratch)
{
    __shared__ double red[4];
    const float inv = guard->inv_scale;
    const f32x4* __restrict__ gv = (const f32x4*)(g + head);
    const int64_t stride = (int64_t)gridDim.x * 256;
    double s = 0.0;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < nvec; i += 4 * stride) {                 // four 16-byte loads in flight
        f32x4 a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = gv[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int e = 0; e < 4; ++e) s += guard_sq(a[u][e], inv);
    }
    for (; i < nvec; i += stride) {
        const f32x4 a = gv[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) s += guard_sq(a[e], inv);
    }
    if (blockIdx.x == 0) {
        const int64_t tail0 = head + 4 * nvec;
        const int t = (int)threadIdx.x;
        if (t < head) s += guard_sq(g[t], inv);
        else if (tail0 + (t - head) < n) s += guard_sq(g[tail0 + (t - head)], inv);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) scratch[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// one wave, fixed order (mse_final_kernel's scheme); lane 0 then writes the decision and commits the state -- the AdamW kernel that
// follows in stream order only reads the block
__global__ void grad_guard_final_kernel(const double* __restrict__ scratch, int nb, ccn_step_guard_t* __restrict__ guard, float max_norm,
                                        float b1, float b2, float growth, float backoff, int interval)
{
    if (blockIdx.x) return;
    double s = 0.0;
    for (int i = (int)threadIdx.x; i < nb; i += 64) s += scratch[i];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (threadIdx.x) return;
    ccn_step_guard_t b = *guard;
    const bool ok = s - s == 0.0;                                     // finite (false for inf and NaN)
    const float norm = (float)sqrt(s);
    float coef = 1.0f;
    if (ok && max_norm > 0.f) coef = fminf(1.0f, __fdiv_rn(max_norm, norm + 1e-6f));      // clip_grad_norm_'s clamped coefficient
    const double step = (double)b.good_steps + 1.0;
    b.apply = ok ? 1 : 0;
    b.grad_norm = norm;
    b.grad_mul = b.inv_scale * coef;
    // launch_adamw's expressions, except that the powers are fp64 pow rounded to fp32 where the host calls powf: the two can differ
    // by one fp32 ulp of the power
    b.bc1 = 1.0f - (float)pow((double)b1, step);
    b.bc2_sqrt = __fsqrt_rn(1.0f - (float)pow((double)b2, step));
    if (ok) {
        b.good_steps += 1;
        if (++b.growth_tracker >= interval) {
            const float grown = b.scale * growth;
            if (grown - grown == 0.f) b.scale = grown;               // torch keeps the scale when growing would overflow
            b.growth_tracker = 0;
        }
    } else {
        b.skipped_steps += 1;
        b.scale *= backoff;
        b.growth_tracker = 0;
    }
    b.inv_scale = (float)(1.0 / (double)b.scale);
    *guard = b;
}
hipError_t launch_grad_guard(const float* g, int64_t n, void* guard, float max_norm, float b1, float b2, float growth, float backoff,
                             int interval, double* scratch, hipStream_t s)
{
    const QuadSplit q = quad_split(g, n);
    // the number of partials depends on n alone (not on the alignment): ceil(n / 4) quads, 256 per workgroup, at most GUARD_MAX_WG
    const int64_t want = ((n + 3) / 4 + 255) / 256;
    const int nb = (int)(want < GUARD_MAX_WG ? want : GUARD_MAX_WG);
    hipLaunchKernelGGL(grad_guard_partial_kernel, dim3(nb), dim3(256), 0, s, g, n, q.head, q.nvec, (const ccn_step_guard_t*)guard, scratch);
    hipLaunchKernelGGL(grad_guard_final_kernel, dim3(1), dim3(64), 0, s, (const double*)scratch, nb, (ccn_step_guard_t*)guard, max_norm, b1, b2,
                       growth, backoff, interval);
    return hipGetLastError();
}

// ---- the weight EMA's state (torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn(decay)) --------------------------------
// ema_tick_kernel is the only writer of the 32-byte ccn_ema_state_t, as grad_guard_final_kernel is of the guard block; it runs before
// adamw_kernel<.., EMA>, which only reads the block.  A skipped step (guard->apply == 0) is no update: neither the average nor the
// count of updates (the warm-up's clock) moves.
__global__ void ema_init_kernel(ccn_ema_state_t* __restrict__ st, int updates)
{
    if (blockIdx.x || threadIdx.x) return;
    ccn_ema_state_t b{};
    b.updates = updates;
    *st = b;
}
__global__ void ema_tick_kernel(ccn_ema_state_t* __restrict__ st, const ccn_step_guard_t* __restrict__ guard, float w, int warmup)
{
    if (blockIdx.x || threadIdx.x) return;
    const bool apply = guard ? guard->apply != 0 : true;
    if (!apply) { st->apply = 0; return; }
    const int u = st->updates;
    st->apply = 1;
    st->first = u == 0 ? 1 : 0;
    // decay_u = min(decay, (1 + u) / (10 + u)) as its complement 1 - decay_u = max(w, 9 / (10 + u)): no 1 - x cancellation
    st->weight = warmup ? fmaxf(w, __fdiv_rn(9.0f, (float)(10 + u))) : w;
    st->updates = u + 1;
}

// ---- AdamW: torch.optim.AdamW's step (train/diffusion_train.py:105,138), decoupled weight decay, bias-corrected moments -----------
// One element function and one kernel for every entry point.  What differs between them is where four scalars come from, not the
// arithmetic (the build has -ffp-contract=off, so one expression gives the same bits in every instantiation):
//   the gradient   g itself, or g * guard->grad_mul (GUARDED: unscaled and clipped).  The unguarded form multiplies by nothing --
//                  not by 1.0f -- so that no bit depends on the denormal mode
//   bc1, bc2_sqrt  the host's powf without a guard, the guard block's (device pow, one ulp of the power apart) with one
//   apply          the EMA state's copy of the decision (EMA), else the guard's (GUARDED), else always
struct AdamwCoef { float mul, decay, b1, b2, eps, bc2_sqrt, step_size, weight; bool apply, first; };

template <bool GUARDED, bool EMA>
__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float& e, const AdamwCoef& c)
{
    const float gi = GUARDED ? g * c.mul : g;
    float pi = p * c.decay;
    const float mi = c.b1 * m + (1.0f - c.b1) * gi;
    const float vi = c.b2 * v + (1.0f - c.b2) * gi * gi;
    m = mi; v = vi;
    const float denom = sqrtf(vi) / c.bc2_sqrt + c.eps;
    pi -= c.step_size * (mi / denom);
    p = pi;
    if (EMA) e = c.first ? p : fmaf(c.weight, p - e, e);       // the first update copies (AveragedModel's n_averaged == 0), later ones lerp
}
// the EMA buffer is not read on the first update
template <bool GUARDED, bool EMA, bool ZERO>
__device__ __forceinline__ void adamw_scalar(float* p, float* g, float* m, float* v, float* ema, int64_t i, const AdamwCoef& c)
{
    if (c.apply) {
        float pi = p[i], mi = m[i], vi = v[i], ei = EMA && !c.first ? ema[i] : 0.f;
        adamw_elem<GUARDED, EMA>(pi, g[i], mi, vi, ei, c);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (EMA) ema[i] = ei;
    }
    if (ZERO) g[i] = 0.f;
}
// VEC: the buffers share their alignment modulo 16 bytes, so one QuadSplit serves all of them; otherwise 4-byte accesses throughout.
// One quad of each buffer per thread and trip: four or five 16-byte loads in flight at 8 waves per SIMD already cover the HBM latency.
// A guarded step always consumes the gradients (GUARDED implies ZERO); `ema` and `st` are read with EMA only, `guard` with GUARDED.
template <bool GUARDED, bool EMA, bool ZERO, bool VEC>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                     float* __restrict__ ema, int64_t n, int head, int64_t nvec, float lr, float b1, float b2,
                                                     float eps, float wd, float bc1, float bc2_sqrt,
                                                     const ccn_step_guard_t* __restrict__ guard, const ccn_ema_state_t* __restrict__ st)
{
    static_assert(ZERO || !GUARDED, "a guarded step zeroes the gradients");
    AdamwCoef c;
    c.apply = EMA ? st->apply != 0 : (GUARDED ? guard->apply != 0 : true);       // the tick copied the guard's decision (1 without a guard)
    c.mul = GUARDED ? guard->grad_mul : 1.0f;
    if (GUARDED) { bc1 = guard->bc1; bc2_sqrt = guard->bc2_sqrt; }
    c.decay = 1.0f - lr * wd; c.b1 = b1; c.b2 = b2; c.eps = eps; c.bc2_sqrt = bc2_sqrt; c.step_size = lr / bc1;
    c.weight = EMA ? st->weight : 0.f; c.first = EMA ? st->first != 0 : false;
    const int64_t stride = (int64_t)gridDim.x * 256, i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (!VEC) {
        for (int64_t i = i0; i < n; i += stride) adamw_scalar<GUARDED, EMA, ZERO>(p, g, m, v, ema, i, c);
        return;
    }
    f32x4* const pv = (f32x4*)(p + head); f32x4* const gv = (f32x4*)(g + head); f32x4* const mv = (f32x4*)(m + head);
    f32x4* const vv = (f32x4*)(v + head); f32x4* const ev = EMA ? (f32x4*)(ema + head) : nullptr;
    for (int64_t i = i0; i < nvec; i += stride) {
        if (c.apply) {
            const f32x4 gq = gv[i];
            f32x4 pq = pv[i], mq = mv[i], vq = vv[i], eq = f32x4{0.f, 0.f, 0.f, 0.f};
            if (EMA && !c.first) eq = ev[i];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pq[e], me = mq[e], ve = vq[e], ee = eq[e];
                adamw_elem<GUARDED, EMA>(pe, gq[e], me, ve, ee, c);
                pq[e] = pe; mq[e] = me; vq[e] = ve; eq[e] = ee;
            }
            pv[i] = pq; mv[i] = mq; vv[i] = vq;
            if (EMA) ev[i] = eq;
        }
        if (ZERO) gv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (blockIdx.x == 0) {
        const int64_t tail0 = head + 4 * nvec;
        const int t = (int)threadIdx.x;
        const int64_t i = t < head ? t : tail0 + (t - head);
        if (i < n) adamw_scalar<GUARDED, EMA, ZERO>(p, g, m, v, ema, i, c);
    }
}
template <bool GUARDED, bool EMA, bool ZERO, typename... Args> void launch_adamw_as(bool vec, unsigned grid, hipStream_t s, Args... args)
{
    if (vec) hipLaunchKernelGGL((adamw_kernel<GUARDED, EMA, ZERO, true>), dim3(grid), dim3(256), 0, s, args...);
    else hipLaunchKernelGGL((adamw_kernel<GUARDED, EMA, ZERO, false>), dim3(grid), dim3(256), 0, s, args...);
}
// ema / st: NULL, or the EMA buffer and the state block ema_tick_kernel has just written; guard: NULL, or the block launch_grad_guard
// has just written (then `step` and `zero_grad` are not read: the count is the block's, the gradients are consumed).
// Every entry point takes the 16-byte path when its (4-byte aligned) buffers share their alignment -- ccn_adamw_step and ccn_adamw_step_zero_grad,
// which ran a 4-byte kernel of their own before the three were merged, included: the same bits from a quarter of the memory instructions.
hipError_t launch_adamw(float* p, float* g, float* m, float* v, float* ema, int64_t n, float lr, float b1, float b2, float eps, float wd,
                        int step, bool zero_grad, const ccn_step_guard_t* guard, const ccn_ema_state_t* st, hipStream_t s)
{
    const uintptr_t a = (uintptr_t)p & 15;
    const bool vec = (a & 3) == 0 && ((uintptr_t)g & 15) == a && ((uintptr_t)m & 15) == a && ((uintptr_t)v & 15) == a && (!ema || ((uintptr_t)ema & 15) == a);
    const QuadSplit q = vec ? quad_split(p, n) : QuadSplit{0, 0};
    const int64_t want = ((vec ? q.nvec : n) + 255) / 256;
    const unsigned grid = (unsigned)(want < 8192 ? (want > 0 ? want : 1) : 8192);
    float bc1 = 1.0f, bc2_sqrt = 1.0f;                                   // not read under a guard
    if (!guard) { bc1 = 1.0f - powf(b1, (float)step); bc2_sqrt = sqrtf(1.0f - powf(b2, (float)step)); }
#define CCN_ADAMW(G, E, Z) launch_adamw_as<G, E, Z>(vec, grid, s, p, g, m, v, ema, n, q.head, q.nvec, lr, b1, b2, eps, wd, bc1, bc2_sqrt, guard, st)
    if (guard) { if (ema) CCN_ADAMW(true, true, true); else CCN_ADAMW(true, false, true); }
    else if (zero_grad) { if (ema) CCN_ADAMW(false, true, true); else CCN_ADAMW(false, false, true); }
    else { if (ema) CCN_ADAMW(false, true, false); else CCN_ADAMW(false, false, false); }
#undef CCN_ADAMW
    return hipGetLastError();
}

}  // namespace
}  // namespace ccn

using namespace ccn;

// the two objectives share their argument checks; VP: x_t is not read when both weights are zero
template <bool VP>
static int objective_entry(const float* eps_dev, const float* noise_dev, const float* x_t_dev, const float* x0_dev, const float* a_dev,
                           const float* s_dev, int32_t B, int32_t C, int32_t H, int32_t W, float recon_w, float tv_w, float* loss_dev,
                           float* d_eps_dev, float* scratch_dev, void* stream)
{
    const bool need_xt = !VP || recon_w != 0.f || tv_w != 0.f;
    if (!eps_dev || !noise_dev || (need_xt && !x_t_dev) || !x0_dev || !a_dev || !s_dev || !loss_dev || !scratch_dev || B <= 0 || C <= 0)
        return fail(CCN_EINVAL, "bad argument");
    if (H < 2 || W < 2) return fail(CCN_EINVAL, "H and W must be at least 2 (the total variation of a one-pixel-wide image is a mean over nothing)");
    if (!(recon_w >= 0.f) || !(tv_w >= 0.f)) return fail(CCN_EINVAL, "recon_w and tv_w must be non-negative");
    if (((uintptr_t)scratch_dev & 7) != 0) return fail(CCN_EINVAL, "scratch_dev must be 8-byte aligned");
    if ((int64_t)B * C * H * W > (int64_t)1 << 40) return fail(CCN_EINVAL, "tensor too large");
    if (launch_objective<VP>(eps_dev, noise_dev, x_t_dev, x0_dev, a_dev, s_dev, B, C, H, W, recon_w, tv_w, loss_dev, d_eps_dev, scratch_dev,
                             (hipStream_t)stream) != hipSuccess)
        return fail(CCN_EHIP, "objective launch failed");
    return CCN_OK;
}

extern "C" {

int ccn_mse_loss_grad(const float* eps_dev, const float* target_dev, int64_t n, float* loss_dev, float* d_eps_dev, float* scratch_dev, void* stream)
{
    if (!eps_dev || !target_dev || !loss_dev || !scratch_dev || n <= 0) return fail(CCN_EINVAL, "bad argument");
    if (launch_mse_loss_grad(eps_dev, target_dev, n, loss_dev, d_eps_dev, scratch_dev, (hipStream_t)stream) != hipSuccess) return fail(CCN_EHIP, "mse launch failed");
    return CCN_OK;
}

int ccn_diffusion_loss_grad(const float* eps_dev, const float* noise_dev, const float* x_t_dev, const float* x0_dev, const float* a_dev,
                            const float* s_dev, int32_t B, int32_t C, int32_t H, int32_t W, float recon_w, float tv_w, float* loss_dev,
                            float* d_eps_dev, float* scratch_dev, void* stream)
{
    return objective_entry<false>(eps_dev, noise_dev, x_t_dev, x0_dev, a_dev, s_dev, B, C, H, W, recon_w, tv_w, loss_dev, d_eps_dev, scratch_dev, stream);
}

int ccn_diffusion_loss_grad_v(const float* v_dev, const float* noise_dev, const float* x_t_dev, const float* x0_dev, const float* a_dev,
                              const float* s_dev, int32_t B, int32_t C, int32_t H, int32_t W, float recon_w, float tv_w, float* loss_dev,
                              float* d_v_dev, float* scratch_dev, void* stream)
{
    return objective_entry<true>(v_dev, noise_dev, x_t_dev, x0_dev, a_dev, s_dev, B, C, H, W, recon_w, tv_w, loss_dev, d_v_dev, scratch_dev, stream);
}

int ccn_adamw_step(float* params_dev, const float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t n, float lr, float beta1, float beta2,
                   float eps, float weight_decay, int32_t step, void* stream)
{
    if (!params_dev || !grads_dev || !exp_avg_dev || !exp_avg_sq_dev || n <= 0 || step <= 0) return fail(CCN_EINVAL, "bad argument");
    if (launch_adamw(params_dev, (float*)grads_dev, exp_avg_dev, exp_avg_sq_dev, nullptr, n, lr, beta1, beta2, eps, weight_decay, step, false, nullptr,
                     nullptr, (hipStream_t)stream) != hipSuccess)
        return fail(CCN_EHIP, "adamw launch failed");
    return CCN_OK;
}

int ccn_adamw_step_zero_grad(float* params_dev, float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t n, float lr, float beta1, float beta2,
                   float eps, float weight_decay, int32_t step, void* stream)
{
    if (!params_dev || !grads_dev || !exp_avg_dev || !exp_avg_sq_dev || n <= 0 || step <= 0) return fail(CCN_EINVAL, "bad argument");
    if (launch_adamw(params_dev, grads_dev, exp_avg_dev, exp_avg_sq_dev, nullptr, n, lr, beta1, beta2, eps, weight_decay, step, true, nullptr, nullptr,
                     (hipStream_t)stream) != hipSuccess)
        return fail(CCN_EHIP, "adamw launch failed");
    return CCN_OK;
}

int ccn_step_guard_init(void* guard_dev, float init_scale, int32_t growth_tracker0, int32_t good_steps0, int32_t skipped_steps0, void* stream)
{
    if (!guard_dev || ((uintptr_t)guard_dev & 3) != 0) return fail(CCN_EINVAL, "guard_dev must be a 4-byte aligned device pointer");
    if (!(init_scale > 0.f) || init_scale - init_scale != 0.f) return fail(CCN_EINVAL, "init_scale must be positive and finite");
    if (growth_tracker0 < 0 || good_steps0 < 0 || skipped_steps0 < 0) return fail(CCN_EINVAL, "counters must be non-negative");
    hipLaunchKernelGGL(step_guard_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (ccn_step_guard_t*)guard_dev, init_scale, growth_tracker0,
                       good_steps0, skipped_steps0);
    if (hipGetLastError() != hipSuccess)
        return fail(CCN_EHIP, "step guard init launch failed");
    return CCN_OK;
}

int ccn_grad_guard(const float* grads_dev, int64_t n, void* guard_dev, float max_grad_norm, float beta1, float beta2, float growth_factor,
                   float backoff_factor, int32_t growth_interval, float* scratch_dev, void* stream)
{
    if (!grads_dev || !guard_dev || !scratch_dev || n <= 0) return fail(CCN_EINVAL, "bad argument");
    if (((uintptr_t)grads_dev & 3) != 0 || ((uintptr_t)guard_dev & 3) != 0) return fail(CCN_EINVAL, "grads_dev and guard_dev must be 4-byte aligned");
    if (((uintptr_t)scratch_dev & 7) != 0) return fail(CCN_EINVAL, "scratch_dev must be 8-byte aligned");
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return fail(CCN_EINVAL, "betas must be in [0, 1)");
    if (!(growth_factor > 0.f) || !(backoff_factor > 0.f) || growth_interval <= 0)
        return fail(CCN_EINVAL, "growth_factor, backoff_factor and growth_interval must be positive");
    if (max_grad_norm != max_grad_norm) return fail(CCN_EINVAL, "max_grad_norm is NaN");
    if (launch_grad_guard(grads_dev, n, guard_dev, max_grad_norm, beta1, beta2, growth_factor, backoff_factor, growth_interval,
                          (double*)scratch_dev, (hipStream_t)stream) != hipSuccess)
        return fail(CCN_EHIP, "grad guard launch failed");
    return CCN_OK;
}

int ccn_adamw_step_guarded(float* params_dev, float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, int64_t n, float lr, float beta1,
                           float beta2, float eps, float weight_decay, const void* guard_dev, void* stream)
{
    if (!params_dev || !grads_dev || !exp_avg_dev || !exp_avg_sq_dev || !guard_dev || n <= 0) return fail(CCN_EINVAL, "bad argument");
    if ((((uintptr_t)params_dev | (uintptr_t)grads_dev | (uintptr_t)exp_avg_dev | (uintptr_t)exp_avg_sq_dev | (uintptr_t)guard_dev) & 3) != 0)
        return fail(CCN_EINVAL, "buffers must be 4-byte aligned");
    if (launch_adamw(params_dev, grads_dev, exp_avg_dev, exp_avg_sq_dev, nullptr, n, lr, beta1, beta2, eps, weight_decay, 0, true,
                     (const ccn_step_guard_t*)guard_dev, nullptr, (hipStream_t)stream) != hipSuccess)
        return fail(CCN_EHIP, "guarded adamw launch failed");
    return CCN_OK;
}

int ccn_ema_init(void* ema_state_dev, int32_t updates0, void* stream)
{
    if (!ema_state_dev || ((uintptr_t)ema_state_dev & 3) != 0) return fail(CCN_EINVAL, "ema_state_dev must be a 4-byte aligned device pointer");
    if (updates0 < 0) return fail(CCN_EINVAL, "updates0 must be non-negative");
    hipLaunchKernelGGL(ema_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (ccn_ema_state_t*)ema_state_dev, updates0);
    if (hipGetLastError() != hipSuccess) return fail(CCN_EHIP, "ema init launch failed");
    return CCN_OK;
}

int ccn_adamw_step_ema(float* params_dev, float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* ema_dev, int64_t n, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int32_t step, int32_t zero_grad, double ema_decay,
                       int32_t ema_warmup, const void* guard_dev, void* ema_state_dev, void* stream)
{
    if (!params_dev || !grads_dev || !exp_avg_dev || !exp_avg_sq_dev || !ema_dev || !ema_state_dev)
        return fail(CCN_EINVAL, "a buffer or the EMA state block is NULL");
    if (n < 0) return fail(CCN_EINVAL, "n is negative");
    if (!(ema_decay >= 0.0 && ema_decay < 1.0)) return fail(CCN_EINVAL, "ema_decay must be in [0, 1)");
    if (guard_dev && !zero_grad) return fail(CCN_EINVAL, "a guarded step consumes the gradients: zero_grad must be non-zero with guard_dev");
    if (!guard_dev && step <= 0) return fail(CCN_EINVAL, "step must be at least 1 without guard_dev");
    if ((((uintptr_t)params_dev | (uintptr_t)grads_dev | (uintptr_t)exp_avg_dev | (uintptr_t)exp_avg_sq_dev | (uintptr_t)ema_dev |
          (uintptr_t)guard_dev | (uintptr_t)ema_state_dev) & 3) != 0)
        return fail(CCN_EINVAL, "buffers must be 4-byte aligned");
    if (n == 0) return CCN_OK;                       // nothing to average: no launch, the count of updates stays
    const float w = (float)(1.0 - ema_decay);        // the weight get_ema_multi_avg_fn(decay) hands to lerp_, rounded once to fp32
    // two launches: the one-wave tick that writes the state block, then the fused pass that reads it
    hipLaunchKernelGGL(ema_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (ccn_ema_state_t*)ema_state_dev, (const ccn_step_guard_t*)guard_dev, w,
                       ema_warmup ? 1 : 0);
    if (launch_adamw(params_dev, grads_dev, exp_avg_dev, exp_avg_sq_dev, ema_dev, n, lr, beta1, beta2, eps, weight_decay, step, zero_grad != 0,
                     (const ccn_step_guard_t*)guard_dev, (const ccn_ema_state_t*)ema_state_dev, (hipStream_t)stream) != hipSuccess)
        return fail(CCN_EHIP, "adamw + ema launch failed");
    return CCN_OK;
}

}  // extern "C"
