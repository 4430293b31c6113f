// Projector schedule of the W+ loop: a learning-rate multiplier, Gaussian noise on the latent before the generator pass and
// a pull towards an anchor latent.  Everything that varies per step is derived on the device from the loop's step counter, so a recorded
// step (oodgan_plan_run) replays unchanged, and the noise is a pure function of (seed, image id, step, element): a window the range guard
// repeats, a sub-batch on another stream or another grouping of the files sees the same draws.  No state lives here.
#include "loss_common.hpp"

namespace {
using namespace oodgan;

constexpr double kPi = 3.14159265358979323846;

// ---------------------------------------------------------------------------------------------------------------- scheduled Adam
__global__ void sched_counter_inc_kernel(int* __restrict__ t) { t[0] += 1; }

// rosinality projector.py get_lr, without its initial lr: min(1, (1 - tau) / rampdown) through the cosine, times min(1, tau / rampup)
__device__ __forceinline__ double lr_multiplier(int i, int total_steps, float rampup, float rampdown) {
    const double tau = (double)i / (double)total_steps;
    double r = 1.0;
    if (rampdown > 0.f) {
        r = fmin(1.0, (1.0 - tau) / (double)rampdown);
        r = 0.5 - 0.5 * cos(kPi * r);
    }
    if (rampup > 0.f) r *= fmin(1.0, tau / (double)rampup);
    return r;
}

// adam_dev_kernel (elementwise.hip) with lr * lr_multiplier(t - 1); both ramps off: the same bits
__global__ __launch_bounds__(256) void adam_dev_sched_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, long n, float lr, float beta1, float beta2, float eps,
                                                             const int* __restrict__ t_dev, int total_steps, float rampup, float rampdown) {
    const int t = t_dev[0];
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    const float step_size = (float)((double)lr * lr_multiplier(t - 1, total_steps, rampup, rampdown) / bc1);
    const float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride) {
        const float gi = g[i];
        const float mi = m[i] + (gi - m[i]) * (1.f - beta1);
        const float vi = v[i] * beta2 + (1.f - beta2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        w[i] = w[i] - step_size * (mi / (sqrtf(vi) * inv_bc2_sqrt + eps));
    }
}

// ---------------------------------------------------------------------------------------------------------------- latent noise
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const unsigned lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

// u = ((x >> 8) + 0.5) 2^-24 in (0, 1).  In double: (x >> 8) + 0.5 needs 25 bits, and the radius sqrt(-2 ln u) of a u next to 1 moves by
// 2e-4 when u is rounded to float
__device__ __forceinline__ double unit_open(unsigned x) { return ((double)(x >> 8) + 0.5) * (1.0 / 16777216.0); }

__device__ __forceinline__ void box_muller(unsigned xa, unsigned xb, float& n0, float& n1) {
    const double r = sqrt(-2.0 * log(unit_open(xa)));
    double s, c;
    sincospi(2.0 * unit_open(xb), &s, &c);
    n0 = (float)(r * c);
    n1 = (float)(r * s);
}

// grid: (quads of one image / 256, B); one thread = the four values of one Philox call.  VEC: n % 4 == 0 and both pointers 16-byte aligned.
// TIED: quad q takes the draw of quad q mod qperiod (the W mode of the loop: one 512-vector of noise repeated over the layers)
template <bool VEC, bool TIED>
__global__ __launch_bounds__(256) void latent_noise_kernel(const float* __restrict__ w, float* __restrict__ w_in, const long* __restrict__ ids,
                                                           const int* __restrict__ t_dev, long n, unsigned seed_lo, unsigned seed_hi,
                                                           int total_steps, float sigma0, float noise_ramp, long qperiod) {
    const long q = (long)blockIdx.x * 256 + threadIdx.x;
    const long e0 = q * 4;
    if (e0 >= n) return;
    const int b = blockIdx.y;
    const int i = t_dev[0];
    double sig = (double)sigma0;
    if (noise_ramp > 0.f) {
        const double f = fmax(0.0, 1.0 - ((double)i / (double)total_steps) / (double)noise_ramp);
        sig *= f * f;
    }
    const float sigma = (float)sig;
    const float* src = w + (long)b * n + e0;
    float* dst = w_in + (long)b * n + e0;
    float nz[4] = {0.f, 0.f, 0.f, 0.f};
    if (sigma != 0.f) {      // sigma == 0: w_in = w bit for bit, and no draw is made
        const unsigned long id = (unsigned long)ids[b];
        const unsigned qd = (unsigned)(TIED ? q % qperiod : q);
        const uint4 x = philox4x32_10(make_uint4(qd, (unsigned)id, (unsigned)i, (unsigned)(id >> 32)), make_uint2(seed_lo, seed_hi));
        box_muller(x.x, x.y, nz[0], nz[1]);
        box_muller(x.z, x.w, nz[2], nz[3]);
    }
    if (VEC) {
        const float4 a = *reinterpret_cast<const float4*>(src);
        *reinterpret_cast<float4*>(dst) = sigma != 0.f ? make_float4(a.x + sigma * nz[0], a.y + sigma * nz[1], a.z + sigma * nz[2], a.w + sigma * nz[3]) : a;
    } else {
        const int cnt = n - e0 < 4 ? (int)(n - e0) : 4;
        for (int k = 0; k < cnt; ++k) dst[k] = sigma != 0.f ? src[k] + sigma * nz[k] : src[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------- latent prior
// grid: (B), one block per image: p_b = mean_e (w - a)^2 (summed in double: one rounding at the end), g += coef * (w - a)
__global__ __launch_bounds__(256) void latent_prior_kernel(const float* __restrict__ w, const float* __restrict__ a, float* __restrict__ g,
                                                           float* __restrict__ loss, long n, long a_stride, float coef, double inv_n,
                                                           const int* __restrict__ row_dev, int nrows) {
    __shared__ double red[4];
    const int b = blockIdx.x;
    const float* wp = w + (long)b * n;
    const float* ap = a + (long)b * a_stride;
    float* gp = g ? g + (long)b * n : nullptr;
    double acc = 0.0;
    for (long e = threadIdx.x; e < n; e += 256) {
        const float d = wp[e] - ap[e];
        acc += (double)d * (double)d;
        if (gp) gp[e] += coef * d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) loss[loss_row(row_dev, nrows, gridDim.x) + b] = (float)(((red[0] + red[1]) + (red[2] + red[3])) * inv_n);
}

int latent_prior(const float* w, const float* a, float* g, float* loss, const int* row_dev, int nrows, int B, long n, int a_batched,
                 float weight, void* stream) {
    OODGAN_REQUIRE(B <= 65535 * 1024, "latent_prior: B = %d: too large", B);
    hipLaunchKernelGGL(latent_prior_kernel, dim3(B), dim3(256), 0, as_stream(stream), w, a, g, loss, n, a_batched ? n : 0L,
                       (float)(2.0 * (double)weight / (double)n), 1.0 / (double)n, row_dev, nrows);
    return check_launch("latent_prior");
}

// period == 0: every element its own draw (oodgan_latent_noise); otherwise element e takes the draw of element e mod period
int latent_noise(const float* w, float* w_in, const long* ids, const int* t_dev, int B, long n_per_image, long period, long seed, int total_steps,
                 float sigma0, float noise_ramp, void* stream) {
    const long quads = (n_per_image + 3) / 4;
    OODGAN_REQUIRE(B <= 65535 && quads <= (1L << 32), "latent_noise: B = %d images of %ld values: too large", B, n_per_image);
    const unsigned long s = (unsigned long)seed;
    const dim3 grid((unsigned)((quads + 255) / 256), B);
    const bool vec = (n_per_image & 3) == 0 && ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(w_in)) & 15) == 0;
    const bool tied = period > 0 && period != n_per_image;
    auto kernel = vec ? (tied ? latent_noise_kernel<true, true> : latent_noise_kernel<true, false>)
                      : (tied ? latent_noise_kernel<false, true> : latent_noise_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, as_stream(stream), w, w_in, ids, t_dev, n_per_image, (unsigned)s, (unsigned)(s >> 32),
                       total_steps, sigma0, noise_ramp, tied ? period / 4 : quads);
    return check_launch("latent_noise");
}

// ---------------------------------------------------------------------------------------------------------------- latent step
// The latent side of a step with the latent controls on: the spread of the layers about their mean (value and gradient), the
// W tie of the gradient, Adam with a step size per layer.  grid: (B), one block per image; a thread owns the columns e = tid, tid + 256, ...
// and walks the L layers of each: every pass over the layers is coalesced across the block.  w, g, m, v (B, L, D).
//   d_le = w_le - mean_l w_le (the mean from a double sum); R_b = mean_le d^2 (double sum, one rounding) -> table row t - 1, the zero-based step;
//   coef != 0: g += coef * d;  tied: g_le = (float) sum_l (double) g_le, in layer order — what autograd hands a (B, D) leaf expanded to L layers;
//   the g Adam consumes is written back when either changed it; Adam: the expressions of adam_dev_sched_kernel with lr * layer_lr[l].
// Nothing on: the bits of adam_dev_sched_kernel.
__global__ __launch_bounds__(256) void latent_step_kernel(float* __restrict__ w, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                          int L, int D, float lr, float beta1, float beta2, float eps,
                                                          const int* __restrict__ t_dev, int total_steps, float rampup, float rampdown,
                                                          const float* __restrict__ layer_lr, float coef, int tied, float* __restrict__ table,
                                                          int nrows, double inv_n) {
    __shared__ double red[4];
    const int t = t_dev[0];
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    const double mult = lr_multiplier(t - 1, total_steps, rampup, rampdown);
    const float step_all = (float)((double)lr * mult / bc1);
    const float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    const bool spread = table != nullptr || coef != 0.f;
    const long base = (long)blockIdx.x * L * D;
    double acc = 0.0;
    for (int e = threadIdx.x; e < D; e += 256) {
        const long c = base + e;
        if (spread) {
            double sw = 0.0;
            for (int l = 0; l < L; ++l) sw += (double)w[c + (long)l * D];
            const double mean = sw / (double)L;
            for (int l = 0; l < L; ++l) {
                const long i = c + (long)l * D;
                const float d = (float)((double)w[i] - mean);
                acc += (double)d * (double)d;
                if (coef != 0.f) g[i] += coef * d;
            }
        }
        float s = 0.f;
        if (tied) {
            double sg = 0.0;
            for (int l = 0; l < L; ++l) sg += (double)g[c + (long)l * D];
            s = (float)sg;
        }
        for (int l = 0; l < L; ++l) {
            const long i = c + (long)l * D;
            const float step_size = layer_lr ? (float)((double)lr * (double)layer_lr[l] * mult / bc1) : step_all;
            const float gi = tied ? s : g[i];
            if (tied) g[i] = gi;
            const float mi = m[i] + (gi - m[i]) * (1.f - beta1);
            const float vi = v[i] * beta2 + (1.f - beta2) * gi * gi;
            m[i] = mi;
            v[i] = vi;
            w[i] = w[i] - step_size * (mi / (sqrtf(vi) * inv_bc2_sqrt + eps));
        }
    }
    if (table == nullptr) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    const int row = t - 1;
    if (threadIdx.x == 0) table[loss_row(&row, nrows, gridDim.x) + blockIdx.x] = (float)(((red[0] + red[1]) + (red[2] + red[3])) * inv_n);
}

// ---------------------------------------------------------------------------------------------------------------- style step
// The StyleSpace side of a step: the loop optimises an offset d (B, R) on the styles, gs is dL/ds as the backward pass left it
// (times the loss scale).  grid: (B), one block per image; a thread owns the columns r = tid, tid + 256, ...: every access is coalesced.
//   g_r = gs_r / grad_div (a correctly rounded division; grad_div == 1: gs_r);  R_b = mean_r d_r^2 (double sum, one rounding) -> table row t - 1;
//   coef != 0: g_r += coef * d_r;  g is written back: gs holds what Adam consumed;
//   Adam: the expressions of adam_dev_sched_kernel with lr * layer_lr[row_lat[r]].
// grad_div 1, no factors, coef 0: the bits of adam_dev_sched_kernel.
__global__ __launch_bounds__(256) void style_step_kernel(float* __restrict__ w, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                         int R, float lr, float beta1, float beta2, float eps, const int* __restrict__ t_dev,
                                                         int total_steps, float rampup, float rampdown, float grad_div,
                                                         const int* __restrict__ row_lat, const float* __restrict__ layer_lr, float coef,
                                                         float* __restrict__ table, int nrows, double inv_n) {
    __shared__ double red[4];
    const int t = t_dev[0];
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    const double mult = lr_multiplier(t - 1, total_steps, rampup, rampdown);
    const float step_all = (float)((double)lr * mult / bc1);
    const float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    const long base = (long)blockIdx.x * R;
    double acc = 0.0;
    for (int r = threadIdx.x; r < R; r += 256) {
        const long i = base + r;
        const float d = w[i];
        acc += (double)d * (double)d;
        float gi = g[i] / grad_div;
        if (coef != 0.f) gi += coef * d;
        g[i] = gi;
        const float step_size = layer_lr ? (float)((double)lr * (double)layer_lr[row_lat[r]] * mult / bc1) : step_all;
        const float mi = m[i] + (gi - m[i]) * (1.f - beta1);
        const float vi = v[i] * beta2 + (1.f - beta2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        w[i] = d - step_size * (mi / (sqrtf(vi) * inv_bc2_sqrt + eps));
    }
    if (table == nullptr) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    const int row = t - 1;
    if (threadIdx.x == 0) table[loss_row(&row, nrows, gridDim.x) + blockIdx.x] = (float)(((red[0] + red[1]) + (red[2] + red[3])) * inv_n);
}

}  // namespace

extern "C" int oodgan_adam_step_dev_sched(float* w, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                                          int* t_dev, int total_steps, float rampup, float rampdown, void* stream) {
    OODGAN_REQUIRE(w && g && m && v && t_dev && n > 0 && total_steps > 0, "adam_dev_sched: bad args");
    hipLaunchKernelGGL(sched_counter_inc_kernel, dim3(1), dim3(1), 0, as_stream(stream), t_dev);
    hipLaunchKernelGGL(adam_dev_sched_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream), w, g, m, v, n, lr, beta1, beta2, eps,
                       t_dev, total_steps, rampup, rampdown);
    return check_launch("adam_dev_sched");
}

extern "C" int oodgan_latent_noise(const float* w, float* w_in, const long* ids, const int* t_dev, int B, long n_per_image, long seed,
                                   int total_steps, float sigma0, float noise_ramp, void* stream) {
    OODGAN_REQUIRE(w && w_in && ids && t_dev && B > 0 && n_per_image > 0 && total_steps > 0, "latent_noise: bad args");
    return latent_noise(w, w_in, ids, t_dev, B, n_per_image, 0, seed, total_steps, sigma0, noise_ramp, stream);
}

extern "C" int oodgan_latent_noise_tied(const float* w, float* w_in, const long* ids, const int* t_dev, int B, long n_per_image, long period,
                                        long seed, int total_steps, float sigma0, float noise_ramp, void* stream) {
    OODGAN_REQUIRE(w && w_in && ids && t_dev && B > 0 && n_per_image > 0 && total_steps > 0, "latent_noise_tied: bad args");
    OODGAN_REQUIRE(period > 0 && (period & 3) == 0 && n_per_image % period == 0,
                   "latent_noise_tied: period = %ld must be a multiple of 4 that divides n_per_image = %ld", period, n_per_image);
    return latent_noise(w, w_in, ids, t_dev, B, n_per_image, period, seed, total_steps, sigma0, noise_ramp, stream);
}

extern "C" int oodgan_latent_prior_fwd_bwd(const float* w, const float* a, float* g, float* loss, int B, long n, int a_batched, float weight,
                                           void* stream) {
    OODGAN_REQUIRE(w && a && loss && B > 0 && n > 0, "latent_prior: bad args");
    return latent_prior(w, a, g, loss, nullptr, 1, B, n, a_batched, weight, stream);
}

extern "C" int oodgan_latent_prior_fwd_bwd_row(const float* w, const float* a, float* g, float* loss_table, const int* row_dev, int nrows, int B,
                                               long n, int a_batched, float weight, void* stream) {
    OODGAN_REQUIRE(w && a && loss_table && row_dev && nrows > 0 && B > 0 && n > 0, "latent_prior_row: bad args");
    return latent_prior(w, a, g, loss_table, row_dev, nrows, B, n, a_batched, weight, stream);
}

extern "C" int oodgan_latent_step(float* w, float* g, float* m, float* v, int B, int L, int D, float lr, float beta1, float beta2, float eps,
                                  int* t_dev, int total_steps, float rampup, float rampdown, const float* layer_lr, float delta_reg, int tied,
                                  float* delta_table, int nrows, void* stream) {
    OODGAN_REQUIRE(w && g && m && v && t_dev && B > 0 && L > 0 && D > 0 && total_steps > 0, "latent_step: bad args");
    OODGAN_REQUIRE(delta_reg >= 0.f && (delta_table == nullptr || nrows > 0), "latent_step: delta_reg = %g, nrows = %d", (double)delta_reg, nrows);
    const double n = (double)L * (double)D;
    hipLaunchKernelGGL(sched_counter_inc_kernel, dim3(1), dim3(1), 0, as_stream(stream), t_dev);
    hipLaunchKernelGGL(latent_step_kernel, dim3(B), dim3(256), 0, as_stream(stream), w, g, m, v, L, D, lr, beta1, beta2, eps, t_dev, total_steps,
                       rampup, rampdown, layer_lr, (float)(2.0 * (double)delta_reg / n), tied, delta_table, nrows, 1.0 / n);
    return check_launch("latent_step");
}

extern "C" int oodgan_style_step(float* delta, float* gs, float* m, float* v, int B, int R, float lr, float beta1, float beta2, float eps,
                                 int* t_dev, int total_steps, float rampup, float rampdown, float grad_div, const int* row_lat,
                                 const float* layer_lr, float style_reg, float* reg_table, int nrows, void* stream) {
    OODGAN_REQUIRE(delta && gs && m && v && t_dev && B > 0 && R > 0 && total_steps > 0, "style_step: bad args");
    OODGAN_REQUIRE(B <= 65535 * 1024, "style_step: B = %d: too large", B);
    OODGAN_REQUIRE(layer_lr == nullptr || row_lat != nullptr, "style_step: layer_lr without row_lat");
    OODGAN_REQUIRE(grad_div > 0.f && style_reg >= 0.f && (reg_table == nullptr || nrows > 0), "style_step: grad_div = %g, style_reg = %g, nrows = %d",
                   (double)grad_div, (double)style_reg, nrows);
    hipLaunchKernelGGL(sched_counter_inc_kernel, dim3(1), dim3(1), 0, as_stream(stream), t_dev);
    hipLaunchKernelGGL(style_step_kernel, dim3(B), dim3(256), 0, as_stream(stream), delta, gs, m, v, R, lr, beta1, beta2, eps, t_dev, total_steps,
                       rampup, rampdown, grad_div, row_lat, layer_lr, (float)(2.0 * (double)style_reg / (double)R), reg_table, nrows,
                       1.0 / (double)R);
    return check_launch("style_step");
}
