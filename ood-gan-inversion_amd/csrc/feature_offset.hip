// Feature offset of the W+ loop: the loop optimises, beside the latents, an offset D (B, C, h, h) added to the input of one
// styled up-conv, x' = x(w) + D.  Two plain streaming kernels: the addition (a launch of this library, so that a launch plan replays it) and
// the feature side of a step (division by the loss scale, regulariser, Adam).  Everything that varies per step comes from the loop's device
// counter; no state lives here, no float atomics: both are bit-reproducible.
#include "loss_common.hpp"

namespace {
using namespace oodgan;

constexpr double kPi = 3.14159265358979323846;

// elements per block of feature_step_kernel = elements per partial sum (oodgan_feature_step_nparts): 256 threads x 4 quads.  512*32*32
// values per image are 128 blocks per image, 1024 blocks for a batch of 8.
constexpr int kFeatChunk = 4096;

// ---------------------------------------------------------------------------------------------------------------- y = x + delta
// VEC: all three pointers 16-byte aligned — n / 4 quads, 16 bytes per lane, and the n % 4 last elements one by one; otherwise every element
// on its own.  One fp32 addition per element either way.
template <bool VEC>
__global__ __launch_bounds__(256) void feature_add_kernel(const float* __restrict__ x, const float* __restrict__ d, float* __restrict__ y,
                                                          long n) {
    const long stride = (long)gridDim.x * blockDim.x;
    const long i0 = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (VEC) {
        const long nq = n >> 2;
        for (long q = i0; q < nq; q += stride) {
            const float4 a = reinterpret_cast<const float4*>(x)[q], b = reinterpret_cast<const float4*>(d)[q];
            reinterpret_cast<float4*>(y)[q] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
        }
        const long tail = (nq << 2) + i0;
        if (tail < n) y[tail] = x[tail] + d[tail];      // at most three elements: the first threads of the first block
    } else {
        for (long i = i0; i < n; i += stride) y[i] = x[i] + d[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------- feature step
// wplus_sched.hip's lr_multiplier (rosinality projector.py get_lr without its initial lr): the same expressions, the same bits
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

// one element: the arithmetic of adam_dev_sched_kernel (wplus_sched.hip), returns d^2 in double.  Its expressions, m + (g - m) * (1 - beta1),
// v * beta2 + (1 - beta2) * g * g, w - step * (m / (sqrt(v) * c + eps)), leave the compiler a choice of which product to fuse into the addition;
// the roundings it took there are written out here (the second moment: both products rounded, then one fused multiply-add), so that the
// all-off configuration keeps that kernel's bits in the vector and the element-by-element form alike — tests/test_hip_fspace.py pins it.
__device__ __forceinline__ double feature_step_elem(float& d, float& g, float& m, float& v, float grad_div, float coef, float step_size,
                                                    float inv_bc2_sqrt, float beta1, float beta2, float eps) {
    const float d0 = d;
    float gi = g / grad_div;
    if (coef != 0.f) gi = fmaf(coef, d0, gi);
    g = gi;
    const float mi = fmaf(gi - m, 1.f - beta1, m);
    const float vi = fmaf(gi, __fmul_rn(1.f - beta2, gi), __fmul_rn(v, beta2));
    m = mi;
    v = vi;
    d = fmaf(-step_size, mi / fmaf(sqrtf(vi), inv_bc2_sqrt, eps), d0);
    return (double)d0 * (double)d0;
}

// grid: (nparts, B); block j of image b owns elements [j * kFeatChunk, min(n, (j + 1) * kFeatChunk)).  part (B, nparts) double, may be NULL
// (no table): part[b][j] = sum of d^2 over the block's elements BEFORE the update — per thread in element order, then the wave's xor
// tree, then the four waves in order.  VEC: n % 4 == 0 and all four pointers 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void feature_step_kernel(float* __restrict__ delta, float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, long n, float lr, float beta1, float beta2, float eps,
                                                           const int* __restrict__ t_dev, int total_steps, float rampup, float rampdown,
                                                           float grad_div, float coef, double* __restrict__ part) {
    __shared__ double red[4];
    const int t = t_dev[0] + 1;         // the latent-side call of the same step increments the counter afterwards
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    const float step_size = (float)((double)lr * lr_multiplier(t - 1, total_steps, rampup, rampdown) / bc1);
    const float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    const long base = (long)blockIdx.y * n;
    const long e0 = (long)blockIdx.x * kFeatChunk;
    const long e1 = e0 + kFeatChunk < n ? e0 + kFeatChunk : n;
    double acc = 0.0;
    if (VEC) {
        for (long e = e0 + 4 * (long)threadIdx.x; e < e1; e += 1024) {
            float4 d4 = *reinterpret_cast<const float4*>(delta + base + e), g4 = *reinterpret_cast<const float4*>(g + base + e);
            float4 m4 = *reinterpret_cast<const float4*>(m + base + e), v4 = *reinterpret_cast<const float4*>(v + base + e);
            acc += feature_step_elem(d4.x, g4.x, m4.x, v4.x, grad_div, coef, step_size, inv_bc2_sqrt, beta1, beta2, eps);
            acc += feature_step_elem(d4.y, g4.y, m4.y, v4.y, grad_div, coef, step_size, inv_bc2_sqrt, beta1, beta2, eps);
            acc += feature_step_elem(d4.z, g4.z, m4.z, v4.z, grad_div, coef, step_size, inv_bc2_sqrt, beta1, beta2, eps);
            acc += feature_step_elem(d4.w, g4.w, m4.w, v4.w, grad_div, coef, step_size, inv_bc2_sqrt, beta1, beta2, eps);
            *reinterpret_cast<float4*>(delta + base + e) = d4;
            *reinterpret_cast<float4*>(g + base + e) = g4;
            *reinterpret_cast<float4*>(m + base + e) = m4;
            *reinterpret_cast<float4*>(v + base + e) = v4;
        }
    } else {
        for (long e = e0 + threadIdx.x; e < e1; e += 256) {
            const long i = base + e;
            float di = delta[i], gi = g[i], mi = m[i], vi = v[i];
            acc += feature_step_elem(di, gi, mi, vi, grad_div, coef, step_size, inv_bc2_sqrt, beta1, beta2, eps);
            delta[i] = di;
            g[i] = gi;
            m[i] = mi;
            v[i] = vi;
        }
    }
    if (part == nullptr) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// grid: (B), one wave per image: R_b = (sum of the image's partials) / n, rounded once, to row min(t_dev[0], nrows - 1) of the table — the
// zero-based step, the counter not yet incremented.  A lane adds its partials in index order, then the wave's xor tree.
__global__ __launch_bounds__(64) void feature_reg_finish_kernel(const double* __restrict__ part, float* __restrict__ table, int nparts,
                                                                double inv_n, const int* __restrict__ t_dev, int nrows) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double s = 0.0;
    for (int j = lane; j < nparts; j += 64) s += part[(long)b * nparts + j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) table[loss_row(t_dev, nrows, gridDim.x) + b] = (float)(s * inv_n);
}

inline bool aligned16(const void* a, const void* b, const void* c, const void* d) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) | reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

}  // namespace

extern "C" int oodgan_feature_add(const float* x, const float* delta, float* y, long n, void* stream) {
    OODGAN_REQUIRE(x && delta && y && n > 0, "feature_add: bad args");
    const bool vec = n >= 4 && aligned16(x, delta, y, nullptr);
    if (vec)
        hipLaunchKernelGGL(feature_add_kernel<true>, dim3(stream_grid(n >> 2, 256)), dim3(256), 0, as_stream(stream), x, delta, y, n);
    else
        hipLaunchKernelGGL(feature_add_kernel<false>, dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream), x, delta, y, n);
    return check_launch("feature_add");
}

extern "C" int oodgan_feature_step_nparts(long n_per_image) {
    if (n_per_image <= 0 || (n_per_image + kFeatChunk - 1) / kFeatChunk > 65535L * 1024L) return 0;
    return (int)((n_per_image + kFeatChunk - 1) / kFeatChunk);
}

extern "C" int oodgan_feature_step(float* delta, float* g, float* m, float* v, int B, long n_per_image, float lr, float beta1, float beta2,
                                   float eps, const int* t_dev, int total_steps, float rampup, float rampdown, float grad_div,
                                   float feature_reg, float* reg_table, int nrows, double* part, void* stream) {
    OODGAN_REQUIRE(delta && g && m && v && t_dev && B > 0 && n_per_image > 0 && total_steps > 0, "feature_step: bad args");
    const int nparts = oodgan_feature_step_nparts(n_per_image);
    OODGAN_REQUIRE(B <= 65535 && nparts > 0, "feature_step: B = %d images of %ld values: too large", B, n_per_image);
    OODGAN_REQUIRE(grad_div > 0.f && feature_reg >= 0.f && (reg_table == nullptr || nrows > 0),
                   "feature_step: grad_div = %g, feature_reg = %g, nrows = %d", (double)grad_div, (double)feature_reg, nrows);
    OODGAN_REQUIRE(reg_table == nullptr || part != nullptr, "feature_step: reg_table without part, the (B, oodgan_feature_step_nparts) partial sums");
    const float coef = (float)(2.0 * (double)feature_reg / (double)n_per_image);
    double* pp = reg_table ? part : nullptr;
    const bool vec = (n_per_image & 3) == 0 && aligned16(delta, g, m, v);
    if (vec)
        hipLaunchKernelGGL(feature_step_kernel<true>, dim3(nparts, B), dim3(256), 0, as_stream(stream), delta, g, m, v, n_per_image, lr, beta1,
                           beta2, eps, t_dev, total_steps, rampup, rampdown, grad_div, coef, pp);
    else
        hipLaunchKernelGGL(feature_step_kernel<false>, dim3(nparts, B), dim3(256), 0, as_stream(stream), delta, g, m, v, n_per_image, lr, beta1,
                           beta2, eps, t_dev, total_steps, rampup, rampdown, grad_div, coef, pp);
    if (reg_table)
        hipLaunchKernelGGL(feature_reg_finish_kernel, dim3(B), dim3(64), 0, as_stream(stream), (const double*)part, reg_table, nparts,
                           1.0 / (double)n_per_image, t_dev, nrows);
    return check_launch("feature_step");
}
