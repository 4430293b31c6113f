// P_N+ prior of the W+ loop (II2S: Zhu et al., "Improved StyleGAN Embedding: Where are the Good Latents?"): the squared length
// of the latent in the whitened space of the mapping network's outputs,
//   q = l5(w) - mu,  l5(t) = t > 0 ? t : 5 t  (the inverse of the mapping network's last LeakyReLU(0.2));   pn_b = mean_{l,d} q^T M q,
// M = C diag(1 / sigma^2) C^T the symmetric float32 matrix oodgan/pn.py forms once per set of mapping weights.  Two kernels, the two-stage
// pattern of the pixel terms: one block per latent row (b, l) computes y = M q, adds coef * l5'(w) * y into the latent gradient and leaves
// q . y in a persistent (B * L) buffer of doubles; one wave per image sums its L partials into the loss row.  M (1 MB at D = 512) stays in L2
// for the B * L blocks that read it.  The products M q and q . y are accumulated in double in a fixed order; no float atomics, no state:
// bit-reproducible.
#include "loss_common.hpp"

namespace {
using namespace oodgan;

constexpr int kPnMaxD = 4096;           // y (double) and q (float) of one row in LDS: 12 bytes per column, 48 KB
constexpr int kPnThreads = 1024;        // sixteen waves per row: at D = 512 a wave owns 32 of the 512 columns of y (with four waves a call is 37 us, latency-bound)
constexpr int kPnWaves = kPnThreads / 64;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// grid: (B * L), one block of sixteen waves per row.  LDS: y[D] doubles, then q[D] floats.
//   1. q_d = l5(w_d) - mu_d, one fp32 multiplication and one fp32 subtraction;
//   2. wave v owns the output columns 64 i + 4 v ... + 3: y_d = sum_k M[d][k] q_k, every product exact in double, a lane adds its k in
//      ascending order (VEC: k = 4 lane + 256 j and the four values of a quad in order, 16-byte reads of M and q; otherwise k = lane + 64 j),
//      then the wave's xor tree.  Four columns at a time keep four independent loads in flight per lane;
//   3. thread t owns the columns d = t + 1024 j: g_d += (w_d > 0 ? coef : 5 coef) * (float) y_d (one fused multiply-add; l5'(0) = 5, torch's
//      leaky_relu backward) and p += q_d y_d in double, in column order; the wave's xor tree, the sixteen waves in order -> part[row].
// VEC needs D % 4 == 0 and a 16-byte aligned M (its rows are then aligned too); g NULL: the loss only, the same bits.
template <bool VEC>
__global__ __launch_bounds__(kPnThreads) void pn_row_kernel(const float* __restrict__ w, const float* __restrict__ mu, const float* __restrict__ M,
                                                     float* __restrict__ g, double* __restrict__ part, int D, float coef, float coef5) {
    extern __shared__ __align__(16) double pn_lds[];
    __shared__ double red[kPnWaves];
    double* y = pn_lds;
    float* q = reinterpret_cast<float*>(pn_lds + D);
    const long base = (long)blockIdx.x * D;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int d = threadIdx.x; d < D; d += kPnThreads) {
        const float t = w[base + d];
        q[d] = __fsub_rn(t > 0.f ? t : __fmul_rn(5.f, t), mu[d]);
    }
    __syncthreads();
    for (int d0 = 4 * wv; d0 < D; d0 += 4 * kPnWaves) {
        const float* r0 = M + (long)d0 * D;                     // columns past the end re-read the last one; their sums are not stored
        const float* r1 = M + (long)min(d0 + 1, D - 1) * D;
        const float* r2 = M + (long)min(d0 + 2, D - 1) * D;
        const float* r3 = M + (long)min(d0 + 3, D - 1) * D;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (VEC) {
            for (int k = 4 * lane; k < D; k += 256) {
                const float4 qq = *reinterpret_cast<const float4*>(q + k);
                const float4 m0 = *reinterpret_cast<const float4*>(r0 + k), m1 = *reinterpret_cast<const float4*>(r1 + k);
                const float4 m2 = *reinterpret_cast<const float4*>(r2 + k), m3 = *reinterpret_cast<const float4*>(r3 + k);
                const double qx = (double)qq.x, qy = (double)qq.y, qz = (double)qq.z, qw = (double)qq.w;
                a0 = fma((double)m0.w, qw, fma((double)m0.z, qz, fma((double)m0.y, qy, fma((double)m0.x, qx, a0))));
                a1 = fma((double)m1.w, qw, fma((double)m1.z, qz, fma((double)m1.y, qy, fma((double)m1.x, qx, a1))));
                a2 = fma((double)m2.w, qw, fma((double)m2.z, qz, fma((double)m2.y, qy, fma((double)m2.x, qx, a2))));
                a3 = fma((double)m3.w, qw, fma((double)m3.z, qz, fma((double)m3.y, qy, fma((double)m3.x, qx, a3))));
            }
        } else {
            for (int k = lane; k < D; k += 64) {
                const double qk = (double)q[k];
                a0 = fma((double)r0[k], qk, a0);
                a1 = fma((double)r1[k], qk, a1);
                a2 = fma((double)r2[k], qk, a2);
                a3 = fma((double)r3[k], qk, a3);
            }
        }
        a0 = wave_sum_f64(a0);
        a1 = wave_sum_f64(a1);
        a2 = wave_sum_f64(a2);
        a3 = wave_sum_f64(a3);
        if (lane < 4 && d0 + lane < D) y[d0 + lane] = lane == 0 ? a0 : lane == 1 ? a1 : lane == 2 ? a2 : a3;
    }
    __syncthreads();
    double p = 0.0;
    for (int d = threadIdx.x; d < D; d += kPnThreads) {
        const double yd = y[d];
        p = fma((double)q[d], yd, p);
        if (g) g[base + d] = fmaf(w[base + d] > 0.f ? coef : coef5, (float)yd, g[base + d]);
    }
    p = wave_sum_f64(p);
    if (lane == 0) red[wv] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < kPnWaves; ++i) s += red[i];
        part[blockIdx.x] = s;
    }
}

// grid: (B), one wave per image: pn_b = (sum of the image's L partials) / (L D), rounded once, to loss[row + b].  A lane adds its partials in
// index order, then the wave's xor tree.
__global__ __launch_bounds__(64) void pn_finish_kernel(const double* __restrict__ part, float* __restrict__ loss, int L, double inv_n,
                                                       const int* __restrict__ row_dev, int nrows) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double s = 0.0;
    for (int l = lane; l < L; l += 64) s += part[(long)b * L + l];
    s = wave_sum_f64(s);
    if (lane == 0) loss[loss_row(row_dev, nrows, gridDim.x) + b] = (float)(s * inv_n);
}

int pn_prior(const float* w, const float* mu, const float* M, float* g, float* loss, const int* row_dev, int nrows, int B, int L, int D,
             float weight, double* part, void* stream) {
    OODGAN_REQUIRE(D <= kPnMaxD, "pn_prior: D = %d: at most %d columns", D, kPnMaxD);
    OODGAN_REQUIRE(B <= 65535 && (long)B * L <= 0x7fffffffL, "pn_prior: B = %d images of %d rows: too large", B, L);
    OODGAN_REQUIRE(weight >= 0.f, "pn_prior: weight = %g", (double)weight);
    const double n = (double)L * (double)D;
    const float coef = (float)(2.0 * (double)weight / n);
    const float coef5 = coef * 5.f;
    const size_t lds = (size_t)D * (sizeof(double) + sizeof(float));
    const bool vec = (D & 3) == 0 && (reinterpret_cast<uintptr_t>(M) & 15) == 0;
    count_dispatch(OODGAN_DC_PN);
    if (vec)
        hipLaunchKernelGGL(pn_row_kernel<true>, dim3(B * L), dim3(kPnThreads), lds, as_stream(stream), w, mu, M, g, part, D, coef, coef5);
    else
        hipLaunchKernelGGL(pn_row_kernel<false>, dim3(B * L), dim3(kPnThreads), lds, as_stream(stream), w, mu, M, g, part, D, coef, coef5);
    hipLaunchKernelGGL(pn_finish_kernel, dim3(B), dim3(64), 0, as_stream(stream), (const double*)part, loss, L, 1.0 / n, row_dev, nrows);
    return check_launch("pn_prior");
}

}  // namespace

extern "C" int oodgan_pn_prior_fwd_bwd(const float* w, const float* mu, const float* M, float* g, float* loss, int B, int L, int D, float weight,
                                       double* part, void* stream) {
    OODGAN_REQUIRE(w && mu && M && loss && part && B > 0 && L > 0 && D > 0, "pn_prior: bad args");
    return pn_prior(w, mu, M, g, loss, nullptr, 1, B, L, D, weight, part, stream);
}

extern "C" int oodgan_pn_prior_fwd_bwd_row(const float* w, const float* mu, const float* M, float* g, float* loss_table, const int* row_dev,
                                           int nrows, int B, int L, int D, float weight, double* part, void* stream) {
    OODGAN_REQUIRE(w && mu && M && loss_table && row_dev && part && nrows > 0 && B > 0 && L > 0 && D > 0, "pn_prior_row: bad args");
    return pn_prior(w, mu, M, g, loss_table, row_dev, nrows, B, L, D, weight, part, stream);
}
