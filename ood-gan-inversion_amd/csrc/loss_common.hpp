// What the loss terms of the W+ step share (loss_pixel.hip: MSE, composite MSE, robust rho; loss_ssim.hip; lpips.hip; loss_pool.hip: the pooled view a term may be taken on): every term
// reduces per-block partial sums to one value per image and writes it either to loss[b] or to a row of the loop's (nrows, B) loss table.
#pragma once
#include "common.hpp"

namespace oodgan {

// elements per block of the pixel-term kernels (loss_pixel.hip) = elements per partial sum (oodgan_mse_nparts)
constexpr int kMseChunk = 16384;

// Offset of the row the losses of B images go to.  row_dev != NULL: row min(row_dev[0], nrows - 1) of a (nrows, B) table — the W+ loop's
// loss table indexed by its device step counter, so that a recorded / replayed step (oodgan_plan_run, hipGraph) writes a new row each
// time; NULL: a plain loss[B].
__device__ __forceinline__ long loss_row(const int* __restrict__ row_dev, int nrows, unsigned B) {
    return row_dev ? (long)min(max(row_dev[0], 0), nrows - 1) * B : 0;
}

// loss[row + b] = (sum of image b's partials) * inv_n: one wave per image, the same order for every term.  grid: (B).
// A template so that only the units that launch it carry a copy.
template <typename T = float>
__global__ __launch_bounds__(64) void mean_finish_kernel(const T* __restrict__ part, T* __restrict__ loss, int nparts, T inv_n,
                                                         const int* __restrict__ row_dev, int nrows) {
    const int b = blockIdx.x, lane = threadIdx.x;
    T s = 0;
    for (int j = lane; j < nparts; j += 64) s += part[(long)b * nparts + j];
    s = wave_sum(s);
    const long row = loss_row(row_dev, nrows, gridDim.x);
    if (lane == 0) loss[row + b] = s * inv_n;
}

// ---- rho and psi of the pixel terms (loss_pixel.hip; loss_resample.hip)
// the square next to the public OODGAN_ROBUST_* kinds (1..3); it has no scale
constexpr int kSquare = 0;

// rho(d) (returned) and psi(d) of one element; s2 is a normal float (the robust entry points check it), so no denominator is zero
template <int KIND>
__device__ __forceinline__ float rho_psi(float d, float s, float s2, float& psi) {
    if constexpr (KIND == kSquare) {
        psi = d;
        return d * d;
    } else if constexpr (KIND == OODGAN_ROBUST_CHARBONNIER) {
        const float q = sqrtf(d * d + s2);
        psi = d / q;
        return q;
    } else if constexpr (KIND == OODGAN_ROBUST_HUBER) {
        const float a = fabsf(d);
        psi = fminf(fmaxf(d, -s), s);
        return a <= s ? 0.5f * d * d : s * (a - 0.5f * s);
    } else {
        const float r = s2 / (d * d + s2);
        psi = d * r * r;
        return 0.5f * d * d * r;
    }
}

// ---- F x F windows of the area pool (loss_pool.hip) and of the pooled pixel term (loss_pixel.hip): one thread owns a window
template <int F>
struct Row {                                     // the vector a window row is read in, and how many of them a row has
    using V = float4;
    static constexpr int N = F / 4;
};
template <>
struct Row<2> {
    using V = float2;
    static constexpr int N = 1;
};

// the window's sum: fp32, row-major order, never reassociated
__device__ __forceinline__ float sum_in_order(float acc, const float2 v) { return (acc + v.x) + v.y; }
__device__ __forceinline__ float sum_in_order(float acc, const float4 v) { return (((acc + v.x) + v.y) + v.z) + v.w; }

// what a full-resolution pointer must be aligned to for the row vectors of factor f (W % f == 0 then aligns every window row)
inline int pool_row_align(int f) { return f == 2 ? 8 : 16; }

}  // namespace oodgan
