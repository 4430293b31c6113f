// Fitted out-of-domain mask of the W+ loop (loss_region='fit'): beside the latents the loop optimises the logits l (B,1,m,m) of
// a low-resolution mask a = sigmoid(l); the loss weight of the composite objective (§5) is its bilinear enlargement beta = U(a), (B,1,S,S),
// U exactly F.interpolate(a, size=(S,S), mode='bilinear', align_corners=False) (source coordinates below 0 clamped to 0), F = S / m.
// The mask carries the reference's MaskLoss with target 1 on alpha = 1 - a (src/losses/mask_loss.py): an area hinge
// area_weight * max(0, mean(1 - a) - area) and a binarisation term binary_weight * mean(min(a, 1 - a)), per image.
//
// Three entries, five kernels, all HBM- or latency-bound streaming kernels; no float atomics, every sum in a fixed order: bit-reproducible.
//   expand  l -> a (one thread per cell), a -> beta (one thread per four pixels of a row);
//   chain   one pass over dL/dc, G, x and beta: e(p) = sum_c dL/dc_c(p) (G_c - x_c)(p), then dL/dc <- beta (.) dL/dc in place — what
//           scale_by_plane does for a frozen plane, plus the plane of dL/dbeta;
//   step    the per-image means of 1 - a and min(a, 1 - a) (one block per image, double), then per row of cells the gather U^T e — a cell
//           reads its own separable tent support, at most 2F x 2F pixels: the vertical sums of the row's 2F pixel rows per pixel column
//           (coalesced, 16 bytes per lane) into LDS, then one thread per cell the horizontal sum — the regulariser's gradients, the
//           sigmoid's derivative and Adam on l.
// S and m are powers of two, 16 <= S <= 1024, 2 <= m <= 256, F >= 2: F/2 is an integer and every tent weight is an exact binary fraction.
#include "loss_common.hpp"

namespace {
using namespace oodgan;

constexpr double kPi = 3.14159265358979323846;
constexpr int kMaxS = 1024;       // the step kernel keeps one double per pixel column (padded) in LDS
constexpr int kMaxM = 256;        // ... and owns a row of cells with one thread per cell

// the weight pixel y gives cell j along one axis: the tent about the clamped source coordinate of F.interpolate(align_corners=False).
// Pixels left of the first cell's centre (and right of the last one's) give that cell their whole weight, as the clamping implies.
__device__ __forceinline__ float tent_weight(int y, int j, float inv_f, int m) {
    const float src = fminf(fmaxf(((float)y + 0.5f) * inv_f - 0.5f, 0.f), (float)(m - 1));
    return fmaxf(0.f, 1.f - fabsf(src - (float)j));
}

// ---------------------------------------------------------------------------------------------------------------- expand
__global__ __launch_bounds__(256) void maskfit_sigmoid_kernel(const float* __restrict__ logit, float* __restrict__ a, long n) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride) {
        const float l = logit[i];
        const float em = expf(-fabsf(l));                      // in (0, 1]: neither branch overflows
        a[i] = l >= 0.f ? 1.f / (1.f + em) : em / (1.f + em);
    }
}

// one thread per four pixels of an output row; a (B, m, m) stays in the caches (at most 256 KB per image)
__global__ __launch_bounds__(256) void maskfit_upsample_kernel(const float* __restrict__ a, float* __restrict__ beta, int m, int S, float inv_f,
                                                               long nquads) {
    const long stride = (long)gridDim.x * blockDim.x;
    const int S4 = S >> 2;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < nquads; q += stride) {
        const int x4 = (int)(q % S4);
        const long row = q / S4;
        const int y = (int)(row % S);
        const long b = row / S;
        const float sy = fmaxf(((float)y + 0.5f) * inv_f - 0.5f, 0.f);
        const int y0 = (int)sy, y1 = y0 + (y0 < m - 1 ? 1 : 0);
        const float ly = sy - (float)y0;
        const float* __restrict__ r0 = a + (b * m + y0) * m;
        const float* __restrict__ r1 = a + (b * m + y1) * m;
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float sx = fmaxf(((float)(4 * x4 + k) + 0.5f) * inv_f - 0.5f, 0.f);
            const int x0 = (int)sx, x1 = x0 + (x0 < m - 1 ? 1 : 0);
            const float lx = sx - (float)x0;
            const float top = (1.f - lx) * r0[x0] + lx * r0[x1];
            const float bot = (1.f - lx) * r1[x0] + lx * r1[x1];
            o[k] = (1.f - ly) * top + ly * bot;
        }
        reinterpret_cast<float4*>(beta)[q] = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- chain
// one thread per four pixels: beta read once for the C channels; e = sum_c g_c (G_c - x_c) in channel order, then g_c <- beta g_c
__global__ __launch_bounds__(256) void maskfit_chain_kernel(float* __restrict__ g, const float* __restrict__ gen, const float* __restrict__ x,
                                                            const float* __restrict__ beta, float* __restrict__ e, int C, long HW4, long nquads) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < nquads; q += stride) {
        const long b = q / HW4, p = q - b * HW4;
        const float4 w = reinterpret_cast<const float4*>(beta)[q];
        const long base = b * C * HW4 + p;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c = 0; c < C; ++c) {
            const long i = base + c * HW4;
            float4 gv = reinterpret_cast<const float4*>(g)[i];
            const float4 iv = reinterpret_cast<const float4*>(gen)[i], xv = reinterpret_cast<const float4*>(x)[i];
            acc.x = fmaf(gv.x, iv.x - xv.x, acc.x);
            acc.y = fmaf(gv.y, iv.y - xv.y, acc.y);
            acc.z = fmaf(gv.z, iv.z - xv.z, acc.z);
            acc.w = fmaf(gv.w, iv.w - xv.w, acc.w);
            gv.x *= w.x;
            gv.y *= w.y;
            gv.z *= w.z;
            gv.w *= w.w;
            reinterpret_cast<float4*>(g)[i] = gv;
        }
        reinterpret_cast<float4*>(e)[q] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------------------- step
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

// grid: (B), one block per image.  stat[2b] = mean(1 - a_b), stat[2b + 1] = mean(min(a_b, 1 - a_b)), both double: a thread adds its cells in
// index order, then the wave's xor tree, then the four waves in order (two deterministic stages).  Row min(t_dev[0], nrows - 1) of the two
// tables receives the hinge max(0, mean(1 - a) - area) and the binarisation mean, each rounded once; NULL tables: not written.
__global__ __launch_bounds__(256) void maskfit_stats_kernel(const float* __restrict__ a, double* __restrict__ stat, float* __restrict__ area_table,
                                                            float* __restrict__ binary_table, int n, float area, const int* __restrict__ t_dev,
                                                            int nrows) {
    __shared__ double red[8];
    const int b = blockIdx.x;
    const float* __restrict__ ap = a + (long)b * n;
    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) {
        const double ai = (double)ap[i], r = 1.0 - ai;
        s1 += r;
        s2 += fmin(ai, r);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = s1;
        red[4 + (threadIdx.x >> 6)] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double m1 = ((red[0] + red[1]) + (red[2] + red[3])) / (double)n, m2 = ((red[4] + red[5]) + (red[6] + red[7])) / (double)n;
        stat[2 * b] = m1;
        stat[2 * b + 1] = m2;
        const long row = loss_row(t_dev, nrows, gridDim.x);
        const double over = m1 - (double)area;
        if (area_table) area_table[row + b] = (float)(over > 0.0 ? over : 0.0);
        if (binary_table) binary_table[row + b] = (float)m2;
    }
}

// grid: (m, B); block (j, b) owns the m cells of cell row j of image b.  ncol4 = S / 4 <= 256 float4 columns; the 256 threads form
// G = 256 / ncol4 groups, group g takes the pixel rows y0 + g, y0 + g + G, ... of the row's support and leaves its vertical sum per pixel
// column in LDS (double; one pad slot per F columns: adjacent cells are then F + 1 slots apart).  Thread jx < m then adds, pixel column by
// pixel column in ascending order, the G group sums (ascending) times the column's tent weight.
__global__ __launch_bounds__(256) void maskfit_step_kernel(float* __restrict__ logit, float* __restrict__ g, float* __restrict__ mom,
                                                           float* __restrict__ var, const float* __restrict__ a, const float* __restrict__ e,
                                                           const double* __restrict__ stat, int m, int S, int F, float inv_f, float lr, float beta1,
                                                           float beta2, float eps, const int* __restrict__ t_dev, int total_steps, float rampup,
                                                           float rampdown, float grad_div, float area, float coef_area, float coef_binary) {
    __shared__ double vs[kMaxS + kMaxS / 2];
    const int j = blockIdx.x, b = blockIdx.y;
    const int ncol4 = S >> 2, G = 256 / ncol4;
    const int grp = threadIdx.x / ncol4, c4 = threadIdx.x - grp * ncol4;
    const int half = F >> 1;
    const int y0 = max(F * j - half, 0), y1 = min(F * j + F + half, S);
    const float* __restrict__ ep = e + (long)b * S * S;
    if (grp < G) {
        double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
        for (int y = y0 + grp; y < y1; y += G) {
            const double w = (double)tent_weight(y, j, inv_f, m);
            const float4 v = *reinterpret_cast<const float4*>(ep + (long)y * S + 4 * c4);
            acc0 += w * (double)v.x;
            acc1 += w * (double)v.y;
            acc2 += w * (double)v.z;
            acc3 += w * (double)v.w;
        }
        const int i0 = grp * S + 4 * c4;                       // F >= 2 is even or 2: the four columns may straddle a pad slot
        vs[i0 + i0 / F] = acc0;
        vs[i0 + 1 + (i0 + 1) / F] = acc1;
        vs[i0 + 2 + (i0 + 2) / F] = acc2;
        vs[i0 + 3 + (i0 + 3) / F] = acc3;
    }
    __syncthreads();
    const int jx = threadIdx.x;
    if (jx >= m) return;
    const int x0 = max(F * jx - half, 0), x1 = min(F * jx + F + half, S);
    double sum = 0.0;
    for (int x = x0; x < x1; ++x) {
        double col = 0.0;
        for (int k = 0; k < G; ++k) {
            const int i = k * S + x;
            col += vs[i + i / F];
        }
        sum += (double)tent_weight(x, jx, inv_f, m) * col;
    }
    // regulariser: d/da of area_weight * max(0, mean(1 - a) - area) is -area_weight / m^2 where the hinge is open (0 at a tie, as torch's);
    // d/da of binary_weight * mean(min(a, 1 - a)) is +-binary_weight / m^2, 0 at a = 1/2
    const long ci = ((long)b * m + j) * m + jx;
    const float ai = a[ci];
    float gi = (float)sum / grad_div;
    if (stat[2 * b] - (double)area > 0.0) gi -= coef_area;
    gi += ai < 0.5f ? coef_binary : ai > 0.5f ? -coef_binary : 0.f;
    // da/dl = a (1 - a) from the logit itself: exp(-|l|) / (1 + exp(-|l|))^2 keeps its relative accuracy where a rounds to 0 or 1
    const float l0 = logit[ci];
    const float em = expf(-fabsf(l0)), op = 1.f + em;
    gi *= em / (op * op);
    g[ci] = gi;
    // Adam as feature_step_kernel (feature_offset.hip): the same roundings, t = t_dev[0] + 1, the counter left alone
    const int t = t_dev[0] + 1;
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    const float step_size = (float)((double)lr * lr_multiplier(t - 1, total_steps, rampup, rampdown) / bc1);
    const float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    const float mi = fmaf(gi - mom[ci], 1.f - beta1, mom[ci]);
    const float vi = fmaf(gi, __fmul_rn(1.f - beta2, gi), __fmul_rn(var[ci], beta2));
    mom[ci] = mi;
    var[ci] = vi;
    logit[ci] = fmaf(-step_size, mi / fmaf(sqrtf(vi), inv_bc2_sqrt, eps), l0);
}

inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
inline bool shape_ok(int B, int m, int S) {
    return B > 0 && B <= 65535 && pow2(S) && pow2(m) && S >= 16 && S <= kMaxS && m >= 2 && m <= kMaxM && S / m >= 2;
}
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" int oodgan_maskfit_expand(const float* logit, float* a, float* beta, int B, int m, int S, void* stream) {
    OODGAN_REQUIRE(logit && a && beta, "maskfit_expand: bad args");
    OODGAN_REQUIRE(shape_ok(B, m, S), "maskfit_expand: B = %d, m = %d, S = %d: S and m must be powers of two, 16 <= S <= %d, 2 <= m <= %d, S / m >= 2",
                   B, m, S, kMaxS, kMaxM);
    OODGAN_REQUIRE(aligned16(beta), "maskfit_expand: beta must be 16-byte aligned");
    const long n = (long)B * m * m, nquads = (long)B * S * (S >> 2);
    hipLaunchKernelGGL(maskfit_sigmoid_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream), logit, a, n);
    hipLaunchKernelGGL(maskfit_upsample_kernel, dim3(stream_grid(nquads, 256)), dim3(256), 0, as_stream(stream), (const float*)a, beta, m, S,
                       1.f / (float)(S / m), nquads);
    return check_launch("maskfit_expand");
}

extern "C" int oodgan_maskfit_chain(float* gimg, const float* gen, const float* x, const float* beta, float* e, int B, int C, int S, void* stream) {
    OODGAN_REQUIRE(gimg && gen && x && beta && e && B > 0 && C > 0, "maskfit_chain: bad args");
    OODGAN_REQUIRE(pow2(S) && S >= 16 && S <= kMaxS, "maskfit_chain: S = %d must be a power of two in [16, %d]", S, kMaxS);
    OODGAN_REQUIRE(aligned16(gimg) && aligned16(gen) && aligned16(x) && aligned16(beta) && aligned16(e), "maskfit_chain: pointers must be 16-byte aligned");
    const long HW4 = ((long)S * S) >> 2, nquads = (long)B * HW4;
    hipLaunchKernelGGL(maskfit_chain_kernel, dim3(stream_grid(nquads, 256)), dim3(256), 0, as_stream(stream), gimg, gen, x, beta, e, C, HW4, nquads);
    return check_launch("maskfit_chain");
}

extern "C" int oodgan_maskfit_step(float* logit, float* g, float* m, float* v, const float* a, const float* e, int B, int msize, int S, float lr,
                                   float beta1, float beta2, float eps, const int* t_dev, int total_steps, float rampup, float rampdown,
                                   float grad_div, float area, float area_weight, float binary_weight, float* area_table, float* binary_table,
                                   int nrows, double* stat, void* stream) {
    OODGAN_REQUIRE(logit && g && m && v && a && e && t_dev && stat && total_steps > 0, "maskfit_step: bad args");
    OODGAN_REQUIRE(shape_ok(B, msize, S), "maskfit_step: B = %d, m = %d, S = %d: S and m must be powers of two, 16 <= S <= %d, 2 <= m <= %d, S / m >= 2",
                   B, msize, S, kMaxS, kMaxM);
    OODGAN_REQUIRE(grad_div > 0.f && area >= 0.f && area <= 1.f && area_weight >= 0.f && binary_weight >= 0.f,
                   "maskfit_step: grad_div = %g, area = %g, area_weight = %g, binary_weight = %g", (double)grad_div, (double)area,
                   (double)area_weight, (double)binary_weight);
    OODGAN_REQUIRE((area_table == nullptr && binary_table == nullptr) || nrows > 0, "maskfit_step: tables with nrows = %d", nrows);
    OODGAN_REQUIRE(aligned16(e), "maskfit_step: e must be 16-byte aligned");
    const int n = msize * msize, F = S / msize;
    hipLaunchKernelGGL(maskfit_stats_kernel, dim3(B), dim3(256), 0, as_stream(stream), a, stat, area_table, binary_table, n, area, t_dev, nrows);
    hipLaunchKernelGGL(maskfit_step_kernel, dim3(msize, B), dim3(256), 0, as_stream(stream), logit, g, m, v, a, e, (const double*)stat, msize, S, F,
                       1.f / (float)F, lr, beta1, beta2, eps, t_dev, total_steps, rampup, rampdown, grad_div, area,
                       (float)((double)area_weight / (double)n), (float)((double)binary_weight / (double)n));
    return check_launch("maskfit_step");
}
