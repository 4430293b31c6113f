// Colour map of the generator image beside the latents of the W+ loop.  Per image theta = (M row-major, b), 12 floats:
// the pixel term of the step is taken on c = M G + b instead of G, and theta takes an Adam step of its own.  The GENERATOR image is
// mapped, not the photograph: with the map on the target (M, b) -> (0, const) shrinks any residual.
//   oodgan_color_pixel_loss_fwd_bwd[_row]:  one streaming pass — a thread owns four neighbouring pixels in all three planes, forms c,
//       d = c - x (times beta), rho and psi (rho_psi<KIND>, loss_common.hpp), g = gscale psi (times beta), writes gimg = M^T g and
//       accumulates the loss partial (float) and the 12 sums  sum g_i G_j, sum g_i  (double) — read G, read x, write the gradient, the
//       bytes of the MSE kernel;  then mean_finish_kernel over the loss partials
//   oodgan_color_step:   one wave per image adds the partials in double, divides by grad_div, rounds once, adds the regulariser, zeroes
//       what is not free, and takes Adam's step (feature_step_kernel's roundings)
//   oodgan_color_apply:  out = M src + b, the same fused multiply-adds in the same order as the term
// No float atomics, no state: equal inputs give equal bits.  The map and its transpose are written as explicit fma chains in ONE order,
//   c_i = fma(M_i2, G_2, fma(M_i1, G_1, fma(M_i0, G_0, b_i)))  in DOUBLE,   gimg_j = fmaf(M_2j, g_2, fmaf(M_1j, g_1, M_0j g_0))  in float,
// so at the identity (1 G_i, + 0 G_j and + 0 are exact for finite G) c == G and gimg == g bit for bit.  The chain of c is in double and
// the term takes d = float(c - x) from it, ONE rounding of the residual, as the plain kernels' a - t is one rounding: with c rounded to
// float first a residual far below the image's size (|d| ~ 1e-5 |c|) keeps two digits, and the redescending psi of Geman-McClure at a
// small scale, ~ d^-3, is then wrong in its largest entries.  (At the identity float(G - x) in double is the float subtraction's result:
// the difference of two floats is exact in double unless they are 2^29 apart, where both roundings return the larger.)
// oodgan_color_apply rounds the same double chain to float once.  Everything after d — rho, psi, g — is loss_pixel.hip's expression
// compiled under the unit's default contraction, as there: the gradient at the identity is the plain kernels' gradient bit for bit
// (tests/test_hip_color.py).  An explicit fused multiply-add is never re-contracted, so no pragma is needed.
#include <cmath>
#include <cstdint>
#include <string>
#include "loss_common.hpp"

using namespace oodgan;

namespace {

constexpr double kPi = 3.14159265358979323846;
constexpr int kColorChunk = 2048;            // pixels per block of the term = pixels per partial sum (oodgan_color_nparts)
constexpr int kColorSums = 12;
constexpr int kApplyChunk = 4096;            // pixels per block of oodgan_color_apply

struct Theta {
    float M[3][3];          // for the transpose, in float
    double Md[3][3], bd[3]; // the same numbers for the chain of c, in double
};

// a block reads theta once: the first 12 threads, through LDS.  Ends with a barrier.
__device__ __forceinline__ Theta load_theta(const float* __restrict__ theta, float* sh /* 12 floats LDS */) {
    if (threadIdx.x < kColorSums) sh[threadIdx.x] = theta[threadIdx.x];
    __syncthreads();
    Theta t;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            t.M[i][j] = sh[3 * i + j];
            t.Md[i][j] = (double)sh[3 * i + j];
        }
        t.bd[i] = (double)sh[9 + i];
    }
    return t;
}

// c_i of one pixel in double, the one order
__device__ __forceinline__ double map_row(const Theta& t, int i, double g0, double g1, double g2) {
    return fma(t.Md[i][2], g2, fma(t.Md[i][1], g1, fma(t.Md[i][0], g0, t.bd[i])));
}

// four neighbouring elements of a plane from element p: one 16-byte access (VEC: HW % 4 == 0 and aligned pointers, so p + 3 < HW), or
// four guarded scalar ones
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ plane, long p, long HW, float* v) {
    if constexpr (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(plane + p);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = p + e < HW ? plane[p + e] : 0.f;
    }
}
template <bool VEC>
__device__ __forceinline__ void store4(float* __restrict__ plane, long p, long HW, const float* v) {
    if constexpr (VEC) {
        *reinterpret_cast<float4*>(plane + p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (p + e < HW) plane[p + e] = v[e];
    }
}

// grid: (nparts, B); thread t of block j owns pixels 4 (j kColorChunk/4 + 256 k + t) .. + 3, k = 0 .. kColorChunk/1024 - 1.
// part (B, nparts) float; dpart (B, nparts, 12) double: a thread's pixels in index order, the wave's xor tree, the four waves in order.
template <int KIND, bool BETA, bool VEC>
__global__ __launch_bounds__(256) void color_pixel_kernel(const float* __restrict__ img, const float* __restrict__ target,
                                                          const float* __restrict__ beta, const float* __restrict__ theta,
                                                          float* __restrict__ gout, float* __restrict__ part, double* __restrict__ dpart,
                                                          long HW, float s, float s2, float gscale) {
    __shared__ float sth[kColorSums];
    __shared__ float red[4];
    __shared__ double dred[4][kColorSums];
    const int b = blockIdx.y;
    const Theta th = load_theta(theta + (long)kColorSums * b, sth);
    const float* gp = img + (long)b * 3 * HW;
    const float* xp = target + (long)b * 3 * HW;
    const float* wp = BETA ? beta + (long)b * HW : nullptr;
    float* op = gout + (long)b * 3 * HW;
    float acc = 0.f;
    double ds[kColorSums];
#pragma unroll
    for (int q = 0; q < kColorSums; ++q) ds[q] = 0.0;
    for (int k = 0; k < kColorChunk / 1024; ++k) {
        const long p = 4 * ((long)blockIdx.x * (kColorChunk / 4) + 256 * k + threadIdx.x);
        if (p >= HW) break;
        float G[3][4], X[3][4], Wt[4], out[3][4];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            load4<VEC>(gp + c * HW, p, HW, G[c]);
            load4<VEC>(xp + c * HW, p, HW, X[c]);
        }
        if constexpr (BETA) load4<VEC>(wp, p, HW, Wt);
        float rsum[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (!VEC && p + e >= HW) break;
            float g[3];
            const double Gd[3] = {(double)G[0][e], (double)G[1][e], (double)G[2][e]};
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                float d = (float)(map_row(th, i, Gd[0], Gd[1], Gd[2]) - (double)X[i][e]);
                if constexpr (BETA) d = Wt[e] * d;
                float psi;
                rsum[i] += rho_psi<KIND>(d, s, s2, psi);
                float gs = gscale;
                if constexpr (BETA) gs = gscale * Wt[e];
                g[i] = psi * gs;
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) out[j][e] = fmaf(th.M[2][j], g[2], fmaf(th.M[1][j], g[1], __fmul_rn(th.M[0][j], g[0])));
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double gi = (double)g[i];
#pragma unroll
                for (int j = 0; j < 3; ++j) ds[3 * i + j] += gi * Gd[j];
                ds[9 + i] += gi;
            }
        }
        acc += (rsum[0] + rsum[1]) + rsum[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) store4<VEC>(op + c * HW, p, HW, out[c]);
    }
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) part[(long)b * gridDim.x + blockIdx.x] = acc;
#pragma unroll
    for (int q = 0; q < kColorSums; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) ds[q] += __shfl_xor(ds[q], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < kColorSums; ++q) dred[threadIdx.x >> 6][q] = ds[q];
    }
    __syncthreads();
    if (threadIdx.x < kColorSums)
        dpart[((long)b * gridDim.x + blockIdx.x) * kColorSums + threadIdx.x] =
            ((dred[0][threadIdx.x] + dred[1][threadIdx.x]) + dred[2][threadIdx.x]) + dred[3][threadIdx.x];
}

// grid: (ceil(HW / kApplyChunk), B); out may be src: a thread reads its pixels in all three planes before it writes them
template <bool VEC>
__global__ __launch_bounds__(256) void color_apply_kernel(const float* __restrict__ src, const float* __restrict__ theta, float* out, long HW) {
    __shared__ float sth[kColorSums];
    const int b = blockIdx.y;
    const Theta th = load_theta(theta + (long)kColorSums * b, sth);
    const float* gp = src + (long)b * 3 * HW;
    float* op = out + (long)b * 3 * HW;
    for (int k = 0; k < kApplyChunk / 1024; ++k) {
        const long p = 4 * ((long)blockIdx.x * (kApplyChunk / 4) + 256 * k + threadIdx.x);
        if (p >= HW) break;
        float G[3][4], c[3][4];
#pragma unroll
        for (int i = 0; i < 3; ++i) load4<VEC>(gp + i * HW, p, HW, G[i]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
            for (int i = 0; i < 3; ++i) c[i][e] = (float)map_row(th, i, (double)G[0][e], (double)G[1][e], (double)G[2][e]);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) store4<VEC>(op + i * HW, p, HW, c[i]);
    }
}

// wplus_sched.hip's lr_multiplier: the same expressions, the same bits (as feature_offset.hip, loss_align.hip)
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

// grid: (B), one wave per image.  A lane adds its partials in index order, then the wave's xor tree; lane 0 finishes the 12 numbers:
// g_k = float(sum_k / grad_div) + 2 mu (theta_k - id_k), 0 where bit k of free_mask is clear (theta, m, v of such a number are not
// touched); the table row sum_k (theta_k - id_k)^2 before the update; Adam with feature_step_kernel's roundings, t = t_dev[0] + 1, the
// counter left alone.
__global__ __launch_bounds__(64) void color_step_kernel(const double* __restrict__ dpart, int nparts, float* __restrict__ theta,
                                                        float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int free_mask,
                                                        float lr, float beta1, float beta2, float eps, const int* __restrict__ t_dev,
                                                        int total_steps, float rampup, float rampdown, float grad_div, float color_reg,
                                                        float* __restrict__ table, int nrows) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double s[kColorSums];
#pragma unroll
    for (int q = 0; q < kColorSums; ++q) s[q] = 0.0;
    for (int j = lane; j < nparts; j += 64) {
#pragma unroll
        for (int q = 0; q < kColorSums; ++q) s[q] += dpart[((long)b * nparts + j) * kColorSums + q];
    }
#pragma unroll
    for (int q = 0; q < kColorSums; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[q] += __shfl_xor(s[q], o, 64);
    }
    if (lane != 0) return;
    const int t = t_dev[0] + 1;
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    const float step_size = (float)((double)lr * lr_multiplier(t - 1, total_steps, rampup, rampdown) / bc1);
    const float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    const float coef = 2.f * color_reg;
    double r2 = 0.0;
#pragma unroll
    for (int k = 0; k < kColorSums; ++k) {
        const long o = (long)kColorSums * b + k;
        const float th0 = theta[o];
        const float off = th0 - ((k == 0 || k == 4 || k == 8) ? 1.f : 0.f);
        r2 += (double)off * (double)off;
        if (!((free_mask >> k) & 1)) {
            g[o] = 0.f;
            continue;
        }
        float gi = (float)(s[k] / (double)grad_div);
        if (coef != 0.f) gi = fmaf(coef, off, gi);
        g[o] = gi;
        const float mi = fmaf(gi - m[o], 1.f - beta1, m[o]);
        const float vi = fmaf(gi, __fmul_rn(1.f - beta2, gi), __fmul_rn(v[o], beta2));
        m[o] = mi;
        v[o] = vi;
        theta[o] = fmaf(-step_size, mi / fmaf(sqrtf(vi), inv_bc2_sqrt, eps), th0);
    }
    if (table) table[loss_row(t_dev, nrows, gridDim.x) + b] = (float)r2;
}

bool kind_ok(int kind) {
    return kind == kSquare || kind == OODGAN_ROBUST_CHARBONNIER || kind == OODGAN_ROBUST_HUBER || kind == OODGAN_ROBUST_GEMAN_MCCLURE;
}
// the robust entries' rule: s*s is a normal, finite float32
bool scale_ok(float scale) { return scale > 0.f && std::isnormal(scale * scale); }
bool shape_ok(int B, int H, int W) { return B > 0 && B <= 65535 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768; }
bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

template <int KIND, bool BETA>
void launch_form(bool vec, dim3 grid, void* stream, const float* img, const float* target, const float* beta, const float* theta, float* gimg,
                 float* part, double* dpart, long HW, float s, float s2, float gscale) {
    if (vec)
        hipLaunchKernelGGL((color_pixel_kernel<KIND, BETA, true>), grid, dim3(256), 0, as_stream(stream), img, target, beta, theta, gimg, part,
                           dpart, HW, s, s2, gscale);
    else
        hipLaunchKernelGGL((color_pixel_kernel<KIND, BETA, false>), grid, dim3(256), 0, as_stream(stream), img, target, beta, theta, gimg, part,
                           dpart, HW, s, s2, gscale);
}

template <int KIND>
void launch_kind(bool vec, dim3 grid, void* stream, const float* img, const float* target, const float* beta, const float* theta, float* gimg,
                 float* part, double* dpart, long HW, float s, float s2, float gscale) {
    if (beta) launch_form<KIND, true>(vec, grid, stream, img, target, beta, theta, gimg, part, dpart, HW, s, s2, gscale);
    else launch_form<KIND, false>(vec, grid, stream, img, target, beta, theta, gimg, part, dpart, HW, s, s2, gscale);
}

// Both entry points of the term end here: every argument checked (a status, nothing launched), the kernel of the kind in its form, then
// the mean over the loss partials.  loss / row_dev / nrows: the sink as in loss_pixel.hip's pixel_term.
int color_pixel_term(const char* what, const float* img, const float* target, const float* beta, const float* theta, float* gimg, float* part,
                     double* dpart, float* loss, const int* row_dev, int nrows, int B, int H, int W, int kind, float scale, float grad_mul,
                     void* stream) {
    OODGAN_REQUIRE(img && target && theta && gimg && part && dpart && loss, "%s: bad args (null pointer)", what);
    OODGAN_REQUIRE(shape_ok(B, H, W), "%s: bad shape (%d, 3, %d, %d): B in [1, 65535], H and W in [1, 32768]", what, B, H, W);
    OODGAN_REQUIRE(kind_ok(kind), "%s: unknown kind %d", what, kind);
    OODGAN_REQUIRE(kind == kSquare || scale_ok(scale), "%s: scale %g: must be finite and > 0, with a normal float32 square", what, (double)scale);
    OODGAN_REQUIRE(grad_mul == grad_mul, "%s: grad_mul is NaN", what);
    const long HW = (long)H * W, CHW = 3 * HW;
    const int nparts = oodgan_color_nparts(H, W);
    const bool vec = (HW & 3) == 0 && aligned16(img) && aligned16(target) && aligned16(beta) && aligned16(gimg);
    const float s2 = scale * scale;
    const float gscale = kind == kSquare ? grad_mul * 2.0f / (float)CHW : grad_mul / (float)CHW;
    const dim3 grid(nparts, B);
    count_dispatch(OODGAN_DC_COLOR);
    if (kind == kSquare) launch_kind<kSquare>(vec, grid, stream, img, target, beta, theta, gimg, part, dpart, HW, scale, s2, gscale);
    else if (kind == OODGAN_ROBUST_CHARBONNIER)
        launch_kind<OODGAN_ROBUST_CHARBONNIER>(vec, grid, stream, img, target, beta, theta, gimg, part, dpart, HW, scale, s2, gscale);
    else if (kind == OODGAN_ROBUST_HUBER)
        launch_kind<OODGAN_ROBUST_HUBER>(vec, grid, stream, img, target, beta, theta, gimg, part, dpart, HW, scale, s2, gscale);
    else
        launch_kind<OODGAN_ROBUST_GEMAN_MCCLURE>(vec, grid, stream, img, target, beta, theta, gimg, part, dpart, HW, scale, s2, gscale);
    int rc = check_launch(what);
    if (rc != OODGAN_OK) return rc;
    hipLaunchKernelGGL(mean_finish_kernel<>, dim3(B), dim3(64), 0, as_stream(stream), (const float*)part, loss, nparts, 1.0f / (float)CHW,
                       row_dev, nrows);
    return check_launch((std::string(what) + "_finish").c_str());
}

}  // namespace

// partial sums per image of the colour term: `part` is (B, nparts) floats, `dpart` (B, nparts, 12) doubles; 0: H or W outside [1, 32768]
extern "C" int oodgan_color_nparts(int H, int W) {
    if (H < 1 || W < 1 || H > 32768 || W > 32768) return 0;
    return (int)(((long)H * W + kColorChunk - 1) / kColorChunk);
}

extern "C" int oodgan_color_pixel_loss_fwd_bwd(const float* img, const float* target, const float* beta, const float* theta, float* gimg,
                                               float* part, double* dpart, float* loss, int B, int H, int W, int kind, float scale,
                                               float grad_mul, void* stream) {
    return color_pixel_term("color_pixel_loss", img, target, beta, theta, gimg, part, dpart, loss, nullptr, 1, B, H, W, kind, scale, grad_mul,
                            stream);
}

extern "C" int oodgan_color_pixel_loss_fwd_bwd_row(const float* img, const float* target, const float* beta, const float* theta, float* gimg,
                                                   float* part, double* dpart, float* loss_table, const int* row_dev, int nrows, int B, int H,
                                                   int W, int kind, float scale, float grad_mul, void* stream) {
    OODGAN_REQUIRE(row_dev && nrows > 0, "color_pixel_loss_row: bad args (no row counter, or nrows = %d)", nrows);
    return color_pixel_term("color_pixel_loss_row", img, target, beta, theta, gimg, part, dpart, loss_table, row_dev, nrows, B, H, W, kind, scale,
                            grad_mul, stream);
}

extern "C" int oodgan_color_step(float* theta, float* g, float* m, float* v, const double* dpart, int B, int nparts, int free_mask, float lr,
                                 float beta1, float beta2, float eps, const int* t_dev, int total_steps, float rampup, float rampdown,
                                 float grad_div, float color_reg, float* reg_table, int nrows, void* stream) {
    OODGAN_REQUIRE(theta && g && m && v && dpart && t_dev, "color_step: bad args (null pointer)");
    OODGAN_REQUIRE(B > 0 && B <= 65535 && nparts > 0, "color_step: B = %d images of %d partial sums", B, nparts);
    OODGAN_REQUIRE(free_mask >= 0 && free_mask < (1 << kColorSums), "color_step: free_mask 0x%x has bits above the 12 numbers", free_mask);
    OODGAN_REQUIRE(lr >= 0.f && total_steps > 0 && grad_div > 0.f && color_reg >= 0.f && (reg_table == nullptr || nrows > 0),
                   "color_step: lr = %g, total_steps = %d, grad_div = %g, color_reg = %g, nrows = %d", (double)lr, total_steps,
                   (double)grad_div, (double)color_reg, nrows);
    count_dispatch(OODGAN_DC_COLOR);
    hipLaunchKernelGGL(color_step_kernel, dim3(B), dim3(64), 0, as_stream(stream), dpart, nparts, theta, g, m, v, free_mask, lr, beta1, beta2,
                       eps, t_dev, total_steps, rampup, rampdown, grad_div, color_reg, reg_table, nrows);
    return check_launch("color_step");
}

extern "C" int oodgan_color_apply(const float* src, const float* theta, float* out, int B, int H, int W, void* stream) {
    OODGAN_REQUIRE(src && theta && out, "color_apply: bad args (null pointer)");
    OODGAN_REQUIRE(shape_ok(B, H, W), "color_apply: bad shape (%d, 3, %d, %d): B in [1, 65535], H and W in [1, 32768]", B, H, W);
    const long HW = (long)H * W;
    const bool vec = (HW & 3) == 0 && aligned16(src) && aligned16(out);
    const dim3 grid((unsigned)((HW + kApplyChunk - 1) / kApplyChunk), B);
    count_dispatch(OODGAN_DC_COLOR);
    if (vec) hipLaunchKernelGGL(color_apply_kernel<true>, grid, dim3(256), 0, as_stream(stream), src, theta, out, HW);
    else hipLaunchKernelGGL(color_apply_kernel<false>, grid, dim3(256), 0, as_stream(stream), src, theta, out, HW);
    return check_launch("color_apply");
}
