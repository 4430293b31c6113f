// Similarity alignment of the target beside the latents of the W+ loop.  Per image theta = (lambda, phi, tx, ty): the
// target x is resampled to x_theta by a bicubic (Keys, A = -0.75) border-padded warp about the image centre, the pixel term of the step is
// taken against x_theta, and theta takes an Adam step of its own on dL/dtheta = -sum gimg * dx_theta/dtheta.  The TARGET is warped, not the
// generator image: the backward pass, the range scales and every pixel-term kernel stay as they are.
//   oodgan_similarity_warp:  one thread per pixel and image, the C planes in a loop; coalesced stores, the gather reads src
//   oodgan_align_grad_step:  (1) per block of kAlignChunk pixels the six sums  sum P, sum Q, sum P px, sum P py, sum Q px, sum Q py  with
//                            P = sum_c gimg_c dx_theta_c/du, Q = sum_c gimg_c dx_theta_c/dv (the taps gathered AGAIN from src: no derivative
//                            planes in HBM; tau, the weights and every product in double: the derivative weights sum to zero, in fp32 the
//                            16-tap sum would cancel to a few bits), in a fixed order, to the caller's `part`;  (2) one wave per image adds the partials in
//                            double, forms the four derivatives, rounds once, adds the regulariser and takes Adam's step.
// No float atomics, no state: equal inputs give equal bits.  Contraction is off in the whole unit: at theta = 0 the weights are exactly
// (0, 1, 0, 0) and x_theta == x bit for bit, and the fp32 arithmetic is the one the tests' fp32 formula does operation by operation; the
// fused multiply-adds of Adam are written out.
#include "loss_common.hpp"

#pragma clang fp contract(off)

namespace {
using namespace oodgan;

constexpr double kPi = 3.14159265358979323846;
constexpr float kA = -0.75f;                 // Keys' cubic, the constant of torch's and OpenCV's bicubic
constexpr int kAlignChunk = 1024;            // pixels per block of both kernels = pixels per partial sum (oodgan_align_grad_nparts)
constexpr int kAlignSums = 6;

// a - 1 = e^lambda cos(phi) - 1 and s = e^lambda sin(phi), in double from the float32 theta, and the translations in pixels
struct Sim {
    double am1, s, tu, tv;
};

__device__ __forceinline__ Sim sim_of(const float* __restrict__ theta, int H, int W) {
    const double e = exp((double)theta[0]), phi = (double)theta[1];
    Sim r;
    r.am1 = e * cos(phi) - 1.0;
    r.s = e * sin(phi);
    r.tu = (double)theta[2] * (0.5 * (double)W);
    r.tv = (double)theta[3] * (0.5 * (double)H);
    return r;
}

// (A (x+1) - 5A)(x+1) ... : the two pieces of the cubic, at distance x from the sample, and their derivatives in x
// T = float: the warp, as the contract words it; T = double: the gradient, which keeps tau and every product in double
template <typename T>
__device__ __forceinline__ T cubic_near(T x) { return ((T(kA) + T(2)) * x - (T(kA) + T(3))) * x * x + T(1); }                 // |x| <= 1
template <typename T>
__device__ __forceinline__ T cubic_far(T x) { return ((T(kA) * x - T(5) * T(kA)) * x + T(8) * T(kA)) * x - T(4) * T(kA); }     // 1 < |x| < 2
__device__ __forceinline__ double dcubic_near(double x) { return (3.0 * (kA + 2.0) * x - 2.0 * (kA + 3.0)) * x; }
__device__ __forceinline__ double dcubic_far(double x) { return (3.0 * kA * x - 10.0 * kA) * x + 8.0 * kA; }

// One axis of one output pixel: the offset d (double), clamped to [-2 - X, n + 1 - X] (a NaN goes to the lower end: fmax returns its
// other operand), the four clamped tap indices and the weights at tau = d - floor(d) — T = float: tau rounded to float once.
template <typename T>
struct Axis {
    int i[4];
    T w[4];
    T tau;
};

template <typename T>
__device__ __forceinline__ Axis<T> axis_of(double d, int X, int n) {
    d = fmin(fmax(d, (double)(-2 - X)), (double)(n + 1 - X));
    const double fl = floor(d);
    const int i0 = X + (int)fl;
    Axis<T> a;
    a.tau = (T)(d - fl);
#pragma unroll
    for (int k = 0; k < 4; ++k) a.i[k] = min(max(i0 - 1 + k, 0), n - 1);
    a.w[0] = cubic_far<T>(a.tau + T(1));
    a.w[1] = cubic_near<T>(a.tau);
    a.w[2] = cubic_near<T>(T(1) - a.tau);
    a.w[3] = cubic_far<T>(T(2) - a.tau);
    return a;
}

// d w / d tau of the same four taps
__device__ __forceinline__ void axis_deriv(double tau, double* dw) {
    dw[0] = dcubic_far(tau + 1.0);
    dw[1] = dcubic_near(tau);
    dw[2] = -dcubic_near(1.0 - tau);
    dw[3] = -dcubic_far(2.0 - tau);
}

// the two axes of pixel (X, Y)
template <typename T>
__device__ __forceinline__ void axes_of(const Sim& S, int X, int Y, int H, int W, double& px, double& py, Axis<T>& ax, Axis<T>& ay) {
    px = (double)X - 0.5 * (double)(W - 1);
    py = (double)Y - 0.5 * (double)(H - 1);
    const double du = (S.am1 * px - (S.s * ((double)W / (double)H)) * py) + S.tu;
    const double dv = ((S.s * ((double)H / (double)W)) * px + S.am1 * py) + S.tv;
    ax = axis_of<T>(du, X, W);
    ay = axis_of<T>(dv, Y, H);
}

__device__ __forceinline__ float row4(const float* __restrict__ row, const int* i, const float* w) {
    return ((w[0] * row[i[0]] + w[1] * row[i[1]]) + w[2] * row[i[2]]) + w[3] * row[i[3]];
}

// grid: (ceil(HW / kAlignChunk), B); thread t of block j owns pixels j * kAlignChunk + t + 256 k, k = 0..3
__global__ __launch_bounds__(256) void similarity_warp_kernel(const float* __restrict__ src, const float* __restrict__ theta,
                                                              float* __restrict__ out, int C, int H, int W) {
    __shared__ Sim sh;
    const int b = blockIdx.y;
    if (threadIdx.x == 0) sh = sim_of(theta + 4 * b, H, W);
    __syncthreads();
    const Sim S = sh;
    const long HW = (long)H * W;
    const long p0 = (long)blockIdx.x * kAlignChunk + threadIdx.x;
    for (int k = 0; k < kAlignChunk / 256; ++k) {
        const long p = p0 + 256 * k;
        if (p >= HW) break;
        const int Y = (int)(p / W), X = (int)(p - (long)Y * W);
        double px, py;
        Axis<float> ax, ay;
        axes_of<float>(S, X, Y, H, W, px, py, ax, ay);
        for (int c = 0; c < C; ++c) {
            const float* plane = src + ((long)b * C + c) * HW;
            float r[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) r[j] = row4(plane + (long)ay.i[j] * W, ax.i, ax.w);
            out[((long)b * C + c) * HW + p] = ((ay.w[0] * r[0] + ay.w[1] * r[1]) + ay.w[2] * r[2]) + ay.w[3] * r[3];
        }
    }
}

// grid: (nparts, B).  part (B, nparts, 6) double: a thread's pixels in index order, the wave's xor tree, the four waves in order.
__global__ __launch_bounds__(256) void align_grad_kernel(const float* __restrict__ gimg, const float* __restrict__ src,
                                                         const float* __restrict__ theta, double* __restrict__ part, int C, int H, int W) {
    __shared__ Sim sh;
    __shared__ double red[4][kAlignSums];
    const int b = blockIdx.y;
    if (threadIdx.x == 0) sh = sim_of(theta + 4 * b, H, W);
    __syncthreads();
    const Sim S = sh;
    const long HW = (long)H * W;
    const long p0 = (long)blockIdx.x * kAlignChunk + threadIdx.x;
    double acc[kAlignSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < kAlignChunk / 256; ++k) {
        const long p = p0 + 256 * k;
        if (p >= HW) break;
        const int Y = (int)(p / W), X = (int)(p - (long)Y * W);
        double px, py;
        Axis<double> ax, ay;
        axes_of<double>(S, X, Y, H, W, px, py, ax, ay);
        double dwx[4], dwy[4];
        axis_deriv(ax.tau, dwx);
        axis_deriv(ay.tau, dwy);
        double Pd = 0.0, Qd = 0.0;
        for (int c = 0; c < C; ++c) {
            const float* plane = src + ((long)b * C + c) * HW;
            double Dx = 0.0, Dy = 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float* row = plane + (long)ay.i[j] * W;
                const double v0 = (double)row[ax.i[0]], v1 = (double)row[ax.i[1]], v2 = (double)row[ax.i[2]], v3 = (double)row[ax.i[3]];
                Dx += ay.w[j] * (((dwx[0] * v0 + dwx[1] * v1) + dwx[2] * v2) + dwx[3] * v3);
                Dy += dwy[j] * (((ax.w[0] * v0 + ax.w[1] * v1) + ax.w[2] * v2) + ax.w[3] * v3);
            }
            const double gi = (double)gimg[((long)b * C + c) * HW + p];
            Pd += gi * Dx;
            Qd += gi * Dy;
        }
        acc[0] += Pd;
        acc[1] += Qd;
        acc[2] += Pd * px;
        acc[3] += Pd * py;
        acc[4] += Qd * px;
        acc[5] += Qd * py;
    }
#pragma unroll
    for (int q = 0; q < kAlignSums; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[q] += __shfl_xor(acc[q], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < kAlignSums; ++q) red[threadIdx.x >> 6][q] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < kAlignSums)
        part[((long)b * gridDim.x + blockIdx.x) * kAlignSums + threadIdx.x] =
            (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// wplus_sched.hip's lr_multiplier: the same expressions, the same bits (as feature_offset.hip)
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

// grid: (B), one wave per image.  A lane adds its partials in index order, then the wave's xor tree; lane 0 finishes:
//   dL/dlambda = -[a (S_Ppx + S_Qpy) + s (H/W S_Qpx - W/H S_Ppy)],  dL/dphi = -[a (H/W S_Qpx - W/H S_Ppy) - s (S_Ppx + S_Qpy)],
//   dL/dtx = -W/2 S_P,  dL/dty = -H/2 S_Q,  each divided by grad_div in double and rounded once; + 2 mu theta_k; g written; the table row
//   sum_k theta_k^2 (before the update); Adam with feature_step_kernel's roundings, t = t_dev[0] + 1, the counter left alone.
__global__ __launch_bounds__(64) void align_finish_kernel(const double* __restrict__ part, int nparts, float* __restrict__ theta,
                                                          float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int H, int W,
                                                          float lr, float beta1, float beta2, float eps, const int* __restrict__ t_dev,
                                                          int total_steps, float rampup, float rampdown, float grad_div, float align_reg,
                                                          float* __restrict__ table, int nrows) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double s[kAlignSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = lane; j < nparts; j += 64) {
#pragma unroll
        for (int q = 0; q < kAlignSums; ++q) s[q] += part[((long)b * nparts + j) * kAlignSums + q];
    }
#pragma unroll
    for (int q = 0; q < kAlignSums; ++q) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[q] += __shfl_xor(s[q], o, 64);
    }
    if (lane != 0) return;
    float* th = theta + 4 * b;
    const double e = exp((double)th[0]), phi = (double)th[1];
    const double a = e * cos(phi), sn = e * sin(phi);
    const double rad = s[2] + s[5];                                                                   // d/dlambda: the radial field
    const double rot = ((double)H / (double)W) * s[4] - ((double)W / (double)H) * s[3];             // d/dphi at theta = 0: the rotational one
    const double inv = 1.0 / (double)grad_div;
    double gd[4];
    gd[0] = -(a * rad + sn * rot) * inv;
    gd[1] = -(a * rot - sn * rad) * inv;
    gd[2] = -(0.5 * (double)W) * s[0] * inv;
    gd[3] = -(0.5 * (double)H) * s[1] * inv;
    const int t = t_dev[0] + 1;
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    const float step_size = (float)((double)lr * lr_multiplier(t - 1, total_steps, rampup, rampdown) / bc1);
    const float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    const float coef = 2.f * align_reg;
    double r2 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float th0 = th[k];
        r2 += (double)th0 * (double)th0;
        float gi = (float)gd[k];
        if (coef != 0.f) gi = fmaf(coef, th0, gi);
        g[4 * b + k] = gi;
        const float mi = fmaf(gi - m[4 * b + k], 1.f - beta1, m[4 * b + k]);
        const float vi = fmaf(gi, __fmul_rn(1.f - beta2, gi), __fmul_rn(v[4 * b + k], beta2));
        m[4 * b + k] = mi;
        v[4 * b + k] = vi;
        th[k] = fmaf(-step_size, mi / fmaf(sqrtf(vi), inv_bc2_sqrt, eps), th0);
    }
    if (table) table[loss_row(t_dev, nrows, gridDim.x) + b] = (float)r2;
}

int check_image(const char* what, int B, int C, int H, int W) {
    OODGAN_REQUIRE(B > 0 && C > 0 && (long)B * C <= 0x7fffffffL, "%s: B = %d images of C = %d planes", what, B, C);
    OODGAN_REQUIRE(H >= 4 && W >= 4 && H <= 32768 && W <= 32768, "%s: a %dx%d plane: each side must be in [4, 32768]", what, H, W);
    OODGAN_REQUIRE(B <= 65535, "%s: B = %d: too many images for one grid", what, B);
    return OODGAN_OK;
}

}  // namespace

extern "C" int oodgan_similarity_warp(const float* src, const float* theta, float* out, int B, int C, int H, int W, void* stream) {
    OODGAN_REQUIRE(src && theta && out && src != out, "similarity_warp: bad args (null pointer, or out == src: the gather reads src)");
    int rc = check_image("similarity_warp", B, C, H, W);
    if (rc != OODGAN_OK) return rc;
    count_dispatch(OODGAN_DC_ALIGN);
    hipLaunchKernelGGL(similarity_warp_kernel, dim3(oodgan_align_grad_nparts(H, W), B), dim3(256), 0, as_stream(stream), src, theta, out, C, H, W);
    return check_launch("similarity_warp");
}

extern "C" int oodgan_align_grad_nparts(int H, int W) {
    if (H < 4 || W < 4 || H > 32768 || W > 32768) return 0;
    return (int)(((long)H * W + kAlignChunk - 1) / kAlignChunk);
}

extern "C" int oodgan_align_grad_step(const float* gimg, const float* src, float* theta, float* g, float* m, float* v, int B, int C, int H,
                                      int W, float lr, float beta1, float beta2, float eps, const int* t_dev, int total_steps, float rampup,
                                      float rampdown, float grad_div, float align_reg, float* reg_table, int nrows, double* part,
                                      void* stream) {
    OODGAN_REQUIRE(gimg && src && theta && g && m && v && t_dev && part, "align_grad_step: bad args (null pointer)");
    int rc = check_image("align_grad_step", B, C, H, W);
    if (rc != OODGAN_OK) return rc;
    OODGAN_REQUIRE(lr >= 0.f && total_steps > 0 && grad_div > 0.f && align_reg >= 0.f && (reg_table == nullptr || nrows > 0),
                   "align_grad_step: lr = %g, total_steps = %d, grad_div = %g, align_reg = %g, nrows = %d", (double)lr, total_steps,
                   (double)grad_div, (double)align_reg, nrows);
    count_dispatch(OODGAN_DC_ALIGN);
    const int nparts = oodgan_align_grad_nparts(H, W);
    hipLaunchKernelGGL(align_grad_kernel, dim3(nparts, B), dim3(256), 0, as_stream(stream), gimg, src, (const float*)theta, part, C, H, W);
    hipLaunchKernelGGL(align_finish_kernel, dim3(B), dim3(64), 0, as_stream(stream), (const double*)part, nparts, theta, g, m, v, H, W, lr,
                       beta1, beta2, eps, t_dev, total_steps, rampup, rampdown, grad_div, align_reg, reg_table, nrows);
    return check_launch("align_grad_step");
}
