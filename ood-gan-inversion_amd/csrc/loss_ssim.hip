// SSIM term of the W+ loss: loss[b] = 1 - SSIM_b, SSIM as BasicSR's calculate_ssim computes it on float images (11-tap
// Gaussian window, sigma 1.5, valid region only, c1 = (0.01*255)^2, c2 = (0.03*255)^2, mean over channels and window positions), for
// v = 127.5*(G+1), y = 127.5*(x+1), and its gradient w.r.t. G ACCUMULATED into the buffer the MSE kernel wrote.
// Arithmetic on the [-1,1] data: variances are shift-invariant, the luminance factor uses mu+1, c1 and c2 are divided by 127.5^2 —
// the same value as the 255-scale formula, without its 65025-scale cancellation in E[v^2] - mu^2.
// One fused kernel per step: a block owns a 32x32 pixel tile of one (image, channel) plane and
//   0. stages G and x on the tile + 10 pixels on every side (52x52; zero outside the image) in LDS;
//   H. filters the moments a, b, a^2+b^2, ab along x for the 42 window columns that touch the tile (window q covers pixels q..q+10);
//   V. filters them along y, forms S and the three per-window derivative maps dS/dmu_a, dS/dE[a^2], dS/dE[ab] on 42x42 windows, zero
//      outside the valid (H-10)x(W-10) region, and sums S over the 32x32 windows the tile owns (q = pixel);
//   FH/FV. gather form of the backward: correlates the three maps with the window (x, then y) at the tile's 32x32 pixels and
//      combines them with a_p, b_p: dS_sum/da_p = F1 + 2 a_p F2 + b_p F3.  No scatter, no atomics: gimg is read-modified-written by
//      the one thread that owns the pixel.
// The forward-only mode (gimg NULL) is the same kernel without FH/FV, so its value is the fwd+bwd value bit for bit.  Sums: one
// partial per block (block_sum_256), then one wave per image over the partials in float64 — deterministic, no float atomics.
// Bytes per image at 1024²: G and x read (25 MB, the halo comes from L2), gimg read + written (25 MB).
#include "loss_common.hpp"

#include <cmath>

using namespace oodgan;

namespace {

constexpr int kT = 32;                  // pixel tile
constexpr int kR = 10;                  // window size - 1
constexpr int kQ = kT + kR;             // 42 window positions per axis touch the tile
constexpr int kIn = kQ + kR;            // 52 staged pixels per axis
constexpr int kInS = kIn + 1;           // LDS row strides: odd, so that lanes walking down a column hit distinct banks
constexpr int kQS = kQ + 1;
constexpr int kTS = kT + 1;
constexpr int kRun = 6;                 // outputs per thread along the filtered axis in H (16 LDS reads for 6 outputs); 42 = 7*6
constexpr int kRunV = 7;                // ... in V: 6 runs x 42 columns = 252 items, one trip of the block through the divisions
constexpr int kRunF = 4;                // ... in FH and FV (14 reads for 4); 32 = 8*4
constexpr int kNM = 4;                  // filtered moments
static_assert(kQ % kRun == 0 && kQ % kRunV == 0 && kT % kRunF == 0, "runs tile the axes");
static_assert(3 * kQ * kTS <= kNM * kIn * kQS, "the FH rows alias the H rows");

struct SsimTaps {
    float w[11];
};

// acc[o] = sum_t w[t] * in[o + t]
template <int RUN>
__device__ __forceinline__ void corr_run(const float (&in)[RUN + kR], const SsimTaps& g, float (&acc)[RUN]) {
#pragma unroll
    for (int o = 0; o < RUN; ++o) {
        float s = 0.f;
#pragma unroll
        for (int t = 0; t <= kR; ++t) s = fmaf(g.w[t], in[o + t], s);
        acc[o] = s;
    }
}

// grid: (tiles_x, tiles_y, B*C); part: one float per block, image-major
__global__ __launch_bounds__(256, 2) void ssim_fused_kernel(const float* __restrict__ img, const float* __restrict__ target,
                                                            float* __restrict__ gimg, float* __restrict__ part, int H, int W,
                                                            float c1, float c2, float coef, SsimTaps g) {
    __shared__ float sa[kIn * kInS], sb[kIn * kInS];
    __shared__ float hm[kNM * kIn * kQS];           // H: [moment][staged row][window column]; later FH: [map][window row][pixel column]
    __shared__ float sd[3 * kQ * kQS];              // [map][window row][window column]
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const long plane = (long)blockIdx.z * H * W;
    const int py0 = blockIdx.y * kT, px0 = blockIdx.x * kT;
    const int y0 = py0 - kR, x0 = px0 - kR;         // first staged pixel = first window position

    for (int i = tid; i < kIn * kIn; i += 256) {
        const int r = i / kIn, c = i - r * kIn;
        const int gy = y0 + r, gx = x0 + c;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        const long k = plane + (long)(in ? gy : 0) * W + (in ? gx : 0);
        const float a = img[k], b = target[k];
        sa[r * kInS + c] = in ? a : 0.f;
        sb[r * kInS + c] = in ? b : 0.f;
    }
    __syncthreads();

    // H: lanes walk down the staged rows
    for (int it = tid; it < kIn * (kQ / kRun); it += 256) {
        const int grp = it / kIn, r = it - grp * kIn;
        float a[kRun + kR], b[kRun + kR], m[kRun + kR], acc[kRun];
#pragma unroll
        for (int j = 0; j < kRun + kR; ++j) {
            a[j] = sa[r * kInS + grp * kRun + j];
            b[j] = sb[r * kInS + grp * kRun + j];
        }
        float* out = hm + r * kQS + grp * kRun;
        corr_run<kRun>(a, g, acc);
#pragma unroll
        for (int o = 0; o < kRun; ++o) out[o] = acc[o];
        corr_run<kRun>(b, g, acc);
#pragma unroll
        for (int o = 0; o < kRun; ++o) out[kIn * kQS + o] = acc[o];
#pragma unroll
        for (int j = 0; j < kRun + kR; ++j) m[j] = fmaf(a[j], a[j], b[j] * b[j]);
        corr_run<kRun>(m, g, acc);
#pragma unroll
        for (int o = 0; o < kRun; ++o) out[2 * kIn * kQS + o] = acc[o];
#pragma unroll
        for (int j = 0; j < kRun + kR; ++j) m[j] = a[j] * b[j];
        corr_run<kRun>(m, g, acc);
#pragma unroll
        for (int o = 0; o < kRun; ++o) out[3 * kIn * kQS + o] = acc[o];
    }
    __syncthreads();

    // V: lanes walk along the window columns; S and the derivative maps
    float ssum = 0.f;
    for (int it = tid; it < kQ * (kQ / kRunV); it += 256) {
        const int grp = it / kQ, i = it - grp * kQ;
        float mom[kNM][kRunV];
#pragma unroll
        for (int k = 0; k < kNM; ++k) {
            float v[kRunV + kR];
#pragma unroll
            for (int j = 0; j < kRunV + kR; ++j) v[j] = hm[k * kIn * kQS + (grp * kRunV + j) * kQS + i];
            corr_run<kRunV>(v, g, mom[k]);
        }
        const int qx = x0 + i;
#pragma unroll
        for (int o = 0; o < kRunV; ++o) {
            const int i2 = grp * kRunV + o, qy = y0 + i2;
            const bool valid = qy >= 0 && qy <= H - 11 && qx >= 0 && qx <= W - 11;
            const float mua = mom[0][o], mub = mom[1][o];
            const float ma = mua + 1.f, mb = mub + 1.f;
            const float A1 = fmaf(2.f * ma, mb, c1), B1 = fmaf(ma, ma, fmaf(mb, mb, c1));
            const float A2 = fmaf(2.f, mom[3][o] - mua * mub, c2);
            const float B2 = (mom[2][o] - fmaf(mua, mua, mub * mub)) + c2;
            const float r1 = 1.f / B1, r2 = 1.f / B2, inv = r1 * r2;       // B1 >= c1, B2 >= c2 up to rounding: two divisions per window
            const float S = A1 * A2 * inv;
            const float d1 = 2.f * (mb * A2 - mub * A1) * inv - 2.f * S * (ma * r1 - mua * r2);
            const float d2 = -S * r2;
            const float d3 = 2.f * A1 * inv;
            sd[i2 * kQS + i] = valid ? d1 : 0.f;
            sd[kQ * kQS + i2 * kQS + i] = valid ? d2 : 0.f;
            sd[2 * kQ * kQS + i2 * kQS + i] = valid ? d3 : 0.f;
            if (valid && i2 >= kR && i >= kR) ssum += S;
        }
    }
    ssum = block_sum_256(ssum, red);       // (its barriers also close the reads of hm and the writes of sd)
    if (tid == 0) part[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = ssum;
    if (!gimg) return;

    // FH: F(p) = sum_q w(p - q) D(q), q = p-10..p: in tile coordinates the same correlation (the window is symmetric)
    float* fh = hm;
    for (int it = tid; it < 3 * kQ * (kT / kRunF); it += 256) {
        const int row = it % kQ, rest = it / kQ;
        const int grp = rest % (kT / kRunF), k = rest / (kT / kRunF);
        float v[kRunF + kR], acc[kRunF];
#pragma unroll
        for (int j = 0; j < kRunF + kR; ++j) v[j] = sd[k * kQ * kQS + row * kQS + grp * kRunF + j];
        corr_run<kRunF>(v, g, acc);
#pragma unroll
        for (int o = 0; o < kRunF; ++o) fh[k * kQ * kTS + row * kTS + grp * kRunF + o] = acc[o];
    }
    __syncthreads();

    // FV and the combination with a_p, b_p: one thread per pixel column and run of four rows
    {
        const int px = tid % kT, grp = tid / kT;
        float f[3][kRunF];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float v[kRunF + kR];
#pragma unroll
            for (int j = 0; j < kRunF + kR; ++j) v[j] = fh[k * kQ * kTS + (grp * kRunF + j) * kTS + px];
            corr_run<kRunF>(v, g, f[k]);
        }
        const int gx = px0 + px;
#pragma unroll
        for (int o = 0; o < kRunF; ++o) {
            const int py = grp * kRunF + o, gy = py0 + py;
            if (gy < H && gx < W) {
                const float a = sa[(py + kR) * kInS + px + kR], b = sb[(py + kR) * kInS + px + kR];
                const long k = plane + (long)gy * W + gx;
                gimg[k] = fmaf(coef, fmaf(2.f * a, f[1][o], fmaf(b, f[2][o], f[0][o])), gimg[k]);
            }
        }
    }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// loss[row + b] = 1 - (sum of the image's partials) / n, the sum in float64; the row: loss_row
__global__ __launch_bounds__(64) void ssim_finish_kernel(const float* __restrict__ part, float* __restrict__ loss, int nparts, double inv_n,
                                                         const int* __restrict__ row_dev, int nrows) {
    const int b = blockIdx.x, lane = threadIdx.x;
    double s = 0.0;
    for (int j = lane; j < nparts; j += 64) s += (double)part[(long)b * nparts + j];
    s = wave_sum_f64(s);
    const long row = loss_row(row_dev, nrows, gridDim.x);
    if (lane == 0) loss[row + b] = (float)(1.0 - s * inv_n);
}

int ssim_loss(const float* img, const float* target, float* gimg, float* part, float* loss, const int* row_dev, int nrows, int B, int C,
              int H, int W, float grad_mul, void* stream) {
    OODGAN_REQUIRE(H >= 11 && W >= 11, "ssim_loss: the 11x11 window needs H, W >= 11 (got %dx%d)", H, W);
    OODGAN_REQUIRE((long)B * C <= 65535 && (long)H * W < (1L << 31), "ssim_loss: B*C = %ld planes of %dx%d: too large", (long)B * C, H, W);
    static const SsimTaps taps = [] {           // imgio._gauss_window: float64 taps, normalised, rounded once
        double w[11], sum = 0.0;
        for (int i = 0; i < 11; ++i) sum += w[i] = std::exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        SsimTaps t;
        for (int i = 0; i < 11; ++i) t.w[i] = (float)(w[i] / sum);
        return t;
    }();
    const int tx = (W + kT - 1) / kT, ty = (H + kT - 1) / kT;
    const double n = (double)C * (H - 10) * (W - 10);
    const float c1 = (float)((0.01 * 255) * (0.01 * 255) / (127.5 * 127.5)), c2 = (float)((0.03 * 255) * (0.03 * 255) / (127.5 * 127.5));
    count_dispatch(OODGAN_DC_SSIM);
    hipLaunchKernelGGL(ssim_fused_kernel, dim3(tx, ty, B * C), dim3(256), 0, as_stream(stream), img, target, gimg, part, H, W, c1, c2,
                       (float)(-(double)grad_mul / n), taps);
    int rc = check_launch("ssim_fused");
    if (rc != OODGAN_OK) return rc;
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(B), dim3(64), 0, as_stream(stream), part, loss, C * ty * tx, 1.0 / n, row_dev, nrows);
    return check_launch("ssim_finish");
}

}  // namespace

extern "C" int oodgan_ssim_nparts(int C, int H, int W) {
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    return C * ((H + kT - 1) / kT) * ((W + kT - 1) / kT);
}

extern "C" int oodgan_ssim_loss_fwd_bwd(const float* img, const float* target, float* gimg, float* part, float* loss, int B, int C, int H,
                                        int W, float grad_mul, void* stream) {
    OODGAN_REQUIRE(img && target && part && loss && B > 0 && C > 0, "ssim_loss: bad args");
    return ssim_loss(img, target, gimg, part, loss, nullptr, 1, B, C, H, W, grad_mul, stream);
}

extern "C" int oodgan_ssim_loss_fwd_bwd_row(const float* img, const float* target, float* gimg, float* part, float* loss_table,
                                            const int* row_dev, int nrows, int B, int C, int H, int W, float grad_mul, void* stream) {
    OODGAN_REQUIRE(img && target && part && loss_table && row_dev && nrows > 0 && B > 0 && C > 0, "ssim_loss_row: bad args");
    return ssim_loss(img, target, gimg, part, loss_table, row_dev, nrows, B, C, H, W, grad_mul, stream);
}
