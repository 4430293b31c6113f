// The uint8 side of the command-line tool (oodgan/imgio.py): what the harness did per image on the host — file bytes -> network
// input, network output -> file bytes, PSNR / SSIM of two uint8 images — as kernels on the current stream.
//   u8_to_input    uint8 (B,H,W,3) BGR -> fp32 (B,3,H,W) RGB through a 256-entry table the caller computed with the host's own expression:
//                  no arithmetic here, so the result is the host's bit for bit.
//   tensor2img_u8  fp32 (B,C,H,W) -> uint8 (B,H,W,C): imgio.tensor2img operation for operation in float32 (clamp, subtract, divide, x255,
//                  round half to even), compiled with contraction off: an fma of the division's result and 255 would round once, not twice.
//   psnr_ssim_u8   BasicSR calculate_psnr / calculate_ssim (test_y_channel=False) up to the closing formulas: per image the exact integer sum
//                  of squared differences over the cropped region, per (image, channel) the float64 sum of the SSIM map over its valid region.
// No state, no float atomics: one partial per block, summed by a finish kernel in a fixed order.
#include "common.hpp"

#include <cmath>
#include <cstdint>

using namespace oodgan;

namespace {

// ---------------------------------------------------------------------------------------------------------------- u8 -> input
// VEC: four pixels (12 bytes, three aligned dwords) per thread and a float4 per plane; needs H*W % 4 == 0.  grid-stride over B*H*W / (VEC ? 4 : 1)
template <bool VEC>
__global__ __launch_bounds__(256) void u8_to_input_kernel(const unsigned char* __restrict__ in, const float* __restrict__ lut,
                                                          float* __restrict__ out, long HW, long items) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < items; i += (long)gridDim.x * 256) {
        if constexpr (VEC) {
            const long pix = i * 4, b = pix / HW, p = pix - b * HW;
            const unsigned* src = reinterpret_cast<const unsigned*>(in + pix * 3);
            const unsigned w0 = src[0], w1 = src[1], w2 = src[2];
            unsigned char v[12];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                v[k] = (w0 >> (8 * k)) & 255u;
                v[4 + k] = (w1 >> (8 * k)) & 255u;
                v[8 + k] = (w2 >> (8 * k)) & 255u;
            }
            float* dst = out + b * 3 * HW + p;
#pragma unroll
            for (int c = 0; c < 3; ++c)          // output channel c (RGB) is input channel 2 - c (BGR)
                *reinterpret_cast<float4*>(dst + c * HW) = make_float4(lut[v[2 - c]], lut[v[5 - c]], lut[v[8 - c]], lut[v[11 - c]]);
        } else {
            const long b = i / HW, p = i - b * HW;
            const unsigned char* src = in + i * 3;
            float* dst = out + b * 3 * HW + p;
            dst[0] = lut[src[2]];
            dst[HW] = lut[src[1]];
            dst[2 * HW] = lut[src[0]];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- tensor -> u8
__device__ __forceinline__ unsigned to_u8(float t, float lo, float hi, float w) {
#pragma clang fp contract(off)
    float v = fminf(fmaxf(t, lo), hi);
    v = (v - lo) / w;                       // IEEE float32 subtraction and division, as torch's CPU kernels
    return (unsigned)(int)rintf(v * 255.0f) & 255u;
}

// The output is one flat array of B*H*W*C bytes; a thread owns four consecutive ones (one dword store; image b starts at b*H*W*C, a
// multiple of four or not, so a dword may span two pixels, rows or images) and the last thread the 1-3 bytes of the tail.  (b, p, ch) of the
// first byte come from divisions, the next three by stepping.
template <int C>
__global__ __launch_bounds__(256) void tensor2img_u8_kernel(const float* __restrict__ in, unsigned char* __restrict__ out, long HW, long total,
                                                            int reverse, float lo, float hi, float w) {
    const long ngroups = (total + 3) >> 2;
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g < ngroups; g += (long)gridDim.x * 256) {
        const long j0 = g * 4;
        long pix = j0 / C;
        int ch = (int)(j0 - pix * C);
        long b = pix / HW, p = pix - b * HW;
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (j0 + k < total) word |= to_u8(in[(b * C + (reverse ? C - 1 - ch : ch)) * HW + p], lo, hi, w) << (8 * k);
            if (++ch == C) {
                ch = 0;
                if (++p == HW) {
                    p = 0;
                    ++b;
                }
            }
        }
        if (j0 + 4 <= total) {
            *reinterpret_cast<unsigned*>(out + j0) = word;
        } else {
            for (int k = 0; j0 + k < total; ++k) out[j0 + k] = (unsigned char)(word >> (8 * k));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- PSNR / SSIM
constexpr int kTW = 32, kTH = 16;       // window positions (= SSIM map entries) per block
constexpr int kR = 10;                  // window size - 1
constexpr int kInW = kTW + kR, kInH = kTH + kR;        // 42 x 26 staged pixels
constexpr int kNM = 5;                  // windowed moments: a, b, a^2, b^2, ab

struct GaussTaps {
    double w[11];
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// grid: (tiles_x, tiles_y, B*C).  The block at (bx, by) owns the map entries [by*16, +16) x [bx*32, +32) of plane (b, ch) of the CROPPED
// images (Hc x Wc = (H-2c) x (W-2c), map (Hc-10) x (Wc-10)) and, for the squared error, the pixels of the same rectangle; the last tile of
// an axis also owns what lies beyond it (the 10 pixels no map entry starts at).  Every pixel value is an integer <= 255: a block's squared
// error is < 2^31 (26*42*255^2 = 7.1e7).
__global__ __launch_bounds__(256) void psnr_ssim_u8_kernel(const unsigned char* __restrict__ A, const unsigned char* __restrict__ Bm,
                                                           long long* __restrict__ part_sse, double* __restrict__ part_ssim, int C, int H,
                                                           int W, int crop, GaussTaps g) {
    __shared__ float sa[kInH * kInW], sb[kInH * kInW];
    __shared__ double hm[kNM * kInH * kTW];         // [moment][staged row][map column]
    __shared__ double redd[4];
    __shared__ int redi[4];
    const int tid = threadIdx.x;
    const int Hc = H - 2 * crop, Wc = W - 2 * crop;
    const int b = blockIdx.z / C, ch = blockIdx.z - b * C;
    const int y0 = blockIdx.y * kTH, x0 = blockIdx.x * kTW;
    const bool last_y = blockIdx.y == gridDim.y - 1, last_x = blockIdx.x == gridDim.x - 1;
    const long base = (long)b * H * W * C + ch;

    int sse = 0;
    for (int i = tid; i < kInH * kInW; i += 256) {
        const int r = i / kInW, c = i - r * kInW;
        const int gy = y0 + r, gx = x0 + c;
        const bool in = gy < Hc && gx < Wc;
        const long k = base + ((long)((in ? gy : 0) + crop) * W + (in ? gx : 0) + crop) * C;
        const int a = in ? A[k] : 0, bb = in ? Bm[k] : 0;
        sa[i] = (float)a;
        sb[i] = (float)bb;
        if ((r < kTH || last_y) && (c < kTW || last_x)) sse += (a - bb) * (a - bb);
    }
    __syncthreads();

    // along x: the five moments at (staged row r, map column c)
    for (int it = tid; it < kInH * kTW; it += 256) {
        const int r = it / kTW, c = it - r * kTW;
        double m[kNM] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t <= kR; ++t) {
            const double a = (double)sa[r * kInW + c + t], bb = (double)sb[r * kInW + c + t], w = g.w[t];
            m[0] = fma(w, a, m[0]);
            m[1] = fma(w, bb, m[1]);
            m[2] = fma(w, a * a, m[2]);          // products of integers <= 255: exact
            m[3] = fma(w, bb * bb, m[3]);
            m[4] = fma(w, a * bb, m[4]);
        }
#pragma unroll
        for (int k = 0; k < kNM; ++k) hm[(k * kInH + r) * kTW + c] = m[k];
    }
    __syncthreads();

    // along y, then the map
    const double c1 = (0.01 * 255) * (0.01 * 255), c2 = (0.03 * 255) * (0.03 * 255);
    double ssum = 0.0;
    for (int it = tid; it < kTH * kTW; it += 256) {
        const int r = it / kTW, c = it - r * kTW;
        double m[kNM] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int t = 0; t <= kR; ++t) {
#pragma unroll
            for (int k = 0; k < kNM; ++k) m[k] = fma(g.w[t], hm[(k * kInH + r + t) * kTW + c], m[k]);
        }
        const double mu1 = m[0], mu2 = m[1];
        const double s1 = m[2] - mu1 * mu1, s2 = m[3] - mu2 * mu2, s12 = m[4] - mu1 * mu2;
        const double v = ((2.0 * mu1 * mu2 + c1) * (2.0 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2));
        if (y0 + r < Hc - kR && x0 + c < Wc - kR) ssum += v;
    }

    ssum = wave_sum_f64(ssum);
    sse = wave_sum_i32(sse);
    if ((tid & 63) == 0) {
        redd[tid >> 6] = ssum;
        redi[tid >> 6] = sse;
    }
    __syncthreads();
    if (tid == 0) {
        const long slot = ((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        part_ssim[slot] = (redd[0] + redd[1]) + (redd[2] + redd[3]);
        part_sse[slot] = (long long)redi[0] + redi[1] + redi[2] + redi[3];
    }
}

// grid: (B).  sse[b]: the sum of image b's C*ntiles integer partials; ssim_sum[b, ch]: the sum of that plane's ntiles partials, lane-strided
// then across the wave — one order for a given shape.
__global__ __launch_bounds__(64) void psnr_ssim_finish_kernel(const long long* __restrict__ part_sse, const double* __restrict__ part_ssim,
                                                              long long* __restrict__ sse, double* __restrict__ ssim_sum, int C, int ntiles) {
    const int b = blockIdx.x, lane = threadIdx.x;
    long long s = 0;
    for (int j = lane; j < C * ntiles; j += 64) s += part_sse[(long)b * C * ntiles + j];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) sse[b] = s;
    for (int ch = 0; ch < C; ++ch) {
        double d = 0.0;
        for (int j = lane; j < ntiles; j += 64) d += part_ssim[((long)b * C + ch) * ntiles + j];
        d = wave_sum_f64(d);
        if (lane == 0) ssim_sum[b * C + ch] = d;
    }
}

inline int tiles_of(int n, int t) { return (n + t - 1) / t; }

}  // namespace

extern "C" int oodgan_u8_to_input(const unsigned char* bgr, const float* lut, float* out, int B, int H, int W, void* stream) {
    OODGAN_REQUIRE(bgr && lut && out && B > 0 && H > 0 && W > 0, "u8_to_input: bad args");
    const long HW = (long)H * W, n = (long)B * HW;
    if (HW % 4 == 0 && reinterpret_cast<uintptr_t>(bgr) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0) {
        hipLaunchKernelGGL(u8_to_input_kernel<true>, dim3(stream_grid(n / 4, 256)), dim3(256), 0, as_stream(stream), bgr, lut, out, HW, n / 4);
    } else {
        hipLaunchKernelGGL(u8_to_input_kernel<false>, dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream), bgr, lut, out, HW, n);
    }
    return check_launch("u8_to_input");
}

extern "C" int oodgan_tensor2img_u8(const float* t, unsigned char* out, int B, int C, int H, int W, int rgb2bgr, double vmin, double vmax,
                                    void* stream) {
    OODGAN_REQUIRE(t && out && B > 0 && H > 0 && W > 0, "tensor2img_u8: bad args");
    OODGAN_REQUIRE(reinterpret_cast<uintptr_t>(out) % 4 == 0, "tensor2img_u8: out must be 4-byte aligned");
    OODGAN_REQUIRE(C == 1 || C == 3, "tensor2img_u8: C must be 1 or 3, got %d", C);
    OODGAN_REQUIRE(std::isfinite(vmin) && std::isfinite(vmax) && vmax > vmin, "tensor2img_u8: need finite min < max, got (%g, %g)", vmin, vmax);
    const long HW = (long)H * W, total = (long)B * C * HW;
    const float lo = (float)vmin, hi = (float)vmax, w = (float)(vmax - vmin);
    const int grid = stream_grid((total + 3) / 4, 256);
    if (C == 3) {
        hipLaunchKernelGGL(tensor2img_u8_kernel<3>, dim3(grid), dim3(256), 0, as_stream(stream), t, out, HW, total, rgb2bgr ? 1 : 0, lo, hi, w);
    } else {
        hipLaunchKernelGGL(tensor2img_u8_kernel<1>, dim3(grid), dim3(256), 0, as_stream(stream), t, out, HW, total, 0, lo, hi, w);
    }
    return check_launch("tensor2img_u8");
}

extern "C" int oodgan_psnr_ssim_nparts(int C, int H, int W, int crop_border) {
    if (C <= 0 || crop_border < 0 || H <= 0 || W <= 0) return 0;
    const long Hc = (long)H - 2L * crop_border, Wc = (long)W - 2L * crop_border;
    if (Hc < 11 || Wc < 11) return 0;
    return C * tiles_of((int)Hc - kR, kTH) * tiles_of((int)Wc - kR, kTW);
}

extern "C" int oodgan_psnr_ssim_u8(const unsigned char* a, const unsigned char* b, long long* part_sse, double* part_ssim, long long* sse,
                                   double* ssim_sum, int B, int C, int H, int W, int crop_border, void* stream) {
    OODGAN_REQUIRE(a && b && part_sse && part_ssim && sse && ssim_sum && B > 0 && C > 0 && C <= 4, "psnr_ssim_u8: bad args");
    const int nparts = oodgan_psnr_ssim_nparts(C, H, W, crop_border);
    OODGAN_REQUIRE(nparts > 0, "psnr_ssim_u8: the 11x11 window needs a cropped image of at least 11x11 (got %dx%d, crop_border %d)", H, W,
                   crop_border);
    const int Hc = H - 2 * crop_border, Wc = W - 2 * crop_border;
    const int tx = tiles_of(Wc - kR, kTW), ty = tiles_of(Hc - kR, kTH);
    OODGAN_REQUIRE((long)B * C <= 65535 && ty <= 65535, "psnr_ssim_u8: B*C = %ld planes of %dx%d: too large", (long)B * C, H, W);
    static const GaussTaps taps = [] {          // imgio._gauss_window
        GaussTaps t;
        double sum = 0.0;
        for (int i = 0; i < 11; ++i) sum += t.w[i] = std::exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5));
        for (int i = 0; i < 11; ++i) t.w[i] /= sum;
        return t;
    }();
    hipLaunchKernelGGL(psnr_ssim_u8_kernel, dim3(tx, ty, B * C), dim3(256), 0, as_stream(stream), a, b, part_sse, part_ssim, C, H, W, crop_border,
                       taps);
    int rc = check_launch("psnr_ssim_u8");
    if (rc != OODGAN_OK) return rc;
    hipLaunchKernelGGL(psnr_ssim_finish_kernel, dim3(B), dim3(64), 0, as_stream(stream), part_sse, part_ssim, sse, ssim_sum, C, ty * tx);
    return check_launch("psnr_ssim_finish");
}
