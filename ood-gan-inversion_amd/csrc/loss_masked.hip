// Masked W+ objective ("composite objective"): the loss is evaluated on the composite c = x + beta*(G - x), beta a
// (B,1,HW) plane per image broadcast over the C colour channels.  HBM-bound streaming kernels, like the plain MSE of elementwise.hip:
//   composite MSE: loss[b] = mean_{c,p} d^2, d = beta*(G - x); the gradient w.r.t. c (grad_mul*2/CHW*d) or w.r.t. G (that times beta);
//                  optionally c itself (the LPIPS term reads it);
//   scale_by_plane: g <- beta (.) g (the chain rule from c to G once LPIPS has accumulated into the gradient w.r.t. c);
//   loss_weight_from_alpha: beta = clip(1 - alpha, 0, 1)^n (the composite that `blend` applied n times produces).
// With beta == 1 the loss and the gradient are bit-identical to oodgan_mse_fwd_bwd: the same chunks of kMseChunk elements per block,
// the same float4 order per thread, the same two-stage sums (block_sum_256, then mean_finish_kernel's one wave over the partials); no float atomics.
#include "loss_common.hpp"

using namespace oodgan;

namespace {

// Plane form (HW a multiple of kMseChunk): block j of image b owns pixel chunk j of ALL C channel planes — beta is read once per
// pixel and used for every channel — and keeps one accumulator per channel, so that the partial sum of channel chunk c*HW/kMseChunk + j
// is formed in exactly the order mse_kernel forms it.  grid: (HW / kMseChunk, B).
template <int C>
__global__ __launch_bounds__(256) void composite_mse_plane_kernel(const float* __restrict__ img, const float* __restrict__ target,
                                                                  const float* __restrict__ beta, float* __restrict__ gout,
                                                                  float* __restrict__ comp, float* __restrict__ part, long HW,
                                                                  int nparts, float gscale, int wrt_gen) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const long HW4 = HW >> 2;
    const long base4 = (long)b * C * HW4;
    const long p0 = (long)blockIdx.x * (kMseChunk >> 2);
    const float4* a4 = reinterpret_cast<const float4*>(img) + base4;
    const float4* t4 = reinterpret_cast<const float4*>(target) + base4;
    const float4* b4 = reinterpret_cast<const float4*>(beta) + (long)b * HW4;
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    for (long i = p0 + threadIdx.x; i < p0 + (kMseChunk >> 2); i += 256) {
        const float4 w = b4[i];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const long k = c * HW4 + i;
            const float4 a = a4[k];
            const float4 t = t4[k];
            float4 d = make_float4(w.x * (a.x - t.x), w.y * (a.y - t.y), w.z * (a.z - t.z), w.w * (a.w - t.w));
            acc[c] += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
            if (gout) {
                // gscale * 1 == gscale: with beta == 1 both forms store d * gscale, as mse_kernel does
                const float4 s = wrt_gen ? make_float4(gscale * w.x, gscale * w.y, gscale * w.z, gscale * w.w)
                                         : make_float4(gscale, gscale, gscale, gscale);
                reinterpret_cast<float4*>(gout)[base4 + k] = make_float4(d.x * s.x, d.y * s.y, d.z * s.z, d.w * s.w);
            }
            if (comp) reinterpret_cast<float4*>(comp)[base4 + k] = make_float4(t.x + d.x, t.y + d.y, t.z + d.z, t.w + d.w);
        }
    }
    const int chunks_per_plane = (int)(HW / kMseChunk);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float s = block_sum_256(acc[c], red);
        if (threadIdx.x == 0) part[(long)b * nparts + c * chunks_per_plane + blockIdx.x] = s;
    }
}

// Flat form (any C, HW): mse_kernel's walk over the image's C*HW elements, beta looked up per element (its C planes hit the same
// cache lines).  grid: (nparts, B).
__global__ __launch_bounds__(256) void composite_mse_flat_kernel(const float* __restrict__ img, const float* __restrict__ target,
                                                                 const float* __restrict__ beta, float* __restrict__ gout,
                                                                 float* __restrict__ comp, float* __restrict__ part, long HW, long CHW,
                                                                 int nparts, float gscale, int wrt_gen) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const long base = (long)b * CHW;
    const float* bp = beta + (long)b * HW;
    const long p0 = (long)blockIdx.x * kMseChunk;
    const long p1 = p0 + kMseChunk < CHW ? p0 + kMseChunk : CHW;
    float acc = 0.f;
    if ((HW & 3) == 0) {            // HW % 4 == 0: a float4 of one channel plane; beta as a float4 of the same pixels
        const long HW4 = HW >> 2;
        for (long i = (p0 >> 2) + threadIdx.x; i < (p1 >> 2); i += 256) {
            const float4 a = reinterpret_cast<const float4*>(img + base)[i];
            const float4 t = reinterpret_cast<const float4*>(target + base)[i];
            const float4 w = reinterpret_cast<const float4*>(bp)[i % HW4];
            float4 d = make_float4(w.x * (a.x - t.x), w.y * (a.y - t.y), w.z * (a.z - t.z), w.w * (a.w - t.w));
            acc += d.x * d.x + d.y * d.y + d.z * d.z + d.w * d.w;
            if (gout) {
                const float4 s = wrt_gen ? make_float4(gscale * w.x, gscale * w.y, gscale * w.z, gscale * w.w)
                                         : make_float4(gscale, gscale, gscale, gscale);
                reinterpret_cast<float4*>(gout + base)[i] = make_float4(d.x * s.x, d.y * s.y, d.z * s.z, d.w * s.w);
            }
            if (comp) reinterpret_cast<float4*>(comp + base)[i] = make_float4(t.x + d.x, t.y + d.y, t.z + d.z, t.w + d.w);
        }
    } else {
        for (long i = p0 + threadIdx.x; i < p1; i += 256) {
            const float w = bp[i % HW];
            const float t = target[base + i];
            const float d = w * (img[base + i] - t);
            acc += d * d;
            if (gout) gout[base + i] = d * (wrt_gen ? gscale * w : gscale);
            if (comp) comp[base + i] = t + d;
        }
    }
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) part[(long)b * nparts + blockIdx.x] = acc;
}

// g[b, c, p] *= beta[b, p]: one thread per pixel (four with float4), beta read once for the C channels
__global__ __launch_bounds__(256) void scale_by_plane_kernel(float* __restrict__ g, const float* __restrict__ beta, int C, long HW, long npix) {
    const long stride = (long)gridDim.x * blockDim.x;
    if ((HW & 3) == 0) {
        const long HW4 = HW >> 2;
        for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < (npix >> 2); q += stride) {
            const long b = q / HW4, p = q - b * HW4;
            const float4 w = reinterpret_cast<const float4*>(beta)[q];
            float4* gp = reinterpret_cast<float4*>(g) + b * C * HW4 + p;
            for (int c = 0; c < C; ++c) {
                float4 v = gp[c * HW4];
                v.x *= w.x;
                v.y *= w.y;
                v.z *= w.z;
                v.w *= w.w;
                gp[c * HW4] = v;
            }
        }
    } else {
        for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < npix; q += stride) {
            const long b = q / HW, p = q - b * HW;
            const float w = beta[q];
            float* gp = g + b * C * HW + p;
            for (int c = 0; c < C; ++c) gp[c * HW] *= w;
        }
    }
}

// beta = clip(1 - alpha, 0, 1)^n
__global__ __launch_bounds__(256) void loss_weight_from_alpha_kernel(const float* __restrict__ alpha, float* __restrict__ beta, long n, int power) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += stride) {
        const float q = fminf(fmaxf(1.f - alpha[i], 0.f), 1.f);
        float r = 1.f;
        for (int k = 0; k < power; ++k) r *= q;
        beta[i] = r;
    }
}

int composite_mse(const float* img, const float* target, const float* beta, float* gimg, float* comp, float* part, float* loss,
                  const int* row_dev, int nrows, int B, int C, long HW, int wrt_gen, float grad_mul, void* stream) {
    const long CHW = (long)C * HW;
    const int nparts = oodgan_mse_nparts(CHW);
    const float gscale = grad_mul * 2.0f / (float)CHW;
    count_dispatch(OODGAN_DC_COMPOSITE_MSE);
    if (C == 3 && HW % kMseChunk == 0) {
        hipLaunchKernelGGL(composite_mse_plane_kernel<3>, dim3((unsigned)(HW / kMseChunk), B), dim3(256), 0, as_stream(stream), img, target,
                           beta, gimg, comp, part, HW, nparts, gscale, wrt_gen);
    } else {
        hipLaunchKernelGGL(composite_mse_flat_kernel, dim3(nparts, B), dim3(256), 0, as_stream(stream), img, target, beta, gimg, comp,
                           part, HW, CHW, nparts, gscale, wrt_gen);
    }
    int rc = check_launch("composite_mse");
    if (rc != OODGAN_OK) return rc;
    hipLaunchKernelGGL(mean_finish_kernel<>, dim3(B), dim3(64), 0, as_stream(stream), part, loss, nparts, 1.0f / (float)CHW, row_dev, nrows);
    return check_launch("composite_mse_finish");
}

}  // namespace

extern "C" int oodgan_composite_mse_fwd_bwd(const float* img, const float* target, const float* beta, float* gimg, float* comp, float* part,
                                            float* loss, int B, int C, long HW, int wrt_gen, float grad_mul, void* stream) {
    OODGAN_REQUIRE(img && target && beta && part && loss && B > 0 && B <= 65535 && C > 0 && HW > 0, "composite_mse: bad args");
    return composite_mse(img, target, beta, gimg, comp, part, loss, nullptr, 1, B, C, HW, wrt_gen, grad_mul, stream);
}

extern "C" int oodgan_composite_mse_fwd_bwd_row(const float* img, const float* target, const float* beta, float* gimg, float* comp,
                                                float* part, float* loss_table, const int* row_dev, int nrows, int B, int C, long HW,
                                                int wrt_gen, float grad_mul, void* stream) {
    OODGAN_REQUIRE(img && target && beta && part && loss_table && row_dev && nrows > 0 && B > 0 && B <= 65535 && C > 0 && HW > 0,
                   "composite_mse_row: bad args");
    return composite_mse(img, target, beta, gimg, comp, part, loss_table, row_dev, nrows, B, C, HW, wrt_gen, grad_mul, stream);
}

extern "C" int oodgan_scale_by_plane(float* g, const float* beta, int B, int C, long HW, void* stream) {
    OODGAN_REQUIRE(g && beta && B > 0 && C > 0 && HW > 0, "scale_by_plane: bad args");
    const long npix = (long)B * HW;
    const long work = (HW & 3) == 0 ? npix >> 2 : npix;
    hipLaunchKernelGGL(scale_by_plane_kernel, dim3(stream_grid(work, 256)), dim3(256), 0, as_stream(stream), g, beta, C, HW, npix);
    return check_launch("scale_by_plane");
}

extern "C" int oodgan_loss_weight_from_alpha(const float* alpha, float* beta, long n, int power, void* stream) {
    OODGAN_REQUIRE(alpha && beta && n > 0 && power >= 0, "loss_weight_from_alpha: bad args");
    hipLaunchKernelGGL(loss_weight_from_alpha_kernel, dim3(stream_grid(n, 256)), dim3(256), 0, as_stream(stream), alpha, beta, n, power);
    return check_launch("loss_weight_from_alpha");
}
