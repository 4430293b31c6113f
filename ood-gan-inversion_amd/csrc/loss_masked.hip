// Masked W+ objective ("composite objective"): the loss is evaluated on the composite c = x + beta*(G - x), beta a
// (B,1,HW) plane per image broadcast over the C colour channels.  The pixel term on the composite (the composite MSE and the robust
// terms with beta) is the kernel family of loss_pixel.hip; here is what the objective needs besides, two HBM-bound streaming kernels:
//   scale_by_plane: g <- beta (.) g (the chain rule from c to G once LPIPS has accumulated into the gradient w.r.t. c);
//   loss_weight_from_alpha: beta = clip(1 - alpha, 0, 1)^n (the composite that `blend` applied n times produces).
#include "common.hpp"

using namespace oodgan;

namespace {

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

}  // namespace

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
