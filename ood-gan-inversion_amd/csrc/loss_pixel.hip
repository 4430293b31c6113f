// Pixel terms of the W+ loss: loss[b] = mean_{c,p} rho(d), d = G - x on the full image or d = beta*(G - x) on the
// composite c = x + d of the masked objective (beta a (B,1,HW) plane per image, loss_masked.hip); s = the scale, s2 = s*s in float32.
//   square (MSE)   rho = d^2                                psi = d                      (basicsr MSELoss; gradient scale 2*grad_mul/CHW)
//   Charbonnier    rho = sqrt(d^2 + s2)                     psi = d / sqrt(d^2 + s2)     (BasicSR charbonnier_loss with eps = s2)
//   Huber          rho = d^2/2 (|d| <= s), s(|d| - s/2)     psi = clamp(d, -s, s)        (torch huber_loss, delta = s)
//   Geman-McClure  rho = d^2 r / 2, r = s2 / (d^2 + s2)     psi = d r^2                  (redescending; through r, never through s^4)
// The gradient is gscale * psi(d), gscale = grad_mul/CHW (twice that for the square), times beta once more w.r.t. G on a composite.
// One walk for every term, HBM-bound: kMseChunk elements per block and per partial sum, one float4 order per thread, block_sum_256,
// then mean_finish_kernel's one wave over the partials; no float atomics.  The MSE, the composite MSE and the robust entry points
// are instantiations of the two kernels below, so beta == 1 gives the plain form's loss and gradient bit for bit by construction.
#include <cmath>
#include <string>
#include "loss_common.hpp"

using namespace oodgan;

namespace {

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

// one float4 of the walk: the sum of its four rho, x to w; gradient and composite as asked for.
// w: the loss weights of the four pixels (BETA) — gscale * 1 == gscale, so beta == 1 stores what the plain form stores
template <int KIND, bool BETA>
__device__ __forceinline__ float rho4(const float4 a, const float4 t, const float4 w, float s, float s2, float gscale, int wrt_gen,
                                      float4* gout, float4* comp) {
    float4 d = make_float4(a.x - t.x, a.y - t.y, a.z - t.z, a.w - t.w);
    if constexpr (BETA) d = make_float4(w.x * d.x, w.y * d.y, w.z * d.z, w.w * d.w);
    float4 psi;
    const float rx = rho_psi<KIND>(d.x, s, s2, psi.x), ry = rho_psi<KIND>(d.y, s, s2, psi.y);
    const float rz = rho_psi<KIND>(d.z, s, s2, psi.z), rw = rho_psi<KIND>(d.w, s, s2, psi.w);
    if (gout) {
        float4 g = make_float4(gscale, gscale, gscale, gscale);
        if constexpr (BETA)
            if (wrt_gen) g = make_float4(gscale * w.x, gscale * w.y, gscale * w.z, gscale * w.w);
        *gout = make_float4(psi.x * g.x, psi.y * g.y, psi.z * g.z, psi.w * g.w);
    }
    if constexpr (BETA)
        if (comp) *comp = make_float4(t.x + d.x, t.y + d.y, t.z + d.z, t.w + d.w);
    return rx + ry + rz + rw;
}

// Plane form (beta, HW a multiple of kMseChunk): block j of image b owns pixel chunk j of all C channel planes, reads beta once per
// pixel and keeps one accumulator per channel — the partial of channel chunk c*HW/kMseChunk + j is formed in the order the flat form
// forms it.  grid: (HW / kMseChunk, B).
template <int KIND, int C>
__global__ __launch_bounds__(256) void pixel_plane_kernel(const float* __restrict__ img, const float* __restrict__ target,
                                                          const float* __restrict__ beta, float* __restrict__ gout,
                                                          float* __restrict__ comp, float* __restrict__ part, long HW, int nparts,
                                                          float s, float s2, float gscale, int wrt_gen) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const long HW4 = HW >> 2;
    const long base4 = (long)b * C * HW4;
    const long p0 = (long)blockIdx.x * (kMseChunk >> 2);
    const float4* a4 = reinterpret_cast<const float4*>(img) + base4;
    const float4* t4 = reinterpret_cast<const float4*>(target) + base4;
    const float4* b4 = reinterpret_cast<const float4*>(beta) + (long)b * HW4;
    float4* g4 = gout ? reinterpret_cast<float4*>(gout) + base4 : nullptr;
    float4* c4 = comp ? reinterpret_cast<float4*>(comp) + base4 : nullptr;
    float acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 0.f;
    for (long i = p0 + threadIdx.x; i < p0 + (kMseChunk >> 2); i += 256) {
        const float4 w = b4[i];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const long k = c * HW4 + i;
            acc[c] += rho4<KIND, true>(a4[k], t4[k], w, s, s2, gscale, wrt_gen, g4 ? g4 + k : nullptr, c4 ? c4 + k : nullptr);
        }
    }
    const int chunks_per_plane = (int)(HW / kMseChunk);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float v = block_sum_256(acc[c], red);
        if (threadIdx.x == 0) part[(long)b * nparts + c * chunks_per_plane + blockIdx.x] = v;
    }
}

// Flat form (any C, HW; with or without beta): block j of image b owns chunk j of the image's C*HW elements, beta looked up per element
// (its C planes hit the same cache lines).  float4 accesses where HW % 4 == 0 (a float4 then lies in one channel plane), a scalar form
// otherwise.  grid: (nparts, B).
template <int KIND, bool BETA>
__global__ __launch_bounds__(256) void pixel_flat_kernel(const float* __restrict__ img, const float* __restrict__ target,
                                                         const float* __restrict__ beta, float* __restrict__ gout,
                                                         float* __restrict__ comp, float* __restrict__ part, long HW, long CHW, int nparts,
                                                         float s, float s2, float gscale, int wrt_gen) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const long base = (long)b * CHW;
    const float* bp = BETA ? beta + (long)b * HW : nullptr;
    const long p0 = (long)blockIdx.x * kMseChunk;
    const long p1 = p0 + kMseChunk < CHW ? p0 + kMseChunk : CHW;
    float acc = 0.f;
    if ((HW & 3) == 0) {
        const long HW4 = HW >> 2;
        float4* g4 = gout ? reinterpret_cast<float4*>(gout + base) : nullptr;
        float4* c4 = (BETA && comp) ? reinterpret_cast<float4*>(comp + base) : nullptr;
        for (long i = (p0 >> 2) + threadIdx.x; i < (p1 >> 2); i += 256) {
            const float4 a = reinterpret_cast<const float4*>(img + base)[i];
            const float4 t = reinterpret_cast<const float4*>(target + base)[i];
            float4 w = make_float4(1.f, 1.f, 1.f, 1.f);
            if constexpr (BETA) w = reinterpret_cast<const float4*>(bp)[i % HW4];
            acc += rho4<KIND, BETA>(a, t, w, s, s2, gscale, wrt_gen, g4 ? g4 + i : nullptr, c4 ? c4 + i : nullptr);
        }
    } else {
        for (long i = p0 + threadIdx.x; i < p1; i += 256) {
            const float t = target[base + i];
            float d = img[base + i] - t, w = 1.f;
            if constexpr (BETA) {
                w = bp[i % HW];
                d *= w;
            }
            float psi;
            acc += rho_psi<KIND>(d, s, s2, psi);
            if (gout) gout[base + i] = psi * ((BETA && wrt_gen) ? gscale * w : gscale);
            if constexpr (BETA)
                if (comp) comp[base + i] = t + d;
        }
    }
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) part[(long)b * nparts + blockIdx.x] = acc;
}

template <int KIND>
void launch_kind(const float* img, const float* target, const float* beta, float* gimg, float* comp, float* part, int B, int C, long HW,
                 long CHW, int nparts, float s, float s2, float gscale, int wrt_gen, void* stream) {
    if (beta && C == 3 && HW % kMseChunk == 0) {
        hipLaunchKernelGGL((pixel_plane_kernel<KIND, 3>), dim3((unsigned)(HW / kMseChunk), B), dim3(256), 0, as_stream(stream), img, target,
                           beta, gimg, comp, part, HW, nparts, s, s2, gscale, wrt_gen);
    } else if (beta) {
        hipLaunchKernelGGL((pixel_flat_kernel<KIND, true>), dim3(nparts, B), dim3(256), 0, as_stream(stream), img, target, beta, gimg, comp,
                           part, HW, CHW, nparts, s, s2, gscale, wrt_gen);
    } else {
        hipLaunchKernelGGL((pixel_flat_kernel<KIND, false>), dim3(nparts, B), dim3(256), 0, as_stream(stream), img, target, beta, gimg, comp,
                           part, HW, CHW, nparts, s, s2, gscale, wrt_gen);
    }
}

// Every entry point ends here: the kernel of the kind in its plane, flat-with-beta or flat-plain form, then the mean over the partials.
// what: the entry point's name in a launch error; counter: its dispatch counter, or -1 (the plain MSE counts nothing).
int pixel_term(const char* what, int counter, const float* img, const float* target, const float* beta, float* gimg, float* comp,
               float* part, float* loss, const int* row_dev, int nrows, int B, int C, long HW, int kind, float scale, int wrt_gen,
               float grad_mul, void* stream) {
    const long CHW = (long)C * HW;
    const int nparts = oodgan_mse_nparts(CHW);
    const float s2 = scale * scale;
    const float gscale = kind == kSquare ? grad_mul * 2.0f / (float)CHW : grad_mul / (float)CHW;
    if (counter >= 0) count_dispatch(counter);
    if (kind == kSquare)
        launch_kind<kSquare>(img, target, beta, gimg, comp, part, B, C, HW, CHW, nparts, scale, s2, gscale, wrt_gen, stream);
    else if (kind == OODGAN_ROBUST_CHARBONNIER)
        launch_kind<OODGAN_ROBUST_CHARBONNIER>(img, target, beta, gimg, comp, part, B, C, HW, CHW, nparts, scale, s2, gscale, wrt_gen, stream);
    else if (kind == OODGAN_ROBUST_HUBER)
        launch_kind<OODGAN_ROBUST_HUBER>(img, target, beta, gimg, comp, part, B, C, HW, CHW, nparts, scale, s2, gscale, wrt_gen, stream);
    else
        launch_kind<OODGAN_ROBUST_GEMAN_MCCLURE>(img, target, beta, gimg, comp, part, B, C, HW, CHW, nparts, scale, s2, gscale, wrt_gen, stream);
    int rc = check_launch(what);
    if (rc != OODGAN_OK) return rc;
    hipLaunchKernelGGL(mean_finish_kernel<>, dim3(B), dim3(64), 0, as_stream(stream), part, loss, nparts, 1.0f / (float)CHW, row_dev, nrows);
    return check_launch((std::string(what) + "_finish").c_str());
}

// the kind is one of the three and s*s is a normal, finite float32 (so d^2 + s2 > 0 for every d, beta = 0 pixels included)
bool kind_ok(int kind) { return kind == OODGAN_ROBUST_CHARBONNIER || kind == OODGAN_ROBUST_HUBER || kind == OODGAN_ROBUST_GEMAN_MCCLURE; }
bool scale_ok(float scale) { return scale > 0.f && std::isnormal(scale * scale); }

}  // namespace

// elements per partial sum = elements per block of the flat form: part is (B, oodgan_mse_nparts(C*HW)) for every pixel term
extern "C" int oodgan_mse_nparts(long CHW) { return (int)((CHW + kMseChunk - 1) / kMseChunk); }

// the plain MSE knows only CHW: one plane of CHW pixels, so the flat form takes float4 accesses where CHW % 4 == 0
extern "C" int oodgan_mse_fwd_bwd(const float* img, const float* target, float* gimg, float* part, float* loss, int B, long CHW,
                                  float grad_mul, void* stream) {
    OODGAN_REQUIRE(img && target && part && loss && B > 0 && CHW > 0, "mse: bad args");
    return pixel_term("mse", -1, img, target, nullptr, gimg, nullptr, part, loss, nullptr, 1, B, 1, CHW, kSquare, 0.f, 0, grad_mul, stream);
}

extern "C" int oodgan_mse_fwd_bwd_row(const float* img, const float* target, float* gimg, float* part, float* loss_table,
                                      const int* row_dev, int nrows, int B, long CHW, float grad_mul, void* stream) {
    OODGAN_REQUIRE(img && target && part && loss_table && row_dev && nrows > 0 && B > 0 && CHW > 0, "mse_row: bad args");
    return pixel_term("mse", -1, img, target, nullptr, gimg, nullptr, part, loss_table, row_dev, nrows, B, 1, CHW, kSquare, 0.f, 0, grad_mul,
                      stream);
}

extern "C" int oodgan_composite_mse_fwd_bwd(const float* img, const float* target, const float* beta, float* gimg, float* comp, float* part,
                                            float* loss, int B, int C, long HW, int wrt_gen, float grad_mul, void* stream) {
    OODGAN_REQUIRE(img && target && beta && part && loss && B > 0 && B <= 65535 && C > 0 && HW > 0, "composite_mse: bad args");
    return pixel_term("composite_mse", OODGAN_DC_COMPOSITE_MSE, img, target, beta, gimg, comp, part, loss, nullptr, 1, B, C, HW, kSquare, 0.f,
                      wrt_gen, grad_mul, stream);
}

extern "C" int oodgan_composite_mse_fwd_bwd_row(const float* img, const float* target, const float* beta, float* gimg, float* comp,
                                                float* part, float* loss_table, const int* row_dev, int nrows, int B, int C, long HW,
                                                int wrt_gen, float grad_mul, void* stream) {
    OODGAN_REQUIRE(img && target && beta && part && loss_table && row_dev && nrows > 0 && B > 0 && B <= 65535 && C > 0 && HW > 0,
                   "composite_mse_row: bad args");
    return pixel_term("composite_mse", OODGAN_DC_COMPOSITE_MSE, img, target, beta, gimg, comp, part, loss_table, row_dev, nrows, B, C, HW,
                      kSquare, 0.f, wrt_gen, grad_mul, stream);
}

extern "C" int oodgan_robust_loss_fwd_bwd(const float* img, const float* target, const float* beta, float* gimg, float* comp, float* part,
                                          float* loss, int B, int C, long HW, int kind, float scale, int wrt_gen, float grad_mul,
                                          void* stream) {
    OODGAN_REQUIRE(img && target && part && loss && B > 0 && B <= 65535 && C > 0 && HW > 0, "robust_loss: bad args");
    OODGAN_REQUIRE(kind_ok(kind), "robust_loss: unknown kind %d", kind);
    OODGAN_REQUIRE(scale_ok(scale), "robust_loss: scale %g: must be finite and > 0, with a normal float32 square", (double)scale);
    OODGAN_REQUIRE(beta || !comp, "robust_loss: a composite needs beta");
    return pixel_term("robust_loss", OODGAN_DC_ROBUST, img, target, beta, gimg, comp, part, loss, nullptr, 1, B, C, HW, kind, scale, wrt_gen,
                      grad_mul, stream);
}

extern "C" int oodgan_robust_loss_fwd_bwd_row(const float* img, const float* target, const float* beta, float* gimg, float* comp,
                                              float* part, float* loss_table, const int* row_dev, int nrows, int B, int C, long HW, int kind,
                                              float scale, int wrt_gen, float grad_mul, void* stream) {
    OODGAN_REQUIRE(img && target && part && loss_table && row_dev && nrows > 0 && B > 0 && B <= 65535 && C > 0 && HW > 0,
                   "robust_loss_row: bad args");
    OODGAN_REQUIRE(kind_ok(kind), "robust_loss_row: unknown kind %d", kind);
    OODGAN_REQUIRE(scale_ok(scale), "robust_loss_row: scale %g: must be finite and > 0, with a normal float32 square", (double)scale);
    OODGAN_REQUIRE(beta || !comp, "robust_loss_row: a composite needs beta");
    return pixel_term("robust_loss", OODGAN_DC_ROBUST, img, target, beta, gimg, comp, part, loss_table, row_dev, nrows, B, C, HW, kind, scale,
                      wrt_gen, grad_mul, stream);
}
