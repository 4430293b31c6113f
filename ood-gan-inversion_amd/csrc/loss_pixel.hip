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
#include <cstdint>
#include <string>
#include "loss_common.hpp"

using namespace oodgan;

namespace {

// kSquare, rho_psi<KIND>: loss_common.hpp (the resampled pixel term of loss_resample.hip applies the same rho and psi)

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

// ---- The pixel term on an area-pooled view (pixel_size): r = P(G) - P(x), or r = P(beta*(G - x)) with a loss weight, P the
// mean over F x F windows exactly as area_pool_fwd_kernel forms it (fp32, row-major order, times the exact 1/F^2); loss = mean rho(r) over
// the C*Hs*Ws pooled pixels; every pixel of window q receives gscale * psi(r_q) (times beta(y,x) w.r.t. G).  loss_pool.hip's ownership: one
// thread owns a window in both directions and adjacent lanes own adjacent windows — no scatter, no atomics, LDS only in block_sum_256.
// The window is summed in one pass and walked again to write: without beta the second pass only stores, with beta it reads beta again (and
// G and x for the composite), lines the first pass left in L2.  NC = 3 (beta, C = 3, F <= 8): the thread owns the pooled position in all
// three planes and reads beta's window once (the plane form's idea); NC = 1: one plane per thread, any C — also with beta at F = 16, where
// a third of the threads (2 waves per CU at B = 8, 1024²) cannot hide the latency of a window walked row by row and the three reads of
// beta meet in L2 (measured both ways, DESIGN.md §20: F = 16 is 9 % faster so, F = 8 7 % slower).

// windows per thread: a block covers at least 16 KB of the image (4096 elements) at every factor
template <int F>
constexpr int kPoolTrips = F == 2 ? 4 : F == 4 ? 2 : 1;
// rows of a window in flight in the summing pass; with beta a row is up to seven vectors per element: F = 8 (three planes) goes row by row,
// F = 16 (one plane) two rows at a time
template <int F, bool BETA>
constexpr int kPoolRowUnroll = (BETA && F >= 8) ? F / 8 : (F <= 4 ? F : 4);
// with beta at C = 3: does a thread own all three planes of its pooled position?
constexpr bool pooled_plane_form(bool beta, int C, int f) { return beta && C == 3 && f <= 8; }

// beta * (a - t), two roundings per pixel as rho4 forms it.  The product must reach the window's sum (and the composite's add) rounded:
// contraction is off in these two functions, or the compiler folds it into the add that follows (v_fmac) and the sum is no longer the
// area pool of the elementwise product.
__device__ __forceinline__ float weighted_diff(float a, float t, float w) {
#pragma clang fp contract(off)
    const float d = a - t;
    return w * d;
}
__device__ __forceinline__ float2 weighted_diff(const float2 a, const float2 t, const float2 w) {
    return make_float2(weighted_diff(a.x, t.x, w.x), weighted_diff(a.y, t.y, w.y));
}
__device__ __forceinline__ float4 weighted_diff(const float4 a, const float4 t, const float4 w) {
    return make_float4(weighted_diff(a.x, t.x, w.x), weighted_diff(a.y, t.y, w.y), weighted_diff(a.z, t.z, w.z), weighted_diff(a.w, t.w, w.w));
}
// the composite of one pixel as rho4 stores it: t + d, d the rounded product
__device__ __forceinline__ float composite_of(float a, float t, float w) {
#pragma clang fp contract(off)
    const float d = weighted_diff(a, t, w);
    return t + d;
}
__device__ __forceinline__ float2 composite_of(const float2 a, const float2 t, const float2 w) {
    return make_float2(composite_of(a.x, t.x, w.x), composite_of(a.y, t.y, w.y));
}
__device__ __forceinline__ float4 composite_of(const float4 a, const float4 t, const float4 w) {
    return make_float4(composite_of(a.x, t.x, w.x), composite_of(a.y, t.y, w.y), composite_of(a.z, t.z, w.z), composite_of(a.w, t.w, w.w));
}
// psi * g on every element (no beta), or psi * (g * w) element by element, rho4's order
__device__ __forceinline__ float2 grad_of(float psi, float g, const float2 w) { return make_float2(psi * (g * w.x), psi * (g * w.y)); }
__device__ __forceinline__ float4 grad_of(float psi, float g, const float4 w) {
    return make_float4(psi * (g * w.x), psi * (g * w.y), psi * (g * w.z), psi * (g * w.w));
}
__device__ __forceinline__ void splat(float2& v, float x) { v = make_float2(x, x); }
__device__ __forceinline__ void splat(float4& v, float x) { v = make_float4(x, x, x, x); }

// grid: (nparts, B); block j of image b owns items [j, j + 1) * 256 * kPoolTrips<F> of the image: pooled pixels of all C planes (NC = 1)
// or pooled positions (NC = 3 = C).  tpool: the pooled target (B,C,Hs,Ws), read without beta; target: the full one, read with beta.
template <int KIND, int F, int NC, bool BETA>
__global__ __launch_bounds__(256) void pooled_pixel_kernel(const float* __restrict__ img, const float* __restrict__ target,
                                                           const float* __restrict__ tpool, const float* __restrict__ beta,
                                                           float* __restrict__ gout, float* __restrict__ comp, float* __restrict__ part, int C,
                                                           int Ws, long HWs, int W, int nparts, float s, float s2, float gscale, int wrt_gen) {
    using V = typename Row<F>::V;
    constexpr int N = Row<F>::N;
    __shared__ float red[4];
    const int b = blockIdx.y;
    const long HW = HWs * (F * F);
    const long items = (NC == 1 ? (long)C : 1L) * HWs;
    const bool with_comp = BETA && comp != nullptr;
    const bool by_beta = BETA && wrt_gen != 0;
    float acc = 0.f;
    for (int trip = 0; trip < kPoolTrips<F>; ++trip) {
        const long q = ((long)blockIdx.x * kPoolTrips<F> + trip) * 256 + threadIdx.x;
        if (q >= items) break;
        const long plane = q / HWs;                                   // 0 for NC = 3
        const long pos = q - plane * HWs;
        const long oy = pos / Ws;
        const long win = oy * F * (long)W + (pos - oy * Ws) * F;      // the window's first element within its plane
        const long off = ((long)b * C + plane) * HW + win;
        const long boff = (long)b * HW + win;
        float sum[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) sum[c] = 0.f;
#pragma unroll kPoolRowUnroll<F, BETA>
        for (int r = 0; r < F; ++r) {
            const long ro = (long)r * W;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                V w;
                if constexpr (BETA) w = reinterpret_cast<const V*>(beta + boff + ro)[j];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const V a = reinterpret_cast<const V*>(img + off + c * HW + ro)[j];
                    if constexpr (BETA) {
                        const V t = reinterpret_cast<const V*>(target + off + c * HW + ro)[j];
                        sum[c] = sum_in_order(sum[c], weighted_diff(a, t, w));
                    } else {
                        sum[c] = sum_in_order(sum[c], a);
                    }
                }
            }
        }
        float psi[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float r = sum[c] * (1.0f / (F * F));
            if constexpr (!BETA) r -= tpool[((long)b * C + plane + c) * HWs + pos];
            acc += rho_psi<KIND>(r, s, s2, psi[c]);
        }
        if (!gout && !with_comp) continue;
        for (int r = 0; r < F; ++r) {
            const long ro = (long)r * W;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                V w;
                splat(w, 1.f);
                if constexpr (BETA)
                    if (by_beta || with_comp) w = reinterpret_cast<const V*>(beta + boff + ro)[j];
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const long k = off + c * HW + ro;
                    if constexpr (BETA)
                        if (with_comp)
                            reinterpret_cast<V*>(comp + k)[j] =
                                composite_of(reinterpret_cast<const V*>(img + k)[j], reinterpret_cast<const V*>(target + k)[j], w);
                    if (gout) {
                        V g;
                        if (by_beta) g = grad_of(psi[c], gscale, w);
                        else splat(g, psi[c] * gscale);
                        reinterpret_cast<V*>(gout + k)[j] = g;
                    }
                }
            }
        }
    }
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) part[(long)b * nparts + blockIdx.x] = acc;
}

int pooled_nparts(long items, int f) {
    const long per_block = 256L * (f == 2 ? kPoolTrips<2> : f == 4 ? kPoolTrips<4> : f == 8 ? kPoolTrips<8> : kPoolTrips<16>);
    return (int)((items + per_block - 1) / per_block);
}

template <int KIND, int F>
void launch_pooled(const float* img, const float* target, const float* tpool, const float* beta, float* gimg, float* comp, float* part, int B,
                   int C, int Ws, long HWs, int W, int nparts, float s, float s2, float gscale, int wrt_gen, void* stream) {
    if constexpr (pooled_plane_form(true, 3, F)) {
        if (pooled_plane_form(beta != nullptr, C, F)) {
            hipLaunchKernelGGL((pooled_pixel_kernel<KIND, F, 3, true>), dim3(nparts, B), dim3(256), 0, as_stream(stream), img, target, tpool,
                               beta, gimg, comp, part, C, Ws, HWs, W, nparts, s, s2, gscale, wrt_gen);
            return;
        }
    }
    if (beta)
        hipLaunchKernelGGL((pooled_pixel_kernel<KIND, F, 1, true>), dim3(nparts, B), dim3(256), 0, as_stream(stream), img, target, tpool, beta,
                           gimg, comp, part, C, Ws, HWs, W, nparts, s, s2, gscale, wrt_gen);
    else
        hipLaunchKernelGGL((pooled_pixel_kernel<KIND, F, 1, false>), dim3(nparts, B), dim3(256), 0, as_stream(stream), img, target, tpool, beta,
                           gimg, comp, part, C, Ws, HWs, W, nparts, s, s2, gscale, wrt_gen);
}

template <int KIND>
void launch_pooled_kind(int f, const float* img, const float* target, const float* tpool, const float* beta, float* gimg, float* comp,
                        float* part, int B, int C, int Ws, long HWs, int W, int nparts, float s, float s2, float gscale, int wrt_gen,
                        void* stream) {
    if (f == 2) launch_pooled<KIND, 2>(img, target, tpool, beta, gimg, comp, part, B, C, Ws, HWs, W, nparts, s, s2, gscale, wrt_gen, stream);
    else if (f == 4) launch_pooled<KIND, 4>(img, target, tpool, beta, gimg, comp, part, B, C, Ws, HWs, W, nparts, s, s2, gscale, wrt_gen, stream);
    else if (f == 8) launch_pooled<KIND, 8>(img, target, tpool, beta, gimg, comp, part, B, C, Ws, HWs, W, nparts, s, s2, gscale, wrt_gen, stream);
    else launch_pooled<KIND, 16>(img, target, tpool, beta, gimg, comp, part, B, C, Ws, HWs, W, nparts, s, s2, gscale, wrt_gen, stream);
}

bool aligned_for(const void* p, int f) { return reinterpret_cast<uintptr_t>(p) % pool_row_align(f) == 0; }

// Both pooled entry points end here: every argument checked (a status, nothing launched), then the kernel of the kind and factor in its
// form, then the mean over the partials.  loss / row_dev / nrows: the sink as in pixel_term.
int pooled_pixel_term(const char* what, const float* img, const float* target, const float* tpool, const float* beta, float* gimg,
                      float* comp, float* part, float* loss, const int* row_dev, int nrows, int B, int C, int H, int W, int f, int kind,
                      float scale, int wrt_gen, float grad_mul, void* stream) {
    OODGAN_REQUIRE(f == 2 || f == 4 || f == 8 || f == 16, "%s: factor %d: must be 2, 4, 8 or 16", what, f);
    OODGAN_REQUIRE(B > 0 && B <= 65535 && C > 0 && H > 0 && W > 0, "%s: bad shape (%d, %d, %d, %d)", what, B, C, H, W);
    OODGAN_REQUIRE(H % f == 0 && W % f == 0, "%s: a %dx%d plane is not a multiple of the factor %d", what, H, W, f);
    OODGAN_REQUIRE(kind == kSquare || kind_ok(kind), "%s: unknown kind %d", what, kind);
    OODGAN_REQUIRE(kind == kSquare || scale_ok(scale), "%s: scale %g: must be finite and > 0, with a normal float32 square", what, (double)scale);
    OODGAN_REQUIRE(beta || !comp, "%s: a composite needs beta", what);
    OODGAN_REQUIRE(!beta || (target && !tpool), "%s: with beta the residual is pooled from the full target: target, and no target_pooled", what);
    OODGAN_REQUIRE(beta || (tpool && !target), "%s: without beta the pooled target is read: target_pooled, and no target", what);
    OODGAN_REQUIRE(aligned_for(img, f) && aligned_for(target, f) && aligned_for(beta, f) && aligned_for(gimg, f) && aligned_for(comp, f),
                   "%s: the full-resolution tensors must be %d-byte aligned", what, pool_row_align(f));
    const int Ws = W / f;
    const long HWs = (long)(H / f) * Ws, CHW = (long)C * H * W;
    OODGAN_REQUIRE(CHW / 256 <= 0x7fffffffL, "%s: %ld elements per image: too many for one grid", what, CHW);
    const int nparts = pooled_nparts(pooled_plane_form(beta != nullptr, C, f) ? HWs : C * HWs, f);
    const float s2 = scale * scale;
    const float gscale = kind == kSquare ? grad_mul * 2.0f / (float)CHW : grad_mul / (float)CHW;
    count_dispatch(OODGAN_DC_POOLED_PIXEL);
    if (kind == kSquare)
        launch_pooled_kind<kSquare>(f, img, target, tpool, beta, gimg, comp, part, B, C, Ws, HWs, W, nparts, scale, s2, gscale, wrt_gen, stream);
    else if (kind == OODGAN_ROBUST_CHARBONNIER)
        launch_pooled_kind<OODGAN_ROBUST_CHARBONNIER>(f, img, target, tpool, beta, gimg, comp, part, B, C, Ws, HWs, W, nparts, scale, s2, gscale,
                                                      wrt_gen, stream);
    else if (kind == OODGAN_ROBUST_HUBER)
        launch_pooled_kind<OODGAN_ROBUST_HUBER>(f, img, target, tpool, beta, gimg, comp, part, B, C, Ws, HWs, W, nparts, scale, s2, gscale, wrt_gen,
                                                stream);
    else
        launch_pooled_kind<OODGAN_ROBUST_GEMAN_MCCLURE>(f, img, target, tpool, beta, gimg, comp, part, B, C, Ws, HWs, W, nparts, scale, s2, gscale,
                                                        wrt_gen, stream);
    int rc = check_launch(what);
    if (rc != OODGAN_OK) return rc;
    hipLaunchKernelGGL(mean_finish_kernel<>, dim3(B), dim3(64), 0, as_stream(stream), part, loss, nparts, 1.0f / (float)(C * HWs), row_dev,
                       nrows);
    return check_launch((std::string(what) + "_finish").c_str());
}

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

// part of the pooled term: (B, oodgan_pooled_pixel_loss_nparts(C*Hs*Ws, f)) holds every form (with beta at C = 3 fewer are used); 0: bad factor
extern "C" int oodgan_pooled_pixel_loss_nparts(long CHWs, int f) {
    if (CHWs <= 0 || !(f == 2 || f == 4 || f == 8 || f == 16)) return 0;
    return pooled_nparts(CHWs, f);
}

extern "C" int oodgan_pooled_pixel_loss_fwd_bwd(const float* img, const float* target, const float* target_pooled, const float* beta,
                                                float* gimg, float* comp, float* part, float* loss, int B, int C, int H, int W, int f,
                                                int kind, float scale, int wrt_gen, float grad_mul, void* stream) {
    OODGAN_REQUIRE(img && part && loss, "pooled_pixel_loss: bad args");
    return pooled_pixel_term("pooled_pixel_loss", img, target, target_pooled, beta, gimg, comp, part, loss, nullptr, 1, B, C, H, W, f, kind, scale,
                             wrt_gen, grad_mul, stream);
}

extern "C" int oodgan_pooled_pixel_loss_fwd_bwd_row(const float* img, const float* target, const float* target_pooled, const float* beta,
                                                    float* gimg, float* comp, float* part, float* loss_table, const int* row_dev, int nrows,
                                                    int B, int C, int H, int W, int f, int kind, float scale, int wrt_gen, float grad_mul,
                                                    void* stream) {
    OODGAN_REQUIRE(img && part && loss_table && row_dev && nrows > 0, "pooled_pixel_loss_row: bad args");
    return pooled_pixel_term("pooled_pixel_loss", img, target, target_pooled, beta, gimg, comp, part, loss_table, row_dev, nrows, B, C, H, W, f,
                             kind, scale, wrt_gen, grad_mul, stream);
}
