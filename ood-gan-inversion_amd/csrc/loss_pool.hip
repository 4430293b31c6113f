// Area-pooled view of an image for a loss term of the W+ step ("pooled view"): y = the mean of every FxF window of x, and its
// exact adjoint added into an image gradient.  The step takes LPIPS on the pooled composite: pool (which also zeroes the term's gradient
// buffer — no torch kernel may run inside a recorded step), the term at the small size, unpool-add into gimg.  Term-agnostic.
//   area_pool_fwd:      y[p] = (sum of the window, fp32, row-major order) * 1/F^2 (an exact power of two);  gzero[p] = 0 if given
//   area_pool_bwd_add:  gimg[., y, x] += gs[., y/F, x/F] * 1/F^2, in place
// One thread per pooled pixel and plane owns its FxF block in both directions: no scatter, no atomics, no LDS, bit-reproducible.  A window
// row is one float2 (F = 2) or F/4 float4 (F >= 4); W % F == 0 and an aligned base make every row 8- / 16-byte aligned, and adjacent lanes
// own adjacent runs, so a wave's access to one row is one contiguous span of 64*F*4 bytes.  HBM-bound streaming, F in {2, 4, 8, 16} only:
// the generator's sizes are powers of two, nothing reaches another factor.
#include <cstdint>
#include "loss_common.hpp"

using namespace oodgan;

namespace {

// Row<F>, sum_in_order: loss_common.hpp (the pooled pixel term of loss_pixel.hip walks a window the same way)
__device__ __forceinline__ float2 add_all(float2 v, float g) { return make_float2(v.x + g, v.y + g); }
__device__ __forceinline__ float4 add_all(float4 v, float g) { return make_float4(v.x + g, v.y + g, v.z + g, v.w + g); }

// rows of a window in flight per trip of the row loop (the sum's order does not depend on it: fp32 adds are not reassociated)
template <int F>
constexpr int kRowUnroll = F <= 4 ? F : 4;

// pooled pixel p = (plane, oy, ox) -> offset of its window's first element in the (BC, H, W) tensor
template <int F>
__device__ __forceinline__ long window_offset(long p, int Ho, int Wo, int W) {
    const long row = p / Wo;                     // plane * Ho + oy: the planes lie back to back, so window row r starts at (row*F + r) * W
    const int ox = (int)(p - row * Wo);
    return row * F * (long)W + (long)ox * F;
}

// grid: (ceil(total / 256)); total = BC * Ho * Wo pooled pixels
template <int F>
__global__ __launch_bounds__(256) void area_pool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, float* __restrict__ gzero,
                                                            long total, int Ho, int Wo, int W) {
    using V = typename Row<F>::V;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const float* xp = x + window_offset<F>(p, Ho, Wo, W);
    float acc = 0.f;
#pragma unroll kRowUnroll<F>
    for (int r = 0; r < F; ++r) {
        const V* rp = reinterpret_cast<const V*>(xp + (long)r * W);
#pragma unroll
        for (int j = 0; j < Row<F>::N; ++j) acc = sum_in_order(acc, rp[j]);
    }
    y[p] = acc * (1.0f / (F * F));
    if (gzero) gzero[p] = 0.0f;
}

template <int F>
__global__ __launch_bounds__(256) void area_pool_bwd_add_kernel(const float* __restrict__ gs, float* __restrict__ gimg, long total, int Ho,
                                                                int Wo, int W) {
    using V = typename Row<F>::V;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= total) return;
    const float g = gs[p] * (1.0f / (F * F));
    float* gp = gimg + window_offset<F>(p, Ho, Wo, W);
    // kRowUnroll rows are loaded before the first of them is stored: written row by row, each row's load waits for the store before it
    // (W is a run-time value: the compiler cannot tell the rows apart), F dependent round trips per thread
    constexpr int U = kRowUnroll<F>, N = Row<F>::N;
    for (int r0 = 0; r0 < F; r0 += U) {
        V v[U][N];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < N; ++j) v[u][j] = reinterpret_cast<const V*>(gp + (long)(r0 + u) * W)[j];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < N; ++j) reinterpret_cast<V*>(gp + (long)(r0 + u) * W)[j] = add_all(v[u][j], g);
    }
}

// what both entry points require of (BC, H, W, f) and of the full-resolution pointer; the pooled pixel count through *total
int check_shape(const char* what, const void* full, int BC, int H, int W, int f, long* total) {
    OODGAN_REQUIRE(f == 2 || f == 4 || f == 8 || f == 16, "%s: factor %d: must be 2, 4, 8 or 16", what, f);
    OODGAN_REQUIRE(BC > 0 && H > 0 && W > 0, "%s: bad shape (%d, %d, %d)", what, BC, H, W);
    OODGAN_REQUIRE(H % f == 0 && W % f == 0, "%s: a %dx%d plane is not a multiple of the factor %d", what, H, W, f);
    OODGAN_REQUIRE(reinterpret_cast<uintptr_t>(full) % pool_row_align(f) == 0, "%s: the full-resolution tensor must be %d-byte aligned", what,
                   pool_row_align(f));
    *total = (long)BC * (H / f) * (W / f);
    OODGAN_REQUIRE((*total + 255) / 256 <= 0x7fffffffL, "%s: %ld pooled pixels: too many for one grid", what, *total);
    return OODGAN_OK;
}

template <int F>
void launch_fwd(const float* x, float* y, float* gzero, long total, int Ho, int Wo, int W, void* stream) {
    hipLaunchKernelGGL(area_pool_fwd_kernel<F>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), x, y, gzero, total, Ho,
                       Wo, W);
}

template <int F>
void launch_bwd(const float* gs, float* gimg, long total, int Ho, int Wo, int W, void* stream) {
    hipLaunchKernelGGL(area_pool_bwd_add_kernel<F>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), gs, gimg, total,
                       Ho, Wo, W);
}

}  // namespace

extern "C" int oodgan_area_pool_fwd(const float* x, float* y, float* gzero, int BC, int H, int W, int f, void* stream) {
    OODGAN_REQUIRE(x && y, "area_pool_fwd: bad args");
    long total = 0;
    int rc = check_shape("area_pool_fwd", x, BC, H, W, f, &total);
    if (rc != OODGAN_OK) return rc;
    count_dispatch(OODGAN_DC_AREA_POOL);
    const int Ho = H / f, Wo = W / f;
    if (f == 2) launch_fwd<2>(x, y, gzero, total, Ho, Wo, W, stream);
    else if (f == 4) launch_fwd<4>(x, y, gzero, total, Ho, Wo, W, stream);
    else if (f == 8) launch_fwd<8>(x, y, gzero, total, Ho, Wo, W, stream);
    else launch_fwd<16>(x, y, gzero, total, Ho, Wo, W, stream);
    return check_launch("area_pool_fwd");
}

extern "C" int oodgan_area_pool_bwd_add(const float* gs, float* gimg, int BC, int H, int W, int f, void* stream) {
    OODGAN_REQUIRE(gs && gimg, "area_pool_bwd_add: bad args");
    long total = 0;
    int rc = check_shape("area_pool_bwd_add", gimg, BC, H, W, f, &total);
    if (rc != OODGAN_OK) return rc;
    count_dispatch(OODGAN_DC_AREA_POOL);
    const int Ho = H / f, Wo = W / f;
    if (f == 2) launch_bwd<2>(gs, gimg, total, Ho, Wo, W, stream);
    else if (f == 4) launch_bwd<4>(gs, gimg, total, Ho, Wo, W, stream);
    else if (f == 8) launch_bwd<8>(gs, gimg, total, Ho, Wo, W, stream);
    else launch_bwd<16>(gs, gimg, total, Ho, Wo, W, stream);
    return check_launch("area_pool_bwd_add");
}
