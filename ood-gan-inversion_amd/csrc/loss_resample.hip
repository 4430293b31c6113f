// The pixel term on an antialiased resampled view (pixel_filter): D(G) = Ay · G · Axᵀ per plane, Ay (Hs,T) and Ax (Ws,T) the
// per-axis tap tables of a separable filter of support s at factor F (T = s*F taps per output; output q reads inputs F*q - (T-F)/2 + j,
// j = 0 .. T-1; a tap that falls outside the image has weight 0 in the table, the rest are renormalised by the host).  r = D(G) - y,
// loss = mean rho(r) over the C*Hs*Ws pooled pixels, gradient = gs * Ayᵀ psi(r) Ax, gs = grad_mul/(C*Hs*Ws) (twice that for the square).
//
// Two kernels, both gathers, both separable inside a block, no float atomics:
//   resample_fwd_kernel   a block owns a TQ x TQ tile of pooled pixels of one plane.  It stages its table rows, walks the (TQ+s-1)*F input
//                         rows it reads in chunks of 256/TQ rows (coalesced loads into LDS, indices clamped: a clamped tap has weight 0),
//                         one thread per (row, pooled column) forms the horizontal sum of T taps into LDS, then one thread per pooled pixel
//                         forms the vertical sum of T taps.  LOSS: r, rho, psi(r) to the pooled scratch, the block's partial of rho;
//                         otherwise the view itself (the same sums, so the same bits).
//   resample_bwd_kernel   a block owns the (TQ*F)² pixels of the same tile.  A pixel is read by at most s pooled positions per axis: the block
//                         stages the (TQ+s)² pooled psi it needs (zero outside the view) and the table rows of those positions, forms
//                         v[y][qx] = sum_qy Ay[qy][y - y0(qy)] psi[qy][qx] in LDS (s terms), then g[y][x] = gs * sum_qx Ax[qx][x - x0(qx)] v[y][qx].
// Every sum runs in a fixed order (S runs of F taps ascending, the runs pairwise; pooled positions descending): a call is bit-reproducible.
// LDS rows are padded by one dword per F inputs (the input chunk) or per table row: adjacent pooled columns are F (T) dwords apart.
#include <cmath>
#include <string>
#include <type_traits>
#include "loss_common.hpp"

using namespace oodgan;

namespace {

// pooled pixels per tile edge: 64 input pixels per edge up to F = 8, 128 at F = 16 (a 4 x 4 tile would read its inputs 5 times at s = 6)
template <int F>
constexpr int kTileQ = F == 16 ? 8 : 64 / F;
inline int tile_q(int f) { return f == 16 ? 8 : 64 / f; }

// The T = S*F taps of an output are summed as S runs of F taps (one accumulator each, taps ascending: S independent chains), then the runs
// pairwise in this fixed order
template <int S>
__device__ __forceinline__ float sum_of(const float (&a)[S]) {
    static_assert(S == 2 || S == 4 || S == 6, "support");
    if constexpr (S == 2) return a[0] + a[1];
    else if constexpr (S == 4) return (a[0] + a[1]) + (a[2] + a[3]);
    else return ((a[0] + a[1]) + (a[2] + a[3])) + (a[4] + a[5]);
}

// rho(d) and psi(d) of the kind chosen at run time: one call per pooled pixel
__device__ __forceinline__ float rho_psi_kind(int kind, float d, float s, float s2, float& psi) {
    if (kind == kSquare) return rho_psi<kSquare>(d, s, s2, psi);
    if (kind == OODGAN_ROBUST_CHARBONNIER) return rho_psi<OODGAN_ROBUST_CHARBONNIER>(d, s, s2, psi);
    if (kind == OODGAN_ROBUST_HUBER) return rho_psi<OODGAN_ROBUST_HUBER>(d, s, s2, psi);
    return rho_psi<OODGAN_ROBUST_GEMAN_MCCLURE>(d, s, s2, psi);
}

// grid: (tiles * C, B); block (t, c, b) owns tile t of plane b*C + c.  out: the view (B,C,Hs,Ws), or with LOSS psi(r) of the same shape.
template <int F, int S, bool LOSS>
__global__ __launch_bounds__(256) void resample_fwd_kernel(const float* __restrict__ img, const float* __restrict__ tview,
                                                           const float* __restrict__ Ay, const float* __restrict__ Ax, float* __restrict__ out,
                                                           float* __restrict__ part, int C, int H, int W, int tilesX, int tiles, int nparts,
                                                           int kind, float s, float s2) {
    constexpr int T = S * F, TQ = kTileQ<F>, OFF = (T - F) / 2, NQ = TQ + S - 1;
    constexpr int RH = NQ * F, CW = NQ * F, CWP = NQ * (F + 1), RC = 256 / TQ, TP = T + 1;
    __shared__ float in_s[RC * CWP];             // a chunk of input rows, one pad dword per F inputs
    __shared__ float h_s[RH * TQ];               // horizontal sums: (input row, pooled column)
    __shared__ float ax_s[TQ * TP], ay_s[TQ * TP];
    __shared__ float red[4];
    const int Hs = H / F, Ws = W / F;
    const int tile = blockIdx.x % tiles, c = blockIdx.x / tiles, b = blockIdx.y;
    const int qy0 = (tile / tilesX) * TQ, qx0 = (tile % tilesX) * TQ;
    const long plane = (long)b * C + c;
    const float* __restrict__ src = img + plane * H * W;
    for (int i = threadIdx.x; i < TQ * T; i += 256) {
        const int q = i / T, j = i - q * T;
        ax_s[q * TP + j] = qx0 + q < Ws ? Ax[(long)(qx0 + q) * T + j] : 0.f;
        ay_s[q * TP + j] = qy0 + q < Hs ? Ay[(long)(qy0 + q) * T + j] : 0.f;
    }
    const int gy0 = F * qy0 - OFF, gx0 = F * qx0 - OFF;
    const int lq = threadIdx.x % TQ, lr = threadIdx.x / TQ;
    for (int r0 = 0; r0 < RH; r0 += RC) {
        __syncthreads();                         // the tables are staged; the previous chunk has been read
        for (int i = threadIdx.x; i < RC * CW; i += 256) {
            const int r = i / CW, cc = i - r * CW;
            const int gy = min(max(gy0 + r0 + r, 0), H - 1), gx = min(max(gx0 + cc, 0), W - 1);
            in_s[r * CWP + cc + cc / F] = src[(long)gy * W + gx];
        }
        __syncthreads();
        if (r0 + lr < RH) {
            const float* __restrict__ row = in_s + lr * CWP + lq * (F + 1);
            const float* __restrict__ wt = ax_s + lq * TP;
            float acc[S];
#pragma unroll
            for (int k = 0; k < S; ++k) {
                acc[k] = 0.f;
#pragma unroll
                for (int j = 0; j < F; ++j) acc[k] += wt[k * F + j] * row[k * (F + 1) + j];
            }
            h_s[(r0 + lr) * TQ + lq] = sum_of<S>(acc);
        }
    }
    __syncthreads();
    float lsum = 0.f;
    for (int o = threadIdx.x; o < TQ * TQ; o += 256) {
        const int ly = o / TQ, lx = o - ly * TQ;
        const int qy = qy0 + ly, qx = qx0 + lx;
        if (qy < Hs && qx < Ws) {
            const float* __restrict__ wt = ay_s + ly * TP;
            const float* __restrict__ col = h_s + (ly * F) * TQ + lx;
            float acc[S];
#pragma unroll
            for (int k = 0; k < S; ++k) {
                acc[k] = 0.f;
#pragma unroll
                for (int j = 0; j < F; ++j) acc[k] += wt[k * F + j] * col[(k * F + j) * TQ];
            }
            const float v = sum_of<S>(acc);
            const long oi = (plane * Hs + qy) * Ws + qx;
            if constexpr (LOSS) {
                float psi;
                lsum += rho_psi_kind(kind, v - tview[oi], s, s2, psi);
                out[oi] = psi;
            } else {
                out[oi] = v;
            }
        }
    }
    if constexpr (LOSS) {
        lsum = block_sum_256(lsum, red);
        if (threadIdx.x == 0) part[(long)b * nparts + blockIdx.x] = lsum;
    }
}

// grid: (tiles * B*C); block t of plane p owns the (TQ*F)² pixels of tile t.  psi: (B*C, Hs, Ws).
template <int F, int S>
__global__ __launch_bounds__(256) void resample_bwd_kernel(const float* __restrict__ psi, const float* __restrict__ Ay,
                                                           const float* __restrict__ Ax, float* __restrict__ gimg, int H, int W, int tilesX,
                                                           int tiles, float gs) {
    constexpr int T = S * F, TQ = kTileQ<F>, OFF = (T - F) / 2, PH = TQ + S, PX = TQ * F, TP = T + 1;
    __shared__ float p_s[PH * PH];               // psi of the pooled positions that read this tile's pixels, zero outside the view
    __shared__ float ay_s[PH * TP], ax_s[PH * TP];
    __shared__ float v_s[PX * PH];               // vertical sums: (pixel row, pooled column)
    const int Hs = H / F, Ws = W / F;
    const int tile = blockIdx.x % tiles;
    const long plane = blockIdx.x / tiles;
    const int qy0 = (tile / tilesX) * TQ, qx0 = (tile % tilesX) * TQ;
    const int qyb = qy0 - S / 2, qxb = qx0 - S / 2;        // the first pooled row / column of the halo
    const float* __restrict__ ps = psi + plane * Hs * Ws;
    for (int i = threadIdx.x; i < PH * PH; i += 256) {
        const int py = i / PH, px = i - py * PH;
        const int qy = qyb + py, qx = qxb + px;
        const bool in = qy >= 0 && qy < Hs && qx >= 0 && qx < Ws;
        p_s[i] = in ? ps[(long)qy * Ws + qx] : 0.f;
    }
    for (int i = threadIdx.x; i < PH * T; i += 256) {
        const int q = i / T, j = i - q * T;
        const int qy = qyb + q, qx = qxb + q;
        ay_s[q * TP + j] = (qy >= 0 && qy < Hs) ? Ay[(long)qy * T + j] : 0.f;
        ax_s[q * TP + j] = (qx >= 0 && qx < Ws) ? Ax[(long)qx * T + j] : 0.f;
    }
    __syncthreads();
    // pixel row ly (relative to F*qy0) is read by the pooled rows hi, hi-1, .. hi-S+1 (relative to qy0), hi = (ly + OFF) / F, at tap
    // ly + OFF - F*(hi - k): in [0, F) for k = 0, F more for each step down; hi - k + S/2 in [0, PH) is the row of the halo
    for (int i = threadIdx.x; i < PX * PH; i += 256) {
        const int ly = i / PH, px = i - ly * PH;
        const int hi = (ly + OFF) / F;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < S; ++k) {
            const int qr = hi - k + S / 2;
            acc += ay_s[qr * TP + (ly + OFF - F * (hi - k))] * p_s[qr * PH + px];
        }
        v_s[i] = acc;
    }
    __syncthreads();
    float* __restrict__ dst = gimg + plane * H * W;
    for (int i = threadIdx.x; i < PX * PX; i += 256) {
        const int ly = i / PX, lx = i - ly * PX;
        const int y = F * qy0 + ly, x = F * qx0 + lx;
        if (y < H && x < W) {
            const int hi = (lx + OFF) / F;
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const int qr = hi - k + S / 2;
                acc += ax_s[qr * TP + (lx + OFF - F * (hi - k))] * v_s[ly * PH + qr];
            }
            dst[(long)y * W + x] = gs * acc;
        }
    }
}

struct Geometry {
    int tilesX, tiles;
};

// F, s, the plane and the tables as every entry point needs them
int check_geometry(const char* what, const void* Ay, const void* Ax, int H, int W, int f, int s, Geometry* g) {
    OODGAN_REQUIRE(f == 2 || f == 4 || f == 8 || f == 16, "%s: factor %d: must be 2, 4, 8 or 16", what, f);
    OODGAN_REQUIRE(s == 2 || s == 4 || s == 6, "%s: support %d: must be 2, 4 or 6", what, s);
    OODGAN_REQUIRE(H > 0 && W > 0, "%s: bad shape: a %dx%d plane", what, H, W);
    OODGAN_REQUIRE(H % f == 0 && W % f == 0, "%s: a %dx%d plane is not a multiple of the factor %d", what, H, W, f);
    OODGAN_REQUIRE(Ay && Ax, "%s: null tables", what);
    const int tq = tile_q(f);
    g->tilesX = (W / f + tq - 1) / tq;
    g->tiles = g->tilesX * ((H / f + tq - 1) / tq);
    return OODGAN_OK;
}

// calls `body` with the kernels' <F, S> as integral constants
template <typename Body>
void with_factor_support(int f, int s, Body body) {
#define OODGAN_RS_CASE(F_, S_)       \
    if (f == F_ && s == S_) {        \
        body(std::integral_constant<int, F_>(), std::integral_constant<int, S_>()); \
        return;                      \
    }
    OODGAN_RS_CASE(2, 2) OODGAN_RS_CASE(2, 4) OODGAN_RS_CASE(2, 6)
    OODGAN_RS_CASE(4, 2) OODGAN_RS_CASE(4, 4) OODGAN_RS_CASE(4, 6)
    OODGAN_RS_CASE(8, 2) OODGAN_RS_CASE(8, 4) OODGAN_RS_CASE(8, 6)
    OODGAN_RS_CASE(16, 2) OODGAN_RS_CASE(16, 4) OODGAN_RS_CASE(16, 6)
#undef OODGAN_RS_CASE
}

bool kind_ok(int kind) {
    return kind == kSquare || kind == OODGAN_ROBUST_CHARBONNIER || kind == OODGAN_ROBUST_HUBER || kind == OODGAN_ROBUST_GEMAN_MCCLURE;
}
bool scale_ok(float scale) { return scale > 0.f && std::isnormal(scale * scale); }

// Both loss entry points end here: every argument checked (a status, nothing launched), kernel one, the mean over its partials, then —
// with gimg — kernel two.  loss / row_dev / nrows: the sink as in loss_pixel.hip.
int resampled_pixel_term(const char* what, const float* img, const float* tview, const float* Ay, const float* Ax, float* gimg, float* rs,
                         float* part, float* loss, const int* row_dev, int nrows, int B, int C, int H, int W, int f, int s, int kind,
                         float scale, float grad_mul, void* stream) {
    Geometry g;
    int rc = check_geometry(what, Ay, Ax, H, W, f, s, &g);
    if (rc != OODGAN_OK) return rc;
    OODGAN_REQUIRE(B > 0 && B <= 65535 && C > 0, "%s: bad shape (%d, %d, %d, %d)", what, B, C, H, W);
    OODGAN_REQUIRE(kind_ok(kind), "%s: unknown kind %d", what, kind);
    OODGAN_REQUIRE(kind == kSquare || scale_ok(scale), "%s: scale %g: must be finite and > 0, with a normal float32 square", what, (double)scale);
    const long nparts = (long)g.tiles * C, nblocks2 = nparts * B;
    OODGAN_REQUIRE(nblocks2 <= 0x7fffffffL, "%s: %ld tiles: too many for one grid", what, nblocks2);
    const long n = (long)C * (H / f) * (W / f);
    const float s2 = scale * scale;
    const float gs = kind == kSquare ? grad_mul * 2.0f / (float)n : grad_mul / (float)n;
    count_dispatch(OODGAN_DC_RESAMPLED_PIXEL);
    with_factor_support(f, s, [&](auto Fc, auto Sc) {
        hipLaunchKernelGGL((resample_fwd_kernel<decltype(Fc)::value, decltype(Sc)::value, true>), dim3((unsigned)nparts, B), dim3(256), 0, as_stream(stream), img, tview, Ay, Ax,
                           rs, part, C, H, W, g.tilesX, g.tiles, (int)nparts, kind, scale, s2);
    });
    rc = check_launch(what);
    if (rc != OODGAN_OK) return rc;
    hipLaunchKernelGGL(mean_finish_kernel<>, dim3(B), dim3(64), 0, as_stream(stream), part, loss, (int)nparts, 1.0f / (float)n, row_dev, nrows);
    rc = check_launch((std::string(what) + "_finish").c_str());
    if (rc != OODGAN_OK || !gimg) return rc;
    with_factor_support(f, s, [&](auto Fc, auto Sc) {
        hipLaunchKernelGGL((resample_bwd_kernel<decltype(Fc)::value, decltype(Sc)::value>), dim3((unsigned)nblocks2), dim3(256), 0, as_stream(stream), rs, Ay, Ax, gimg, H, W,
                           g.tilesX, g.tiles, gs);
    });
    return check_launch((std::string(what) + "_bwd").c_str());
}

}  // namespace

extern "C" int oodgan_resample_fwd(const float* img, const float* Ay, const float* Ax, float* out, int BC, int H, int W, int F, int s,
                                   void* stream) {
    OODGAN_REQUIRE(img && out, "resample_fwd: bad args");
    Geometry g;
    int rc = check_geometry("resample_fwd", Ay, Ax, H, W, F, s, &g);
    if (rc != OODGAN_OK) return rc;
    OODGAN_REQUIRE(BC > 0, "resample_fwd: bad shape: %d planes", BC);
    const long nblocks = (long)g.tiles * BC;
    OODGAN_REQUIRE(nblocks <= 0x7fffffffL, "resample_fwd: %ld tiles: too many for one grid", nblocks);
    with_factor_support(F, s, [&](auto Fc, auto Sc) {
        hipLaunchKernelGGL((resample_fwd_kernel<decltype(Fc)::value, decltype(Sc)::value, false>), dim3((unsigned)nblocks, 1), dim3(256), 0, as_stream(stream), img,
                           (const float*)nullptr, Ay, Ax, out, (float*)nullptr, BC, H, W, g.tilesX, g.tiles, 0, 0, 0.f, 0.f);
    });
    return check_launch("resample_fwd");
}

// part of the resampled term: (B, oodgan_resampled_pixel_loss_nparts(C, H, W, F)), one partial per tile and plane; 0: bad factor or shape
extern "C" int oodgan_resampled_pixel_loss_nparts(int C, int H, int W, int F) {
    if (C <= 0 || H <= 0 || W <= 0 || !(F == 2 || F == 4 || F == 8 || F == 16) || H % F || W % F) return 0;
    const int tq = tile_q(F);
    const long n = (long)C * ((W / F + tq - 1) / tq) * ((H / F + tq - 1) / tq);
    return n <= 0x7fffffffL ? (int)n : 0;
}

extern "C" int oodgan_resampled_pixel_loss_fwd_bwd(const float* img, const float* target_view, const float* Ay, const float* Ax, float* gimg,
                                                   float* r_scratch, float* part, float* loss, int B, int C, int H, int W, int F, int s,
                                                   int kind, float scale, float grad_mul, void* stream) {
    OODGAN_REQUIRE(img && target_view && r_scratch && part && loss, "resampled_pixel_loss: bad args");
    return resampled_pixel_term("resampled_pixel_loss", img, target_view, Ay, Ax, gimg, r_scratch, part, loss, nullptr, 1, B, C, H, W, F, s, kind,
                                scale, grad_mul, stream);
}

extern "C" int oodgan_resampled_pixel_loss_fwd_bwd_row(const float* img, const float* target_view, const float* Ay, const float* Ax,
                                                       float* gimg, float* r_scratch, float* part, float* loss_table, const int* row_dev,
                                                       int nrows, int B, int C, int H, int W, int F, int s, int kind, float scale,
                                                       float grad_mul, void* stream) {
    OODGAN_REQUIRE(img && target_view && r_scratch && part && loss_table && row_dev && nrows > 0, "resampled_pixel_loss_row: bad args");
    return resampled_pixel_term("resampled_pixel_loss", img, target_view, Ay, Ax, gimg, r_scratch, part, loss_table, row_dev, nrows, B, C, H, W, F,
                                s, kind, scale, grad_mul, stream);
}
