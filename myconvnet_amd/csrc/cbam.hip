// cbam.hip — the attention tail of the reference's ResNet-CBAM residual unit (models/resnet_v2_d_cbam.py:159-165, _channel_mask 172-197,
// _spatial_mask 199-211) on [N][H][W][C] NHWC activations: x * channel_mask, then * spatial_mask, without ever storing the product
// xp = round(x * cm).  Everything here is HBM-bound; the budget is 3 full-size reads + 1 write forward, 3 passes backward.
//
//   pools (mcn_global_avgmax_pool_fwd) — the house column layout of bn.hip / gn.hip: a thread owns one 16-byte channel chunk and walks
//       the rows of its (image, row slice) with streaming loads, keeping a running sum AND a running max; the row lanes of a
//       workgroup fold through LDS, the slices in a second tiny kernel in slice order.  One read of x -> [2][N][C] (means, then maxima).
//   chpool (mcn_cbam_chpool_fwd) — the reduction runs over a pixel's CHANNELS, which in NHWC lie across lanes: a pixel owns G lanes,
//       G = the next power of two >= C/vec chunks (<= 64), 64/G pixels share a wave, and sum / max fold with xor-shuffles over exactly
//       those G lanes (lanes past a non-power-of-two chunk count hold the neutral element).  C/vec <= G: one chunk per lane, cm in
//       registers, 4 pixels per trip with the loads first.  C/vec > 64: the wave loops over the pixel's chunks, 4 per trip.
//   apply (mcn_cbam_apply_fwd) — a workgroup owns a band of R full image rows.  It stages the band's 2-channel s window with its K/2
//       halo in LDS as fp32 (zero outside the image: SAME padding), one lane per pixel evaluates the K x K x 2 stencil + bias + sigmoid
//       from LDS (98 MACs per pixel: no MFMA tile would be more than 1/16 full) and leaves sm in LDS and in memory, then the band
//       streams x in the column layout (cm chunk in registers, sm from LDS) and writes y = round(round(x * cm) * sm).
//   backward (mcn_cbam_bwd) — (A) the chpool kernel's other mode: dsm = sum_c dy * xp and the tie count of the channel max per pixel,
//       dt = dsm * sm * (1 - sm); (B) the band kernel again on fp32 tiles of dt and s: ds by the flipped stencil, per-band partial
//       sums of dw / db (one lane per tap walks the band; a second kernel adds the bands in order), and the four per-pixel
//       coefficients of pass C as one 16-byte record; (C) the column layout: dxp = dy * sm + ds0 / C + [xp == max] * ds1 / ties,
//       dx = round(dxp * cm), and per (image, channel) the sums dcm = sum_p dxp * x and the tie count of the spatial max, folded like
//       the pools.  mcn_global_avgmax_pool_bwd then adds the pool gradient to dx in place (the MLP between the two has to run first).
//   No floating-point atomics anywhere: a repeated call is bit-identical.  All per-pixel / per-(image, channel) intermediates are fp32 in
//   caller-owned workspace.
#include "common.h"
#include <math.h>

#define CB_TARGET_BLOCKS 2048       /* workgroups of a column-layout kernel */
#define CB_MAX_SLICES 64            /* row slices per image (workspace sizing) */
#define CB_MAX_K 7
#define CB_MAX_W 512                /* a band is at least one full image row + halo in LDS */
#define CB_TILE_MAX 4096            /* (R + K - 1) * (W + K - 1) positions: 3 fp32 planes = 48 KB in the backward band kernel */
#define CB_BAND_PIXELS 256
#define CB_DW_STRIDE 100            /* floats per band in the dw / db partials: 2 * 7 * 7 taps + bias, padded */

template <typename T, int VEC>
__device__ __forceinline__ void cb_unpack(const Chunk<T>& c, float (&o)[VEC]) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = c.get(i);
}
template <typename T, int VEC>
__device__ __forceinline__ void cb_ld(const T* p, float (&o)[VEC]) { cb_unpack<T, VEC>(load_chunk<T>(p), o); }
// small per-image operands (cm, pools): read by every workgroup of the image, kept cacheable
template <typename T, int VEC>
__device__ __forceinline__ void cb_ldc(const T* p, float (&o)[VEC]) {
    Chunk<T> c;
    *reinterpret_cast<i32x4*>(&c.v) = *reinterpret_cast<const i32x4*>(p);
    cb_unpack<T, VEC>(c, o);
}
template <typename T, int VEC>
__device__ __forceinline__ void cb_st(T* p, const float (&v)[VEC]) {
    Chunk<T> c;
#pragma unroll
    for (int i = 0; i < VEC; ++i) c.set(i, v[i]);
    store_chunk<T>(p, c);
}
template <typename T>
__device__ __forceinline__ float cb_round(float v) { return to_f32(from_f32<T>(v)); }
// xp = round(x * cm): a product of its own (never contracted into a following add), so that every kernel reproduces it bit for bit
template <typename T>
__device__ __forceinline__ float cb_xp(float x, float m) { return cb_round<T>(__fmul_rn(x, m)); }

// ---- column layout (pools, backward pass C, pool gradient) ----------------------------------------------------------------
struct CbLayout {
    int cols, TX, TY, gx, S;   // chunk columns, columns / row lanes per workgroup, column blocks, row slices per image
    long rps;                  // rows per slice (multiple of TY)
};
static CbLayout cb_layout(int N, long HW, int C, int vec) {
    CbLayout L;
    L.cols = C / vec;
    L.TX = L.cols < 256 ? L.cols : 256;
    L.TY = 256 / L.TX;
    L.gx = (L.cols + L.TX - 1) / L.TX;
    const long per_image = (CB_TARGET_BLOCKS + (long)N * L.gx - 1) / ((long)N * L.gx);
    const long most = (HW + (long)L.TY * 4 - 1) / ((long)L.TY * 4);               // >= 4 rows per thread
    long S = per_image < most ? per_image : most;
    if (S > CB_MAX_SLICES) S = CB_MAX_SLICES;
    if (S < 1) S = 1;
    L.rps = ((HW + S - 1) / S + L.TY - 1) / L.TY * L.TY;
    L.S = (int)((HW + L.rps - 1) / L.rps);
    return L;
}

// fold the TY row lanes of a workgroup through LDS (plane 0: sum; plane 1: sum or max) and write part[(row * 2 + {0, 1}) * C + c]
template <int VEC, bool MAX1>
__device__ __forceinline__ void cb_fold_rows(float* red, const float (&s1)[VEC], const float (&s2)[VEC], int tx, int ty, int TX, int TY, bool col_ok,
                                             float* __restrict__ part, long row, int C, int c0) {
    float* r1p = red;                       // [TY][TX * VEC]
    float* r2p = red + 256 * VEC;
    if (ty < TY) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            r1p[(ty * TX + tx) * VEC + i] = s1[i];
            r2p[(ty * TX + tx) * VEC + i] = s2[i];
        }
    }
    __syncthreads();
    if (ty == 0 && col_ok) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            float a = 0.f, b = MAX1 ? -INFINITY : 0.f;
            for (int k = 0; k < TY; ++k) {
                a += r1p[(k * TX + tx) * VEC + i];
                const float q = r2p[(k * TX + tx) * VEC + i];
                b = MAX1 ? fmaxf(b, q) : b + q;
            }
            part[(row * 2 + 0) * C + c0 + i] = a;
            part[(row * 2 + 1) * C + c0 + i] = b;
        }
    }
}

// part[((n * S + s) * 2 + {0, 1}) * C + c] = sum, max of x over the slice's rows
template <typename T, int VEC>
__global__ __launch_bounds__(256) void cb_pool_partial_kernel(const T* __restrict__ x, float* __restrict__ part, long HW, int C, int TX, int TY, int S, long rps) {
    extern __shared__ float red[];
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int col = blockIdx.y * TX + tx;
    const long n = blockIdx.x / S;
    const int s = blockIdx.x % S;
    const bool col_ok = col * VEC < C;
    float s1[VEC], s2[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) { s1[i] = 0.f; s2[i] = -INFINITY; }
    if (ty < TY && col_ok) {
        const T* xi = x + n * HW * C + (long)col * VEC;
        const long r0 = (long)s * rps, r1 = min(HW, r0 + rps);
        auto row = [&](const float* v) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                s1[i] += v[i];
                s2[i] = fmaxf(s2[i], v[i]);
            }
        };
        constexpr int U = 4;                  // rows per trip, loads first
        long r = r0 + ty;
        for (; r + (long)(U - 1) * TY < r1; r += (long)U * TY) {
            float v[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) cb_ld<T, VEC>(xi + (r + (long)u * TY) * C, v[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) row(v[u]);
        }
        for (; r < r1; r += TY) {
            float v[VEC];
            cb_ld<T, VEC>(xi + r * C, v);
            row(v);
        }
    }
    cb_fold_rows<VEC, true>(red, s1, s2, tx, ty, TX, TY, col_ok, part, blockIdx.x, C, col * VEC);
}

// slices merged in slice order, one thread per (image, channel): MODE 0 -> pools[0][n][c] = round(sum / HW), pools[1][n][c] = max (T);
// MODE 1 -> o0 = round(sum of plane 0) (T: dcm), o1 = sum of plane 1 (fp32: tie counts, may be null)
template <typename T, int MODE>
__global__ __launch_bounds__(256) void cb_slices_kernel(const float* __restrict__ part, T* __restrict__ o0, void* __restrict__ o1, long NC, int C, int S, float hw) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= NC) return;
    const long n = i / C;
    const int c = (int)(i % C);
    float a = 0.f, b = MODE == 0 ? -INFINITY : 0.f;
    for (int s = 0; s < S; ++s) {
        a += part[((n * S + s) * 2 + 0) * C + c];
        const float q = part[((n * S + s) * 2 + 1) * C + c];
        b = MODE == 0 ? fmaxf(b, q) : b + q;
    }
    if (MODE == 0) {
        o0[i] = from_f32<T>(a / hw);
        ((T*)o1)[i] = from_f32<T>(b);
    } else {
        o0[i] = from_f32<T>(a);
        if (o1) ((float*)o1)[i] = b;
    }
}

// cm[n][c] = round(sigmoid(a[n][c] + a[N + n][c])) (models/resnet_v2_d_cbam.py:192); backward: both halves receive dcm * cm * (1 - cm)
template <typename T>
__global__ __launch_bounds__(256) void cb_pair_sigmoid_kernel(const T* __restrict__ a, T* __restrict__ cm, long NC) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= NC) return;
    cm[i] = from_f32<T>(fast_sigmoid(to_f32(a[i]) + to_f32(a[NC + i])));
}
template <typename T>
__global__ __launch_bounds__(256) void cb_pair_sigmoid_bwd_kernel(const T* __restrict__ dcm, const T* __restrict__ cm, T* __restrict__ da, long NC) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= NC) return;
    const float m = to_f32(cm[i]);
    const T d = from_f32<T>(to_f32(dcm[i]) * m * (1.f - m));
    da[i] = d;
    da[NC + i] = d;
}

// ---- per-pixel channel reductions: G lanes per pixel ------------------------------------------------------------------------
// forward : s[n][p][0] = round(mean_c xp), s[n][p][1] = max_c xp, xp = round(x * cm)
// backward: dt[n][p] = (sum_c dy * xp) * sm * (1 - sm), ties[n][p] = #{c : xp == s[n][p][1]}
template <typename T, int VEC, bool BWD>
__global__ __launch_bounds__(256) void cb_pixel_kernel(const T* __restrict__ x, const T* __restrict__ cm, const T* __restrict__ dy, const T* __restrict__ s_in,
                                                       const T* __restrict__ sm, T* __restrict__ s_out, float* __restrict__ dt, float* __restrict__ ties, long HW, int C,
                                                       int G, int bpi, long ppb) {
    const int cols = C / VEC;
    const int lg = threadIdx.x % G, grp = threadIdx.x / G, ngrp = 256 / G;
    const long n = blockIdx.x / bpi;
    const long p0 = (long)(blockIdx.x % bpi) * ppb, p1 = min(HW, p0 + ppb);
    const T* xi = x + n * HW * C;
    const T* gi = BWD ? dy + n * HW * C : nullptr;
    const T* cmn = cm + n * C;
    // one chunk of one pixel: a += xp (fwd) / dy * xp (bwd); b = max(b, xp) (fwd) / b += [xp == smax] (bwd)
    auto chunk = [&](const float* v, const float* g, const float* m, float smax, float& a, float& b) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float xp = cb_xp<T>(v[i], m[i]);
            if (BWD) {
                a = fmaf(g[i], xp, a);
                b += xp == smax ? 1.f : 0.f;
            } else {
                a += xp;
                b = fmaxf(b, xp);
            }
        }
    };
    auto finish = [&](long p, float a, float b) {                       // fold over the pixel's G lanes; lane 0 writes
        for (int o = 1; o < G; o <<= 1) {
            a += __shfl_xor(a, o);
            const float q = __shfl_xor(b, o);
            b = BWD ? b + q : fmaxf(b, q);
        }
        if (lg == 0 && p < p1) {
            const long q = n * HW + p;
            if (BWD) {
                const float sg = to_f32(sm[q]);
                dt[q] = a * sg * (1.f - sg);
                ties[q] = b;
            } else {
                s_out[q * 2 + 0] = from_f32<T>(a / (float)C);      // (a true division, one per pixel: an exactly representable mean stays exact)
                s_out[q * 2 + 1] = from_f32<T>(b);
            }
        }
    };
    constexpr int U = 4;
    if (cols <= G) {
        // one chunk per lane: cm stays in registers, U pixels per trip with the loads first (trip count uniform over the workgroup)
        const bool on = lg < cols;
        float m[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) m[i] = 0.f;
        if (on) cb_ldc<T, VEC>(cmn + lg * VEC, m);
        for (long base = p0; base < p1; base += (long)ngrp * U) {
            float v[U][VEC], g[U][VEC], smax[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long p = base + grp + (long)u * ngrp;
                const bool ok = on && p < p1;
#pragma unroll
                for (int i = 0; i < VEC; ++i) v[u][i] = g[u][i] = 0.f;
                smax[u] = 0.f;
                if (ok) {
                    cb_ld<T, VEC>(xi + p * C + lg * VEC, v[u]);
                    if (BWD) {
                        cb_ld<T, VEC>(gi + p * C + lg * VEC, g[u]);
                        smax[u] = to_f32(s_in[(n * HW + p) * 2 + 1]);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long p = base + grp + (long)u * ngrp;
                float a = 0.f, b = BWD ? 0.f : -INFINITY;
                if (on && p < p1) chunk(v[u], g[u], m, smax[u], a, b);
                finish(p, a, b);
            }
        }
    } else {
        // more chunks than a wave has lanes (G = 64): the wave loops over its pixel's chunks, U per trip
        for (long base = p0; base < p1; base += ngrp) {
            const long p = base + grp;
            const bool pix = p < p1;
            const float smax = (BWD && pix) ? to_f32(s_in[(n * HW + p) * 2 + 1]) : 0.f;
            float a = 0.f, b = BWD ? 0.f : -INFINITY;
            for (int k0 = 0; k0 < cols; k0 += G * U) {
                float v[U][VEC], g[U][VEC], m[U][VEC];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = k0 + u * G + lg;
                    if (pix && k < cols) {
                        cb_ld<T, VEC>(xi + p * C + k * VEC, v[u]);
                        if (BWD) cb_ld<T, VEC>(gi + p * C + k * VEC, g[u]);
                        cb_ldc<T, VEC>(cmn + k * VEC, m[u]);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int k = k0 + u * G + lg;
                    if (pix && k < cols) chunk(v[u], g[u], m[u], smax, a, b);
                }
            }
            finish(p, a, b);
        }
    }
}

// ---- band kernels: the K x K x 2 stencil from LDS ---------------------------------------------------------------------------------
struct CbBands { int R, bands; };
static CbBands cb_bands(int N, int H, int W, int K) {
    int R = (CB_BAND_PIXELS + W - 1) / W;
    if (R > H) R = H;
    while (R > 1 && (long)N * ((H + R - 1) / R) < CB_TARGET_BLOCKS / 2) R = (R + 1) / 2;      // small batches: narrower bands fill the chip
    while (R > 1 && (R + K - 1) * (W + K - 1) > CB_TILE_MAX) --R;
    CbBands b = {R, (H + R - 1) / R};
    return b;
}

// forward: sm = round(sigmoid(round(conv_KxK_SAME(s, round(w)) + b))) for the band's pixels, then y = round(round(x * cm) * sm)
template <typename T, int VEC>
__global__ __launch_bounds__(256) void cb_apply_kernel(const T* __restrict__ x, const T* __restrict__ cm, const T* __restrict__ s, const float* __restrict__ w,
                                                       const float* __restrict__ bias, T* __restrict__ sm_out, T* __restrict__ y, int H, int W, int C, int K, int R,
                                                       int bands) {
    extern __shared__ float lds[];
    const int P = K / 2, TH = R + K - 1, TW = W + K - 1;
    float* tile = lds;                        // [TH][TW][2]
    float* smv = tile + TH * TW * 2;          // [R * W]
    float* wq = smv + R * W;                  // [K][K][2]
    const long n = blockIdx.x / bands;
    const int r0 = (blockIdx.x % bands) * R, r1 = min(H, r0 + R);
    for (int i = threadIdx.x; i < TH * TW; i += 256) {
        const int gy = r0 + i / TW - P, gx = i % TW - P;
        float v0 = 0.f, v1 = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const long q = ((n * H + gy) * W + gx) * 2;
            v0 = to_f32(s[q]);
            v1 = to_f32(s[q + 1]);
        }
        tile[i * 2] = v0;
        tile[i * 2 + 1] = v1;
    }
    for (int i = threadIdx.x; i < 2 * K * K; i += 256) wq[i] = cb_round<T>(w[i]);            // the per-use cast of the fp32 master (convnet.py:1421)
    __syncthreads();
    const int npix = (r1 - r0) * W;
    const long pix0 = (n * H + r0) * W;
    for (int i = threadIdx.x; i < npix; i += 256) {
        const int py = i / W, px = i % W;
        float acc = bias ? bias[0] : 0.f;
        for (int a = 0; a < K; ++a)
            for (int c = 0; c < K; ++c) {
                const int t = ((py + a) * TW + px + c) * 2, k = (a * K + c) * 2;
                acc = fmaf(tile[t], wq[k], acc);
                acc = fmaf(tile[t + 1], wq[k + 1], acc);
            }
        const T sg = from_f32<T>(fast_sigmoid(cb_round<T>(acc)));
        smv[i] = to_f32(sg);
        sm_out[pix0 + i] = sg;
    }
    __syncthreads();
    const int cols = C / VEC, TX = cols < 256 ? cols : 256, TY = 256 / TX;
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    if (ty >= TY) return;
    const T* xb = x + pix0 * C;
    T* yb = y + pix0 * C;
    for (int cb = 0; cb < cols; cb += TX) {
        const int col = cb + tx;
        if (col >= cols) continue;
        float m[VEC];
        cb_ldc<T, VEC>(cm + n * C + col * VEC, m);
        auto row = [&](float (&v)[VEC], int p) {
            const float sg = smv[p];
#pragma unroll
            for (int i = 0; i < VEC; ++i) v[i] = cb_xp<T>(v[i], m[i]) * sg;
            cb_st<T, VEC>(yb + (long)p * C + col * VEC, v);
        };
        constexpr int U = 4;
        int p = ty;
        for (; p + (U - 1) * TY < npix; p += U * TY) {
            float v[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) cb_ld<T, VEC>(xb + (long)(p + u * TY) * C + col * VEC, v[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) row(v[u], p + u * TY);
        }
        for (; p < npix; p += TY) {
            float v[VEC];
            cb_ld<T, VEC>(xb + (long)p * C + col * VEC, v);
            row(v, p);
        }
    }
}

// backward: ds[p][j] = sum_taps dt[p - tap] * round(w)[tap][j]; coef[p] = {sm, ds0 / C, ds1 / ties, max_c xp} for pass C;
// dwpart[band][tap * 2 + j] = sum_{p in band} dt[p] * s[p + tap][j], dwpart[band][2 K K] = sum dt
template <typename T>
__global__ __launch_bounds__(256) void cb_stencil_bwd_kernel(const float* __restrict__ dt, const float* __restrict__ ties, const T* __restrict__ s, const T* __restrict__ sm,
                                                             const float* __restrict__ w, f32x4* __restrict__ coef, float* __restrict__ dwpart, int H, int W, int C,
                                                             int K, int R, int bands) {
    extern __shared__ float lds[];
    const int P = K / 2, TH = R + K - 1, TW = W + K - 1;
    float* tile = lds;                        // [TH][TW][2]  s
    float* dtile = tile + TH * TW * 2;        // [TH][TW]     dt
    float* wq = dtile + TH * TW;              // [K][K][2]
    const long n = blockIdx.x / bands;
    const int r0 = (blockIdx.x % bands) * R, r1 = min(H, r0 + R);
    for (int i = threadIdx.x; i < TH * TW; i += 256) {
        const int gy = r0 + i / TW - P, gx = i % TW - P;
        float v0 = 0.f, v1 = 0.f, d = 0.f;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const long q = (n * H + gy) * W + gx;
            v0 = to_f32(s[q * 2]);
            v1 = to_f32(s[q * 2 + 1]);
            d = dt[q];
        }
        tile[i * 2] = v0;
        tile[i * 2 + 1] = v1;
        dtile[i] = d;
    }
    for (int i = threadIdx.x; i < 2 * K * K; i += 256) wq[i] = cb_round<T>(w[i]);
    __syncthreads();
    const int npix = (r1 - r0) * W;
    const long pix0 = (n * H + r0) * W;
    const float inv_c = 1.f / (float)C;
    for (int i = threadIdx.x; i < npix; i += 256) {
        const int py = i / W, px = i % W;
        float d0 = 0.f, d1 = 0.f;
        for (int a = 0; a < K; ++a)
            for (int c = 0; c < K; ++c) {
                const float d = dtile[(py + K - 1 - a) * TW + px + K - 1 - c];
                d0 = fmaf(d, wq[(a * K + c) * 2], d0);
                d1 = fmaf(d, wq[(a * K + c) * 2 + 1], d1);
            }
        const f32x4 r = {to_f32(sm[pix0 + i]), d0 * inv_c, d1 / ties[pix0 + i], tile[((py + P) * TW + px + P) * 2 + 1]};
        coef[pix0 + i] = r;
    }
    if (threadIdx.x <= 2 * K * K) {           // one lane per tap (+ one for the bias) walks the band's pixels in order
        const int t = threadIdx.x, j = t & 1, a = (t >> 1) / K, c = (t >> 1) % K;
        const bool is_b = t == 2 * K * K;
        float acc = 0.f;
        for (int i = 0; i < npix; ++i) {
            const int py = i / W, px = i % W;
            const float d = dtile[(py + P) * TW + px + P];
            acc = is_b ? acc + d : fmaf(d, tile[((py + a) * TW + px + c) * 2 + j], acc);
        }
        dwpart[(long)blockIdx.x * CB_DW_STRIDE + t] = acc;
    }
}

// dw[t] = grad_scale * sum over the bands (in order; double) of dwpart[band][t]; one workgroup per tap, the last one is db
__global__ __launch_bounds__(256) void cb_dw_kernel(const float* __restrict__ dwpart, long nb, int taps, float* __restrict__ dw, float* __restrict__ db, float grad_scale) {
    __shared__ double sh[4];
    const int t = blockIdx.x;
    double a = 0.0;
    for (long k = threadIdx.x; k < nb; k += 256) a += (double)dwpart[k * CB_DW_STRIDE + t];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float v = (float)(sh[0] + sh[1] + sh[2] + sh[3]) * grad_scale;
        if (t < taps) { if (dw) dw[t] = v; }
        else if (db) db[0] = v;
    }
}

// pass C: dxp = dy * sm + ds0 / C + [xp == max_c xp] * ds1 / ties; dx = round(dxp * cm);
// part[((n * S + s) * 2 + {0, 1}) * C + c] = sum dxp * x, #{p : x == pmax[n][c]} over the slice's rows
template <typename T, int VEC>
__global__ __launch_bounds__(256) void cb_bwd_dx_kernel(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ cm, const f32x4* __restrict__ coef,
                                                        const T* __restrict__ pmax, T* __restrict__ dx, float* __restrict__ part, long HW, int C, int TX, int TY, int S,
                                                        long rps) {
    extern __shared__ float red[];
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int col = blockIdx.y * TX + tx;
    const long n = blockIdx.x / S;
    const int s = blockIdx.x % S;
    const bool col_ok = col * VEC < C;
    float s1[VEC], s2[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s1[i] = s2[i] = 0.f;
    if (ty < TY && col_ok) {
        float m[VEC], pm[VEC];
        cb_ldc<T, VEC>(cm + n * C + col * VEC, m);
#pragma unroll
        for (int i = 0; i < VEC; ++i) pm[i] = NAN;                       // (no pools: nothing compares equal)
        if (pmax) cb_ldc<T, VEC>(pmax + n * C + col * VEC, pm);
        const long base = n * HW * C + (long)col * VEC;
        const f32x4* cf = coef + n * HW;
        const long r0 = (long)s * rps, r1 = min(HW, r0 + rps);
        auto row = [&](const float* g, float (&v)[VEC], const f32x4 k, long off) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float xv = v[i];
                const float xp = cb_xp<T>(xv, m[i]);
                const float d = fmaf(g[i], k[0], k[1]) + (xp == k[3] ? k[2] : 0.f);
                s1[i] = fmaf(d, xv, s1[i]);
                s2[i] += xv == pm[i] ? 1.f : 0.f;
                v[i] = d * m[i];
            }
            cb_st<T, VEC>(dx + off, v);
        };
        constexpr int U = 2;
        long r = r0 + ty;
        for (; r + (long)(U - 1) * TY < r1; r += (long)U * TY) {
            float g[U][VEC], v[U][VEC];
            f32x4 k[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long off = base + (r + (long)u * TY) * C;
                cb_ld<T, VEC>(dy + off, g[u]);
                cb_ld<T, VEC>(x + off, v[u]);
                k[u] = cf[r + (long)u * TY];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) row(g[u], v[u], k[u], base + (r + (long)u * TY) * C);
        }
        for (; r < r1; r += TY) {
            float g[VEC], v[VEC];
            cb_ld<T, VEC>(dy + base + r * C, g);
            cb_ld<T, VEC>(x + base + r * C, v);
            row(g, v, cf[r], base + r * C);
        }
    }
    cb_fold_rows<VEC, false>(red, s1, s2, tx, ty, TX, TY, col_ok, part, blockIdx.x, C, col * VEC);
}

// gradient of the two global pools: dx (+)= dpool[0][n][c] / HW + [x == pools[1][n][c]] * dpool[1][n][c] / ties[n][c]
template <typename T, int VEC, bool ACC>
__global__ __launch_bounds__(256) void cb_pool_bwd_kernel(const T* __restrict__ dpool, const T* __restrict__ x, const T* __restrict__ pools, const float* __restrict__ ties,
                                                          T* __restrict__ dx, long NC, long HW, int C, int TX, int TY, int S, long rps, float inv_hw) {
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int col = blockIdx.y * TX + tx;
    if (ty >= TY || col * VEC >= C) return;
    const long n = blockIdx.x / S;
    const int s = blockIdx.x % S;
    float da[VEC], dm[VEC], pm[VEC];
    cb_ldc<T, VEC>(dpool + n * C + col * VEC, da);
    cb_ldc<T, VEC>(dpool + NC + n * C + col * VEC, dm);
    cb_ldc<T, VEC>(pools + NC + n * C + col * VEC, pm);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        da[i] *= inv_hw;
        dm[i] /= ties[n * C + col * VEC + i];
    }
    const long base = n * HW * C + (long)col * VEC;
    const long r0 = (long)s * rps, r1 = min(HW, r0 + rps);
    auto row = [&](const float* v, float (&d)[VEC], long off) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) d[i] = (ACC ? d[i] : 0.f) + (da[i] + (v[i] == pm[i] ? dm[i] : 0.f));
        cb_st<T, VEC>(dx + off, d);
    };
    constexpr int U = 2;
    long r = r0 + ty;
    for (; r + (long)(U - 1) * TY < r1; r += (long)U * TY) {
        float v[U][VEC], d[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long off = base + (r + (long)u * TY) * C;
            cb_ld<T, VEC>(x + off, v[u]);
            if (ACC) cb_ld<T, VEC>(dx + off, d[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) row(v[u], d[u], base + (r + (long)u * TY) * C);
    }
    for (; r < r1; r += TY) {
        float v[VEC], d[VEC];
        cb_ld<T, VEC>(x + base + r * C, v);
        if (ACC) cb_ld<T, VEC>(dx + base + r * C, d);
        row(v, d, base + r * C);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static size_t cb_parts_bytes(int N, long HW, int C) {
    const CbLayout a = cb_layout(N, HW, C, 4), b = cb_layout(N, HW, C, 8);
    return align_up((size_t)N * (a.S > b.S ? a.S : b.S) * 2 * C * sizeof(float), 256);
}
extern "C" size_t mcn_global_avgmax_pool_workspace_bytes(int32_t N, int64_t HW, int32_t C) {
    if (N <= 0 || HW <= 0 || C <= 0) return 0;
    return cb_parts_bytes(N, HW, C);
}
// [slice partials | dt | per-pixel ties | coef (16 bytes per pixel) | dw partials]
extern "C" size_t mcn_cbam_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t K) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || K <= 0 || K > CB_MAX_K) return 0;
    const size_t px = align_up((size_t)N * H * W * sizeof(float), 256);
    return cb_parts_bytes(N, (long)H * W, C) + 6 * px + align_up((size_t)N * H * CB_DW_STRIDE * sizeof(float), 256);      // (bands <= H)
}

static int cb_check(const char* who, long N, long H, long W, long C, int K, mcn_dtype dtype) {
    if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || N * H * W > 0x7fffffffL || N * H * W * C <= 0) MCN_FAIL(MCN_E_BADARG, "%s: bad argument (N=%ld H=%ld W=%ld C=%ld)", who, N, H, W, C);
    if (K < 1 || K > CB_MAX_K || !(K & 1)) MCN_FAIL(MCN_E_BADARG, "%s: the kernel size must be odd and <= %d (K=%d)", who, CB_MAX_K, K);
    if (!mcn_dtype_ok(dtype)) MCN_FAIL(MCN_E_UNSUPPORTED, "%s: dtype %d unsupported", who, (int)dtype);
    if (C % (dtype == MCN_F32 ? 4 : 8)) MCN_FAIL(MCN_E_UNSUPPORTED, "%s: C = %ld is not a multiple of the 16-byte chunk (%d elements)", who, C, dtype == MCN_F32 ? 4 : 8);
    if (W > CB_MAX_W) MCN_FAIL(MCN_E_UNSUPPORTED, "%s: W = %ld: one image row with its halo does not fit the LDS tile (W <= %d)", who, W, CB_MAX_W);
    return MCN_OK;
}
#define CB_DISPATCH(F, ...)                                           \
    do {                                                              \
        if (dtype == MCN_F32) return F<float, 4>(__VA_ARGS__);        \
        if (dtype == MCN_BF16) return F<bf16_t, 8>(__VA_ARGS__);      \
        return F<f16_t, 8>(__VA_ARGS__);                              \
    } while (0)

template <typename T, int VEC>
static int cb_pool_fwd_t(const void* x, void* pools, int N, long HW, int C, void* ws, hipStream_t st) {
    const CbLayout L = cb_layout(N, HW, C, VEC);
    float* part = (float*)ws;
    hipLaunchKernelGGL((cb_pool_partial_kernel<T, VEC>), dim3((unsigned)((long)N * L.S), L.gx), dim3(256), 2 * 256 * VEC * sizeof(float), st, (const T*)x, part, HW, C, L.TX,
                       L.TY, L.S, L.rps);
    MCN_CHECK_LAUNCH();
    const long NC = (long)N * C;
    hipLaunchKernelGGL((cb_slices_kernel<T, 0>), dim3((unsigned)((NC + 255) / 256)), dim3(256), 0, st, (const float*)part, (T*)pools, (void*)((T*)pools + NC), NC, C, L.S,
                       (float)HW);
    MCN_CHECK_LAUNCH();
    return MCN_OK;
}
extern "C" int mcn_global_avgmax_pool_fwd(const void* x, void* pools, int32_t N, int64_t HW, int32_t C, mcn_dtype dtype, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !pools) MCN_FAIL(MCN_E_BADARG, "global_avgmax_pool_fwd: null tensor");
    const int rc = cb_check("global_avgmax_pool_fwd", N, HW, 1, C, 1, dtype);
    if (rc != MCN_OK) return rc;
    if (!ws || ws_bytes < mcn_global_avgmax_pool_workspace_bytes(N, HW, C)) MCN_FAIL(MCN_E_WORKSPACE, "global_avgmax_pool_fwd: workspace too small");
    CB_DISPATCH(cb_pool_fwd_t, x, pools, N, HW, C, ws, (hipStream_t)stream);
}

template <typename T, int VEC>
static int cb_pool_bwd_t(const void* dpool, const void* x, const void* pools, const float* ties, void* dx, int acc, int N, long HW, int C, hipStream_t st) {
    const CbLayout L = cb_layout(N, HW, C, VEC);
    const dim3 grid((unsigned)((long)N * L.S), L.gx), block(256);
    const long NC = (long)N * C;
    if (acc) hipLaunchKernelGGL((cb_pool_bwd_kernel<T, VEC, true>), grid, block, 0, st, (const T*)dpool, (const T*)x, (const T*)pools, ties, (T*)dx, NC, HW, C, L.TX, L.TY, L.S, L.rps, 1.f / (float)HW);
    else hipLaunchKernelGGL((cb_pool_bwd_kernel<T, VEC, false>), grid, block, 0, st, (const T*)dpool, (const T*)x, (const T*)pools, ties, (T*)dx, NC, HW, C, L.TX, L.TY, L.S, L.rps, 1.f / (float)HW);
    MCN_CHECK_LAUNCH();
    return MCN_OK;
}
extern "C" int mcn_global_avgmax_pool_bwd(const void* dpool, const void* x, const void* pools, const float* ties, void* dx, int32_t accumulate, int32_t N, int64_t HW,
                                          int32_t C, mcn_dtype dtype, void* stream) {
    if (!dpool || !x || !pools || !ties || !dx) MCN_FAIL(MCN_E_BADARG, "global_avgmax_pool_bwd: null tensor");
    const int rc = cb_check("global_avgmax_pool_bwd", N, HW, 1, C, 1, dtype);
    if (rc != MCN_OK) return rc;
    CB_DISPATCH(cb_pool_bwd_t, dpool, x, pools, ties, dx, accumulate, N, HW, C, (hipStream_t)stream);
}

template <typename T, int VEC>
static int cb_pair_t(const void* a, const void* cm, void* o, bool bwd, long NC, hipStream_t st) {
    const dim3 grid((unsigned)((NC + 255) / 256)), block(256);
    if (bwd) hipLaunchKernelGGL((cb_pair_sigmoid_bwd_kernel<T>), grid, block, 0, st, (const T*)a, (const T*)cm, (T*)o, NC);
    else hipLaunchKernelGGL((cb_pair_sigmoid_kernel<T>), grid, block, 0, st, (const T*)a, (T*)o, NC);
    MCN_CHECK_LAUNCH();
    return MCN_OK;
}
extern "C" int mcn_pair_sigmoid_fwd(const void* a, void* cm, int32_t N, int32_t C, mcn_dtype dtype, void* stream) {
    if (!a || !cm) MCN_FAIL(MCN_E_BADARG, "pair_sigmoid_fwd: null tensor");
    if (N <= 0 || C <= 0) MCN_FAIL(MCN_E_BADARG, "pair_sigmoid_fwd: bad argument (N=%d C=%d)", N, C);
    if (!mcn_dtype_ok(dtype)) MCN_FAIL(MCN_E_UNSUPPORTED, "pair_sigmoid_fwd: dtype %d unsupported", (int)dtype);
    CB_DISPATCH(cb_pair_t, a, nullptr, cm, false, (long)N * C, (hipStream_t)stream);
}
extern "C" int mcn_pair_sigmoid_bwd(const void* dcm, const void* cm, void* da, int32_t N, int32_t C, mcn_dtype dtype, void* stream) {
    if (!dcm || !cm || !da) MCN_FAIL(MCN_E_BADARG, "pair_sigmoid_bwd: null tensor");
    if (N <= 0 || C <= 0) MCN_FAIL(MCN_E_BADARG, "pair_sigmoid_bwd: bad argument (N=%d C=%d)", N, C);
    if (!mcn_dtype_ok(dtype)) MCN_FAIL(MCN_E_UNSUPPORTED, "pair_sigmoid_bwd: dtype %d unsupported", (int)dtype);
    CB_DISPATCH(cb_pair_t, dcm, cm, da, true, (long)N * C, (hipStream_t)stream);
}

// lanes per pixel and the pixel split of cb_pixel_kernel
static void cb_pixel_plan(int N, long HW, int cols, int* G, int* bpi, long* ppb) {
    int g = 1;
    while (g < cols && g < 64) g <<= 1;
    const int ngrp = 256 / g;
    long b = (CB_TARGET_BLOCKS + N - 1) / N;
    const long most = (HW + (long)ngrp * 4 - 1) / ((long)ngrp * 4);
    if (b > most) b = most;
    if (b < 1) b = 1;
    *ppb = (HW + b - 1) / b;
    *bpi = (int)((HW + *ppb - 1) / *ppb);
    *G = g;
}

template <typename T, int VEC>
static int cb_chpool_t(const void* x, const void* cm, void* s, int N, long HW, int C, hipStream_t st) {
    int G, bpi;
    long ppb;
    cb_pixel_plan(N, HW, C / VEC, &G, &bpi, &ppb);
    hipLaunchKernelGGL((cb_pixel_kernel<T, VEC, false>), dim3((unsigned)((long)N * bpi)), dim3(256), 0, st, (const T*)x, (const T*)cm, (const T*)nullptr, (const T*)nullptr,
                       (const T*)nullptr, (T*)s, (float*)nullptr, (float*)nullptr, HW, C, G, bpi, ppb);
    MCN_CHECK_LAUNCH();
    return MCN_OK;
}
extern "C" int mcn_cbam_chpool_fwd(const void* x, const void* cm, void* s, int32_t N, int64_t HW, int32_t C, mcn_dtype dtype, void* stream) {
    if (!x || !cm || !s) MCN_FAIL(MCN_E_BADARG, "cbam_chpool_fwd: null tensor");
    const int rc = cb_check("cbam_chpool_fwd", N, HW, 1, C, 1, dtype);
    if (rc != MCN_OK) return rc;
    CB_DISPATCH(cb_chpool_t, x, cm, s, N, HW, C, (hipStream_t)stream);
}

template <typename T, int VEC>
static int cb_apply_t(const void* x, const void* cm, const void* s, const float* w, const float* b, void* sm, void* y, int N, int H, int W, int C, int K, hipStream_t st) {
    const CbBands B = cb_bands(N, H, W, K);
    const size_t lds = ((size_t)(B.R + K - 1) * (W + K - 1) * 2 + (size_t)B.R * W + 2 * K * K) * sizeof(float);
    hipLaunchKernelGGL((cb_apply_kernel<T, VEC>), dim3((unsigned)((long)N * B.bands)), dim3(256), lds, st, (const T*)x, (const T*)cm, (const T*)s, w, b, (T*)sm, (T*)y, H, W,
                       C, K, B.R, B.bands);
    MCN_CHECK_LAUNCH();
    return MCN_OK;
}
extern "C" int mcn_cbam_apply_fwd(const void* x, const void* cm, const void* s, const float* w, const float* b, void* sm, void* y, int32_t N, int32_t H, int32_t W,
                                  int32_t C, int32_t K, mcn_dtype dtype, void* stream) {
    if (!x || !cm || !s || !w || !sm || !y) MCN_FAIL(MCN_E_BADARG, "cbam_apply_fwd: null tensor");
    const int rc = cb_check("cbam_apply_fwd", N, H, W, C, K, dtype);
    if (rc != MCN_OK) return rc;
    CB_DISPATCH(cb_apply_t, x, cm, s, w, b, sm, y, N, H, W, C, K, (hipStream_t)stream);
}

template <typename T, int VEC>
static int cb_bwd_t(const void* dy, const void* x, const void* cm, const void* s, const void* sm, const float* w, const void* pools, void* dx, void* dcm, float* dw,
                    float* db, float* ties, float grad_scale, int N, int H, int W, int C, int K, void* ws, hipStream_t st) {
    const long HW = (long)H * W;
    const size_t px = align_up((size_t)N * HW * sizeof(float), 256);
    char* p = (char*)ws;
    float* part = (float*)p;
    p += cb_parts_bytes(N, HW, C);
    float* dt = (float*)p;
    float* tp = (float*)(p + px);
    f32x4* coef = (f32x4*)(p + 2 * px);
    float* dwpart = (float*)(p + 6 * px);
    // (A) per-pixel reduction over the channels: dt, ties
    int G, bpi;
    long ppb;
    cb_pixel_plan(N, HW, C / VEC, &G, &bpi, &ppb);
    hipLaunchKernelGGL((cb_pixel_kernel<T, VEC, true>), dim3((unsigned)((long)N * bpi)), dim3(256), 0, st, (const T*)x, (const T*)cm, (const T*)dy, (const T*)s, (const T*)sm,
                       (T*)nullptr, dt, tp, HW, C, G, bpi, ppb);
    MCN_CHECK_LAUNCH();
    // (B) flipped stencil, dw / db partials, per-pixel coefficients
    const CbBands B = cb_bands(N, H, W, K);
    const size_t lds = ((size_t)(B.R + K - 1) * (W + K - 1) * 3 + 2 * K * K) * sizeof(float);
    const long nb = (long)N * B.bands;
    hipLaunchKernelGGL((cb_stencil_bwd_kernel<T>), dim3((unsigned)nb), dim3(256), lds, st, (const float*)dt, (const float*)tp, (const T*)s, (const T*)sm, w, coef, dwpart, H, W,
                       C, K, B.R, B.bands);
    MCN_CHECK_LAUNCH();
    if (dw || db) {
        hipLaunchKernelGGL(cb_dw_kernel, dim3(2 * K * K + 1), dim3(256), 0, st, (const float*)dwpart, nb, 2 * K * K, dw, db, grad_scale);
        MCN_CHECK_LAUNCH();
    }
    // (C) dx, and the per-(image, channel) sums
    const CbLayout L = cb_layout(N, HW, C, VEC);
    hipLaunchKernelGGL((cb_bwd_dx_kernel<T, VEC>), dim3((unsigned)((long)N * L.S), L.gx), dim3(256), 2 * 256 * VEC * sizeof(float), st, (const T*)dy, (const T*)x, (const T*)cm,
                       (const f32x4*)coef, (const T*)pools, (T*)dx, part, HW, C, L.TX, L.TY, L.S, L.rps);
    MCN_CHECK_LAUNCH();
    const long NC = (long)N * C;
    hipLaunchKernelGGL((cb_slices_kernel<T, 1>), dim3((unsigned)((NC + 255) / 256)), dim3(256), 0, st, (const float*)part, (T*)dcm, (void*)ties, NC, C, L.S, 0.f);
    MCN_CHECK_LAUNCH();
    return MCN_OK;
}
extern "C" int mcn_cbam_bwd(const void* dy, const void* x, const void* cm, const void* s, const void* sm, const float* w, const void* pools, void* dx, void* dcm, float* dw,
                            float* db, float* ties, float grad_scale, int32_t N, int32_t H, int32_t W, int32_t C, int32_t K, mcn_dtype dtype, void* ws, size_t ws_bytes,
                            void* stream) {
    if (!dy || !x || !cm || !s || !sm || !w || !dx || !dcm) MCN_FAIL(MCN_E_BADARG, "cbam_bwd: null tensor");
    if ((pools != nullptr) != (ties != nullptr)) MCN_FAIL(MCN_E_BADARG, "cbam_bwd: pools and ties go together (the tie counts of the spatial maxima)");
    const int rc = cb_check("cbam_bwd", N, H, W, C, K, dtype);
    if (rc != MCN_OK) return rc;
    if (!ws || ws_bytes < mcn_cbam_workspace_bytes(N, H, W, C, K)) MCN_FAIL(MCN_E_WORKSPACE, "cbam_bwd: workspace too small");
    const void* pmax = pools ? (const char*)pools + (size_t)N * C * mcn_dtype_size(dtype) : nullptr;
    CB_DISPATCH(cb_bwd_t, dy, x, cm, s, sm, w, pmax, dx, dcm, dw, db, ties, grad_scale, N, H, W, C, K, ws, (hipStream_t)stream);
}
