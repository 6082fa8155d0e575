// gn.hip — group normalisation (reference convnet.py:1928-2013) on [N][HW][C] NHWC activations.
//
// The statistic belongs to (image, group): group g owns channels [g*C/G, (g+1)*C/G), mean and BIASED variance are taken over
// HW x C/G in fp32 (convnet.py:2004-2008), y = (x - mean) / sqrt(var + eps) * gamma + beta, rounded once.  In NHWC a group is a
// strip of C/G channels that can be narrower than one 16-byte chunk (C = 64, G = 32: an fp32 chunk spans 2 groups, a 2-byte chunk 4)
// or span many chunks; the parameter gradients still reduce per channel over the whole batch.  HBM-bound like bn.hip; two paths.
//
// Two-pass path (any shape) — the house column layout: a thread owns one 16-byte channel chunk and walks rows with streaming
// loads; sums are shifted by the per-(image, channel) pivot x[n][0][c] (no E[x^2] - E[x]^2 cancellation).
//   launch shape : grid.x = image x row slice of that image, grid.y = blocks of 256 chunk columns.  The slice count fills the chip
//                  (GN_TARGET_BLOCKS) while every thread keeps >= 4 rows: 112^2 x 64 at N = 256 -> 8 slices of 1568 rows per image
//                  (16 row lanes x 16 columns per workgroup); 7^2 x 2048 -> one workgroup per (image, 256 columns, 13-row slice).
//   fwd : stats -> [N][S][2][C] partials -> finalize (8 lanes per (image, group): merges slices and folds channels into the group
//         in double precision, re-centred on the group's first pivot; fixed order) leaves scale = gamma*invstd and
//         shift = beta - mean*scale per (n, c) in workspace -> apply: one read of x (+ skip), one write, no group logic.
//   bwd : reduce (sum dz, sum dz*xhat per (n, slice, c)) -> finalize: the two group sums per (n, g) expanded to per-(n, c)
//         coefficients, and dgamma / dbeta as fixed-order sums over (n, slice) of the channel partials -> apply.
//   No floating-point atomics: a repeated call is bit-identical.
//
// Resident path (slabs that fit in LDS): one workgroup owns one image and a block of whole groups >= 128 contiguous bytes per pixel
// wide (a power-of-two number of chunks), stages that [HW][block] slab in LDS, reduces, and applies from LDS: x is read from HBM
// ONCE (1R + 1W instead of 2R + 1W — batch norm cannot have this, its statistic spans the batch).  Staging is a REGISTER ROUND TRIP
// (global load -> registers -> ds_write_b128), not LDS-DMA as in the depthwise band kernels: the values pass through registers
// anyway, so the staging loop accumulates the shifted sums on the way and the slab is read back only once, by the apply loop —
// with LDS-DMA the reduction would be a second LDS pass.  Every thread re-reads the slots it wrote itself; the row lanes of a wave
// are folded with xor-shuffles, the waves through LDS, channels into groups in double.  The backward keeps TWO slabs (dz = the
// masked dy, and x), so its budget is half the forward's; dgamma / dbeta leave as per-image channel partials ([N][1][2][C]) and are
// summed by the same finalize kernel as the two-pass path.
// LDS budget: 163840 bytes per workgroup — what the compiler accepts for gfx950 (-Rpass-analysis=kernel-resource-usage reports
// "LDS Size"; 163844 bytes of __shared__ is refused with "local memory (163844) exceeds limit (163840)") — minus the fold scratch
// ([waves][2][block] floats + [block][2] doubles + [groups][2] floats).  28^2 x 32 fp32 channels = 100352 bytes fits forward only;
// 14^2 and 7^2 fit both directions.  One workgroup of 1024 threads per CU at the large slabs.
#include "common.h"

#define GN_TARGET_BLOCKS 2048       /* workgroups of a two-pass kernel */
#define GN_MAX_SLICES 64            /* row slices per image (workspace sizing) */
#define GN_LDS_BUDGET 163840
#define GN_FIN_LANES 8              /* threads per (image, group) of the finalize kernels */

template <typename T, int VEC>
__device__ __forceinline__ void gn_unpack(const Chunk<T>& c, float (&o)[VEC]) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = c.get(i);
}
template <typename T, int VEC>
__device__ __forceinline__ void gn_ld(const T* p, float (&o)[VEC]) { gn_unpack<T, VEC>(load_chunk<T>(p), o); }
template <typename T, int VEC>
__device__ __forceinline__ void gn_st(T* p, const float (&v)[VEC]) {
    Chunk<T> c;
#pragma unroll
    for (int i = 0; i < VEC; ++i) c.set(i, v[i]);
    store_chunk<T>(p, c);
}
// VEC consecutive fp32 per-channel values (16-byte aligned); dflt when p is null
template <int VEC>
__device__ __forceinline__ void gn_ldc(const float* __restrict__ p, float (&o)[VEC], float dflt) {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
        const f32x4 v = p ? *reinterpret_cast<const f32x4*>(p + 4 * q) : f32x4{dflt, dflt, dflt, dflt};
        o[4 * q] = v[0]; o[4 * q + 1] = v[1]; o[4 * q + 2] = v[2]; o[4 * q + 3] = v[3];
    }
}
// per-(image, group) values looked up for the VEC channels of a chunk starting at channel c0
template <int VEC>
__device__ __forceinline__ void gn_ldg(const float* __restrict__ p, int c0, int cpg, float (&o)[VEC]) {
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = p[(c0 + i) / cpg];
}

// ---- two-pass path -----------------------------------------------------------------------------------------------------
struct GnLayout {
    int cols, TX, TY, gx, S;   // chunk columns, columns / row lanes per workgroup, column blocks, row slices per image
    long rps;                  // rows per slice (multiple of TY)
};
static GnLayout gn_layout(int N, long HW, int C, int vec) {
    GnLayout L;
    L.cols = C / vec;
    L.TX = L.cols < 256 ? L.cols : 256;
    L.TY = 256 / L.TX;
    L.gx = (L.cols + L.TX - 1) / L.TX;
    const long per_image = (GN_TARGET_BLOCKS + (long)N * L.gx - 1) / ((long)N * L.gx);
    const long most = (HW + (long)L.TY * 4 - 1) / ((long)L.TY * 4);               // >= 4 rows per thread
    long S = per_image < most ? per_image : most;
    if (S > GN_MAX_SLICES) S = GN_MAX_SLICES;
    if (S < 1) S = 1;
    L.rps = ((HW + S - 1) / S + L.TY - 1) / L.TY * L.TY;
    L.S = (int)((HW + L.rps - 1) / L.rps);
    return L;
}

// fold the TY row lanes of a workgroup through LDS and write one partial row pair: part[(row * 2 + {0, 1}) * C + c]
template <int VEC>
__device__ __forceinline__ void gn_fold_rows(float* red, const float (&s1)[VEC], const float (&s2)[VEC], int tx, int ty, int TX, int TY, bool col_ok,
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
            float a = 0.f, b = 0.f;
            for (int k = 0; k < TY; ++k) {
                a += r1p[(k * TX + tx) * VEC + i];
                b += r2p[(k * TX + tx) * VEC + i];
            }
            part[(row * 2 + 0) * C + c0 + i] = a;
            part[(row * 2 + 1) * C + c0 + i] = b;
        }
    }
}

// part[((n * S + s) * 2 + {0, 1}) * C + c] = sum over the slice's rows of (x - piv), (x - piv)^2, piv = x[n][0][c]
template <typename T, int VEC>
__global__ __launch_bounds__(256) void gn_stats_kernel(const T* __restrict__ x, float* __restrict__ part, long HW, int C, int TX, int TY, int S, long rps) {
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
        const T* xi = x + n * HW * C + (long)col * VEC;
        float piv[VEC];
        gn_ld<T, VEC>(xi, piv);
        const long r0 = (long)s * rps, r1 = min(HW, r0 + rps);
        auto row = [&](const float* v) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float d = v[i] - piv[i];
                s1[i] += d;
                s2[i] = fmaf(d, d, s2[i]);
            }
        };
        constexpr int U = 4;                  // rows per trip, loads first (one 16-byte load in flight per thread is latency bound)
        long r = r0 + ty;
        for (; r + (long)(U - 1) * TY < r1; r += (long)U * TY) {
            float v[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) gn_ld<T, VEC>(xi + (r + (long)u * TY) * C, v[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) row(v[u]);
        }
        for (; r < r1; r += TY) {
            float v[VEC];
            gn_ld<T, VEC>(xi + r * C, v);
            row(v);
        }
    }
    gn_fold_rows<VEC>(red, s1, s2, tx, ty, TX, TY, col_ok, part, blockIdx.x, C, col * VEC);
}

// GN_FIN_LANES threads per (image, group): slices and channels of the group merged in double, every channel's shifted sums re-centred
// on the group's first pivot P: sum (x - P) = s1 + r d, sum (x - P)^2 = s2 + 2 d s1 + r d^2 with d = piv_c - P, r = rows of the slice.
// Leaves scale / shift per (n, c) for the apply pass and the saved statistics per (n, g).
template <typename T>
__global__ __launch_bounds__(256) void gn_fwd_finalize_kernel(const T* __restrict__ x, const float* __restrict__ part, int N, long HW, int C, int G, int S, long rps,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                              float* __restrict__ save_mean, float* __restrict__ save_invstd, float* __restrict__ scale,
                                                              float* __restrict__ shift) {
    const long p = (long)blockIdx.x * (256 / GN_FIN_LANES) + threadIdx.x / GN_FIN_LANES;
    const int lane = threadIdx.x % GN_FIN_LANES;
    const bool ok = p < (long)N * G;
    const long n = ok ? p / G : 0;
    const int g = ok ? (int)(p % G) : 0;
    const int cpg = C / G;
    const T* x0 = x + n * HW * C + g * cpg;                  // row 0 of the image: the pivots of the group's channels
    const double P = (double)to_f32(x0[0]);
    double S1 = 0.0, S2 = 0.0;
    if (ok) {
        for (int i = lane; i < cpg * S; i += GN_FIN_LANES) {
            const int cl = i % cpg, s = i / cpg;
            const long row = n * S + s;
            const double a = part[(row * 2 + 0) * C + g * cpg + cl], b = part[(row * 2 + 1) * C + g * cpg + cl];
            const double r = (double)(min(HW, (long)(s + 1) * rps) - (long)s * rps);
            const double d = (double)to_f32(x0[cl]) - P;
            S1 += a + r * d;
            S2 += b + 2.0 * d * a + r * d * d;
        }
    }
#pragma unroll
    for (int o = 1; o < GN_FIN_LANES; o <<= 1) {
        S1 += __shfl_xor(S1, o);
        S2 += __shfl_xor(S2, o);
    }
    if (!ok) return;
    const double inv_m = 1.0 / ((double)HW * cpg);
    const double dm = S1 * inv_m;
    double var = S2 * inv_m - dm * dm;
    if (var < 0.0) var = 0.0;
    const float fmean = (float)(P + dm), finv = (float)(1.0 / sqrt(var + (double)eps));
    if (lane == 0) {
        if (save_mean) save_mean[p] = fmean;
        if (save_invstd) save_invstd[p] = finv;
    }
    for (int cl = lane; cl < cpg; cl += GN_FIN_LANES) {
        const int c = g * cpg + cl;
        const float sc = (gamma ? gamma[c] : 1.f) * finv;
        scale[n * C + c] = sc;
        shift[n * C + c] = (beta ? beta[c] : 0.f) - fmean * sc;
    }
}

// y = act(x * scale[n][c] + shift[n][c] [+ skip]): the rounding points of bn_apply_kernel
template <typename T, int VEC, bool SKIP, bool RELU>
__global__ __launch_bounds__(256) void gn_apply_kernel(const T* __restrict__ x, const T* __restrict__ skip, T* __restrict__ y, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, long HW, int C, int TX, int TY, int S, long rps) {
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int col = blockIdx.y * TX + tx;
    if (ty >= TY || col * VEC >= C) return;
    const long n = blockIdx.x / S;
    const int s = blockIdx.x % S;
    float sc[VEC], sh[VEC];
    gn_ldc<VEC>(scale + n * C + col * VEC, sc, 1.f);
    gn_ldc<VEC>(shift + n * C + col * VEC, sh, 0.f);
    const long base = n * HW * C + (long)col * VEC;
    const long r0 = (long)s * rps, r1 = min(HW, r0 + rps);
    auto row = [&](float (&v)[VEC], const float* k, long off) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            float o = fmaf(v[i], sc[i], sh[i]);
            if (SKIP) o += k[i];
            if (RELU) o = fmaxf(o, 0.f);
            v[i] = o;
        }
        gn_st<T, VEC>(y + off, v);
    };
    constexpr int U = SKIP ? 2 : 4;
    long r = r0 + ty;
    for (; r + (long)(U - 1) * TY < r1; r += (long)U * TY) {
        float v[U][VEC], k[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long off = base + (r + (long)u * TY) * C;
            gn_ld<T, VEC>(x + off, v[u]);
            if (SKIP) gn_ld<T, VEC>(skip + off, k[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) row(v[u], k[u], base + (r + (long)u * TY) * C);
    }
    for (; r < r1; r += TY) {
        float v[VEC], k[VEC];
        gn_ld<T, VEC>(x + base + r * C, v);
        if (SKIP) gn_ld<T, VEC>(skip + base + r * C, k);
        row(v, k, base + r * C);
    }
}

// part[((n * S + s) * 2 + {0, 1}) * C + c] = sum dz, sum dz * xhat over the slice's rows (dz = dy * [y > 0] when RELU)
template <typename T, int VEC, bool RELU>
__global__ __launch_bounds__(256) void gn_bwd_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, float* __restrict__ part, long HW, int C, int G, int TX, int TY,
                                                            int S, long rps) {
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
        float mu[VEC], is[VEC];
        gn_ldg<VEC>(mean + n * G, col * VEC, C / G, mu);
        gn_ldg<VEC>(invstd + n * G, col * VEC, C / G, is);
        const long base = n * HW * C + (long)col * VEC;
        const long r0 = (long)s * rps, r1 = min(HW, r0 + rps);
        auto row = [&](const float* g, const float* v, const float* o) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float gg = RELU ? (o[i] > 0.f ? g[i] : 0.f) : g[i];
                s1[i] += gg;
                s2[i] = fmaf(gg, (v[i] - mu[i]) * is[i], s2[i]);
            }
        };
        constexpr int U = RELU ? 2 : 4;
        long r = r0 + ty;
        for (; r + (long)(U - 1) * TY < r1; r += (long)U * TY) {
            float g[U][VEC], v[U][VEC], o[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long off = base + (r + (long)u * TY) * C;
                gn_ld<T, VEC>(dy + off, g[u]);
                gn_ld<T, VEC>(x + off, v[u]);
                if (RELU) gn_ld<T, VEC>(y + off, o[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) row(g[u], v[u], o[u]);
        }
        for (; r < r1; r += TY) {
            float g[VEC], v[VEC], o[VEC];
            gn_ld<T, VEC>(dy + base + r * C, g);
            gn_ld<T, VEC>(x + base + r * C, v);
            if (RELU) gn_ld<T, VEC>(y + base + r * C, o);
            row(g, v, o);
        }
    }
    gn_fold_rows<VEC>(red, s1, s2, tx, ty, TX, TY, col_ok, part, blockIdx.x, C, col * VEC);
}

// the two group sums of dx per (n, g), A = sum_c gamma_c sum dz, B = sum_c gamma_c sum dz xhat (double, fixed order), expanded to
// per-(n, c) coefficients ca = A / m, cb = B / m for the apply pass
__global__ __launch_bounds__(256) void gn_bwd_groups_kernel(const float* __restrict__ part, int N, long HW, int C, int G, int S, const float* __restrict__ gamma,
                                                            float* __restrict__ ca, float* __restrict__ cb) {
    const long p = (long)blockIdx.x * (256 / GN_FIN_LANES) + threadIdx.x / GN_FIN_LANES;
    const int lane = threadIdx.x % GN_FIN_LANES;
    const bool ok = p < (long)N * G;
    const long n = ok ? p / G : 0;
    const int g = ok ? (int)(p % G) : 0;
    const int cpg = C / G;
    double A = 0.0, B = 0.0;
    if (ok) {
        for (int i = lane; i < cpg * S; i += GN_FIN_LANES) {
            const int c = g * cpg + i % cpg;
            const long row = n * S + i / cpg;
            const double gm = gamma ? (double)gamma[c] : 1.0;
            A += gm * (double)part[(row * 2 + 0) * C + c];
            B += gm * (double)part[(row * 2 + 1) * C + c];
        }
    }
#pragma unroll
    for (int o = 1; o < GN_FIN_LANES; o <<= 1) {
        A += __shfl_xor(A, o);
        B += __shfl_xor(B, o);
    }
    if (!ok) return;
    const double inv_m = 1.0 / ((double)HW * cpg);
    const float fa = (float)(A * inv_m), fb = (float)(B * inv_m);
    for (int cl = lane; cl < cpg; cl += GN_FIN_LANES) {
        ca[n * C + g * cpg + cl] = fa;
        cb[n * C + g * cpg + cl] = fb;
    }
}

// dbeta[c] = grad_scale * sum over the `rows` = N * S partial rows of plane 0, dgamma[c] of plane 1: 8 channels x 32 lanes per workgroup,
// lanes stride over the rows, folded by xor-shuffles inside a wave and through LDS across the 4 waves (double, fixed order)
__global__ __launch_bounds__(256) void gn_bwd_params_kernel(const float* __restrict__ part, long rows, int C, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            float grad_scale) {
    __shared__ double sh[4 * 8 * 2];
    const int ch = threadIdx.x % 8, lane = threadIdx.x / 8;
    const int c = blockIdx.x * 8 + ch;
    double a = 0.0, b = 0.0;
    if (c < C) {
        // U rows per trip, all 2U loads issued before the first use (rows past the end re-read the lane's first row and are zeroed): a one-load-per-trip
        // loop over the 2048 rows of 112^2 x 64 at N = 256 is a chain of L2 round trips in 8 workgroups
        constexpr int U = 8;
        for (long k = lane; k < rows; k += 32 * U) {
            float v0[U], v1[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long row = k + 32 * u < rows ? k + 32 * u : k;
                v0[u] = part[(row * 2 + 0) * C + c];
                v1[u] = part[(row * 2 + 1) * C + c];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool ok = k + 32 * u < rows;
                a += ok ? (double)v0[u] : 0.0;
                b += ok ? (double)v1[u] : 0.0;
            }
        }
    }
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    const int wave = threadIdx.x >> 6, wl = threadIdx.x & 63;
    if (wl < 8) {
        sh[(wave * 8 + wl) * 2 + 0] = a;
        sh[(wave * 8 + wl) * 2 + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x < 8 && c < C) {
        a = b = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            a += sh[(w * 8 + threadIdx.x) * 2 + 0];
            b += sh[(w * 8 + threadIdx.x) * 2 + 1];
        }
        if (dbeta) dbeta[c] = (float)a * grad_scale;
        if (dgamma) dgamma[c] = (float)b * grad_scale;
    }
}

// dx = invstd * (gamma * dz - ca - xhat * cb); dskip = dz
template <typename T, int VEC, bool RELU, bool DSKIP>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ mean,
                                                           const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ ca,
                                                           const float* __restrict__ cb, T* __restrict__ dx, T* __restrict__ dskip, long HW, int C, int G, int TX,
                                                           int TY, int S, long rps) {
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int col = blockIdx.y * TX + tx;
    if (ty >= TY || col * VEC >= C) return;
    const long n = blockIdx.x / S;
    const int s = blockIdx.x % S;
    float mu[VEC], is[VEC], gm[VEC], a[VEC], b[VEC];
    gn_ldg<VEC>(mean + n * G, col * VEC, C / G, mu);
    gn_ldg<VEC>(invstd + n * G, col * VEC, C / G, is);
    gn_ldc<VEC>(gamma ? gamma + col * VEC : nullptr, gm, 1.f);
    gn_ldc<VEC>(ca + n * C + col * VEC, a, 0.f);
    gn_ldc<VEC>(cb + n * C + col * VEC, b, 0.f);
    const long base = n * HW * C + (long)col * VEC;
    const long r0 = (long)s * rps, r1 = min(HW, r0 + rps);
    constexpr int U = 2;
    auto row = [&](float (&g)[VEC], float (&v)[VEC], const float* o, long off) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            if (RELU) g[i] = o[i] > 0.f ? g[i] : 0.f;
            const float xh = (v[i] - mu[i]) * is[i];
            v[i] = is[i] * (gm[i] * g[i] - a[i] - xh * b[i]);
        }
        gn_st<T, VEC>(dx + off, v);
        if (DSKIP) gn_st<T, VEC>(dskip + off, g);
    };
    long r = r0 + ty;
    for (; r + (long)(U - 1) * TY < r1; r += (long)U * TY) {
        float g[U][VEC], v[U][VEC], o[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long off = base + (r + (long)u * TY) * C;
            gn_ld<T, VEC>(dy + off, g[u]);
            gn_ld<T, VEC>(x + off, v[u]);
            if (RELU) gn_ld<T, VEC>(y + off, o[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) row(g[u], v[u], o[u], base + (r + (long)u * TY) * C);
    }
    for (; r < r1; r += TY) {
        float g[VEC], v[VEC], o[VEC];
        gn_ld<T, VEC>(dy + base + r * C, g);
        gn_ld<T, VEC>(x + base + r * C, v);
        if (RELU) gn_ld<T, VEC>(y + base + r * C, o);
        row(g, v, o, base + r * C);
    }
}

// ---- resident path ------------------------------------------------------------------------------------------------------
struct GnSlab {
    int BW;          // channels per workgroup: whole groups, a power-of-two number of chunks, >= 128 bytes per pixel (or all of C)
    int threads;     // workgroup size
    size_t lds;      // slab(s) + fold scratch
};
// 0 when the shape has no resident form
static bool gn_slab_plan(int backward, long HW, int C, int G, mcn_dtype dtype, GnSlab* out) {
    const int vec = dtype == MCN_F32 ? 4 : 8, cpg = C / G;
    const int es = (int)mcn_dtype_size(dtype);
    if (HW > 65536) return false;
    int unit = cpg;                                     // lcm(cpg, vec): whole groups and whole chunks
    while (unit % vec) unit += cpg;
    int BW = 0;
    for (int w = unit; w <= C; w += unit) {
        if (C % w) continue;
        if (w * es >= 128 || w == C) { BW = w; break; }
    }
    const int bwc = BW / vec;
    if (BW == 0 || bwc > 64 || (bwc & (bwc - 1))) return false;
    long t = 256;
    while (t < 1024 && t * 4 < HW * bwc) t *= 2;        // ~4 rows per thread, 4..16 waves
    const size_t slab = (size_t)HW * BW * es;
    const size_t lds = slab * (backward ? 2 : 1) + (size_t)(t / 64) * 2 * BW * sizeof(float) + (size_t)BW * 2 * sizeof(double) + align_up((size_t)(BW / cpg) * 2 * sizeof(float), 16);
    if (lds > GN_LDS_BUDGET) return false;
    out->BW = BW;
    out->threads = (int)t;
    out->lds = lds;
    return true;
}

// the row lanes of a wave (lanes with the same chunk column: lane % BWc) folded by xor-shuffles, one [2][BW] row per wave in `red`
template <int VEC>
__device__ __forceinline__ void gn_wave_fold(float* red, float (&s1)[VEC], float (&s2)[VEC], int BWc, int BW) {
    for (int o = BWc; o < 64; o <<= 1) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            s1[i] += __shfl_xor(s1[i], o);
            s2[i] += __shfl_xor(s2[i], o);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < BWc) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            red[(wave * 2 + 0) * BW + lane * VEC + i] = s1[i];
            red[(wave * 2 + 1) * BW + lane * VEC + i] = s2[i];
        }
    }
}

template <typename T, int VEC, bool SKIP, bool RELU>
__global__ __launch_bounds__(1024) void gn_resident_fwd_kernel(const T* __restrict__ x, const T* __restrict__ skip, T* __restrict__ y, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float* __restrict__ save_mean, float* __restrict__ save_invstd, int HW,
                                                               int C, int G, int BW, float eps) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gn_lds[];
    const int BWc = BW / VEC, cpg = C / G, ng = BW / cpg, nw = blockDim.x >> 6;
    Chunk<T>* slab = reinterpret_cast<Chunk<T>*>(gn_lds);                                              // [HW][BWc]
    float* red = reinterpret_cast<float*>(gn_lds + (size_t)HW * BWc * 16);                             // [nw][2][BW]
    double* chs = reinterpret_cast<double*>(red + nw * 2 * BW);                                         // [BW][2]
    float* stat = reinterpret_cast<float*>(chs + BW * 2);                                               // [ng][2]
    const int cx = threadIdx.x % BWc, ry = threadIdx.x / BWc, TY = blockDim.x / BWc;
    const int nb = C / BW;
    const long n = blockIdx.x / nb;
    const int c_blk = (blockIdx.x % nb) * BW;
    const T* x0 = x + n * HW * C + c_blk;                      // row 0 of the image, first channel of the block
    const long base = n * HW * C + c_blk + cx * VEC;
    float piv[VEC], s1[VEC], s2[VEC];
    gn_ld<T, VEC>(x + base, piv);
#pragma unroll
    for (int i = 0; i < VEC; ++i) s1[i] = s2[i] = 0.f;
    auto stage = [&](const Chunk<T>& c, int r) {
        slab[r * BWc + cx] = c;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float d = c.get(i) - piv[i];
            s1[i] += d;
            s2[i] = fmaf(d, d, s2[i]);
        }
    };
    constexpr int U = 4;
    int r = ry;
    for (; r + (U - 1) * TY < HW; r += U * TY) {
        Chunk<T> c[U];
#pragma unroll
        for (int u = 0; u < U; ++u) c[u] = load_chunk<T>(x + base + (long)(r + u * TY) * C);
#pragma unroll
        for (int u = 0; u < U; ++u) stage(c[u], r + u * TY);
    }
    for (; r < HW; r += TY) stage(load_chunk<T>(x + base + (long)r * C), r);
    gn_wave_fold<VEC>(red, s1, s2, BWc, BW);
    __syncthreads();
    for (int cl = threadIdx.x; cl < BW; cl += blockDim.x) {    // waves merged per channel, re-centred on the group's first pivot (gn_fwd_finalize_kernel)
        const int c0 = cl / cpg * cpg;
        double a = 0.0, b = 0.0;
        for (int w = 0; w < nw; ++w) {
            a += (double)red[(w * 2 + 0) * BW + cl];
            b += (double)red[(w * 2 + 1) * BW + cl];
        }
        const double d = (double)to_f32(x0[cl]) - (double)to_f32(x0[c0]);
        chs[cl * 2 + 0] = a + (double)HW * d;
        chs[cl * 2 + 1] = b + 2.0 * d * a + (double)HW * d * d;
    }
    __syncthreads();
    for (int g = threadIdx.x; g < ng; g += blockDim.x) {
        double S1 = 0.0, S2 = 0.0;
        for (int cl = g * cpg; cl < (g + 1) * cpg; ++cl) {
            S1 += chs[cl * 2 + 0];
            S2 += chs[cl * 2 + 1];
        }
        const double inv_m = 1.0 / ((double)HW * cpg);
        const double dm = S1 * inv_m;
        double var = S2 * inv_m - dm * dm;
        if (var < 0.0) var = 0.0;
        const float fmean = (float)((double)to_f32(x0[g * cpg]) + dm), finv = (float)(1.0 / sqrt(var + (double)eps));
        stat[g * 2 + 0] = fmean;
        stat[g * 2 + 1] = finv;
        const long p = n * G + c_blk / cpg + g;
        if (save_mean) save_mean[p] = fmean;
        if (save_invstd) save_invstd[p] = finv;
    }
    __syncthreads();
    float sc[VEC], sh[VEC];
    gn_ldc<VEC>(gamma ? gamma + c_blk + cx * VEC : nullptr, sc, 1.f);
    gn_ldc<VEC>(beta ? beta + c_blk + cx * VEC : nullptr, sh, 0.f);
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const int g = (cx * VEC + i) / cpg;
        sc[i] *= stat[g * 2 + 1];
        sh[i] -= stat[g * 2 + 0] * sc[i];
    }
    auto apply = [&](const float* k, int q) {
        float v[VEC];
        gn_unpack<T, VEC>(slab[q * BWc + cx], v);               // (the slot this thread staged)
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            float o = fmaf(v[i], sc[i], sh[i]);
            if (SKIP) o += k[i];
            if (RELU) o = fmaxf(o, 0.f);
            v[i] = o;
        }
        gn_st<T, VEC>(y + base + (long)q * C, v);
    };
    r = ry;
    if (SKIP) {
        for (; r + (U - 1) * TY < HW; r += U * TY) {
            float k[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) gn_ld<T, VEC>(skip + base + (long)(r + u * TY) * C, k[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) apply(k[u], r + u * TY);
        }
    }
    for (; r < HW; r += TY) {
        float k[VEC];
        if (SKIP) gn_ld<T, VEC>(skip + base + (long)r * C, k);
        apply(k, r);
    }
}

// backward: dz (the masked dy, exact in T) and x both resident; part (may be null): per-image channel partials [N][2][C] for dgamma / dbeta
template <typename T, int VEC, bool RELU, bool DSKIP>
__global__ __launch_bounds__(1024) void gn_resident_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ gamma,
                                                               const float* __restrict__ mean, const float* __restrict__ invstd, T* __restrict__ dx,
                                                               T* __restrict__ dskip, float* __restrict__ part, int HW, int C, int G, int BW) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gn_lds[];
    const int BWc = BW / VEC, cpg = C / G, ng = BW / cpg, nw = blockDim.x >> 6;
    Chunk<T>* slab_g = reinterpret_cast<Chunk<T>*>(gn_lds);                                            // [HW][BWc] dz
    Chunk<T>* slab_x = slab_g + (size_t)HW * BWc;                                                      // [HW][BWc] x
    float* red = reinterpret_cast<float*>(gn_lds + (size_t)2 * HW * BWc * 16);                         // [nw][2][BW]
    double* chs = reinterpret_cast<double*>(red + nw * 2 * BW);                                         // [BW][2]
    float* stat = reinterpret_cast<float*>(chs + BW * 2);                                               // [ng][2]
    const int cx = threadIdx.x % BWc, ry = threadIdx.x / BWc, TY = blockDim.x / BWc;
    const int nb = C / BW;
    const long n = blockIdx.x / nb;
    const int c_blk = (blockIdx.x % nb) * BW;
    const long base = n * HW * C + c_blk + cx * VEC;
    float mu[VEC], is[VEC], gm[VEC], s1[VEC], s2[VEC];
    gn_ldg<VEC>(mean + n * G, c_blk + cx * VEC, cpg, mu);
    gn_ldg<VEC>(invstd + n * G, c_blk + cx * VEC, cpg, is);
    gn_ldc<VEC>(gamma ? gamma + c_blk + cx * VEC : nullptr, gm, 1.f);
#pragma unroll
    for (int i = 0; i < VEC; ++i) s1[i] = s2[i] = 0.f;
    auto stage = [&](Chunk<T> g, const Chunk<T>& v, const Chunk<T>& o, int q) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            if (RELU && !(o.get(i) > 0.f)) g.set(i, 0.f);
            const float gg = g.get(i);
            s1[i] += gg;
            s2[i] = fmaf(gg, (v.get(i) - mu[i]) * is[i], s2[i]);
        }
        slab_g[q * BWc + cx] = g;
        slab_x[q * BWc + cx] = v;
        if (DSKIP) store_chunk<T>(dskip + base + (long)q * C, g);
    };
    constexpr int U = 2;
    int r = ry;
    for (; r + (U - 1) * TY < HW; r += U * TY) {
        Chunk<T> g[U], v[U], o[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long off = base + (long)(r + u * TY) * C;
            g[u] = load_chunk<T>(dy + off);
            v[u] = load_chunk<T>(x + off);
            if (RELU) o[u] = load_chunk<T>(y + off);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) stage(g[u], v[u], o[u], r + u * TY);
    }
    for (; r < HW; r += TY) {
        const long off = base + (long)r * C;
        Chunk<T> o;
        if (RELU) o = load_chunk<T>(y + off);
        stage(load_chunk<T>(dy + off), load_chunk<T>(x + off), o, r);
    }
    gn_wave_fold<VEC>(red, s1, s2, BWc, BW);
    __syncthreads();
    for (int cl = threadIdx.x; cl < BW; cl += blockDim.x) {
        double a = 0.0, b = 0.0;
        for (int w = 0; w < nw; ++w) {
            a += (double)red[(w * 2 + 0) * BW + cl];
            b += (double)red[(w * 2 + 1) * BW + cl];
        }
        if (part) {
            part[(n * 2 + 0) * C + c_blk + cl] = (float)a;
            part[(n * 2 + 1) * C + c_blk + cl] = (float)b;
        }
        const double g = gamma ? (double)gamma[c_blk + cl] : 1.0;
        chs[cl * 2 + 0] = g * a;
        chs[cl * 2 + 1] = g * b;
    }
    __syncthreads();
    for (int g = threadIdx.x; g < ng; g += blockDim.x) {
        double A = 0.0, B = 0.0;
        for (int cl = g * cpg; cl < (g + 1) * cpg; ++cl) {
            A += chs[cl * 2 + 0];
            B += chs[cl * 2 + 1];
        }
        const double inv_m = 1.0 / ((double)HW * cpg);
        stat[g * 2 + 0] = (float)(A * inv_m);
        stat[g * 2 + 1] = (float)(B * inv_m);
    }
    __syncthreads();
    float a[VEC], b[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) {
        const int g = (cx * VEC + i) / cpg;
        a[i] = stat[g * 2 + 0];
        b[i] = stat[g * 2 + 1];
    }
    for (r = ry; r < HW; r += TY) {
        float g[VEC], v[VEC];
        gn_unpack<T, VEC>(slab_g[r * BWc + cx], g);
        gn_unpack<T, VEC>(slab_x[r * BWc + cx], v);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const float xh = (v[i] - mu[i]) * is[i];
            v[i] = is[i] * (gm[i] * g[i] - a[i] - xh * b[i]);
        }
        gn_st<T, VEC>(dx + base + (long)r * C, v);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static size_t gn_parts_bytes(int N, long HW, int C) {
    const GnLayout a = gn_layout(N, HW, C, 4), b = gn_layout(N, HW, C, 8);
    return align_up((size_t)N * (a.S > b.S ? a.S : b.S) * 2 * C * sizeof(float), 256);
}
extern "C" size_t mcn_gn_workspace_bytes(int32_t N, int64_t HW, int32_t C, int32_t G) {
    if (N <= 0 || HW <= 0 || C <= 0 || G <= 0) return 0;
    return gn_parts_bytes(N, HW, C) + align_up((size_t)2 * N * C * sizeof(float), 256);      // partials + two per-(n, c) coefficient planes
}
extern "C" int32_t mcn_gn_resident_ok(int32_t backward, int32_t N, int64_t HW, int32_t C, int32_t G, mcn_dtype dtype) {
    GnSlab s;
    if (N <= 0 || HW <= 0 || C <= 0 || G <= 0 || C % G || !mcn_dtype_ok(dtype) || C % (dtype == MCN_F32 ? 4 : 8)) return 0;
    return gn_slab_plan(backward, HW, C, G, dtype, &s) ? 1 : 0;
}

// argument checks shared by the two entry points; *resident = the path the call takes
static int gn_check(const char* who, int N, long HW, int C, int G, mcn_act act, mcn_dtype dtype, int path, int backward, const void* ws, size_t ws_bytes,
                    GnSlab* slab, bool* resident) {
    if (N <= 0 || HW <= 0 || C <= 0 || G <= 0 || (long)N * HW * C <= 0) MCN_FAIL(MCN_E_BADARG, "%s: bad argument (N=%d HW=%ld C=%d G=%d)", who, N, HW, C, G);
    if (C % G) MCN_FAIL(MCN_E_BADARG, "%s: %d channels are not a multiple of %d groups", who, C, G);
    if (!mcn_dtype_ok(dtype)) MCN_FAIL(MCN_E_UNSUPPORTED, "%s: dtype %d unsupported", who, (int)dtype);
    if (C % (dtype == MCN_F32 ? 4 : 8)) MCN_FAIL(MCN_E_UNSUPPORTED, "%s: C = %d is not a multiple of the 16-byte chunk (%d elements)", who, C, dtype == MCN_F32 ? 4 : 8);
    if (act != MCN_ACT_NONE && act != MCN_ACT_RELU) MCN_FAIL(MCN_E_UNSUPPORTED, "%s: activation %d is not fused (none / relu)", who, (int)act);
    if (path != 0 && path != MCN_GN_TWO_PASS && path != MCN_GN_RESIDENT) MCN_FAIL(MCN_E_BADARG, "%s: path hint %d", who, path);
    if (!ws || ws_bytes < mcn_gn_workspace_bytes(N, HW, C, G)) MCN_FAIL(MCN_E_WORKSPACE, "%s: workspace too small", who);
    const bool fits = gn_slab_plan(backward, HW, C, G, dtype, slab);
    if (path == MCN_GN_RESIDENT && !fits) MCN_FAIL(MCN_E_UNSUPPORTED, "%s: the %ld x C slab of one group block does not fit in LDS", who, HW);
    *resident = fits && path != MCN_GN_TWO_PASS;
    return MCN_OK;
}

// (returns false when the runtime refuses the request: the launch behind it would fail with a less telling error)
template <typename K>
static bool gn_allow_lds(K kernel) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, GN_LDS_BUDGET) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

template <typename T, int VEC>
static int gn_fwd_t(const void* x, const float* gamma, const float* beta, const void* skip, void* y, float* save_mean, float* save_invstd, int N, long HW, int C, int G,
                    float eps, bool relu, bool resident, const GnSlab& slab, void* ws, hipStream_t st) {
    if (resident) {
#define GN_RES_FWD(SK, RL)                                                                                                               \
    do {                                                                                                                                 \
        static const bool ok = gn_allow_lds(gn_resident_fwd_kernel<T, VEC, SK, RL>);                                                     \
        if (!ok) MCN_FAIL(MCN_E_LAUNCH, "gn_fwd: the runtime refuses %d bytes of LDS", GN_LDS_BUDGET);                                   \
        hipLaunchKernelGGL((gn_resident_fwd_kernel<T, VEC, SK, RL>), dim3((unsigned)((long)N * (C / slab.BW))), dim3(slab.threads), slab.lds, st, (const T*)x, \
                           (const T*)skip, (T*)y, gamma, beta, save_mean, save_invstd, (int)HW, C, G, slab.BW, eps);                     \
    } while (0)
        if (skip) { if (relu) GN_RES_FWD(true, true); else GN_RES_FWD(true, false); }
        else { if (relu) GN_RES_FWD(false, true); else GN_RES_FWD(false, false); }
        MCN_CHECK_LAUNCH();
        return MCN_OK;
    }
    const GnLayout L = gn_layout(N, HW, C, VEC);
    float* part = (float*)ws;
    float* scale = (float*)((char*)ws + gn_parts_bytes(N, HW, C));
    float* shift = scale + (size_t)N * C;
    const dim3 grid((unsigned)((long)N * L.S), L.gx), block(256);
    hipLaunchKernelGGL((gn_stats_kernel<T, VEC>), grid, block, 2 * 256 * VEC * sizeof(float), st, (const T*)x, part, HW, C, L.TX, L.TY, L.S, L.rps);
    MCN_CHECK_LAUNCH();
    const int pairs = 256 / GN_FIN_LANES;
    hipLaunchKernelGGL((gn_fwd_finalize_kernel<T>), dim3((unsigned)(((long)N * G + pairs - 1) / pairs)), block, 0, st, (const T*)x, (const float*)part, N, HW, C, G, L.S,
                       L.rps, gamma, beta, eps, save_mean, save_invstd, scale, shift);
    MCN_CHECK_LAUNCH();
#define GN_APPLY(SK, RL)                                                                                                                       \
    hipLaunchKernelGGL((gn_apply_kernel<T, VEC, SK, RL>), grid, block, 0, st, (const T*)x, (const T*)skip, (T*)y, (const float*)scale, (const float*)shift, HW, C, \
                       L.TX, L.TY, L.S, L.rps)
    if (skip) { if (relu) GN_APPLY(true, true); else GN_APPLY(true, false); }
    else { if (relu) GN_APPLY(false, true); else GN_APPLY(false, false); }
    MCN_CHECK_LAUNCH();
    return MCN_OK;
}

extern "C" int mcn_gn_fwd(const void* x, const float* gamma, const float* beta, const void* skip, void* y, float* save_mean, float* save_invstd, int32_t N, int64_t HW,
                          int32_t C, int32_t G, float eps, mcn_act act, mcn_dtype dtype, int32_t path, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !y) MCN_FAIL(MCN_E_BADARG, "gn_fwd: null tensor");
    GnSlab slab = {0, 0, 0};
    bool resident = false;
    const int rc = gn_check("gn_fwd", N, HW, C, G, act, dtype, path, 0, ws, ws_bytes, &slab, &resident);
    if (rc != MCN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool relu = act == MCN_ACT_RELU;
    if (dtype == MCN_F32) return gn_fwd_t<float, 4>(x, gamma, beta, skip, y, save_mean, save_invstd, N, HW, C, G, eps, relu, resident, slab, ws, st);
    if (dtype == MCN_BF16) return gn_fwd_t<bf16_t, 8>(x, gamma, beta, skip, y, save_mean, save_invstd, N, HW, C, G, eps, relu, resident, slab, ws, st);
    return gn_fwd_t<f16_t, 8>(x, gamma, beta, skip, y, save_mean, save_invstd, N, HW, C, G, eps, relu, resident, slab, ws, st);
}

template <typename T, int VEC>
static int gn_bwd_t(const void* dy, const void* x, const void* y, const float* gamma, const float* save_mean, const float* save_invstd, void* dx, void* dskip, float* dgamma,
                    float* dbeta, float grad_scale, int N, long HW, int C, int G, bool relu, bool resident, const GnSlab& slab, void* ws, hipStream_t st) {
    float* part = (float*)ws;
    const bool params = dgamma || dbeta;
    long rows;
    if (resident) {
#define GN_RES_BWD(RL, DS)                                                                                                               \
    do {                                                                                                                                 \
        static const bool ok = gn_allow_lds(gn_resident_bwd_kernel<T, VEC, RL, DS>);                                                     \
        if (!ok) MCN_FAIL(MCN_E_LAUNCH, "gn_bwd: the runtime refuses %d bytes of LDS", GN_LDS_BUDGET);                                   \
        hipLaunchKernelGGL((gn_resident_bwd_kernel<T, VEC, RL, DS>), dim3((unsigned)((long)N * (C / slab.BW))), dim3(slab.threads), slab.lds, st, (const T*)dy, \
                           (const T*)x, (const T*)y, gamma, save_mean, save_invstd, (T*)dx, (T*)dskip, params ? part : nullptr, (int)HW, C, G, slab.BW); \
    } while (0)
        if (relu) { if (dskip) GN_RES_BWD(true, true); else GN_RES_BWD(true, false); }
        else { if (dskip) GN_RES_BWD(false, true); else GN_RES_BWD(false, false); }
        MCN_CHECK_LAUNCH();
        rows = N;
    } else {
        const GnLayout L = gn_layout(N, HW, C, VEC);
        float* ca = (float*)((char*)ws + gn_parts_bytes(N, HW, C));
        float* cb = ca + (size_t)N * C;
        const dim3 grid((unsigned)((long)N * L.S), L.gx), block(256);
        const size_t lds = 2 * 256 * VEC * sizeof(float);
        if (relu) hipLaunchKernelGGL((gn_bwd_reduce_kernel<T, VEC, true>), grid, block, lds, st, (const T*)dy, (const T*)x, (const T*)y, save_mean, save_invstd, part, HW, C, G, L.TX, L.TY, L.S, L.rps);
        else hipLaunchKernelGGL((gn_bwd_reduce_kernel<T, VEC, false>), grid, block, lds, st, (const T*)dy, (const T*)x, (const T*)y, save_mean, save_invstd, part, HW, C, G, L.TX, L.TY, L.S, L.rps);
        MCN_CHECK_LAUNCH();
        const int pairs = 256 / GN_FIN_LANES;
        hipLaunchKernelGGL(gn_bwd_groups_kernel, dim3((unsigned)(((long)N * G + pairs - 1) / pairs)), block, 0, st, (const float*)part, N, HW, C, G, L.S, gamma, ca, cb);
        MCN_CHECK_LAUNCH();
#define GN_BWD_APPLY(RL, DS)                                                                                                                    \
    hipLaunchKernelGGL((gn_bwd_apply_kernel<T, VEC, RL, DS>), grid, block, 0, st, (const T*)dy, (const T*)x, (const T*)y, save_mean, save_invstd, gamma, (const float*)ca, \
                       (const float*)cb, (T*)dx, (T*)dskip, HW, C, G, L.TX, L.TY, L.S, L.rps)
        if (relu) { if (dskip) GN_BWD_APPLY(true, true); else GN_BWD_APPLY(true, false); }
        else { if (dskip) GN_BWD_APPLY(false, true); else GN_BWD_APPLY(false, false); }
        MCN_CHECK_LAUNCH();
        rows = (long)N * L.S;
    }
    if (params) {
        hipLaunchKernelGGL(gn_bwd_params_kernel, dim3((C + 7) / 8), dim3(256), 0, st, (const float*)part, rows, C, dgamma, dbeta, grad_scale);
        MCN_CHECK_LAUNCH();
    }
    return MCN_OK;
}

extern "C" int mcn_gn_bwd(const void* dy, const void* x, const void* y, const float* gamma, const float* save_mean, const float* save_invstd, void* dx, void* dskip,
                          float* dgamma, float* dbeta, float grad_scale, int32_t N, int64_t HW, int32_t C, int32_t G, mcn_act act, mcn_dtype dtype, int32_t path, void* ws,
                          size_t ws_bytes, void* stream) {
    if (!dy || !x || !dx || !save_mean || !save_invstd) MCN_FAIL(MCN_E_BADARG, "gn_bwd: null tensor");
    GnSlab slab = {0, 0, 0};
    bool resident = false;
    const int rc = gn_check("gn_bwd", N, HW, C, G, act, dtype, path, 1, ws, ws_bytes, &slab, &resident);
    if (rc != MCN_OK) return rc;
    if (act == MCN_ACT_RELU && !y) MCN_FAIL(MCN_E_BADARG, "gn_bwd: ReLU takes its mask from the stored output y");
    hipStream_t st = (hipStream_t)stream;
    const bool relu = act == MCN_ACT_RELU;
    if (dtype == MCN_F32) return gn_bwd_t<float, 4>(dy, x, y, gamma, save_mean, save_invstd, dx, dskip, dgamma, dbeta, grad_scale, N, HW, C, G, relu, resident, slab, ws, st);
    if (dtype == MCN_BF16) return gn_bwd_t<bf16_t, 8>(dy, x, y, gamma, save_mean, save_invstd, dx, dskip, dgamma, dbeta, grad_scale, N, HW, C, G, relu, resident, slab, ws, st);
    return gn_bwd_t<f16_t, 8>(dy, x, y, gamma, save_mean, save_invstd, dx, dskip, dgamma, dbeta, grad_scale, N, HW, C, G, relu, resident, slab, ws, st);
}
