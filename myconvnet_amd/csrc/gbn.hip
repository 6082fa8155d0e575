// gbn.hip — grouped batch normalisation (reference convnet.py:2176-2376) on [M][C] NHWC activations, M = N*H*W.
//
// The statistic belongs to a GROUP of P adjacent channels over the whole batch: group g owns channels [g*P, (g+1)*P), mean and BIASED
// variance run over its M*P elements in fp32 (tf.nn.moments, convnet.py:2331), y = act(gamma[c]*(x - mean_g)/sqrt(var_g + eps) + beta[c]
// [+ skip]) rounded once.  HBM-bound like bn.hip and on its column layout (a thread owns one 16-byte channel chunk and walks rows with
// streaming loads), but the chunk is no longer VEC independent columns: with the reference's P = 8 a 2-byte chunk IS one group (two fp32
// chunks), so a thread folds the lanes of a chunk into the group's sums IN REGISTERS, before any cross-thread step.
//   LP = min(P, VEC) lanes of a chunk belong to one group; a chunk holds VEC/LP groups ("slots"); a group spans K = P/LP adjacent slots
//   (K = 1 when P <= VEC).  S = C/LP slots in all.
//   fwd : stats -> [row blocks][2][S] partials (bn.hip: [row blocks][2][C]: partial traffic, LDS fold scratch and finalize loads drop by LP)
//         -> finalize: the K slots x row blocks of a group merged in double in a fixed order; save_mean / save_invstd [G], the tiled
//         batch statistics and the running update [C], scale = gamma*invstd_g and shift = beta - mean_g*scale [C] in workspace
//         -> apply: one read of x (+ skip), one write, no group logic.
//   Pivot: every lane of a group is shifted by x[0][g*P] (no E[x^2] - E[x]^2 cancellation); one pivot per group, so slots and row
//   blocks add without re-centring.  The finalize re-reads it from x (as bn_fwd_finalize_kernel does) instead of storing G floats per row block.
//   bwd : reduce (sum dz, sum dz*xhat per channel — dgamma / dbeta are per channel) -> [row blocks][2][C] -> finalize: dgamma, dbeta and
//         the two group sums A_g = sum_c gamma_c sum dz, B_g = sum_c gamma_c sum dz*xhat as ca = A/(M P), cb = B/(M P) [G] -> apply:
//         dx = invstd_g * (gamma*dz - ca_g - xhat*cb_g), dskip = dz.
//   dz: dy masked by [y > 0] (stored y when given, else recomputed from x as mcn_bn_bwd does) or scaled by swish'(z), z recomputed from x.
// No floating-point atomics: a repeated call is bit-identical.
#include "common.h"

#define GBN_TARGET_BLOCKS 1024      /* upper bound of the row blocks (workspace sizing) */
#define GBN_FIN_G 8                 /* groups (fwd) / channels (bwd) per trip of a finalize workgroup ... */
#define GBN_FIN_LANES 64            /* ... and lanes per item: the finalize kernels are latency chains over up to 1024 row blocks (bn.hip, FIN_LANES) */
#define GBN_FIN_THREADS (GBN_FIN_G * GBN_FIN_LANES)

template <typename T, int VEC>
__device__ __forceinline__ void gbn_ld(const T* p, float (&o)[VEC]) {
    const Chunk<T> c = load_chunk<T>(p);
#pragma unroll
    for (int i = 0; i < VEC; ++i) o[i] = c.get(i);
}
template <typename T, int VEC>
__device__ __forceinline__ void gbn_st(T* p, const float (&v)[VEC]) {
    Chunk<T> c;
#pragma unroll
    for (int i = 0; i < VEC; ++i) c.set(i, v[i]);
    store_chunk<T>(p, c);
}
// VEC consecutive fp32 per-channel values (16-byte aligned); dflt when p is null
template <int VEC>
__device__ __forceinline__ void gbn_ldc(const float* __restrict__ p, float (&o)[VEC], float dflt) {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
        const f32x4 v = p ? *reinterpret_cast<const f32x4*>(p + 4 * q) : f32x4{dflt, dflt, dflt, dflt};
        o[4 * q] = v[0]; o[4 * q + 1] = v[1]; o[4 * q + 2] = v[2]; o[4 * q + 3] = v[3];
    }
}
// per-group values looked up for the VEC channels of a chunk starting at channel c0
// (P >= VEC: one group, one load; else P is a power of two below VEC and the chunk holds VEC / P consecutive groups)
template <int VEC>
__device__ __forceinline__ void gbn_ldg(const float* __restrict__ p, int c0, int P, float (&o)[VEC]) {
    const int g0 = c0 / P;
    if (P >= VEC) {
        const float v = p[g0];
#pragma unroll
        for (int i = 0; i < VEC; ++i) o[i] = v;
    } else {
        const int sh = 31 - __clz(P);
#pragma unroll
        for (int i = 0; i < VEC; ++i) o[i] = p[g0 + (i >> sh)];
    }
}
// balanced sum of N (power of two) values: a fixed order, and a dependency chain of log2 N adds instead of N
template <int N>
__device__ __forceinline__ float gbn_tree(const float* v) {
    if constexpr (N == 1) return v[0];
    else return gbn_tree<N / 2>(v) + gbn_tree<N / 2>(v + N / 2);
}
__device__ __forceinline__ float gbn_swish_grad(float z) {
    const float sg = fast_sigmoid(z);
    return sg * (1.f + z * (1.f - sg));
}

struct GbnLayout {
    int cols, TX, TY, gx, gy;   // chunk columns, columns / row lanes per workgroup, column blocks, row blocks
    long rpb;                   // rows per row block (multiple of TY)
};
static GbnLayout gbn_layout(long M, int C, int vec) {
    GbnLayout L;
    L.cols = C / vec;
    L.TX = L.cols < 256 ? L.cols : 256;
    L.TY = 256 / L.TX;
    L.gx = (L.cols + L.TX - 1) / L.TX;
    long gy = GBN_TARGET_BLOCKS / L.gx;
    const long most = (M + (long)L.TY * 8 - 1) / ((long)L.TY * 8);             // >= ~8 rows per thread
    if (gy > most) gy = most;
    if (gy < 1) gy = 1;
    L.rpb = ((M + gy - 1) / gy + L.TY - 1) / L.TY * L.TY;
    L.gy = (int)((M + L.rpb - 1) / L.rpb);
    return L;
}

// fold the TY row lanes of a workgroup through LDS and write one partial row pair of NS values per thread column:
// part[(blockIdx.y * 2 + {0, 1}) * stride + col * NS + j]
template <int NS>
__device__ __forceinline__ void gbn_fold_rows(float* red, const float (&s1)[NS], const float (&s2)[NS], int tx, int ty, int TX, int TY, bool col_ok,
                                              float* __restrict__ part, int stride, int col) {
    float* r1p = red;                       // [TY][TX * NS]
    float* r2p = red + 256 * NS;
    if (ty < TY) {
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            r1p[(ty * TX + tx) * NS + j] = s1[j];
            r2p[(ty * TX + tx) * NS + j] = s2[j];
        }
    }
    __syncthreads();
    if (ty == 0 && col_ok) {
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            float a = 0.f, b = 0.f;
            for (int k = 0; k < TY; ++k) {
                a += r1p[(k * TX + tx) * NS + j];
                b += r2p[(k * TX + tx) * NS + j];
            }
            part[((long)blockIdx.y * 2 + 0) * stride + col * NS + j] = a;
            part[((long)blockIdx.y * 2 + 1) * stride + col * NS + j] = b;
        }
    }
}

// ---- forward statistics ----------------------------------------------------------------------------------------------------
// part[(rb * 2 + {0, 1}) * S + slot] = sum over the block's rows and the slot's LP lanes of (x - piv_g), (x - piv_g)^2, piv_g = x[0][g*P].
// The LP lanes of a row are summed by a balanced tree in registers and enter the slot's accumulator as ONE add per row.
template <typename T, int VEC, int LP>
__global__ __launch_bounds__(256) void gbn_stats_kernel(const T* __restrict__ x, float* __restrict__ part, long M, int C, int P, int TX, int TY, long rpb) {
    constexpr int NS = VEC / LP;                     // slots (groups or parts of one group) per chunk
    extern __shared__ float red[];
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int col = blockIdx.x * TX + tx;
    const bool col_ok = col * VEC < C;
    float s1[NS], s2[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) s1[j] = s2[j] = 0.f;
    if (ty < TY && col_ok) {
        const T* xc = x + (long)col * VEC;
        float piv[NS];
        if constexpr (NS == 1) {
            piv[0] = to_f32(x[col * VEC / P * P]);   // P >= VEC: the group may start in an earlier chunk
        } else {
            float v0[VEC];
            gbn_ld<T, VEC>(xc, v0);
#pragma unroll
            for (int j = 0; j < NS; ++j) piv[j] = v0[j * LP];
        }
        auto row = [&](const float* v) {
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                float d[LP], q[LP];
#pragma unroll
                for (int l = 0; l < LP; ++l) {
                    d[l] = v[j * LP + l] - piv[j];
                    q[l] = d[l] * d[l];
                }
                s1[j] += gbn_tree<LP>(d);
                s2[j] += gbn_tree<LP>(q);
            }
        };
        const long r0 = (long)blockIdx.y * rpb, r1 = min(M, r0 + rpb);
        constexpr int U = 4;                         // rows per trip, loads first (one 16-byte load in flight per thread is latency bound)
        long r = r0 + ty;
        for (; r + (long)(U - 1) * TY < r1; r += (long)U * TY) {
            float v[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) gbn_ld<T, VEC>(xc + (r + (long)u * TY) * C, v[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) row(v[u]);
        }
        for (; r < r1; r += TY) {
            float v[VEC];
            gbn_ld<T, VEC>(xc + r * C, v);
            row(v);
        }
    }
    gbn_fold_rows<NS>(red, s1, s2, tx, ty, TX, TY, col_ok, part, C / LP, col);
}

// fold of per-thread (a, b) over the GBN_FIN_LANES lanes of an item: thread = lane * GBN_FIN_G + item, so a wave holds 8 lanes x 8 items — xor-shuffles over
// the lane bits, then the waves' sums through LDS; fixed order, result in the threads of lane 0 (threadIdx.x < GBN_FIN_G)
__device__ __forceinline__ void gbn_fin_fold(double* sh, double& a, double& b) {
#pragma unroll
    for (int o = GBN_FIN_G; o < 64; o <<= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    const int wave = threadIdx.x >> 6, wl = threadIdx.x & 63;
    if (wl < GBN_FIN_G) {
        sh[(wave * GBN_FIN_G + wl) * 2 + 0] = a;
        sh[(wave * GBN_FIN_G + wl) * 2 + 1] = b;
    }
    __syncthreads();
    if (threadIdx.x < GBN_FIN_G) {
        a = b = 0.0;
#pragma unroll
        for (int w = 0; w < GBN_FIN_THREADS / 64; ++w) {
            a += sh[(w * GBN_FIN_G + threadIdx.x) * 2 + 0];
            b += sh[(w * GBN_FIN_G + threadIdx.x) * 2 + 1];
        }
    }
}
// sum over `n` entries of the two planes of the partials; entry i of an item lives at row i / K, column base + i % K of a [rows][2][stride] array.
// U entries per trip, all 2U loads issued before the first use (entries past the end re-read the lane's first and are zeroed).
__device__ __forceinline__ void gbn_fin_sum(const float* __restrict__ part, long n, int K, int stride, int base, int lane, bool ok, double& a, double& b) {
    a = b = 0.0;
    if (!ok) return;
    constexpr int U = 8;
    for (long k = lane; k < n; k += GBN_FIN_LANES * U) {
        float v0[U], v1[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long i = k + GBN_FIN_LANES * u < n ? k + GBN_FIN_LANES * u : k;
            const long row = i / K;
            const int cl = base + (int)(i - row * K);
            v0[u] = part[(row * 2 + 0) * stride + cl];
            v1[u] = part[(row * 2 + 1) * stride + cl];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool in = k + GBN_FIN_LANES * u < n;
            a += in ? (double)v0[u] : 0.0;
            b += in ? (double)v1[u] : 0.0;
        }
    }
}

// GBN_FIN_G groups per workgroup, GBN_FIN_LANES lanes per group over its K slots x nparts row blocks (double, fixed order); then the whole workgroup
// writes the per-channel outputs of its GBN_FIN_G * P channels.  batch_var is the BIASED variance (convnet.py:2337-2340: no M/(M-1)).
template <typename T>
__global__ __launch_bounds__(GBN_FIN_THREADS) void gbn_fwd_finalize_kernel(const T* __restrict__ x, const float* __restrict__ part, int nparts, long M, int C, int P, int K,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                               float* __restrict__ save_mean, float* __restrict__ save_invstd, float* __restrict__ batch_mean,
                                                               float* __restrict__ batch_var, float* __restrict__ running_mean, float* __restrict__ running_var,
                                                               float momentum, float* __restrict__ scale, float* __restrict__ shift) {
    __shared__ double sh[GBN_FIN_THREADS / 64 * GBN_FIN_G * 2];
    __shared__ float stat[GBN_FIN_G][3];
    const int G = C / P;
    const int gl = threadIdx.x % GBN_FIN_G, lane = threadIdx.x / GBN_FIN_G;
    const int g = blockIdx.x * GBN_FIN_G + gl;
    double a, b;
    gbn_fin_sum(part, (long)nparts * K, K, G * K, g * K, lane, g < G, a, b);
    gbn_fin_fold(sh, a, b);
    if (threadIdx.x < GBN_FIN_G && g < G) {
        const double inv_m = 1.0 / ((double)M * P);
        const double dm = a * inv_m;
        double var = b * inv_m - dm * dm;
        if (var < 0.0) var = 0.0;
        const float fmean = (float)((double)to_f32(x[g * P]) + dm), finv = (float)(1.0 / sqrt(var + (double)eps));
        save_mean[g] = fmean;
        save_invstd[g] = finv;
        stat[gl][0] = fmean;
        stat[gl][1] = finv;
        stat[gl][2] = (float)var;
    }
    __syncthreads();
    const int c_lo = blockIdx.x * GBN_FIN_G * P;
    for (int i = threadIdx.x; i < GBN_FIN_G * P && c_lo + i < C; i += GBN_FIN_THREADS) {
        const int c = c_lo + i;
        const float fmean = stat[i / P][0], finv = stat[i / P][1], fvar = stat[i / P][2];
        if (batch_mean) batch_mean[c] = fmean;
        if (batch_var) batch_var[c] = fvar;
        if (running_mean) running_mean[c] = momentum * running_mean[c] + (1.f - momentum) * fmean;
        if (running_var) running_var[c] = momentum * running_var[c] + (1.f - momentum) * fvar;
        const float sc = (gamma ? gamma[c] : 1.f) * finv;
        scale[c] = sc;
        shift[c] = (beta ? beta[c] : 0.f) - fmean * sc;
    }
}

// y = act(x*scale[c] + shift[c] [+ skip]); ACT: 0 none, 1 relu, 2 swish — the rounding points of bn_apply_kernel
template <typename T, int VEC, bool SKIP, int ACT>
__global__ __launch_bounds__(256) void gbn_apply_kernel(const T* __restrict__ x, const T* __restrict__ skip, T* __restrict__ y, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, long M, int C, int TX, int TY, long rpb) {
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int col = blockIdx.x * TX + tx;
    if (ty >= TY || col * VEC >= C) return;
    float sc[VEC], sh[VEC];
    gbn_ldc<VEC>(scale + col * VEC, sc, 1.f);
    gbn_ldc<VEC>(shift + col * VEC, sh, 0.f);
    const long base = (long)col * VEC;
    const long r0 = (long)blockIdx.y * rpb, r1 = min(M, r0 + rpb);
    auto row = [&](float (&v)[VEC], const float* k, long off) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            float o = fmaf(v[i], sc[i], sh[i]);
            if (SKIP) o += k[i];
            if (ACT == 1) o = fmaxf(o, 0.f);
            if (ACT == 2) o = o * fast_sigmoid(o);          // swish = z*sigmoid(z) (convnet.py:2553)
            v[i] = o;
        }
        gbn_st<T, VEC>(y + off, v);
    };
    constexpr int U = SKIP ? 2 : 4;
    long r = r0 + ty;
    for (; r + (long)(U - 1) * TY < r1; r += (long)U * TY) {
        float v[U][VEC], k[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long off = base + (r + (long)u * TY) * C;
            gbn_ld<T, VEC>(x + off, v[u]);
            if (SKIP) gbn_ld<T, VEC>(skip + off, k[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) row(v[u], k[u], base + (r + (long)u * TY) * C);
    }
    for (; r < r1; r += TY) {
        float v[VEC], k[VEC];
        gbn_ld<T, VEC>(x + base + r * C, v);
        if (SKIP) gbn_ld<T, VEC>(skip + base + r * C, k);
        row(v, k, base + r * C);
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// what a backward thread keeps per chunk: the group statistics of its lanes and, for the modes that recompute z = fma(x, sc, sh) from x, sc / sh
template <int VEC>
struct GbnCols {
    float mu[VEC], is[VEC], sc[VEC], sh[VEC];
};
template <int VEC, int MODE>
__device__ __forceinline__ void gbn_cols(GbnCols<VEC>& k, const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ gamma,
                                         const float* __restrict__ beta, int c0, int P) {
    gbn_ldg<VEC>(mean, c0, P, k.mu);
    gbn_ldg<VEC>(invstd, c0, P, k.is);
    if (MODE >= 2) {
        gbn_ldc<VEC>(gamma ? gamma + c0 : nullptr, k.sc, 1.f);
        gbn_ldc<VEC>(beta ? beta + c0 : nullptr, k.sh, 0.f);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            k.sc[i] *= k.is[i];
            k.sh[i] -= k.mu[i] * k.sc[i];
        }
    }
}
// MODE: 0 = no activation, 1 = ReLU mask from the stored output y, 2 = ReLU mask recomputed from x as [fma(x, sc, sh) > 0] (the expression the
// forward apply pass evaluated; forward without a fused residual only), 3 = swish, z recomputed the same way
template <int VEC, int MODE>
__device__ __forceinline__ float gbn_dz(const GbnCols<VEC>& k, int i, float g, float v, const float* o) {
    if (MODE == 1) return o[i] > 0.f ? g : 0.f;
    if (MODE == 2) return fmaf(v, k.sc[i], k.sh[i]) > 0.f ? g : 0.f;
    if (MODE == 3) return g * gbn_swish_grad(fmaf(v, k.sc[i], k.sh[i]));
    return g;
}

// part[(rb * 2 + {0, 1}) * C + c] = sum dz, sum dz * xhat over the block's rows
template <typename T, int VEC, int MODE>
__global__ __launch_bounds__(256) void gbn_bwd_reduce_kernel(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float* __restrict__ part, long M, int C, int P, int TX, int TY, long rpb) {
    extern __shared__ float red[];
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int col = blockIdx.x * TX + tx;
    const bool col_ok = col * VEC < C;
    float s1[VEC], s2[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) s1[i] = s2[i] = 0.f;
    if (ty < TY && col_ok) {
        GbnCols<VEC> k;
        gbn_cols<VEC, MODE>(k, mean, invstd, gamma, beta, col * VEC, P);
        const long base = (long)col * VEC;
        const long r0 = (long)blockIdx.y * rpb, r1 = min(M, r0 + rpb);
        auto row = [&](const float* g, const float* v, const float* o) {
#pragma unroll
            for (int i = 0; i < VEC; ++i) {
                const float gg = gbn_dz<VEC, MODE>(k, i, g[i], v[i], o);
                s1[i] += gg;
                s2[i] = fmaf(gg, (v[i] - k.mu[i]) * k.is[i], s2[i]);
            }
        };
        constexpr int U = (MODE == 1 || MODE == 3) ? 2 : 4;     // (swish at U = 4: 144 registers in the 2-byte types, 3 waves per SIMD)
        long r = r0 + ty;
        for (; r + (long)(U - 1) * TY < r1; r += (long)U * TY) {
            float g[U][VEC], v[U][VEC], o[U][VEC];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const long off = base + (r + (long)u * TY) * C;
                gbn_ld<T, VEC>(dy + off, g[u]);
                gbn_ld<T, VEC>(x + off, v[u]);
                if (MODE == 1) gbn_ld<T, VEC>(y + off, o[u]);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) row(g[u], v[u], o[u]);
        }
        for (; r < r1; r += TY) {
            float g[VEC], v[VEC], o[VEC];
            gbn_ld<T, VEC>(dy + base + r * C, g);
            gbn_ld<T, VEC>(x + base + r * C, v);
            if (MODE == 1) gbn_ld<T, VEC>(y + base + r * C, o);
            row(g, v, o);
        }
    }
    gbn_fold_rows<VEC>(red, s1, s2, tx, ty, TX, TY, col_ok, part, C, col);
}

// A workgroup owns whole groups: max(P, GBN_FIN_G) channels, GBN_FIN_G of them per trip with GBN_FIN_LANES lanes each over the nparts row blocks (double,
// fixed order).  The threads of lane 0 write dgamma / dbeta and keep gamma-weighted running sums; with P < GBN_FIN_G a trip holds
// GBN_FIN_G / P groups, folded over P adjacent threads, else the one group is folded over all GBN_FIN_G threads after the last trip.
// ca[g] = A_g / (M P), cb[g] = B_g / (M P).  (P = 8, the reference's default: one trip, the cost of bn_bwd_finalize_kernel.)
__global__ __launch_bounds__(GBN_FIN_THREADS) void gbn_bwd_finalize_kernel(const float* __restrict__ part, int nparts, long M, int C, int P, const float* __restrict__ gamma,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta, float grad_scale, float* __restrict__ ca,
                                                               float* __restrict__ cb) {
    __shared__ double sh[GBN_FIN_THREADS / 64 * GBN_FIN_G * 2];
    const int nch = P > GBN_FIN_G ? P : GBN_FIN_G;
    const int ch = threadIdx.x % GBN_FIN_G, lane = threadIdx.x / GBN_FIN_G;
    const int c_lo = blockIdx.x * nch;
    double A = 0.0, B = 0.0;
    for (int t = 0; t < nch; t += GBN_FIN_G) {
        const int c = c_lo + t + ch;
        const bool ok = t + ch < nch && c < C;
        double a, b;
        gbn_fin_sum(part, nparts, 1, C, c, lane, ok, a, b);
        if (t) __syncthreads();                              // the previous trip's readers of sh are done
        gbn_fin_fold(sh, a, b);
        if (threadIdx.x < GBN_FIN_G && ok) {
            if (dbeta) dbeta[c] = (float)a * grad_scale;
            if (dgamma) dgamma[c] = (float)b * grad_scale;
            const double gm = gamma ? (double)gamma[c] : 1.0;
            A += gm * a;
            B += gm * b;
        }
    }
    if (threadIdx.x >= 64) return;                           // (whole waves leave: the shuffles below run in wave 0)
    const int width = P < GBN_FIN_G ? P : GBN_FIN_G;
    for (int o = 1; o < width; o <<= 1) {
        A += __shfl_xor(A, o);
        B += __shfl_xor(B, o);
    }
    const int c = c_lo + ch;
    if (threadIdx.x < GBN_FIN_G && ch % width == 0 && c < C) {
        const double inv_m = 1.0 / ((double)M * P);
        ca[c / P] = (float)(A * inv_m);
        cb[c / P] = (float)(B * inv_m);
    }
}

// dx = invstd_g * (gamma*dz - ca_g - xhat*cb_g); dskip = dz
template <typename T, int VEC, int MODE, bool DSKIP>
__global__ __launch_bounds__(256) void gbn_bwd_apply_kernel(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ ca, const float* __restrict__ cb, T* __restrict__ dx, T* __restrict__ dskip,
                                                            long M, int C, int P, int TX, int TY, long rpb) {
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX;
    const int col = blockIdx.x * TX + tx;
    if (ty >= TY || col * VEC >= C) return;
    GbnCols<VEC> k;
    gbn_cols<VEC, MODE>(k, mean, invstd, gamma, beta, col * VEC, P);
    float gm[VEC], a[VEC], b[VEC];
    gbn_ldc<VEC>(gamma ? gamma + col * VEC : nullptr, gm, 1.f);
    gbn_ldg<VEC>(ca, col * VEC, P, a);
    gbn_ldg<VEC>(cb, col * VEC, P, b);
    const long base = (long)col * VEC;
    const long r0 = (long)blockIdx.y * rpb, r1 = min(M, r0 + rpb);
    auto row = [&](float (&g)[VEC], float (&v)[VEC], const float* o, long off) {
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            g[i] = gbn_dz<VEC, MODE>(k, i, g[i], v[i], o);
            const float xh = (v[i] - k.mu[i]) * k.is[i];
            v[i] = k.is[i] * (gm[i] * g[i] - a[i] - xh * b[i]);
        }
        gbn_st<T, VEC>(dx + off, v);
        if (DSKIP) gbn_st<T, VEC>(dskip + off, g);
    };
    constexpr int U = 2;
    long r = r0 + ty;
    for (; r + (long)(U - 1) * TY < r1; r += (long)U * TY) {
        float g[U][VEC], v[U][VEC], o[U][VEC];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long off = base + (r + (long)u * TY) * C;
            gbn_ld<T, VEC>(dy + off, g[u]);
            gbn_ld<T, VEC>(x + off, v[u]);
            if (MODE == 1) gbn_ld<T, VEC>(y + off, o[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) row(g[u], v[u], o[u], base + (r + (long)u * TY) * C);
    }
    for (; r < r1; r += TY) {
        float g[VEC], v[VEC], o[VEC];
        gbn_ld<T, VEC>(dy + base + r * C, g);
        gbn_ld<T, VEC>(x + base + r * C, v);
        if (MODE == 1) gbn_ld<T, VEC>(y + base + r * C, o);
        row(g, v, o, base + r * C);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
static size_t gbn_parts_bytes(int C) { return align_up((size_t)GBN_TARGET_BLOCKS * 2 * C * sizeof(float), 256); }     // (the backward's [row blocks][2][C] is the larger)
extern "C" size_t mcn_gbn_workspace_bytes(int64_t M, int32_t C, int32_t P) {
    if (M <= 0 || C <= 0 || P <= 0) return 0;
    return gbn_parts_bytes(C) + align_up((size_t)2 * C * sizeof(float), 256);      // partials + scale / shift [C] (forward) or ca / cb [G] (backward)
}

// argument checks shared by the two entry points (nothing here touches the device)
static int gbn_check(const char* who, long M, int C, int P, mcn_act act, bool residual, mcn_dtype dtype, const void* ws, size_t ws_bytes) {
    if (M <= 0 || C <= 0 || P <= 0 || M * C <= 0) MCN_FAIL(MCN_E_BADARG, "%s: bad argument (M=%ld C=%d P=%d)", who, M, C, P);
    if (C % P) MCN_FAIL(MCN_E_BADARG, "%s: %d channels are not a multiple of %d channels per group", who, C, P);
    if (!mcn_dtype_ok(dtype)) MCN_FAIL(MCN_E_UNSUPPORTED, "%s: dtype %d unsupported", who, (int)dtype);
    const int vec = dtype == MCN_F32 ? 4 : 8;
    if (C % vec) MCN_FAIL(MCN_E_UNSUPPORTED, "%s: C = %d is not a multiple of the 16-byte chunk (%d elements)", who, C, vec);
    if (P % vec && vec % P) MCN_FAIL(MCN_E_UNSUPPORTED, "%s: %d channels per group neither divide nor are a multiple of the 16-byte chunk (%d elements)", who, P, vec);
    if (act != MCN_ACT_NONE && act != MCN_ACT_RELU && act != MCN_ACT_SWISH) MCN_FAIL(MCN_E_UNSUPPORTED, "%s: activation %d is not fused (none / relu / swish)", who, (int)act);
    if (act == MCN_ACT_SWISH && residual) MCN_FAIL(MCN_E_UNSUPPORTED, "%s: swish with a fused residual is not built", who);
    if (!ws || ws_bytes < mcn_gbn_workspace_bytes(M, C, P)) MCN_FAIL(MCN_E_WORKSPACE, "%s: workspace too small", who);
    return MCN_OK;
}

template <typename T, int VEC, int LP>
static void gbn_launch_stats(const GbnLayout& L, hipStream_t st, const void* x, float* part, long M, int C, int P) {
    hipLaunchKernelGGL((gbn_stats_kernel<T, VEC, LP>), dim3(L.gx, L.gy), dim3(256), 2 * 256 * (VEC / LP) * sizeof(float), st, (const T*)x, part, M, C, P, L.TX, L.TY,
                       L.rpb);
}

template <typename T, int VEC>
static int gbn_fwd_t(const void* x, const float* gamma, const float* beta, const void* skip, void* y, float* save_mean, float* save_invstd, float* batch_mean,
                     float* batch_var, float* running_mean, float* running_var, float momentum, long M, int C, int P, float eps, mcn_act act, void* ws, hipStream_t st) {
    const GbnLayout L = gbn_layout(M, C, VEC);
    float* part = (float*)ws;
    float* scale = (float*)((char*)ws + gbn_parts_bytes(C));
    float* shift = scale + C;
    const int LP = P < VEC ? P : VEC, K = P / LP, G = C / P;
    if (LP == 1) gbn_launch_stats<T, VEC, 1>(L, st, x, part, M, C, P);
    else if (LP == 2) gbn_launch_stats<T, VEC, 2>(L, st, x, part, M, C, P);
    else if (LP == 4) gbn_launch_stats<T, VEC, 4>(L, st, x, part, M, C, P);
    else if constexpr (VEC == 8) gbn_launch_stats<T, VEC, 8>(L, st, x, part, M, C, P);
    MCN_CHECK_LAUNCH();
    hipLaunchKernelGGL((gbn_fwd_finalize_kernel<T>), dim3((G + GBN_FIN_G - 1) / GBN_FIN_G), dim3(GBN_FIN_THREADS), 0, st, (const T*)x, (const float*)part, L.gy, M, C, P, K, gamma, beta,
                       eps, save_mean, save_invstd, batch_mean, batch_var, running_mean, running_var, momentum, scale, shift);
    MCN_CHECK_LAUNCH();
    const dim3 grid(L.gx, L.gy), block(256);
    const int a = (int)act;
#define GBN_APPLY(SK, AC)                                                                                                                                          \
    hipLaunchKernelGGL((gbn_apply_kernel<T, VEC, SK, AC>), grid, block, 0, st, (const T*)x, (const T*)skip, (T*)y, (const float*)scale, (const float*)shift, M, C, L.TX, \
                       L.TY, L.rpb)
    if (skip) { if (a == 1) GBN_APPLY(true, 1); else GBN_APPLY(true, 0); }
    else { if (a == 1) GBN_APPLY(false, 1); else if (a == 2) GBN_APPLY(false, 2); else GBN_APPLY(false, 0); }
#undef GBN_APPLY
    MCN_CHECK_LAUNCH();
    return MCN_OK;
}

extern "C" int mcn_gbn_fwd_train(const void* x, const float* gamma, const float* beta, const void* skip, void* y, float* save_mean, float* save_invstd, float* batch_mean,
                                 float* batch_var, float* running_mean, float* running_var, float momentum, int64_t M, int32_t C, int32_t P, float eps, mcn_act act,
                                 mcn_dtype dtype, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !y || !save_mean || !save_invstd) MCN_FAIL(MCN_E_BADARG, "gbn_fwd_train: null tensor");
    const int rc = gbn_check("gbn_fwd_train", M, C, P, act, skip != nullptr, dtype, ws, ws_bytes);
    if (rc != MCN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
#define GBN_FWD_T(TT, VV) return gbn_fwd_t<TT, VV>(x, gamma, beta, skip, y, save_mean, save_invstd, batch_mean, batch_var, running_mean, running_var, momentum, M, C, P, eps, act, ws, st)
    if (dtype == MCN_F32) GBN_FWD_T(float, 4);
    if (dtype == MCN_BF16) GBN_FWD_T(bf16_t, 8);
    GBN_FWD_T(f16_t, 8);
#undef GBN_FWD_T
}

template <typename T, int VEC>
static int gbn_bwd_t(const void* dy, const void* x, const void* y, const float* gamma, const float* beta, const float* save_mean, const float* save_invstd, void* dx,
                     void* dskip, float* dgamma, float* dbeta, float grad_scale, long M, int C, int P, mcn_act act, void* ws, hipStream_t st) {
    const GbnLayout L = gbn_layout(M, C, VEC);
    float* part = (float*)ws;
    float* ca = (float*)((char*)ws + gbn_parts_bytes(C));
    float* cb = ca + C / P;
    const dim3 grid(L.gx, L.gy), block(256);
    const int mode = act == MCN_ACT_SWISH ? 3 : (act != MCN_ACT_RELU ? 0 : (y ? 1 : 2));
#define GBN_REDUCE(MD)                                                                                                                                         \
    hipLaunchKernelGGL((gbn_bwd_reduce_kernel<T, VEC, MD>), grid, block, 2 * 256 * VEC * sizeof(float), st, (const T*)dy, (const T*)x, (const T*)y, save_mean, \
                       save_invstd, gamma, beta, part, M, C, P, L.TX, L.TY, L.rpb)
    if (mode == 0) GBN_REDUCE(0); else if (mode == 1) GBN_REDUCE(1); else if (mode == 2) GBN_REDUCE(2); else GBN_REDUCE(3);
#undef GBN_REDUCE
    MCN_CHECK_LAUNCH();
    const int nch = P > GBN_FIN_G ? P : GBN_FIN_G;
    hipLaunchKernelGGL(gbn_bwd_finalize_kernel, dim3((C + nch - 1) / nch), dim3(GBN_FIN_THREADS), 0, st, (const float*)part, L.gy, M, C, P, gamma, dgamma, dbeta, grad_scale, ca, cb);
    MCN_CHECK_LAUNCH();
#define GBN_BWD_APPLY(MD, DS)                                                                                                                                   \
    hipLaunchKernelGGL((gbn_bwd_apply_kernel<T, VEC, MD, DS>), grid, block, 0, st, (const T*)dy, (const T*)x, (const T*)y, save_mean, save_invstd, gamma, beta, \
                       (const float*)ca, (const float*)cb, (T*)dx, (T*)dskip, M, C, P, L.TX, L.TY, L.rpb)
    if (mode == 1) { if (dskip) GBN_BWD_APPLY(1, true); else GBN_BWD_APPLY(1, false); }
    else if (mode == 2) { if (dskip) GBN_BWD_APPLY(2, true); else GBN_BWD_APPLY(2, false); }
    else if (mode == 3) GBN_BWD_APPLY(3, false);
    else { if (dskip) GBN_BWD_APPLY(0, true); else GBN_BWD_APPLY(0, false); }
#undef GBN_BWD_APPLY
    MCN_CHECK_LAUNCH();
    return MCN_OK;
}

extern "C" int mcn_gbn_bwd(const void* dy, const void* x, const void* y, const float* gamma, const float* beta, const float* save_mean, const float* save_invstd, void* dx,
                           void* dskip, float* dgamma, float* dbeta, float grad_scale, int64_t M, int32_t C, int32_t P, mcn_act act, mcn_dtype dtype, void* ws,
                           size_t ws_bytes, void* stream) {
    if (!dy || !x || !dx || !save_mean || !save_invstd) MCN_FAIL(MCN_E_BADARG, "gbn_bwd: null tensor");
    const int rc = gbn_check("gbn_bwd", M, C, P, act, dskip != nullptr, dtype, ws, ws_bytes);
    if (rc != MCN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
#define GBN_BWD_T(TT, VV) return gbn_bwd_t<TT, VV>(dy, x, y, gamma, beta, save_mean, save_invstd, dx, dskip, dgamma, dbeta, grad_scale, M, C, P, act, ws, st)
    if (dtype == MCN_F32) GBN_BWD_T(float, 4);
    if (dtype == MCN_BF16) GBN_BWD_T(bf16_t, 8);
    GBN_BWD_T(f16_t, 8);
#undef GBN_BWD_T
}
