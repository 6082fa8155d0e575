// ws.hip — weight standardisation of conv filters (reference convnet.py:1410-1419) for gfx950.
//
// An fp32 HWIO filter is a row-major matrix w[K][C] (K = KH*KW*Cin rows, C = Cout columns, C innermost); per column
//   m = mean_k w,  s = sqrt(mean_k (w - m)^2),  w_hat = (w - m) / (s + eps)                 (epsilon outside the root)
// and, backward, with r = 1 / (s + eps):
//   dw = r * (dw_hat - mean_k dw_hat) - w_hat * mean_k(dw_hat * w_hat) / s.
//
// How the work is split.  A model's filters differ in size by a factor of ~600 (ResNet-50: 64x64 ... 4608x512) and there are 53 of them, so the
// forward runs ALL of them from one descriptor table in two launches: a descriptor is (tensor, 32-column strip, row slice of <= WS_SLICE_ROWS rows),
// one workgroup per descriptor, every descriptor moves at most 32 KB.  A strip is 128 bytes per row: 8 sixteen-byte chunks x 32 row lanes = 256
// threads (C % 4 != 0 or unaligned pointers: 32 scalar columns x 8 row lanes).
//   launch 1: per descriptor the pivot-shifted fp32 sums (sum d, sum d^2, d = w - w[0][c]: the pivot is the tensor's first row, the same for every
//             slice), row lanes folded through LDS in lane order -> one partial row [2][32] per descriptor in the workspace.
//   launch 2: every workgroup folds the slices of its strip in double, in slice order (each slice of a strip repeats the same few additions and
//             gets the same bits), slice 0 writes (m, s); then the workgroup re-reads its rows (32 KB: L2) and writes w_hat with streaming stores.
// The backward is one call per filter with the same strip / slice split as its grid: sums (sum g, sum g * w_hat), then the apply pass; every element
// is read and written by the same thread, so dw may alias dw_hat.  No atomics anywhere: a repeated run is bit-identical, and a tensor's result
// does not depend on what else is in the table.
#include "common.h"

namespace {

constexpr int WS_STRIP = 32;          // columns per strip
constexpr int WS_THREADS = 256;
constexpr int WS_SLICE_ROWS = 256;    // rows per descriptor at most: 256 x 128 bytes = 32 KB
constexpr int WS_PART = 2 * WS_STRIP; // floats of one descriptor's partial row

struct WsDesc {
    const float* w;
    float* w_hat;
    float* stats;                     // [2][C]: m, s
    int32_t K, C, c0, r0, r1;         // strip [c0, c0 + 32), rows [r0, r1)
    int32_t first, nslices;           // descriptor index of this strip's slice 0, slices of the strip
    int32_t vec;                      // 1: rows are 16-byte aligned (C % 4 == 0 and aligned pointers)
};

inline int ws_nstrips(int C) { return (C + WS_STRIP - 1) / WS_STRIP; }
inline int ws_nslices(int K) { return (K + WS_SLICE_ROWS - 1) / WS_SLICE_ROWS; }
inline int ws_slice_rows(int K) { const int n = ws_nslices(K); return (K + n - 1) / n; }
inline bool ws_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

// V columns per thread: 4 (one 16-byte chunk; 8 column lanes x 32 row lanes) or 1 (32 column lanes x 8 row lanes)
template <int V>
struct WsLanes {
    static constexpr int CL = WS_STRIP / V, RL = WS_THREADS / CL;
};

template <int V>
__device__ __forceinline__ void ws_load(const float* p, bool ok, float (&v)[V]) {
    if constexpr (V == 4) {
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        if (ok) t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = t[j];
    } else {
        v[0] = ok ? *p : 0.f;
    }
}
template <int V>
__device__ __forceinline__ void ws_store(float* p, bool ok, const float (&v)[V], bool streaming) {
    if (!ok) return;
    if constexpr (V == 4) {
        const f32x4 t = {v[0], v[1], v[2], v[3]};
        if (streaming) __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(p));
        else *reinterpret_cast<f32x4*>(p) = t;
    } else {
        if (streaming) __builtin_nontemporal_store(v[0], p);
        else *p = v[0];
    }
}

// per-thread accumulators (a, b) of the strip's columns -> part[2][32]: the row lanes are added in lane order by one thread per (plane, column)
template <int V>
__device__ __forceinline__ void ws_fold_lanes(const float (&a)[V], const float (&b)[V], float* part, float* sh) {
    constexpr int CL = WsLanes<V>::CL, RL = WsLanes<V>::RL;
    const int cl = threadIdx.x % CL, lr = threadIdx.x / CL;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        sh[lr * WS_STRIP + cl * V + j] = a[j];
        sh[(RL + lr) * WS_STRIP + cl * V + j] = b[j];
    }
    __syncthreads();
    if (threadIdx.x < WS_PART) {
        const int plane = threadIdx.x / WS_STRIP, c = threadIdx.x % WS_STRIP;
        float s = 0.f;
        for (int l = 0; l < RL; ++l) s += sh[(plane * RL + l) * WS_STRIP + c];
        part[plane * WS_STRIP + c] = s;
    }
}

// sums over rows [r0, r1) of the strip at c0: MODE 0 (forward) a = sum (p - pivot), b = sum (p - pivot)^2 with p = w;
// MODE 1 (backward) a = sum p, b = sum p * q with p = dw_hat, q = w_hat.  Four rows in flight per thread.
template <int V, int MODE>
__device__ __forceinline__ void ws_partial(const float* p, const float* q, int C, int c0, int r0, int r1, float* part, float* sh) {
    constexpr int CL = WsLanes<V>::CL, RL = WsLanes<V>::RL;
    const int cl = threadIdx.x % CL, lr = threadIdx.x / CL;
    const int c = c0 + cl * V;
    const bool ok = c < C;
    float piv[V], a[V], b[V];
    if (MODE == 0) ws_load<V>(p + c, ok, piv);
#pragma unroll
    for (int j = 0; j < V; ++j) a[j] = b[j] = 0.f;
    auto add = [&](const float (&x)[V], const float (&y)[V]) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (MODE == 0) {
                const float d = x[j] - piv[j];
                a[j] += d;
                b[j] = fmaf(d, d, b[j]);
            } else {
                a[j] += x[j];
                b[j] = fmaf(x[j], y[j], b[j]);
            }
        }
    };
    int r = r0 + lr;
    for (; r + 3 * RL < r1; r += 4 * RL) {
        float x[4][V], y[4][V];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ws_load<V>(p + (size_t)(r + u * RL) * C + c, ok, x[u]);
            if (MODE == 1) ws_load<V>(q + (size_t)(r + u * RL) * C + c, ok, y[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) add(x[u], MODE == 1 ? y[u] : x[u]);
    }
    for (; r < r1; r += RL) {
        float x[V], y[V];
        ws_load<V>(p + (size_t)r * C + c, ok, x);
        if (MODE == 1) ws_load<V>(q + (size_t)r * C + c, ok, y);
        add(x, MODE == 1 ? y : x);
    }
    ws_fold_lanes<V>(a, b, part, sh);
}

// the strip's slices folded in double in slice order by one thread per column: (A, B) = (sum a, sum b) / K
__device__ __forceinline__ void ws_fold_slices(const float* parts, int first, int nslices, int K, int col, double* A, double* B) {
    double a = 0.0, b = 0.0;
    for (int s = 0; s < nslices; ++s) {
        const float* p = parts + (size_t)(first + s) * WS_PART;
        a += (double)p[col];
        b += (double)p[WS_STRIP + col];
    }
    *A = a / (double)K;
    *B = b / (double)K;
}

// out = (p - sub[c]) * mul[c] - q * mq[c] over rows [r0, r1) of the strip (forward: q unused, mq = 0)
template <int V, int MODE>
__device__ __forceinline__ void ws_apply(const float* p, const float* q, float* out, int C, int c0, int r0, int r1, const float* sh) {
    constexpr int CL = WsLanes<V>::CL, RL = WsLanes<V>::RL;
    const int cl = threadIdx.x % CL, lr = threadIdx.x / CL;
    const int c = c0 + cl * V;
    const bool ok = c < C;
    float sub[V], mul[V], mq[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        sub[j] = sh[cl * V + j];
        mul[j] = sh[WS_STRIP + cl * V + j];
        mq[j] = sh[2 * WS_STRIP + cl * V + j];
    }
    auto one = [&](const float (&x)[V], const float (&y)[V], size_t at) {
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            o[j] = (x[j] - sub[j]) * mul[j];
            if (MODE == 1) o[j] -= y[j] * mq[j];
        }
        ws_store<V>(out + at, ok, o, MODE == 0);      // w_hat streams out (the pack reads it from memory); dw stays cached for the optimizer
    };
    int r = r0 + lr;
    for (; r + 3 * RL < r1; r += 4 * RL) {
        float x[4][V], y[4][V];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ws_load<V>(p + (size_t)(r + u * RL) * C + c, ok, x[u]);
            if (MODE == 1) ws_load<V>(q + (size_t)(r + u * RL) * C + c, ok, y[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) one(x[u], MODE == 1 ? y[u] : x[u], (size_t)(r + u * RL) * C + c);
    }
    for (; r < r1; r += RL) {
        float x[V], y[V];
        ws_load<V>(p + (size_t)r * C + c, ok, x);
        if (MODE == 1) ws_load<V>(q + (size_t)r * C + c, ok, y);
        one(x, MODE == 1 ? y : x, (size_t)r * C + c);
    }
}

// ---- forward: one workgroup per descriptor -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WS_THREADS) void ws_fwd_sums(const WsDesc* table, float* parts) {
    __shared__ float sh[2 * 32 * WS_STRIP];
    const WsDesc d = table[blockIdx.x];
    float* part = parts + (size_t)blockIdx.x * WS_PART;
    if (d.vec) ws_partial<4, 0>(d.w, nullptr, d.C, d.c0, d.r0, d.r1, part, sh);
    else ws_partial<1, 0>(d.w, nullptr, d.C, d.c0, d.r0, d.r1, part, sh);
}

__global__ __launch_bounds__(WS_THREADS) void ws_fwd_apply(const WsDesc* table, const float* parts, float eps) {
    __shared__ float sh[3 * WS_STRIP];
    const WsDesc d = table[blockIdx.x];
    if (threadIdx.x < WS_STRIP) {
        const int col = threadIdx.x, c = d.c0 + col;
        float m = 0.f, r = 0.f;
        if (c < d.C) {
            double A, B;
            ws_fold_slices(parts, d.first, d.nslices, d.K, col, &A, &B);
            double var = B - A * A;
            if (var < 0.0) var = 0.0;
            m = (float)((double)d.w[c] + A);
            const float s = (float)sqrt(var);
            r = 1.f / (s + eps);
            if (d.r0 == 0) {
                d.stats[c] = m;
                d.stats[d.C + c] = s;
            }
        }
        sh[col] = m;
        sh[WS_STRIP + col] = r;
        sh[2 * WS_STRIP + col] = 0.f;
    }
    __syncthreads();
    if (d.vec) ws_apply<4, 0>(d.w, nullptr, d.w_hat, d.C, d.c0, d.r0, d.r1, sh);
    else ws_apply<1, 0>(d.w, nullptr, d.w_hat, d.C, d.c0, d.r0, d.r1, sh);
}

// ---- backward: grid = strips x slices of one filter ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(WS_THREADS) void ws_bwd_sums(const float* dw_hat, const float* w_hat, float* parts, int K, int C, int nslices, int rows, int vec) {
    __shared__ float sh[2 * 32 * WS_STRIP];
    const int strip = blockIdx.x / nslices, slice = blockIdx.x % nslices;
    const int r0 = min(slice * rows, K), r1 = min(r0 + rows, K);
    float* part = parts + (size_t)blockIdx.x * WS_PART;
    if (vec) ws_partial<4, 1>(dw_hat, w_hat, C, strip * WS_STRIP, r0, r1, part, sh);
    else ws_partial<1, 1>(dw_hat, w_hat, C, strip * WS_STRIP, r0, r1, part, sh);
}

// (dw_hat and dw may be the same buffer: no __restrict__ here)
__global__ __launch_bounds__(WS_THREADS) void ws_bwd_apply(const float* dw_hat, const float* w_hat, const float* stats, float* dw, const float* parts, int K, int C,
                                                          int nslices, int rows, float eps, int vec) {
    __shared__ float sh[3 * WS_STRIP];
    const int strip = blockIdx.x / nslices, slice = blockIdx.x % nslices;
    const int r0 = min(slice * rows, K), r1 = min(r0 + rows, K);
    if (threadIdx.x < WS_STRIP) {
        const int col = threadIdx.x, c = strip * WS_STRIP + col;
        float ma = 0.f, r = 0.f, mb = 0.f;
        if (c < C) {
            double A, B;
            ws_fold_slices(parts, strip * nslices, nslices, K, col, &A, &B);
            const float s = stats[C + c];
            ma = (float)A;
            r = 1.f / (s + eps);
            mb = (float)(B / (double)s);
        }
        sh[col] = ma;
        sh[WS_STRIP + col] = r;
        sh[2 * WS_STRIP + col] = mb;
    }
    __syncthreads();
    if (vec) ws_apply<4, 1>(dw_hat, w_hat, dw, C, strip * WS_STRIP, r0, r1, sh);
    else ws_apply<1, 1>(dw_hat, w_hat, dw, C, strip * WS_STRIP, r0, r1, sh);
}

size_t ws_job_descs(const mcn_ws_job& j) { return (j.K > 0 && j.C > 0) ? (size_t)ws_nstrips(j.C) * ws_nslices(j.K) : 0; }

}  // namespace

extern "C" size_t mcn_ws_table_bytes(const mcn_ws_job* jobs, int32_t njobs) {
    size_t n = 0;
    for (int i = 0; jobs && i < njobs; ++i) n += ws_job_descs(jobs[i]);
    return n * sizeof(WsDesc);
}

extern "C" size_t mcn_ws_fwd_workspace_bytes(const mcn_ws_job* jobs, int32_t njobs) {
    return mcn_ws_table_bytes(jobs, njobs) / sizeof(WsDesc) * WS_PART * sizeof(float);
}

extern "C" int mcn_ws_table_build(const mcn_ws_job* jobs, int32_t njobs, void* host_table, size_t bytes, int32_t* ndesc) {
    if (!jobs || !host_table || !ndesc || njobs <= 0) MCN_FAIL(MCN_E_BADARG, "ws_table_build: bad argument");
    for (int i = 0; i < njobs; ++i) {
        const mcn_ws_job& j = jobs[i];
        if (!j.w || !j.w_hat || !j.stats) MCN_FAIL(MCN_E_BADARG, "ws_table_build: job %d has a null pointer", i);
        if (j.C < 1 || j.K < 1) MCN_FAIL(MCN_E_BADARG, "ws_table_build: job %d has K = %d, C = %d", i, j.K, j.C);
        if (j.K == 1) MCN_FAIL(MCN_E_BADARG, "ws_table_build: job %d has K = 1: the deviation of one row is 0 and its gradient undefined (convnet.py:1410-1419)", i);
    }
    if (bytes < mcn_ws_table_bytes(jobs, njobs)) MCN_FAIL(MCN_E_WORKSPACE, "ws_table_build: table buffer too small");
    WsDesc* out = (WsDesc*)host_table;
    int32_t n = 0;
    for (int i = 0; i < njobs; ++i) {
        const mcn_ws_job& j = jobs[i];
        const int nsl = ws_nslices(j.K), rows = ws_slice_rows(j.K);
        const int vec = (j.C % 4 == 0 && ws_aligned(j.w) && ws_aligned(j.w_hat)) ? 1 : 0;
        for (int s = 0; s < ws_nstrips(j.C); ++s) {
            const int32_t first = n;
            for (int sl = 0; sl < nsl; ++sl) {
                const int r0 = sl * rows < j.K ? sl * rows : j.K;
                const int r1 = r0 + rows < j.K ? r0 + rows : j.K;
                out[n++] = WsDesc{j.w, j.w_hat, j.stats, j.K, j.C, s * WS_STRIP, r0, r1, first, nsl, vec};
            }
        }
    }
    *ndesc = n;
    return MCN_OK;
}

extern "C" int mcn_ws_fwd_run(const void* dev_table, int32_t ndesc, float eps, void* workspace, size_t workspace_bytes, void* stream) {
    if (!dev_table || ndesc <= 0) MCN_FAIL(MCN_E_BADARG, "ws_fwd_run: null or empty table");
    if (!workspace || workspace_bytes < (size_t)ndesc * WS_PART * sizeof(float))
        MCN_FAIL(MCN_E_WORKSPACE, "ws_fwd_run: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0, (size_t)ndesc * WS_PART * sizeof(float));
    hipStream_t st = (hipStream_t)stream;
    ws_fwd_sums<<<dim3(ndesc), dim3(WS_THREADS), 0, st>>>((const WsDesc*)dev_table, (float*)workspace);
    ws_fwd_apply<<<dim3(ndesc), dim3(WS_THREADS), 0, st>>>((const WsDesc*)dev_table, (const float*)workspace, eps);
    MCN_CHECK_LAUNCH();
    return MCN_OK;
}

extern "C" size_t mcn_ws_bwd_workspace_bytes(int32_t K, int32_t C) {
    if (K < 1 || C < 1) return 0;
    return (size_t)ws_nstrips(C) * ws_nslices(K) * WS_PART * sizeof(float);
}

extern "C" int mcn_ws_bwd(const float* dw_hat, const float* w_hat, const float* stats, float* dw, int32_t K, int32_t C, float eps, void* workspace,
                          size_t workspace_bytes, void* stream) {
    if (!dw_hat || !w_hat || !stats || !dw) MCN_FAIL(MCN_E_BADARG, "ws_bwd: null tensor");
    if (K < 1 || C < 1) MCN_FAIL(MCN_E_BADARG, "ws_bwd: K = %d, C = %d", K, C);
    if (K == 1) MCN_FAIL(MCN_E_BADARG, "ws_bwd: K = 1: the deviation of one row is 0 and its gradient undefined (convnet.py:1410-1419)");
    if (!workspace || workspace_bytes < mcn_ws_bwd_workspace_bytes(K, C))
        MCN_FAIL(MCN_E_WORKSPACE, "ws_bwd: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0, mcn_ws_bwd_workspace_bytes(K, C));
    const int nsl = ws_nslices(K), rows = ws_slice_rows(K), grid = ws_nstrips(C) * nsl;
    const int vec = (C % 4 == 0 && ws_aligned(dw_hat) && ws_aligned(w_hat) && ws_aligned(dw)) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    ws_bwd_sums<<<dim3(grid), dim3(WS_THREADS), 0, st>>>(dw_hat, w_hat, (float*)workspace, K, C, nsl, rows, vec);
    ws_bwd_apply<<<dim3(grid), dim3(WS_THREADS), 0, st>>>(dw_hat, w_hat, stats, dw, (const float*)workspace, K, C, nsl, rows, eps, vec);
    MCN_CHECK_LAUNCH();
    return MCN_OK;
}
