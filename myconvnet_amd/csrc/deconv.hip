// deconv.hip — transposed convolution (reference convnet.py:2408-2498 -> tf.nn.conv2d_transpose [+ tf.nn.bias_add]).
//
//   y[n,oy,ox,cb] = bias[cb] + sum_{r,q,cs} x[n,(oy+padT-r)/SH,(ox+padL-q)/SW,cs] * w[r][q][cs][cb]     (divisible, in-range terms only)
//
// deconv_fused: ALL stride phases of the output in one launch from one staged input window.  Base coordinates: output pixel oy belongs to
// phase ph = (oy + padT) % SH and base row by = (oy + padT) / SH; tap r = ph + SH * jr of that phase reads input row by - jr.  A workgroup
// (4 waves) owns a TH x TW tile of base pixels of one image and BN output channels.  Per K-step (128 bytes of Cs) the window — tile plus
// the halo of JH = (KH-1)/SH rows above and JW = (KW-1)/SW columns left — is staged ONCE by LDS-DMA (XOR-swizzled 128-byte rows, the
// conventions of conv_gemm_nt_win; window elements outside the image are zero by the bounds-checked buffer addressing, as are channel
// chunks >= Cs and filter rows >= Cb), double-buffered: the window of step cb + 1 is issued at tap 0 of step cb (the vmcnt(0) in front of
// every tap's barrier makes it land before tap 1: one tap of latency is hidden, no barrier is added at the chunk boundary).  The filter slices of
// the KH*KW taps stream through two LDS buffers in the order the pack wrote them (phase-major), one barrier per (K-step, tap).  Every phase
// keeps its own accumulator set and every wave computes all phases of its own slice of (pixels, Cb): the phases' unequal tap counts
// (9/6/6/4 for 5x5/2) cost no wave any idle time.  Epilogue: bias in fp32, one rounding, the phases interleaved through LDS into full
// resolution rows and stored as contiguous runs (16-byte chunks when Cb is a chunk multiple, scalar otherwise; masked to Cb and the image).
// The narrow instantiation (Cb <= 16: an image-producing layer) uses an N block of one MFMA tile.  No atomics: bit-identical repeats.
//
// deconv_gather: one thread per output element, any geometry (stride >= 3, Cs not a chunk multiple, kernels > 7).
// The backward is the strided convolution of the same geometry on existing kernels: dx = mcn_conv2d_fwd(dy) with the filter's two channel
// axes swapped (filter_swap_io: fp32 tile transpose through LDS), dw = swap(mcn_conv2d_wgrad(x := dy, dy := x)), dbias = mcn_bias_grad(dy).
#include "mma_nt.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define DC_MAXPASS 10            /* window rows <= (8 + 6) * (16 + 6) = 308 -> 10 staging passes of 32 rows */

struct DeconvParams {
    const void* x;
    const void* wp;
    const float* bias;
    void* y;
    int N, h, w, Cs, Cb, OH, OW;
    int SH, SW, padT, padL;
    int JH, JW, WW, wrows;               // halo, window width and rows
    int by_min, bx_min, tiles_y, tiles_x, ntn;
    int ksteps, cchunks, ntaps;          // K-steps of 128 bytes; valid 16-byte chunks per pixel (Cs / CE)
    unsigned img_bytes, wt_bytes, krow_bytes;
    int tap_begin[5];                    // taps of phase p = ph * SW + pw: [tap_begin[p], tap_begin[p + 1])
    int tap[MCN_MAX_TAPS];               // jr | jq << 16
};

template <typename T, int TH, int TW, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void deconv_fused(const DeconvParams p) {
    typedef MmaNT<T> MM;
    constexpr int BM = TH * TW, WTM = BM / WM, WTN = BN / WN, TM = WTM / MM::MT, TN = WTN / MM::MT;
    constexpr int BNL = BN < 32 ? 32 : BN, BR = BNL / 32, CE = VecTraits<T>::CE;
    constexpr int ACCSZ = (int)(sizeof(typename MM::Acc) / 4);
    static_assert(WM * WN == 4 && TM >= 1 && TN >= 1 && WTM % MM::MT == 0 && WTN % MM::MT == 0, "4 waves, whole MFMA tiles");
    static_assert((TW & (TW - 1)) == 0, "tile width is a power of two");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    int b = blockIdx.x;
    const int n0 = (b % p.ntn) * BN;
    b /= p.ntn;
    const int bx0 = p.bx_min + (b % p.tiles_x) * TW;
    b /= p.tiles_x;
    const int by0 = p.by_min + (b % p.tiles_y) * TH;
    const int img = b / p.tiles_y;

    const char* ximg = reinterpret_cast<const char*>(p.x) + (size_t)img * p.img_bytes;
    const __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(ximg), 0, (int)p.img_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsB = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.wp), 0, (int)p.wt_bytes, 0x00020000);

    // LDS: [window 0][window 1][B 0][B 1]
    const int WW = p.WW;
    const int wrows_alloc = (p.wrows + 31) & ~31;
    const int WB = wrows_alloc * 128;
    const int crow = tid >> 3;
    auto wkey = [](int r) -> int { return sizeof(T) == 4 ? ((r >> 1) & 7) : (r & 7); };      // (see conv_gemm_nt_win)
    const int cid = (tid & 7) ^ ((crow >> 1) & 7);       // B tile: source chunk of this thread's LDS slot (pass-invariant: 32 rows per pass)
    const int cidw = (tid & 7) ^ wkey(crow);             // window rows likewise
    unsigned woff[DC_MAXPASS];                           // byte offset of this thread's window pixel per pass (MCN_OOB: outside the image)
#pragma unroll
    for (int ps = 0; ps < DC_MAXPASS; ++ps) {
        const int j = ps * 32 + crow;
        const int wy = j / WW, wx = j - wy * WW;
        const int iy = by0 - p.JH + wy, ix = bx0 - p.JW + wx;
        const bool ok = j < p.wrows && (unsigned)iy < (unsigned)p.h && (unsigned)ix < (unsigned)p.w;
        woff[ps] = ok ? (unsigned)(iy * p.w + ix) * (unsigned)(p.Cs * (int)sizeof(T)) : MCN_OOB;
    }
    unsigned b_off[BR];
#pragma unroll
    for (int i = 0; i < BR; ++i) {
        const int n = n0 + crow + 32 * i;
        b_off[i] = (crow + 32 * i < BN && n < p.Cb) ? (unsigned)n * p.krow_bytes + (unsigned)cid * 16u : MCN_OOB;
    }
    __attribute__((address_space(3))) char* const lds = (__attribute__((address_space(3))) char*)smem;
    auto issue_window = [&](int cb) {
        __attribute__((address_space(3))) char* const base = lds + __builtin_amdgcn_readfirstlane(wave * 1024 + (cb & 1) * WB);
        const int c = cb * 8 + cidw;
        const unsigned coff = c < p.cchunks ? (unsigned)c * 16u : MCN_OOB;
        static_for<DC_MAXPASS>([&](auto pc) {
            constexpr int ps = decltype(pc)::value;
            if (ps * 32 < wrows_alloc)                   // (uniform)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (__attribute__((address_space(3))) void*)(base + ps * 32 * 128), 16, (int)((woff[ps] + (coff & 0x7fffffffu)) | ((woff[ps] | coff) & MCN_OOB)), 0, 0, MCN_DMA_AUX_A);
        });
    };
    auto issue_b = [&](int cb, int t, int buf) {
        __attribute__((address_space(3))) char* const base = lds + __builtin_amdgcn_readfirstlane(wave * 1024 + 2 * WB + buf * (BNL * 128));
        const unsigned koff = (unsigned)(t * p.ksteps + cb) * 128u;
        static_for<BR>([&](auto ic) {
            constexpr int i = decltype(ic)::value;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (__attribute__((address_space(3))) void*)(base + i * 32 * 128), 16, (int)(b_off[i] + koff), 0, 0, 0);
        });
    };

    const int fr = MM::frag_row(lane), fc = MM::frag_chunk(lane);
    int rloc[TM];                                        // window row of the lane's own base pixel (tap (0, 0))
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int mi = wm * WTM + i * MM::MT + fr;
        rloc[i] = (mi / TW + p.JH) * WW + (mi % TW) + p.JW;
    }
    int brow[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) brow[j] = wn * WTN + j * MM::MT + fr;

    typename MM::Acc acc[4][TN][TM];
#pragma unroll
    for (int ph = 0; ph < 4; ++ph)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int e = 0; e < ACCSZ; ++e) acc[ph][j][i][e] = 0.f;

    const int ntaps = p.ntaps, nsteps = p.ksteps * ntaps;
    int sb = 0, s = 0;
    if (nsteps > 0) {
        issue_window(0);
        issue_b(0, 0, 0);
    }
    for (int cb = 0; cb < p.ksteps; ++cb) {
        const char* const win = smem + (cb & 1) * WB;
        static_for<4>([&](auto phc) {
            constexpr int PH = decltype(phc)::value;
            for (int t = p.tap_begin[PH]; t < p.tap_begin[PH + 1]; ++t) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (t == 0 && cb + 1 < p.ksteps) issue_window(cb + 1);
                if (s + 1 < nsteps) {
                    if (t + 1 < ntaps) issue_b(cb, t + 1, sb ^ 1);
                    else issue_b(cb + 1, 0, sb ^ 1);
                }
                const char* const bb = smem + 2 * WB + sb * (BNL * 128);
                const int tw = p.tap[t];
                const int sh = (tw & 0xffff) * WW + (tw >> 16);
                int abase[TM], akey[TM];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int wr = rloc[i] - sh;
                    abase[i] = wr << 7;
                    akey[i] = wkey(wr);
                }
#pragma unroll
                for (int sl = 0; sl < MM::SLABS; ++sl) {
                    const int ch = sl * MM::CPS + fc;
                    typename MM::Frag xa[TM], wb[TN];
#pragma unroll
                    for (int i = 0; i < TM; ++i) xa[i] = *reinterpret_cast<const typename MM::Frag*>(win + abase[i] + ((ch ^ akey[i]) << 4));
#pragma unroll
                    for (int j = 0; j < TN; ++j) wb[j] = *reinterpret_cast<const typename MM::Frag*>(bb + brow[j] * 128 + ((ch ^ ((brow[j] >> 1) & 7)) << 4));
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int i = 0; i < TM; ++i) MM::mma(acc[PH][j][i], wb[j], xa[i]);
                }
                sb ^= 1;
                ++s;
            }
        });
    }

    // ---- epilogue: phases interleaved through LDS into [TH*SH][TW*SW][BN] of T, then contiguous stores ----
    __syncthreads();
    T* const ot = reinterpret_cast<T*>(smem);
    const int OTW = TW * p.SW, OTH = TH * p.SH;
    static_for<4>([&](auto phc) {
        constexpr int PH = decltype(phc)::value;
        if (PH < p.SH * p.SW) {
            const int ph = PH / p.SW, pw = PH - ph * p.SW;
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int mi = wm * WTM + i * MM::MT + (MM::MT == 16 ? (lane & 15) : (lane & 31));
                    const int pix = ((mi / TW) * p.SH + ph) * OTW + (mi % TW) * p.SW + pw;
#pragma unroll
                    for (int e = 0; e < ACCSZ; ++e) {
                        const int nl = wn * WTN + j * MM::MT + (MM::MT == 16 ? (lane >> 4) * 4 + e : (e >> 2) * 8 + (lane >> 5) * 4 + (e & 3));
                        const float bv = (p.bias != nullptr && n0 + nl < p.Cb) ? p.bias[n0 + nl] : 0.f;
                        ot[pix * BN + nl] = from_f32<T>(acc[PH][j][i][e] + bv);
                    }
                }
        }
    });
    __syncthreads();
    const int oy_base = by0 * p.SH - p.padT, ox_base = bx0 * p.SW - p.padL;
    T* const yimg = reinterpret_cast<T*>(p.y) + (size_t)img * p.OH * p.OW * p.Cb;
    const int nvalid = min(BN, p.Cb - n0);
    if (p.Cb % CE == 0) {
        constexpr int CPP = BN / CE;
        const int total = OTH * OTW * CPP;
        for (int idx = tid; idx < total; idx += 256) {
            const int c = idx % CPP, pix = idx / CPP;
            const int orow = pix / OTW, ocol = pix - orow * OTW;
            const int oy = oy_base + orow, ox = ox_base + ocol;
            if ((unsigned)oy < (unsigned)p.OH && (unsigned)ox < (unsigned)p.OW && c * CE < nvalid)
                *reinterpret_cast<i32x4*>(yimg + ((size_t)oy * p.OW + ox) * p.Cb + n0 + c * CE) = *reinterpret_cast<const i32x4*>(ot + pix * BN + c * CE);
        }
    } else {
        const int total = OTH * OTW * BN;
        for (int idx = tid; idx < total; idx += 256) {
            const int c = idx % BN, pix = idx / BN;
            const int orow = pix / OTW, ocol = pix - orow * OTW;
            const int oy = oy_base + orow, ox = ox_base + ocol;
            if ((unsigned)oy < (unsigned)p.OH && (unsigned)ox < (unsigned)p.OW && c < nvalid)
                yimg[((size_t)oy * p.OW + ox) * p.Cb + n0 + c] = ot[pix * BN + c];
        }
    }
}

// ---- gather fallback: one thread per output element ------------------------------------------------------------------------------
struct DeconvGatherParams {
    const void* x;
    const float* w;
    const float* bias;
    void* y;
    int N, h, w_, Cs, Cb, OH, OW, KH, KW, SH, SW, padT, padL;
};
template <typename T>
__global__ __launch_bounds__(256) void deconv_gather(const DeconvGatherParams p) {
    const long total = (long)p.N * p.OH * p.OW * p.Cb;
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int cb = (int)(id % p.Cb);
    long r_ = id / p.Cb;
    const int ox = (int)(r_ % p.OW);
    r_ /= p.OW;
    const int oy = (int)(r_ % p.OH), n = (int)(r_ / p.OH);
    const T* x = reinterpret_cast<const T*>(p.x);
    float acc = 0.f;
    for (int r = 0; r < p.KH; ++r) {
        const int ty = oy + p.padT - r;
        if (ty < 0 || ty % p.SH != 0 || ty / p.SH >= p.h) continue;
        for (int q = 0; q < p.KW; ++q) {
            const int tx = ox + p.padL - q;
            if (tx < 0 || tx % p.SW != 0 || tx / p.SW >= p.w_) continue;
            const T* xp = x + (((size_t)n * p.h + ty / p.SH) * p.w_ + tx / p.SW) * p.Cs;
            const float* wp = p.w + ((size_t)(r * p.KW + q) * p.Cs) * p.Cb + cb;
            for (int cs = 0; cs < p.Cs; ++cs) acc += to_f32(xp[cs]) * to_f32(from_f32<T>(wp[(size_t)cs * p.Cb]));
        }
    }
    reinterpret_cast<T*>(p.y)[id] = from_f32<T>(acc + (p.bias ? p.bias[cb] : 0.f));
}

// bias behind the wide class's mcn_conv2d_dgrad route (that route has no bias epilogue): y = round(y + bias[c]) in place
template <typename T>
__global__ __launch_bounds__(256) void deconv_bias_add(T* __restrict__ y, const float* __restrict__ bias, long total, int Cb) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id < total) y[id] = from_f32<T>(to_f32(y[id]) + bias[id % Cb]);
}

// ---- pack: wp[n][t][k] (T, K-contiguous, taps in the kernel's phase-major order, k zero-padded to whole K-steps) ---------------------
struct DeconvPackParams {
    const float* w;
    void* wp;
    int Cs, Cb, KW, ntaps, kpad;
    int tap[MCN_MAX_TAPS];               // r | q << 16
};
template <typename T>
__global__ __launch_bounds__(256) void deconv_pack(const DeconvPackParams p) {
    const long total = (long)p.Cb * p.ntaps * p.kpad;
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    if (id >= total) return;
    const int k = (int)(id % p.kpad);
    const int t = (int)((id / p.kpad) % p.ntaps), n = (int)(id / ((long)p.kpad * p.ntaps));
    const int r = p.tap[t] & 0xffff, q = p.tap[t] >> 16;
    reinterpret_cast<T*>(p.wp)[id] = from_f32<T>(k < p.Cs ? p.w[((size_t)(r * p.KW + q) * p.Cs + k) * p.Cb + n] : 0.f);
}

// ---- fp32 [taps][A][B] -> [taps][B][A] * scale: 32 x 32 tiles through LDS ----------------------------------------------------------
__global__ __launch_bounds__(256) void filter_swap_io_kernel(const float* __restrict__ src, float* __restrict__ dst, int A, int B, float scale) {
    __shared__ float tile[32][33];
    const int t = blockIdx.z, a0 = blockIdx.y * 32, b0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float* s = src + (size_t)t * A * B;
    float* d = dst + (size_t)t * A * B;
    for (int i = ty; i < 32; i += 8)
        if (a0 + i < A && b0 + tx < B) tile[i][tx] = s[(size_t)(a0 + i) * B + b0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (b0 + i < B && a0 + tx < A) d[(size_t)(b0 + i) * A + a0 + tx] = tile[tx][i] * scale;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------
struct DGeo {
    int N, h, w, Cs, Cb, OH, OW, KH, KW, SH, SW, pT, pL, tile;
};
static bool dc_force_gather() {
    const char* e = getenv("MCN_FORCE_NAIVE");
    return e && e[0] == '1';
}
static int dgeo_from(const mcn_conv_geom* g, mcn_dtype dtype, DGeo* o) {
    if (!g) MCN_FAIL(MCN_E_BADARG, "deconv: null geometry");
    if (!mcn_dtype_ok(dtype)) MCN_FAIL(MCN_E_UNSUPPORTED, "deconv: dtype %d", (int)dtype);
    if (g->N < 0 || g->H <= 0 || g->W <= 0 || g->Cin <= 0 || g->Cout <= 0 || g->KH <= 0 || g->KW <= 0 || g->SH <= 0 || g->SW <= 0 || g->padT < 0 ||
        g->padB < 0 || g->padL < 0 || g->padR < 0 || (g->x_cs != 0 && g->x_cs != g->Cin) || g->KH * g->KW > MCN_MAX_TAPS)
        MCN_FAIL(MCN_E_BADARG, "deconv: bad geometry N=%d OH=%d OW=%d Cb=%d Cs=%d K=%dx%d S=%dx%d", g->N, g->H, g->W, g->Cin, g->Cout, g->KH, g->KW, g->SH, g->SW);
    if (g->DH != 1 || g->DW != 1) MCN_FAIL(MCN_E_UNSUPPORTED, "deconv: dilation %dx%d is not built", g->DH, g->DW);
    o->N = g->N; o->OH = g->H; o->OW = g->W; o->Cb = g->Cin; o->Cs = g->Cout; o->KH = g->KH; o->KW = g->KW; o->SH = g->SH; o->SW = g->SW;
    o->pT = g->padT; o->pL = g->padL; o->tile = g->tile & 0xff;
    if (g->H + g->padT + g->padB < g->KH || g->W + g->padL + g->padR < g->KW) MCN_FAIL(MCN_E_BADARG, "deconv: output %dx%d smaller than the filter", g->H, g->W);
    o->h = (g->H + g->padT + g->padB - g->KH) / g->SH + 1;
    o->w = (g->W + g->padL + g->padR - g->KW) / g->SW + 1;
    // padded (SAME) geometries: the output size must be one that SAME maps back to the small grid
    if ((g->padT || g->padB) && (g->H < (o->h - 1) * g->SH + 1 || g->H > o->h * g->SH))
        MCN_FAIL(MCN_E_BADARG, "deconv: output height %d outside %d..%d of the small height %d", g->H, (o->h - 1) * g->SH + 1, o->h * g->SH, o->h);
    if ((g->padL || g->padR) && (g->W < (o->w - 1) * g->SW + 1 || g->W > o->w * g->SW))
        MCN_FAIL(MCN_E_BADARG, "deconv: output width %d outside %d..%d of the small width %d", g->W, (o->w - 1) * g->SW + 1, o->w * g->SW, o->w);
    return MCN_OK;
}
static inline int dc_ce(mcn_dtype t) { return t == MCN_F32 ? 4 : 8; }
static inline int dc_ksteps(const DGeo& g, mcn_dtype t) { return (g.Cs + dc_ce(t) * 8 - 1) / (dc_ce(t) * 8); }
static bool dc_fused_ok(const DGeo& g, mcn_dtype t) {
    if (dc_force_gather()) return false;
    const size_t es = mcn_dtype_size(t);
    return g.SH <= 2 && g.SW <= 2 && g.KH <= 7 && g.KW <= 7 && g.Cs % dc_ce(t) == 0 && (size_t)g.h * g.w * g.Cs * es < (1u << 31) &&
           (size_t)g.Cb * g.KH * g.KW * dc_ksteps(g, t) * 128 < (1u << 31);
}
// Which geometries the fused kernel serves by default, measured at N = 256 on biased layers against the route that is otherwise dispatched — the
// per-call filter swap, mcn_conv2d_dgrad with its per-call pack (four launches), and a bias pass over the output (profiles/deconv_kernel_bandwidth.txt):
//   narrow (Cb <= 16; that route falls to naive_conv_dgrad): fused 4x (fp32) to 24x (2-byte types) faster;
//   light (few MACs per output element: 3x3/2 on 64 channels = 144): fused 301 against 382 us in fp32, 102 against 186 us in bf16 — the bias pass over
//     the large output costs more than the fused kernel's slower K loop.  Without a bias the route's floor (bare dgrad, 236 / 89 us) is ahead again,
//     so an unbiased light layer takes the route;
//   heavy (5x5/2 on 128-512 channels = 800-3200 MACs per output element): the route is 1.2-3.2x faster.
// The bar between light and heavy sits at 400 MACs per output element, between the two measured classes.  mcn_conv_geom.tile = 1 forces the fused kernel, 2 the route (callers that time both).
static bool dc_narrow(const DGeo& d) { return d.Cb <= 16; }
static bool dc_light(const DGeo& d) { return (long)d.KH * d.KW * d.Cs <= 400L * d.SH * d.SW; }
static bool dc_use_fused(const DGeo& g, mcn_dtype t) { return dc_fused_ok(g, t) && g.tile != 2 && (dc_narrow(g) || g.tile == 1 || dc_light(g)); }      // (takes a packed operand)
static bool dc_routed(const DGeo& g, mcn_dtype t, bool biased) { return dc_fused_ok(g, t) && (g.tile == 2 || (!dc_narrow(g) && g.tile != 1 && !(dc_light(g) && biased))); }
// taps in the order the kernel walks them: phase-major, (r, q) ascending inside a phase
static int dc_taps(const DGeo& g, int* rq, int* jj, int* begin) {
    int n = 0;
    for (int ph = 0; ph < g.SH; ++ph)
        for (int pw = 0; pw < g.SW; ++pw) {
            begin[ph * g.SW + pw] = n;
            for (int r = ph; r < g.KH; r += g.SH)
                for (int q = pw; q < g.KW; q += g.SW) {
                    rq[n] = r | (q << 16);
                    jj[n] = ((r - ph) / g.SH) | (((q - pw) / g.SW) << 16);
                    ++n;
                }
        }
    for (int p = g.SH * g.SW; p <= 4; ++p) begin[p] = n;
    return n;
}

extern "C" size_t mcn_deconv2d_packed_bytes(const mcn_conv_geom* g, mcn_dtype dtype) {
    DGeo d;
    if (dgeo_from(g, dtype, &d) != MCN_OK || !dc_use_fused(d, dtype)) return 0;
    return (size_t)d.Cb * d.KH * d.KW * dc_ksteps(d, dtype) * 128;
}

static size_t dc_swap_bytes(const DGeo& d) { return align_up((size_t)d.KH * d.KW * d.Cs * d.Cb * sizeof(float), 256); }

extern "C" size_t mcn_deconv2d_workspace_bytes(mcn_conv_op op, const mcn_conv_geom* g, mcn_dtype dtype) {
    DGeo d;
    if (dgeo_from(g, dtype, &d) != MCN_OK) return 0;
    switch (op) {
        case MCN_CONV_FWD:
        {
            const size_t a = align_up(mcn_deconv2d_packed_bytes(g, dtype), 256);
            const size_t b = dc_routed(d, dtype, false) ? dc_swap_bytes(d) + mcn_conv2d_workspace_bytes(MCN_CONV_DGRAD, g, dtype) : 0;
            return a > b ? a : b;
        }
        case MCN_CONV_DGRAD: return dc_swap_bytes(d) + mcn_conv2d_workspace_bytes(MCN_CONV_FWD, g, dtype);
        case MCN_CONV_WGRAD: {
            const size_t a = mcn_conv2d_workspace_bytes(MCN_CONV_WGRAD, g, dtype), b = mcn_bias_grad_workspace_bytes((int64_t)d.N * d.OH * d.OW, d.Cb);
            return dc_swap_bytes(d) + (a > b ? a : b);
        }
    }
    return 0;
}

extern "C" int mcn_filter_swap_io(const float* src, float* dst, int32_t taps, int32_t A, int32_t B, float scale, void* stream) {
    if (!src || !dst || src == dst) MCN_FAIL(MCN_E_BADARG, "filter_swap_io: null or aliased tensor");
    if (taps <= 0 || A <= 0 || B <= 0 || taps > 65535 || (A + 31) / 32 > 65535) MCN_FAIL(MCN_E_BADARG, "filter_swap_io: taps=%d A=%d B=%d", taps, A, B);
    hipLaunchKernelGGL(filter_swap_io_kernel, dim3((B + 31) / 32, (A + 31) / 32, taps), dim3(256), 0, (hipStream_t)stream, src, dst, A, B, scale);
    MCN_CHECK_LAUNCH();
    return MCN_OK;
}

template <typename T>
static int dc_pack_t(const float* w, void* packed, const DGeo& d, hipStream_t st) {
    DeconvPackParams pp;
    int jj[MCN_MAX_TAPS], begin[5];
    pp.w = w; pp.wp = packed; pp.Cs = d.Cs; pp.Cb = d.Cb; pp.KW = d.KW;
    pp.ntaps = dc_taps(d, pp.tap, jj, begin);
    pp.kpad = dc_ksteps(d, DtypeOf<T>::value) * (128 / (int)sizeof(T));
    const long total = (long)d.Cb * pp.ntaps * pp.kpad;
    hipLaunchKernelGGL(deconv_pack<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, pp);
    MCN_CHECK_LAUNCH();
    return MCN_OK;
}
extern "C" int mcn_deconv2d_pack(const float* w, void* packed, const mcn_conv_geom* g, mcn_dtype dtype, void* stream) {
    DGeo d;
    int rc = dgeo_from(g, dtype, &d);
    if (rc != MCN_OK) return rc;
    if (!w || !packed) MCN_FAIL(MCN_E_BADARG, "deconv pack: null tensor");
    if (!dc_use_fused(d, dtype)) MCN_FAIL(MCN_E_UNSUPPORTED, "deconv pack: this geometry takes no packed operand (mcn_deconv2d_packed_bytes is 0)");
    hipStream_t st = (hipStream_t)stream;
    return dtype == MCN_F32 ? dc_pack_t<float>(w, packed, d, st) : dtype == MCN_BF16 ? dc_pack_t<bf16_t>(w, packed, d, st) : dc_pack_t<f16_t>(w, packed, d, st);
}

template <typename K>
static bool dc_allow_lds(K kernel, int bytes) {
    if (bytes <= 64 * 1024) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

template <typename T, int TH, int TW, int BN, int WM, int WN>
static int dc_launch(DeconvParams& p, const DGeo& d, hipStream_t st) {
    constexpr int BNL = BN < 32 ? 32 : BN;
    p.by_min = d.pT / d.SH;
    p.bx_min = d.pL / d.SW;
    const int nby = (d.OH - 1 + d.pT) / d.SH - p.by_min + 1, nbx = (d.OW - 1 + d.pL) / d.SW - p.bx_min + 1;
    p.tiles_y = (nby + TH - 1) / TH;
    p.tiles_x = (nbx + TW - 1) / TW;
    p.ntn = (d.Cb + BN - 1) / BN;
    p.WW = TW + p.JW;
    p.wrows = (TH + p.JH) * p.WW;
    if (p.wrows > DC_MAXPASS * 32) MCN_FAIL(MCN_E_UNSUPPORTED, "deconv: window of %d rows", p.wrows);
    const int wrows_alloc = (p.wrows + 31) & ~31;
    const int loop_bytes = 2 * wrows_alloc * 128 + 2 * BNL * 128;
    const int epi_bytes = TH * d.SH * TW * d.SW * BN * (int)sizeof(T);
    const int lds = loop_bytes > epi_bytes ? loop_bytes : epi_bytes;
    const long blocks = (long)d.N * p.tiles_y * p.tiles_x * p.ntn;
    if (blocks <= 0) return MCN_OK;
    if (blocks > 0x7fffffffL) MCN_FAIL(MCN_E_UNSUPPORTED, "deconv: %ld workgroups", blocks);
    auto kern = deconv_fused<T, TH, TW, BN, WM, WN>;
    if (!dc_allow_lds(kern, lds)) MCN_FAIL(MCN_E_LAUNCH, "deconv: %d bytes of LDS refused", lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), lds, st, p);
    MCN_CHECK_LAUNCH();
    return MCN_OK;
}

template <typename T>
static int dc_fwd_t(const void* x, const float* w, const void* w_packed, const float* bias, void* y, const mcn_conv_geom* g, const DGeo& d, void* ws, size_t ws_bytes, hipStream_t st) {
    const mcn_dtype dt = DtypeOf<T>::value;
    if (dc_routed(d, dt, bias != nullptr)) {               // the existing kernels (see dc_use_fused)
        const size_t sb = dc_swap_bytes(d);
        if (!ws || ws_bytes < sb) MCN_FAIL(MCN_E_WORKSPACE, "deconv fwd: workspace %zu < %zu bytes", ws_bytes, sb);
        int rc = mcn_filter_swap_io(w, reinterpret_cast<float*>(ws), d.KH * d.KW, d.Cs, d.Cb, 1.f, st);
        if (rc != MCN_OK) return rc;
        rc = mcn_conv2d_dgrad(x, reinterpret_cast<const float*>(ws), nullptr, y, g, 0, dt, MCN_NHWC, reinterpret_cast<char*>(ws) + sb, ws_bytes - sb, st);
        const long total = (long)d.N * d.OH * d.OW * d.Cb;
        if (rc != MCN_OK || !bias || total == 0) return rc;
        hipLaunchKernelGGL(deconv_bias_add<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, reinterpret_cast<T*>(y), bias, total, d.Cb);
        MCN_CHECK_LAUNCH();
        return MCN_OK;
    }
    if (!dc_fused_ok(d, dt)) {
        DeconvGatherParams gp = {x, w, bias, y, d.N, d.h, d.w, d.Cs, d.Cb, d.OH, d.OW, d.KH, d.KW, d.SH, d.SW, d.pT, d.pL};
        const long total = (long)d.N * d.OH * d.OW * d.Cb;
        if (total == 0) return MCN_OK;
        if ((total + 255) / 256 > 0x7fffffffL) MCN_FAIL(MCN_E_UNSUPPORTED, "deconv: %ld outputs", total);
        hipLaunchKernelGGL(deconv_gather<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, gp);
        MCN_CHECK_LAUNCH();
        return MCN_OK;
    }
    const size_t pb = (size_t)d.Cb * d.KH * d.KW * dc_ksteps(d, dt) * 128;
    if (!w_packed) {
        if (!ws || ws_bytes < pb) MCN_FAIL(MCN_E_WORKSPACE, "deconv fwd: workspace %zu < %zu bytes", ws_bytes, pb);
        int rc = dc_pack_t<T>(w, ws, d, st);
        if (rc != MCN_OK) return rc;
        w_packed = ws;
    }
    DeconvParams p;
    memset(&p, 0, sizeof(p));
    int rq[MCN_MAX_TAPS];
    p.x = x; p.wp = w_packed; p.bias = bias; p.y = y;
    p.N = d.N; p.h = d.h; p.w = d.w; p.Cs = d.Cs; p.Cb = d.Cb; p.OH = d.OH; p.OW = d.OW;
    p.SH = d.SH; p.SW = d.SW; p.padT = d.pT; p.padL = d.pL;
    p.JH = (d.KH - 1) / d.SH; p.JW = (d.KW - 1) / d.SW;
    p.ntaps = dc_taps(d, rq, p.tap, p.tap_begin);
    p.ksteps = dc_ksteps(d, dt);
    p.cchunks = d.Cs / dc_ce(dt);
    p.img_bytes = (unsigned)((size_t)d.h * d.w * d.Cs * sizeof(T));
    p.krow_bytes = (unsigned)(p.ntaps * p.ksteps * 128);
    p.wt_bytes = (unsigned)pb;
    if (dc_narrow(d)) {
        if constexpr (sizeof(T) == 4) return dc_launch<T, 8, 16, 32, 4, 1>(p, d, st);      // (one 32-row MFMA tile: the N block of fp32)
        else return dc_launch<T, 8, 8, 16, 4, 1>(p, d, st);
    }
    return dc_launch<T, 8, 8, 64, 2, 2>(p, d, st);
}

extern "C" int mcn_deconv2d_fwd(const void* x, const float* w, const void* w_packed, const float* bias, void* y, const mcn_conv_geom* g, mcn_dtype dtype,
                                mcn_layout layout, void* workspace, size_t workspace_bytes, void* stream) {
    DGeo d;
    int rc = dgeo_from(g, dtype, &d);
    if (rc != MCN_OK) return rc;
    if (layout != MCN_NHWC) MCN_FAIL(MCN_E_UNSUPPORTED, "deconv: NHWC only");
    if (!x || !w || !y) MCN_FAIL(MCN_E_BADARG, "deconv fwd: null tensor");
    hipStream_t st = (hipStream_t)stream;
    switch (dtype) {
        case MCN_F32: return dc_fwd_t<float>(x, w, w_packed, bias, y, g, d, workspace, workspace_bytes, st);
        case MCN_BF16: return dc_fwd_t<bf16_t>(x, w, w_packed, bias, y, g, d, workspace, workspace_bytes, st);
        default: return dc_fwd_t<f16_t>(x, w, w_packed, bias, y, g, d, workspace, workspace_bytes, st);
    }
}

extern "C" int mcn_deconv2d_kernel_name(const mcn_conv_geom* g, mcn_dtype dtype, char* buf, size_t buflen) {
    DGeo d;
    int rc = dgeo_from(g, dtype, &d);
    if (rc != MCN_OK) return rc;
    if (!buf || buflen < 64) MCN_FAIL(MCN_E_BADARG, "deconv kernel name: buffer of %zu bytes", buflen);
    if (dc_routed(d, dtype, true)) return mcn_conv2d_kernel_name(MCN_CONV_DGRAD, g, dtype, buf, buflen);
    if (!dc_fused_ok(d, dtype)) snprintf(buf, buflen, "deconv_gather");
    else if (dc_narrow(d)) snprintf(buf, buflen, dtype == MCN_F32 ? "deconv_fused<float, 8, 16, 32, 4, 1>" : "deconv_fused<%s, 8, 8, 16, 4, 1>", dtype == MCN_BF16 ? "__bf16" : "_Float16");
    else snprintf(buf, buflen, "deconv_fused<%s, 8, 8, 64, 2, 2>", dtype == MCN_F32 ? "float" : dtype == MCN_BF16 ? "__bf16" : "_Float16");
    return 1;
}

extern "C" int mcn_deconv2d_dgrad(const void* dy, const float* w, const float* w_swapped, const void* w_swapped_packed, void* dx, const mcn_conv_geom* g,
                                  mcn_dtype dtype, mcn_layout layout, void* workspace, size_t workspace_bytes, void* stream) {
    DGeo d;
    int rc = dgeo_from(g, dtype, &d);
    if (rc != MCN_OK) return rc;
    if (!dy || !dx || (!w && !w_swapped)) MCN_FAIL(MCN_E_BADARG, "deconv dgrad: null tensor");
    if (!w_swapped && w_swapped_packed) MCN_FAIL(MCN_E_BADARG, "deconv dgrad: a packed operand without the swapped filter it was packed from");
    char* ws = reinterpret_cast<char*>(workspace);
    if (!w_swapped) {
        const size_t sb = dc_swap_bytes(d);
        if (!ws || workspace_bytes < sb) MCN_FAIL(MCN_E_WORKSPACE, "deconv dgrad: workspace %zu < %zu bytes", workspace_bytes, sb);
        rc = mcn_filter_swap_io(w, reinterpret_cast<float*>(ws), d.KH * d.KW, d.Cs, d.Cb, 1.f, stream);
        if (rc != MCN_OK) return rc;
        w_swapped = reinterpret_cast<const float*>(ws);
        ws += sb;
        workspace_bytes -= sb;
    }
    return mcn_conv2d_fwd(dy, w_swapped, w_swapped_packed, nullptr, dx, g, dtype, layout, ws, workspace_bytes, stream);
}

extern "C" int mcn_deconv2d_wgrad(const void* x, const void* dy, float* dw, float* dbias, const mcn_conv_geom* g, float grad_scale, mcn_dtype dtype,
                                  mcn_layout layout, void* workspace, size_t workspace_bytes, void* stream) {
    DGeo d;
    int rc = dgeo_from(g, dtype, &d);
    if (rc != MCN_OK) return rc;
    if (!x || !dy || !dw) MCN_FAIL(MCN_E_BADARG, "deconv wgrad: null tensor");
    const size_t sb = dc_swap_bytes(d);
    if (!workspace || workspace_bytes < sb) MCN_FAIL(MCN_E_WORKSPACE, "deconv wgrad: workspace %zu < %zu bytes", workspace_bytes, sb);
    float* tmp = reinterpret_cast<float*>(workspace);                       // gradient of the strided conv's filter: [KH][KW][Cb][Cs]
    char* ws = reinterpret_cast<char*>(workspace) + sb;
    rc = mcn_conv2d_wgrad(dy, x, tmp, nullptr, g, 1.f, dtype, layout, ws, workspace_bytes - sb, stream);
    if (rc != MCN_OK) return rc;
    rc = mcn_filter_swap_io(tmp, dw, d.KH * d.KW, d.Cb, d.Cs, grad_scale, stream);
    if (rc != MCN_OK || !dbias) return rc;
    return mcn_bias_grad(dy, dbias, (int64_t)d.N * d.OH * d.OW, d.Cb, grad_scale, dtype, ws, workspace_bytes - sb, stream);
}
