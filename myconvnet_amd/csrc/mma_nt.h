// mma_nt.h — the pieces the NT-form MFMA kernels of conv.hip and deconv.hip share: MFMA policies per storage type, the swizzled LDS image of a
// 128-byte-row tile, the out-of-range marker of the bounds-checked buffer offsets, the LDS-DMA cache-policy switches and static_for.
#pragma once
#include <type_traits>
#include "common.h"

#define MCN_MAX_TAPS 64
#define MCN_OOB 0x80000000u

// Cache policy of the LDS-DMA loads of the activation operands (build-time experiments): the aux immediate of buffer_load ... lds,
// 2 = nt (streaming).  MCN_DMA_AUX_A: A operand of the NT kernels (activations; the packed filter stays cached); MCN_DMA_AUX_X: x and dy
// of the wgrad.
#ifndef MCN_DMA_AUX_A
#define MCN_DMA_AUX_A 0
#endif
#ifndef MCN_DMA_AUX_X
#define MCN_DMA_AUX_X 0
#endif

// ------------------------------------------------------------------------------------------------
// MFMA policies
// ------------------------------------------------------------------------------------------------
template <typename T>
struct MmaNT;

// bf16: 16x16x32, K-step = 64 elements = 2 slabs; fragment = one 16-byte chunk
template <>
struct MmaNT<bf16_t> {
    static constexpr int MT = 16;       // tile edge
    static constexpr int SLABS = 2;     // per 128-byte K-step
    static constexpr int CPS = 4;       // chunks per slab
    typedef f32x4 Acc;
    typedef bf16x8 Frag;
    static __device__ __forceinline__ int frag_row(int lane) { return lane & 15; }
    static __device__ __forceinline__ int frag_chunk(int lane) { return lane >> 4; }
    static __device__ __forceinline__ void mma(Acc& acc, const Frag& w, const Frag& x) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, x, acc, 0, 0, 0);
    }
};
// fp16: the bf16 policy with the f16 MFMA (same cycles, same operand / accumulator lane maps)
template <>
struct MmaNT<f16_t> {
    static constexpr int MT = 16;
    static constexpr int SLABS = 2;
    static constexpr int CPS = 4;
    typedef f32x4 Acc;
    typedef f16x8 Frag;
    static __device__ __forceinline__ int frag_row(int lane) { return lane & 15; }
    static __device__ __forceinline__ int frag_chunk(int lane) { return lane >> 4; }
    static __device__ __forceinline__ void mma(Acc& acc, const Frag& w, const Frag& x) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(w, x, acc, 0, 0, 0);
    }
};
// fp32: 32x32x2; a 16-byte fragment (4 consecutive k) feeds 4 MFMAs (k pairs {e, 4+e})
template <>
struct MmaNT<float> {
    static constexpr int MT = 32;
    static constexpr int SLABS = 4;
    static constexpr int CPS = 2;
    typedef f32x16 Acc;
    typedef f32x4 Frag;
    static __device__ __forceinline__ int frag_row(int lane) { return lane & 31; }
    static __device__ __forceinline__ int frag_chunk(int lane) { return lane >> 5; }
    static __device__ __forceinline__ void mma(Acc& acc, const Frag& w, const Frag& x) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(w[e], x[e], acc, 0, 0, 0);
    }
};

// LDS image of an NT tile: rows of 128 bytes, 16-byte chunk c of row r at r*128 + ((c ^ ((r>>1)&7))<<4)
__device__ __forceinline__ int nt_lds_off(int r, int c) { return r * 128 + ((c ^ ((r >> 1) & 7)) << 4); }

template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (N > 0) {
        static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}
