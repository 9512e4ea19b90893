// Row arithmetic of the LayerNorm kernels, shared by layernorm.hip (ln_fwd / ln_bwd) and mlp_s0.hip (the LayerNorm in front of and
// behind the frozen stage-0 Mlp): 8-channel vector access, the lane sum of a row, the two-pass statistics and the normalise step.
// One copy, so that a LayerNorm computed inside another kernel gives the bits ln_fwd gives.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

namespace {

template <typename T> struct Vec8;
template <> struct Vec8<float> {
    static __device__ __forceinline__ void load(const float* p, float (&v)[8]) {
        const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[8], bool nt = false) {
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
        if (nt) {
            __builtin_nontemporal_store(a, reinterpret_cast<v4f*>(p));
            __builtin_nontemporal_store(b, reinterpret_cast<v4f*>(p + 4));
        } else {
            *reinterpret_cast<v4f*>(p) = a;
            *reinterpret_cast<v4f*>(p + 4) = b;
        }
    }
};
template <> struct Vec8<__hip_bfloat16> {
    static __device__ __forceinline__ void load(const __hip_bfloat16* p, float (&v)[8]) {
#ifdef GRIT_LN_NT_LOADS
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 u = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
        const uint32_t w[4] = {u[0], u[1], u[2], u[3]};
#else
        const uint4 u = *reinterpret_cast<const uint4*>(p);
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#endif
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __uint_as_float(w[i] << 16);
            v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
        }
    }
    static __device__ __forceinline__ void store(__hip_bfloat16* p, const float (&v)[8], bool nt = false) {
        typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
        v8bf o;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (__bf16)v[i];
        // nt (wave-uniform, chosen per launch): maps of tens to hundreds of MB are written once and read by a later kernel from
        // HBM anyway; streamed past L2 they leave the neighbouring GEMMs' operand panels resident (63.5 -> 62.9 ms per training
        // step, A/B on one box).  Small maps (decoders, beam search) stay cached for their consumer.
        if (nt)
            __builtin_nontemporal_store(o, reinterpret_cast<v8bf*>(p));
        else
            *reinterpret_cast<v8bf*>(p) = o;
    }
};

template <typename T> __device__ __forceinline__ float round_to(float v);
template <> __device__ __forceinline__ float round_to<float>(float v) { return v; }
template <> __device__ __forceinline__ float round_to<__hip_bfloat16>(float v) { return __bfloat162float(__float2bfloat16(v)); }

// Sum over the LPR lanes of a row.  Not as __shfl_xor steps: each of those is a ds_bpermute round trip through the LDS pipe with
// a full lgkmcnt wait, twelve of them on the dependent chain load -> mean -> variance -> store of a row, and a wave of these
// kernels is nothing but that chain.  Within a DPP row (16 lanes) four row rotations (plain VALU); across the rows of a wave the
// four row sums are read into scalars.
template <int LPR>
__device__ __forceinline__ float row_sum(float v) {
    if constexpr (LPR >= 16) {
#define GRIT_ROW_ROR(x, n) __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + (n), 0xf, 0xf, false))
        v += GRIT_ROW_ROR(v, 8); v += GRIT_ROW_ROR(v, 4); v += GRIT_ROW_ROR(v, 2); v += GRIT_ROW_ROR(v, 1);
#undef GRIT_ROW_ROR
        if constexpr (LPR == 16) return v;
        const int iv = __builtin_bit_cast(int, v);
        const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 16));
        const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 48));
        if constexpr (LPR == 64) return (r0 + r1) + (r2 + r3);
        return (threadIdx.x & 32) ? r2 + r3 : r0 + r1;
    } else {
#pragma unroll
        for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        return v;
    }
}

// Mean and reciprocal standard deviation of a row of C = LPR * 8 * CH channels held as CH chunks of 8 per lane: the sum in element
// order, then the lane sum; the variance from the register copy, centred (two passes).  `s` is the lane's sum of its own elements.
template <int LPR, int CH>
__device__ __forceinline__ void ln_row_stats(const float (&v)[CH][8], float s, float eps, float& mu, float& rs) {
    constexpr int C = LPR * 8 * CH;
    mu = row_sum<LPR>(s) * (1.0f / C);
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int i = 0; i < 8; ++i) { const float d = v[c][i] - mu; q = fmaf(d, d, q); }
    rs = rsqrtf(row_sum<LPR>(q) * (1.0f / C) + eps);
}

// y = (v - mu) * rs * w + b for one chunk of 8 channels
__device__ __forceinline__ void ln_row_normalise(const float (&v)[8], float mu, float rs, const float (&wv)[8], const float (&bv)[8],
                                                 float (&o)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = fmaf((v[i] - mu) * rs, wv[i], bv[i]);
}

}  // namespace
