// The flat Adam kernel and its launcher, shared by adam.hip (torch.optim.Adam: grit_adam_flat, grit_adam_flat_dev) and adamw.hip
// (torch.optim.AdamW with the clip factor read from device memory: grit_adamw_flat_dev).  AdamW = the same update lines behind one
// multiply of the master by 1 - lr * weight_decay; DECAY = false compiles to the Adam kernel as it was.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/grit_hip.h"

namespace {

template <typename GT> __device__ __forceinline__ void load4(const GT* p, float (&g)[4]);
template <> __device__ __forceinline__ void load4<float>(const float* p, float (&g)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    g[0] = t.x; g[1] = t.y; g[2] = t.z; g[3] = t.w;
}
template <> __device__ __forceinline__ void load4<__hip_bfloat16>(const __hip_bfloat16* p, float (&g)[4]) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    g[0] = __uint_as_float(u.x << 16); g[1] = __uint_as_float(u.x & 0xffff0000u);
    g[2] = __uint_as_float(u.y << 16); g[3] = __uint_as_float(u.y & 0xffff0000u);
}

typedef float f4 __attribute__((ext_vector_type(4)));
template <bool NT> __device__ __forceinline__ f4 ldq(const f4* q) {
    if constexpr (NT) return __builtin_nontemporal_load(q);
    else return *q;
}

template <typename GT, bool NT, bool DECAY>
__global__ __launch_bounds__(256)
void adam_flat(float* __restrict__ p, const GT* __restrict__ grad, float* __restrict__ m, float* __restrict__ v,
               __hip_bfloat16* __restrict__ compute, long n4, float step_size, float beta1, float beta2, float eps,
               float inv_bc2_sqrt, float grad_scale, const float* __restrict__ hyper, const float* __restrict__ clip_scale) {
    // hyper != NULL: the two per-step scalars come from device memory {lr / bias_correction1, 1 / sqrt(bias_correction2)} -- a
    // launch captured in a HIP graph is replayed with the learning rate and the step count of the step it is replayed for
    if (hyper) {
        step_size = hyper[0];
        inv_bc2_sqrt = hyper[1];
    }
    // DECAY (AdamW): hyper is a row of four, hyper[2] = 1 - lr * weight_decay; clip_scale != NULL: the factor every gradient element
    // is multiplied by comes from the clip cell grit_grad_norm_flat wrote (1 / world times the clip coefficient)
    float decay = 1.0f;
    if constexpr (DECAY) {
        decay = hyper[2];
        if (clip_scale) grad_scale = clip_scale[0];
    }
    // masters and moments are touched once per step: nontemporal loads / stores (they need not displace the weights the next
    // forward is about to read); two quads per thread and trip: eight 16-byte loads in flight
    const long stride = (long)gridDim.x * 256;
    auto update = [&](long i, const float (&g)[4], f4 pp, f4 mm, f4 vv) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (DECAY) {
                // torch's order: param.mul_(1 - lr * wd) first, ROUNDED, then Adam's lines.  The empty asm keeps the product out of
                // a fused multiply-add with the subtraction below (which would round lr * m / denom instead, and differ from Adam
                // at decay = 1)
                float t = pp[k] * decay;
                asm("" : "+v"(t));
                pp[k] = t;
            }
            const float gk = g[k] * grad_scale;
            mm[k] = mm[k] + (gk - mm[k]) * (1.0f - beta1);
            vv[k] = beta2 * vv[k] + (1.0f - beta2) * gk * gk;
            const float denom = sqrtf(vv[k]) * inv_bc2_sqrt + eps;
            pp[k] -= step_size * (mm[k] / denom);
        }
        if constexpr (NT) {
            __builtin_nontemporal_store(pp, reinterpret_cast<f4*>(p + 4 * i));
            __builtin_nontemporal_store(mm, reinterpret_cast<f4*>(m + 4 * i));
            __builtin_nontemporal_store(vv, reinterpret_cast<f4*>(v + 4 * i));
        } else {
            *reinterpret_cast<f4*>(p + 4 * i) = pp;
            *reinterpret_cast<f4*>(m + 4 * i) = mm;
            *reinterpret_cast<f4*>(v + 4 * i) = vv;
        }
        if (compute) {
            union { __hip_bfloat16 h[4]; uint2 u; } pk;
#pragma unroll
            for (int k = 0; k < 4; ++k) pk.h[k] = __float2bfloat16(pp[k]);
            *reinterpret_cast<uint2*>(compute + 4 * i) = pk.u;
        }
    };
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    for (; i + stride < n4; i += 2 * stride) {
        const long j = i + stride;
        float g0[4], g1[4];
        load4<GT>(grad + 4 * i, g0);
        load4<GT>(grad + 4 * j, g1);
        const f4 p0 = ldq<NT>(reinterpret_cast<const f4*>(p + 4 * i));
        const f4 m0 = ldq<NT>(reinterpret_cast<const f4*>(m + 4 * i));
        const f4 v0 = ldq<NT>(reinterpret_cast<const f4*>(v + 4 * i));
        const f4 p1 = ldq<NT>(reinterpret_cast<const f4*>(p + 4 * j));
        const f4 m1 = ldq<NT>(reinterpret_cast<const f4*>(m + 4 * j));
        const f4 v1 = ldq<NT>(reinterpret_cast<const f4*>(v + 4 * j));
        update(i, g0, p0, m0, v0);
        update(j, g1, p1, m1, v1);
    }
    if (i < n4) {
        float g0[4];
        load4<GT>(grad + 4 * i, g0);
        update(i, g0, ldq<NT>(reinterpret_cast<const f4*>(p + 4 * i)),
               ldq<NT>(reinterpret_cast<const f4*>(m + 4 * i)),
               ldq<NT>(reinterpret_cast<const f4*>(v + 4 * i)));
    }
}

const long kAdamBlockCap = 8192;  // grid-stride: 32 workgroups per CU

template <bool DECAY>
int adam_launch(float* param, const void* grad, int grad_is_bf16, float* exp_avg, float* exp_avg_sq, void* compute_bf16, long n,
                float lr, float beta1, float beta2, float eps, float bias_correction1, float bias_correction2_sqrt, float grad_scale,
                const float* hyper, const float* clip_scale, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0)
        return GRIT_ERR_BAD_ARG;
    const uintptr_t align = (uintptr_t)param | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq;
    if (n % 4 != 0 || (align % 16) != 0 || ((uintptr_t)grad % (grad_is_bf16 ? 8 : 16)) != 0 ||
        (compute_bf16 && ((uintptr_t)compute_bf16 % 8) != 0))
        return GRIT_ERR_UNSUPPORTED;
    const long n4 = n / 4;
    long blocks = (n4 + 255) / 256;
    if (blocks > kAdamBlockCap) blocks = kAdamBlockCap;
    const float step_size = lr / bias_correction1, inv_bc2_sqrt = 1.0f / bias_correction2_sqrt;
    // GRIT_ADAM_NT=0 (A/B): plain loads / stores of the masters and moments
    static const bool nt = !(getenv("GRIT_ADAM_NT") && atoi(getenv("GRIT_ADAM_NT")) == 0);
#define GRIT_ADAM_LAUNCH(GT_, NT_, GPTR_)                                                                                          \
    hipLaunchKernelGGL((adam_flat<GT_, NT_, DECAY>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, GPTR_,      \
                       exp_avg, exp_avg_sq, (__hip_bfloat16*)compute_bf16, n4, step_size, beta1, beta2, eps, inv_bc2_sqrt,         \
                       grad_scale, hyper, clip_scale)
    if (grad_is_bf16) {
        if (nt) GRIT_ADAM_LAUNCH(__hip_bfloat16, true, (const __hip_bfloat16*)grad);
        else GRIT_ADAM_LAUNCH(__hip_bfloat16, false, (const __hip_bfloat16*)grad);
    } else {
        if (nt) GRIT_ADAM_LAUNCH(float, true, (const float*)grad);
        else GRIT_ADAM_LAUNCH(float, false, (const float*)grad);
    }
#undef GRIT_ADAM_LAUNCH
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

}  // namespace
