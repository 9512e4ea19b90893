// The Mlp half of a frozen stage-0 Swin block (C = 128, hidden = 512, forward only, eval mode) as ONE kernel on gfx950:
//
//   n      = LayerNorm(x)                     (norm2)
//   branch = fc2(gelu(fc1(n) + b1)) + b2      (reference models/common/swin_model.py:31-37)
//   x_out  = x + branch
//   n_out  = LayerNorm_next(x_out)            (the next block's norm1; optional)
//
// At C = 128 a tile of rows holds every channel of its rows, so the whole chain stays with the wave that owns the rows: the
// [rows, 512] hidden map (839 MB at 819 200 rows) and norm2's output are never written, x is read once.  The values are those
// of the launches this replaces -- ln_fwd<bf16, bf16, 16, 1>, gemm_nt_bf16 / GRIT_GEMM_BIAS_GELU (aux == NULL), gemm_nt_bf16 /
// GRIT_GEMM_BIAS_RES without factors (= GRIT_GEMM_BIAS + a bf16 add), ln_fwd -- bit for bit:
//   * the LayerNorms run the row arithmetic of ln_row.h in ln_fwd's lane layout (16 lanes of a DPP row per token, 8 channels each);
//   * both products use v_mfma_f32_16x16x32_bf16 with weight rows as the A operand and tokens as B, lane (l15, lq) holding
//     k = 32 kb + 8 lq .. + 7 of k block kb, the k blocks of an accumulator in ascending order: gemm_nt_bf16's assignment, and a
//     row's result there does not depend on the tile that computed it (tests/test_gemm_gpu.py::test_gemm_full_size_property);
//   * fp32 bias, gelu_f of gemm_math.h, one rounding to bf16 for the hidden values; fp32 bias, rounding to bf16, fp32 add to x,
//     rounding to bf16 for x_out.
//
// Structure: a workgroup = 4 waves x 32 rows.  A wave normalises its rows, passes them through a private 8 KB LDS image into the
// MFMA B-operand layout and keeps them in registers (32 VGPRs) for the whole kernel.  The hidden dimension is walked in 16 chunks of
// 32 channels: fc1 for the chunk (16 MFMAs), bias + GELU on its 16 accumulator registers, through the private image into the B
// layout, then the chunk as one k block of fc2 into the resident [32, 128] fp32 accumulator (16 MFMAs).  The weights of a chunk
// (fc1 rows [32, 128] + fc2 columns [128, 32] = 16 KB) are shared by the four waves: LDS-DMA into a two-slot ring, chunk-permuted
// like the GEMM's stages (chunk_swizzle), one barrier per chunk.  65 KB of LDS: two workgroups per CU, so one wave's GELU (VALU)
// runs beside the other's MFMAs and a workgroup's first loads / last stores beside the other's loop.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include "per_device.h"
#include "../../include/grit_hip.h"
#include "gemm_math.h"
#include "ln_row.h"

namespace {

constexpr int kC = 128, kHidden = 512;
constexpr int kWaves = 4, kRowsWave = 32, kRowsWG = kWaves * kRowsWave;
constexpr int kChunk = 32, kNChunk = kHidden / kChunk;
constexpr int kW1Bytes = kChunk * kC * 2, kW2Bytes = kC * kChunk * 2;  // 8 KB each
constexpr int kStage = kW1Bytes + kW2Bytes;
constexpr int kScratch = kRowsWave * kC * 2;  // per wave: the [32, 128] bf16 image (two [32][64] halves)
constexpr int kBias1 = 2 * kStage + kWaves * kScratch;  // fc1's bias, bf16 [512]: read per chunk from LDS (a global load inside the
                                                        // loop would be waited for behind the DMA pieces issued before it)
constexpr int kLds = kBias1 + kHidden * 2;
static_assert(2 * kLds <= 160 * 1024, "two workgroups per CU");

struct MlpS0Args {
    const __hip_bfloat16* x;
    const __hip_bfloat16 *nw, *nb;
    const __bf16 *w1, *b1, *w2, *b2;
    const __hip_bfloat16 *nnw, *nnb;
    __hip_bfloat16 *x_out, *n_out;
    float eps, next_eps;
    int rows, nt;
};

// byte offset of 16-byte chunk `lc` (0..15) of row `r` in a wave's [32, 128] bf16 image: two [32][64-channel] halves, each with the
// BK = 64 chunk permutation of the GEMM stages (conflict-free ds_read_b128 fragment reads)
__device__ __forceinline__ int img128(int r, int lc) {
    return (lc >> 3) * (kRowsWave * 128) + r * 128 + (((lc & 7) ^ chunk_swizzle<64>(r & 15)) * 16);
}
// the same for the [32, 32] image of a hidden chunk (64-byte rows, BK = 32 permutation)
__device__ __forceinline__ int img32(int r, int lc) { return r * 64 + ((lc ^ chunk_swizzle<32>(r & 15)) * 16); }

template <bool NEXT>
__global__ __launch_bounds__(kWaves * 64, 2)
void mlp_s0_fwd(const MlpS0Args g) {
    extern __shared__ __attribute__((aligned(1024))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, lq = lane >> 4;
    const int row0 = blockIdx.x * kRowsWG + wave * kRowsWave;
    char* sb = lds + 2 * kStage + wave * kScratch;

    // ---- weight chunks by LDS-DMA: fc1 rows [32, 128] as two [32][64] halves, fc2 columns [128, 32] ------------------------
    const __bf16* src1[2];
    const __bf16* src2[2];
    {
        const int row = tid >> 3, pc = tid & 7, lc = pc ^ chunk_swizzle<64>(row & 15);
#pragma unroll
        for (int i = 0; i < 2; ++i) src1[i] = g.w1 + row * kC + i * 64 + lc * 8;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int c = i * 256 + tid, r2 = c >> 2, p2 = c & 3, l2 = p2 ^ chunk_swizzle<32>(r2 & 15);
            src2[i] = g.w2 + r2 * kHidden + l2 * 8;
        }
    }
    auto stage = [&](int slot, int hc) {
        char* base = lds + slot * kStage + wave * 1024;
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_global_load_lds((gptr_t)(src1[i] + hc * kChunk * kC), (lptr_t)(base + i * 4096), 16, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
            __builtin_amdgcn_global_load_lds((gptr_t)(src2[i] + hc * kChunk), (lptr_t)(base + kW1Bytes + i * 4096), 16, 0, 0);
    };
    stage(0, 0);

    const uint32_t b1_pair = *reinterpret_cast<const uint32_t*>(g.b1 + tid * 2);

    // ---- norm2 in ln_fwd's layout: 4 rows per pass (one per DPP row), lane l15 holds channels 8 l15 .. + 7 --------------------
    {
        float wv[8], bv[8];
        Vec8<__hip_bfloat16>::load(g.nw + l15 * 8, wv);
        Vec8<__hip_bfloat16>::load(g.nb + l15 * 8, bv);
#pragma unroll
        for (int it = 0; it < kRowsWave / 4; ++it) {
            const int rr = it * 4 + lq;
            const int rc = min(row0 + rr, g.rows - 1);
            float v[1][8], o[8];
            Vec8<__hip_bfloat16>::load(g.x + (size_t)rc * kC + l15 * 8, v[0]);
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) s += v[0][i];
            float mu, rs;
            ln_row_stats<16, 1>(v, s, g.eps, mu, rs);
            ln_row_normalise(v[0], mu, rs, wv, bv, o);
            Vec8<__hip_bfloat16>::store(reinterpret_cast<__hip_bfloat16*>(sb + img128(rr, l15)), o);
        }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    v8bf xh[2][4];  // B operands of fc1: token 16 i + l15, k = 32 kb + 8 lq .. + 7
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) xh[i][kb] = *reinterpret_cast<const v8bf*>(sb + img128(16 * i + l15, kb * 4 + lq));
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");

    *reinterpret_cast<uint32_t*>(lds + kBias1 + tid * 4) = b1_pair;
    __syncthreads();

    v4f acc2[2][8];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc2[i][j] = v4f{0.f, 0.f, 0.f, 0.f};

    for (int hc = 0; hc < kNChunk; ++hc) {
        // chunk hc has landed (every wave's pieces: barrier), and every wave is done with the slot the next chunk goes to
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (hc + 1 < kNChunk) stage((hc + 1) & 1, hc + 1);
        const char* wb = lds + (hc & 1) * kStage;
        v4f b1c[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const v4bf t = *reinterpret_cast<const v4bf*>(lds + kBias1 + (hc * kChunk + 16 * j + 4 * lq) * 2);
            b1c[j] = v4f{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
        }

        // fc1: hidden channels 32 hc + 16 j + (4 lq + r) of tokens 16 i + l15, k blocks ascending
        v4f acc1[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc1[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) {
            v8bf wf[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) wf[j] = *reinterpret_cast<const v8bf*>(wb + img128(16 * j + l15, kb * 4 + lq));
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xh[i][kb], acc1[i][j], 0, 0, 0);
        }
        // bias + GELU, rounded once to bf16, into the wave's [32, 32] image
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const v4f a = acc1[i][j] + b1c[j];
                v4bf p;
#pragma unroll
                for (int e = 0; e < 4; ++e) p[e] = (__bf16)gelu_f(a[e]);
                *reinterpret_cast<v4bf*>(sb + img32(16 * i + l15, 2 * j + (lq >> 1)) + (lq & 1) * 8) = p;
            }
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
        v8bf hf[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) hf[i] = *reinterpret_cast<const v8bf*>(sb + img32(16 * i + l15, lq));
        // fc2: k block hc of the 16, output channels 16 j + (4 lq + r)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const v8bf w2f = *reinterpret_cast<const v8bf*>(wb + kW1Bytes + img32(16 * j + l15, lq));
#pragma unroll
            for (int i = 0; i < 2; ++i) acc2[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w2f, hf[i], acc2[i][j], 0, 0, 0);
        }
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
    }

    // ---- branch = bf16(acc + b2) into the wave's [32, 128] image, then row-wise: x_out = bf16(x + branch), next norm ------------
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const v4bf t = *reinterpret_cast<const v4bf*>(g.b2 + 16 * j + 4 * lq);
        const v4f b2v = {(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const v4f a = acc2[i][j] + b2v;
            v4bf p;
#pragma unroll
            for (int e = 0; e < 4; ++e) p[e] = (__bf16)a[e];
            *reinterpret_cast<v4bf*>(sb + img128(16 * i + l15, 2 * j + (lq >> 1)) + (lq & 1) * 8) = p;
        }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
    float wv[8], bv[8];
    if constexpr (NEXT) {
        Vec8<__hip_bfloat16>::load(g.nnw + l15 * 8, wv);
        Vec8<__hip_bfloat16>::load(g.nnb + l15 * 8, bv);
    }
    const bool nt = g.nt != 0;
#pragma unroll
    for (int it = 0; it < kRowsWave / 4; ++it) {
        const int rr = it * 4 + lq;
        const int row = row0 + rr;
        const int rc = min(row, g.rows - 1);
        float v[1][8], br[8];
        Vec8<__hip_bfloat16>::load(g.x + (size_t)rc * kC + l15 * 8, v[0]);  // (the wave's own rows again: L2)
        Vec8<__hip_bfloat16>::load(reinterpret_cast<const __hip_bfloat16*>(sb + img128(rr, l15)), br);
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            v[0][i] = round_to<__hip_bfloat16>(__fadd_rn(v[0][i], br[i]));
            s += v[0][i];
        }
        if (row < g.rows) Vec8<__hip_bfloat16>::store(g.x_out + (size_t)row * kC + l15 * 8, v[0], nt);
        if constexpr (NEXT) {
            float mu, rs, o[8];
            ln_row_stats<16, 1>(v, s, g.next_eps, mu, rs);
            ln_row_normalise(v[0], mu, rs, wv, bv, o);
            if (row < g.rows) Vec8<__hip_bfloat16>::store(g.n_out + (size_t)row * kC + l15 * 8, o, nt);
        }
    }
}

template <bool NEXT>
int launch(const MlpS0Args& g, hipStream_t st) {
    auto kern = mlp_s0_fwd<NEXT>;
    static grit_detail::PerDevice<bool> attr_done_pd;
    bool& attr_done = attr_done_pd();  // idempotent: racing threads set the same value
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, kLds) != hipSuccess) return GRIT_ERR_LAUNCH;
        attr_done = true;
    }
    hipLaunchKernelGGL(kern, dim3((g.rows + kRowsWG - 1) / kRowsWG), dim3(kWaves * 64), kLds, st, g);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

}  // namespace

extern "C" int grit_mlp_s0_fwd_bf16(const void* x, const void* norm_w, const void* norm_b, float eps, const void* w1, const void* b1,
                                    const void* w2, const void* b2, const void* next_w, const void* next_b, float next_eps, int rows,
                                    int C, int hidden, void* x_out, void* n_out, void* stream) {
    if (!x || !norm_w || !norm_b || !w1 || !b1 || !w2 || !b2 || !x_out || rows <= 0) return GRIT_ERR_BAD_ARG;
    if ((next_w != nullptr) != (next_b != nullptr) || (next_w != nullptr) != (n_out != nullptr)) return GRIT_ERR_BAD_ARG;
    if (x_out == x || n_out == x) return GRIT_ERR_BAD_ARG;
    if (C != kC || hidden != kHidden || rows > 0x7fffffff / kC) return GRIT_ERR_UNSUPPORTED;
    if (((uintptr_t)x | (uintptr_t)norm_w | (uintptr_t)norm_b | (uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)x_out | (uintptr_t)n_out |
         (uintptr_t)next_w | (uintptr_t)next_b) & 15)
        return GRIT_ERR_UNSUPPORTED;
    if (((uintptr_t)b1 | (uintptr_t)b2) & 7) return GRIT_ERR_UNSUPPORTED;
    MlpS0Args g;
    g.x = (const __hip_bfloat16*)x; g.nw = (const __hip_bfloat16*)norm_w; g.nb = (const __hip_bfloat16*)norm_b;
    g.w1 = (const __bf16*)w1; g.b1 = (const __bf16*)b1; g.w2 = (const __bf16*)w2; g.b2 = (const __bf16*)b2;
    g.nnw = (const __hip_bfloat16*)next_w; g.nnb = (const __hip_bfloat16*)next_b;
    g.x_out = (__hip_bfloat16*)x_out; g.n_out = (__hip_bfloat16*)n_out;
    g.eps = eps; g.next_eps = next_eps; g.rows = rows;
    g.nt = (size_t)rows * kC * 2 >= ((size_t)16 << 20);  // ln_fwd's rule: long maps are streamed past L2
    return next_w ? launch<true>(g, (hipStream_t)stream) : launch<false>(g, (hipStream_t)stream);
}
