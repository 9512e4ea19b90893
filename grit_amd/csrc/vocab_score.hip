// Caption likelihood head (gfx950): the vocabulary projection of the caption decoder followed by log-softmax and the gather of one
// target column per row, without the [rows, V] logit map.
//
//   logit[v] = sum_k x[r, k] w[v, k]         x [R, D] bf16, w [V, D] bf16, fp32 accumulation on v_mfma_f32_16x16x32_bf16
//   lse[r]   = log sum_v exp(logit[v])       fp32, max-subtracted
//   logp[r]  = logit[target[r]] - lse[r]
//
// replaces CaptionGenerator.forward's `fc` + F.log_softmax (davidnvq/grit models/caption/cap_generator.py:157-167) followed by the
// caller's gather, where the caller wants one log-probability per position: scoring a given caption.
//
// Two launches, no atomics, nothing passes between the workgroups of a launch:
//   1. vocab_score_partial: grid (row tiles of 64, vocabulary slices).  A workgroup (4 waves, 2 x 2) keeps its 64 x D tile of x in
//      LDS for its whole life and streams its slice of w through a two-stage LDS ring in 128-column x 64-deep pieces (global ->
//      registers -> LDS, the loads of the next piece in flight under the MFMAs of this one).  The operands go to the MFMA swapped
//      (vocabulary rows as A, token rows as B) as in gemm.hip: a token sits on the lane, four consecutive vocabulary columns in the
//      accumulator registers, so the running (max, sum of exp) of a row is lane-local until the very end.  After the last 64-deep
//      piece of a 128-column tile every lane folds its 16 logits per token into its running pair; columns >= V enter as -inf.
//      The lane that holds column target[r] stores that logit.  At the end the four lane groups and the two column waves are
//      merged in a fixed order and the pair goes to work[slice][row].
//   2. vocab_score_finish: one thread per row merges the pairs in slice order and writes lse and logp.
// The slice width is a constant (kSliceTiles tiles of 128 columns), so which columns meet in which workgroup, lane and register --
// and the order of every floating-point operation of a row -- is a function of V and D alone: a row's result does not depend on
// how many rows the call has or where the row stands among them.
#include <hip/hip_runtime.h>
#include "per_device.h"
#include <math.h>
#include <stdint.h>
#include "../../include/grit_hip.h"
#include "gemm_math.h"

// Every floating-point operation of this file is rounded on its own: no contraction into fused multiply-adds.  The fold below exists
// in several unrolled copies (token block 0 / 1, the register sets of the w stream); left to the compiler, one copy may contract an
// expression that another does not, and a row's bits would then depend on where it stands in its tile.
#pragma clang fp contract(off)

namespace {

constexpr int kBM = 64, kBN = 128, kBK = 64, kThreads = 256;
constexpr int kAhead = 6;                       // w pieces in flight per thread (register sets of 4 x 16 bytes)
constexpr int kSliceTiles = 2;                  // 128-column tiles per vocabulary slice
constexpr int kSlice = kSliceTiles * kBN;
constexpr int kMinD = 64, kMaxD = 512;
constexpr int kWRow = kBK * 2 + 16;             // bytes of a staged w row: 128 + 16 of padding (conflict-free ds_read_b128)
constexpr int kWStage = kBN * kWRow;
constexpr int kLdsMax = kBM * (kMaxD * 2 + 16) + 2 * kWStage;
constexpr float kLog2e = 1.4426950408889634f;

struct VocabScoreArgs {
    const __bf16* x; long ldx;
    const __bf16* w; long ldw;
    const int64_t* target;
    float* part_m;   // [slices][R]
    float* part_s;   // [slices][R]
    float* tlogit;   // [R]
    int R, V, D;
};

// (m, s) <- (m, s) (+) (m2, s2): the pair of the union of two column sets.  Commutative bit for bit.
__device__ __forceinline__ void merge_pair(float& m, float& s, float m2, float s2) {
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) { s = 0.f; return; }  // neither side has seen a column
    s = s * __builtin_amdgcn_exp2f((m - M) * kLog2e) + s2 * __builtin_amdgcn_exp2f((m2 - M) * kLog2e);
    m = M;
}

__global__ __launch_bounds__(kThreads, 1)
void vocab_score_partial(const VocabScoreArgs g) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l15 = lane & 15, lq = lane >> 4;
    const int m0 = blockIdx.x * kBM, sl = blockIdx.y;
    const int v_begin = sl * kSlice, v_end = min(g.V, v_begin + kSlice);
    const int ntile = (v_end - v_begin + kBN - 1) / kBN;
    const int nkc = g.D / kBK, n_it = ntile * nkc;
    const int xrow = g.D * 2 + 16;  // bytes of an x row in LDS, 16 of padding
    char* xs = lds;
    char* wst = lds + kBM * xrow;

    // ---- the x tile: rows past R repeat row R - 1 (never stored) ---------------------------------------------------------------
    // (all loads of a batch are issued before its first store: eight 16-byte chunks per thread in flight)
    auto load_x = [&]() {
        const int cpr = g.D / 8, total = kBM * cpr;  // 16-byte chunks per row; total is a multiple of 2 * kThreads
        for (int c0 = tid; c0 < total; c0 += 8 * kThreads) {
            u32x4 xr[8];
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int c = min(c0 + b * kThreads, total - 1), row = c / cpr, pc = c - row * cpr;
                xr[b] = *reinterpret_cast<const u32x4*>(g.x + (size_t)min(m0 + row, g.R - 1) * g.ldx + pc * 8);
            }
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int c = c0 + b * kThreads, row = c / cpr, pc = c - row * cpr;
                if (c < total) *reinterpret_cast<u32x4*>(xs + row * xrow + pc * 16) = xr[b];
            }
        }
    };

    // ---- w pieces: 128 rows x 128 bytes = 1024 chunks, four per thread; rows past V repeat row V - 1 (masked in the fold) ----------
    u32x4 wreg[kAhead][4];  // pieces it + 1 .. it + kAhead in flight: a piece's loads have kAhead iterations to land
    auto load_w = [&](int it, u32x4 (&wr)[4]) {
        const int tile = it / nkc, kc = it - tile * nkc;
        const int n0 = v_begin + tile * kBN;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = i * kThreads + tid, row = c >> 3, pc = c & 7;
            const int v = min(n0 + row, g.V - 1);
            wr[i] = *reinterpret_cast<const u32x4*>(g.w + (size_t)v * g.ldw + kc * kBK + pc * 8);
        }
    };
    auto store_w = [&](int stage, const u32x4 (&wr)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = i * kThreads + tid, row = c >> 3, pc = c & 7;
            *reinterpret_cast<u32x4*>(wst + stage * kWStage + row * kWRow + pc * 16) = wr[i];
        }
    };

    // ---- per-lane state: two token blocks of 16 (token = lane & 15), the lane's columns are 16 j + 4 lq + reg of the wave's 64 ---
    long long tgt[2];
    float run_m[2], run_s[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = m0 + wm * 32 + i * 16 + l15;
        tgt[i] = row < g.R ? (long long)g.target[row] : -1ll;
        run_m[i] = -INFINITY;
        run_s[i] = 0.f;
    }
    v4f acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};

    const int x_off = (wm * 32 + l15) * xrow + lq * 16;
    const int w_off = (wn * 64 + l15) * kWRow + lq * 16;

    // piece j is loaded into register set j % kAhead at the start of iteration j - kAhead (that set's previous piece went to LDS at the
    // end of iteration j - kAhead - 1) and stored to stage j & 1 at the end of iteration j - 1
#pragma unroll
    for (int u = 0; u < kAhead; ++u)
        if (u < n_it) load_w(u, wreg[u]);
    load_x();
    store_w(0, wreg[0]);
    __syncthreads();  // x tile and stage 0

    for (int it0 = 0; it0 < n_it; it0 += kAhead) {
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
        const int it = it0 + u;
        if (it >= n_it) break;
        const int tile = it / nkc, kc = it - tile * nkc;
        if (it + kAhead < n_it) load_w(it + kAhead, wreg[u]);
        const char* sb = wst + (it & 1) * kWStage;
#pragma unroll
        for (int ks = 0; ks < kBK / 32; ++ks) {
            v8bf wf[4], xf[2];
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = *reinterpret_cast<const v8bf*>(sb + w_off + j * 16 * kWRow + ks * 64);
#pragma unroll
            for (int i = 0; i < 2; ++i) xf[i] = *reinterpret_cast<const v8bf*>(xs + x_off + i * 16 * xrow + (kc * kBK + ks * 32) * 2);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf[i], acc[i][j], 0, 0, 0);
        }
        if (kc == nkc - 1) {
            // fold the finished 128-column tile into the running pairs
            const int vbase = v_begin + tile * kBN + wn * 64 + lq * 4;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = m0 + wm * 32 + i * 16 + l15;
                float tmax = -INFINITY;
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int v = vbase + j * 16 + r;
                        const float val = v < v_end ? acc[i][j][r] : -INFINITY;  // columns past V: not in the maximum, not in the sum
                        acc[i][j][r] = val;
                        tmax = fmaxf(tmax, val);
                        if (v < v_end && (long long)v == tgt[i]) g.tlogit[row] = val;  // one lane of the whole grid per row
                    }
                if (tmax > -INFINITY) {
                    const float mn = fmaxf(run_m[i], tmax);
                    float sum = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int r = 0; r < 4; ++r) sum += __builtin_amdgcn_exp2f((acc[i][j][r] - mn) * kLog2e);
                    run_s[i] = run_s[i] * __builtin_amdgcn_exp2f((run_m[i] - mn) * kLog2e) + sum;
                    run_m[i] = mn;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = v4f{0.f, 0.f, 0.f, 0.f};
            }
        }
        if (it + 1 < n_it) store_w((it + 1) & 1, wreg[(u + 1) % kAhead]);  // that stage was last read in iteration it - 1
        __syncthreads();
    }
    }

    // ---- merge: the four lane groups of a wave, then the two column waves (through LDS), in this fixed order -------------------
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int d = 16; d <= 32; d <<= 1) {
            const float m2 = __shfl_xor(run_m[i], d, 64), s2 = __shfl_xor(run_s[i], d, 64);
            merge_pair(run_m[i], run_s[i], m2, s2);
        }
    }
    float* red = reinterpret_cast<float*>(wst);  // [64 rows][2]; the ring is idle after the loop's last barrier
    if (wn == 1 && lq == 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int lr = wm * 32 + i * 16 + l15;
            red[lr * 2] = run_m[i];
            red[lr * 2 + 1] = run_s[i];
        }
    }
    __syncthreads();
    if (wn == 0 && lq == 0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int lr = wm * 32 + i * 16 + l15, row = m0 + lr;
            merge_pair(run_m[i], run_s[i], red[lr * 2], red[lr * 2 + 1]);
            if (row < g.R) {
                g.part_m[(size_t)sl * g.R + row] = run_m[i];
                g.part_s[(size_t)sl * g.R + row] = run_s[i];
            }
        }
    }
}

__global__ __launch_bounds__(256)
void vocab_score_finish(const float* __restrict__ part_m, const float* __restrict__ part_s, const float* __restrict__ tlogit,
                        const int64_t* __restrict__ target, long long pad_idx, int R, int V, int slices,
                        float* __restrict__ logp, float* __restrict__ lse) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    float M = -INFINITY;
    for (int s = 0; s < slices; ++s) M = fmaxf(M, part_m[(size_t)s * R + r]);
    float S = 0.f;
    for (int s = 0; s < slices; ++s) S += part_s[(size_t)s * R + r] * expf(part_m[(size_t)s * R + r] - M);
    const float l = M + logf(S);
    lse[r] = l;
    const long long t = target[r];
    float lp;
    if (t == pad_idx) lp = 0.0f;
    else if (t < 0 || t >= (long long)V) lp = __builtin_nanf("");
    else lp = tlogit[r] - l;  // written by the one lane of launch 1 that held column t
    logp[r] = lp;
}

inline int slices_of(int V) { return (V + kSlice - 1) / kSlice; }

}  // namespace

extern "C" int grit_vocab_score_slice(int V, int D) {
    if (V < 1 || D < kMinD || D > kMaxD || D % 64 != 0) return 0;
    return kSlice;
}

extern "C" long grit_vocab_score_workspace(int R, int V, int D) {
    if (R < 1 || grit_vocab_score_slice(V, D) == 0) return 0;
    return (long)(2 * (long)slices_of(V) + 1) * (long)R * (long)sizeof(float);
}

extern "C" int grit_vocab_score_bf16(const void* x, long ldx, const void* w, long ldw, const int64_t* target, long pad_idx, int R,
                                     int V, int D, void* work, float* logp, float* lse, void* stream) {
    if (!x || !w || !target || !work || !logp || !lse || R < 1 || V < 1 || D < 1) return GRIT_ERR_BAD_ARG;
    if (D % 64 != 0 || D < kMinD || D > kMaxD) return GRIT_ERR_UNSUPPORTED;
    if (ldx < D || ldw < D || ldx % 8 != 0 || ldw % 8 != 0) return GRIT_ERR_UNSUPPORTED;
    if (((uintptr_t)x | (uintptr_t)w) & 15) return GRIT_ERR_UNSUPPORTED;
    const int slices = slices_of(V);
    if (slices > 65535 || R > 0x7fffffff - kBM) return GRIT_ERR_UNSUPPORTED;  // grid.y; 32-bit row index m0 + 63
    hipStream_t st = (hipStream_t)stream;
    static grit_detail::PerDevice<bool> attr_done_pd;
    bool& attr_done = attr_done_pd();  // idempotent: racing threads set the same value
    if (!attr_done) {
        if (hipFuncSetAttribute((const void*)vocab_score_partial, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax) != hipSuccess)
            return GRIT_ERR_LAUNCH;
        attr_done = true;
    }
    VocabScoreArgs g;
    g.x = (const __bf16*)x; g.ldx = ldx;
    g.w = (const __bf16*)w; g.ldw = ldw;
    g.target = target;
    g.part_m = (float*)work;
    g.part_s = g.part_m + (size_t)slices * R;
    g.tlogit = g.part_s + (size_t)slices * R;
    g.R = R; g.V = V; g.D = D;
    const int lds = kBM * (D * 2 + 16) + 2 * kWStage;
    hipLaunchKernelGGL(vocab_score_partial, dim3((R + kBM - 1) / kBM, slices), dim3(kThreads), lds, st, g);
    hipLaunchKernelGGL(vocab_score_finish, dim3((R + 255) / 256), dim3(256), 0, st, g.part_m, g.part_s, g.tlogit, target,
                       (long long)pad_idx, R, V, slices, logp, lse);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}
