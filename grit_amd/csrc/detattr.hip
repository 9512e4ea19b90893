// The attribute head of detector pre-training (include/grit_hip.h, "Detector attribute head"): the front of AttrHead -- label of
// every query, its class embedding and the concatenation with the query's hidden state -- in one launch, the gradient of the
// embedding table in one launch without atomics, and the weighted attribute loss (reference od_losses.py:141-177) forward and
// backward in one launch each, built like det_loss_{fwd,bwd}_kernel of detloss.hip: blocks over (image, chunk of rows), one wave per
// query row, fp32 per element, every sum in float64, the two counts as integers, the last ticket reduces in a fixed order.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/grit_hip.h"

namespace {

constexpr int kWave = 64;
constexpr int kRows = GRIT_DET_LOSS_ROWS;

__device__ inline float widen(const void* p, long i, bool bf16) {
    if (!bf16) return ((const float*)p)[i];
    return __uint_as_float((unsigned int)((const unsigned short*)p)[i] << 16);
}

__device__ inline unsigned short to_bf16(float v) {  // round to nearest even; NaN stays NaN
    const unsigned int u = __float_as_uint(v);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)((u >> 16) | 0x40u);
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// `bytes` bytes from src to dst by the 64 lanes of a wave: 16 bytes per lane where both ends and the length allow it, else elements.
__device__ inline void wave_copy(void* __restrict__ dst, const void* __restrict__ src, long bytes, int es, int lane) {
    if (((((uintptr_t)dst) | ((uintptr_t)src) | (uintptr_t)bytes) & 15) == 0) {
        const uint4* s = (const uint4*)src;
        uint4* d = (uint4*)dst;
        for (long i = lane; i < bytes / 16; i += kWave) d[i] = s[i];
    } else if (es == 4) {
        const unsigned int* s = (const unsigned int*)src;
        unsigned int* d = (unsigned int*)dst;
        for (long i = lane; i < bytes / 4; i += kWave) d[i] = s[i];
    } else {
        const unsigned short* s = (const unsigned short*)src;
        unsigned short* d = (unsigned short*)dst;
        for (long i = lane; i < bytes / 2; i += kWave) d[i] = s[i];
    }
}

// One wave per row.  label = the FIRST index of the largest fp32 sigmoid (the sigmoid is 1.0f from about 16.7 up, so this is not
// the argmax of the logits); out[row] = [obj_h[row] | embed[label]].
__global__ __launch_bounds__(256) void attr_embed_cat_kernel(const void* __restrict__ obj_h, const void* __restrict__ logits,
                                                             const void* __restrict__ embed, void* __restrict__ out,
                                                             int32_t* __restrict__ labels, int rows, int K, int d, int es,
                                                             bool logits_bf16) {
    const int lane = threadIdx.x & (kWave - 1);
    const long row = (long)blockIdx.x * 4 + threadIdx.x / kWave;
    if (row >= rows) return;
    float top = -INFINITY;
    int arg = INT_MAX;
    for (int k = lane; k < K; k += kWave) {
        const float x = widen(logits, row * K + k, logits_bf16);
        const float s = 1.0f / (1.0f + expf(-x));
        if (s > top) {  // k rises within a lane: the first of equals stays
            top = s;
            arg = k;
        }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const float ot = __shfl_xor(top, off, kWave);
        const int oa = __shfl_xor(arg, off, kWave);
        if (ot > top || (ot == top && oa < arg)) {
            top = ot;
            arg = oa;
        }
    }
    if (arg >= K) arg = 0;  // a row of NaNs: outside the contract, but never an index outside the table
    if (lane == 0) labels[row] = arg;
    const long half = (long)d * es;
    char* o = (char*)out + row * 2 * half;
    wave_copy(o, (const char*)obj_h + row * half, half, es, lane);
    wave_copy(o + half, (const char*)embed + (long)arg * half, half, es, lane);
}

// Block (class k, tile of 64 columns), one wave.  The wave reads the labels 64 at a time and adds the rows that chose k in row
// order: the sum's order is a function of the labels alone.  A class nobody chose gets zeros.
__global__ __launch_bounds__(kWave) void attr_embed_grad_kernel(const void* __restrict__ dcat, const int32_t* __restrict__ labels,
                                                                void* __restrict__ dweight, int rows, int d, long ld, int col0,
                                                                bool bf16) {
    const int lane = threadIdx.x;
    const int k = blockIdx.x, c = blockIdx.y * kWave + lane;
    const bool live = c < d;
    float acc = 0.0f;
    for (int r0 = 0; r0 < rows; r0 += kWave) {
        const int r = r0 + lane;
        unsigned long long hits = __ballot(r < rows && labels[r] == k);
        while (hits) {
            const int i = __ffsll((long long)hits) - 1;
            hits &= hits - 1;
            if (live) acc += widen(dcat, (long)(r0 + i) * ld + col0 + c, bf16);
        }
    }
    if (!live) return;
    if (bf16)
        ((unsigned short*)dweight)[(long)k * d + c] = to_bf16(acc);
    else
        ((float*)dweight)[(long)k * d + c] = acc;
}

// ---- weighted attribute loss -----------------------------------------------------------------------------------------------------

__device__ inline double wave_sum(double v) {
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

__device__ inline long long wave_sum(long long v) {
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// Block (image, chunk of kRows queries), one wave per query row.  A row takes part when its image has attributes and the row is
// matched; its target row is attributes[offset_b + t].  partials [blocks, 2] = sum of bce over the ones, over the zeros; counts
// [blocks, 2] = the ones, the zeros.  The block that takes the last ticket adds them up in block order and writes loss[0] and
// totals = (N1, N0).
__global__ __launch_bounds__(256) void det_attr_fwd_kernel(const float* __restrict__ x, const uint8_t* __restrict__ attributes,
                                                           const int32_t* __restrict__ tgt_offsets, const uint8_t* __restrict__ has_attr,
                                                           const int32_t* __restrict__ match_t, int Q, int A, int chunks,
                                                           double* partials, int64_t* counts, unsigned int* ticket,
                                                           float* __restrict__ loss, int64_t* __restrict__ totals) {
    __shared__ double red[4][2];
    __shared__ long long redn[4][2];
    __shared__ int is_last;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const int first = tgt_offsets[b], T = tgt_offsets[b + 1] - first;
    const int q_end = min(Q, (chunk + 1) * kRows);
    double s1 = 0.0, s0 = 0.0;
    long long n1 = 0, n0 = 0;
    if (has_attr[b] && first >= 0) {
        for (int q = chunk * kRows + wave; q < q_end; q += 4) {
            const int t = match_t[(long)b * Q + q];
            if (t < 0 || t >= T) continue;
            const float* xr = x + ((long)b * Q + q) * A;
            const uint8_t* yr = attributes + (long)(first + t) * A;
            for (int a = lane; a < A; a += kWave) {
                const float v = xr[a];
                const float l = log1pf(expf(-fabsf(v)));
                if (yr[a]) {  // max(x, 0) - x + log1p(exp(-|x|))
                    s1 += fmaxf(-v, 0.0f) + l;
                    n1 += 1;
                } else {
                    s0 += fmaxf(v, 0.0f) + l;
                    n0 += 1;
                }
            }
        }
    }
    s1 = wave_sum(s1), s0 = wave_sum(s0);
    n1 = wave_sum(n1), n0 = wave_sum(n0);
    if (lane == 0) {
        red[wave][0] = s1, red[wave][1] = s0;
        redn[wave][0] = n1, redn[wave][1] = n0;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        partials[(long)blockIdx.x * 2 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        counts[(long)blockIdx.x * 2 + threadIdx.x] = redn[0][threadIdx.x] + redn[1][threadIdx.x] + redn[2][threadIdx.x] + redn[3][threadIdx.x];
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) is_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    const volatile double* part = partials;
    const volatile int64_t* cnt = counts;
    double a1 = 0.0, a0 = 0.0;
    long long c1 = 0, c0 = 0;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += 256) {
        a1 += part[(long)i * 2], a0 += part[(long)i * 2 + 1];
        c1 += cnt[(long)i * 2], c0 += cnt[(long)i * 2 + 1];
    }
    a1 = wave_sum(a1), a0 = wave_sum(a0);
    c1 = wave_sum(c1), c0 = wave_sum(c0);
    __syncthreads();
    if (lane == 0) {
        red[wave][0] = a1, red[wave][1] = a0;
        redn[wave][0] = c1, redn[wave][1] = c0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double t1 = red[0][0] + red[1][0] + red[2][0] + red[3][0], t0 = red[0][1] + red[1][1] + red[2][1] + red[3][1];
        const long long N1 = redn[0][0] + redn[1][0] + redn[2][0] + redn[3][0], N0 = redn[0][1] + redn[1][1] + redn[2][1] + redn[3][1];
        const double inside = N1 > 0 ? t1 / (double)N1 : 0.0, outside = N0 > 0 ? t0 / (double)N0 : 0.0;
        loss[0] = (float)(inside + outside);
        totals[0] = N1;
        totals[1] = N0;
    }
}

// Same blocks and rows as the forward; every element of dx is written.
__global__ __launch_bounds__(256) void det_attr_bwd_kernel(const float* __restrict__ x, const uint8_t* __restrict__ attributes,
                                                           const int32_t* __restrict__ tgt_offsets, const uint8_t* __restrict__ has_attr,
                                                           const int32_t* __restrict__ match_t, int Q, int A, int chunks,
                                                           const int64_t* __restrict__ totals, const float* __restrict__ upstream,
                                                           float* __restrict__ dx) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const int first = tgt_offsets[b], T = tgt_offsets[b + 1] - first;
    const int q_end = min(Q, (chunk + 1) * kRows);
    const bool image = has_attr[b] && first >= 0;
    const long long N1 = totals[0], N0 = totals[1];
    const double up = (double)upstream[0];
    const float w1 = N1 > 0 ? (float)(up / (double)N1) : 0.0f, w0 = N0 > 0 ? (float)(up / (double)N0) : 0.0f;
    for (int q = chunk * kRows + wave; q < q_end; q += 4) {
        const int t = image ? match_t[(long)b * Q + q] : -1;
        const bool hit = t >= 0 && t < T;
        const float* xr = x + ((long)b * Q + q) * A;
        float* dr = dx + ((long)b * Q + q) * A;
        if (!hit) {
            for (int a = lane; a < A; a += kWave) dr[a] = 0.0f;
            continue;
        }
        const uint8_t* yr = attributes + (long)(first + t) * A;
        for (int a = lane; a < A; a += kWave) {
            const float v = xr[a];
            const float e = expf(-fabsf(v));
            const float inv = 1.0f / (1.0f + e);
            const float p = v >= 0.0f ? inv : e * inv, qq = v >= 0.0f ? e * inv : inv;  // sigmoid(x), 1 - sigmoid(x)
            dr[a] = yr[a] ? -qq * w1 : p * w0;
        }
    }
}

bool loss_sizes_ok(int B, int Q, int A) {
    if (B <= 0 || Q <= 0 || A <= 0) return false;
    return (double)B * Q * (double)A < 9.0e15 && (long)B * ((Q + kRows - 1) / kRows) < INT_MAX;
}

}  // namespace

extern "C" {

int grit_attr_embed_cat(const void* obj_h, const void* logits, const void* embed, void* out, int32_t* labels, int rows, int K, int d,
                        int bf16, int logits_bf16, void* stream) {
    if (!obj_h || !logits || !embed || !out || !labels || rows <= 0 || K <= 0 || d <= 0) return GRIT_ERR_BAD_ARG;
    if ((double)rows * (double)K >= 9.0e15 || (double)rows * 2.0 * (double)d >= 9.0e15 || (double)K * (double)d >= 9.0e15)
        return GRIT_ERR_BAD_ARG;
    hipLaunchKernelGGL(attr_embed_cat_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, obj_h, logits, embed, out, labels,
                       rows, K, d, bf16 ? 2 : 4, logits_bf16 != 0);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

int grit_attr_embed_grad(const void* dcat, const int32_t* labels, void* dweight, int rows, int K, int d, int ld, int col0, int bf16,
                         void* stream) {
    if (!dcat || !labels || !dweight || rows <= 0 || K <= 0 || d <= 0 || col0 < 0 || (long)col0 + d > ld) return GRIT_ERR_BAD_ARG;
    if ((double)rows * (double)ld >= 9.0e15 || (double)K * (double)d >= 9.0e15) return GRIT_ERR_BAD_ARG;
    const int tiles = (d + kWave - 1) / kWave;
    if (tiles > 65535) return GRIT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(attr_embed_grad_kernel, dim3(K, tiles), dim3(kWave), 0, (hipStream_t)stream, dcat, labels, dweight, rows, d,
                       (long)ld, col0, bf16 != 0);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

int grit_det_attr_fwd_f32(const float* attr_logits, const uint8_t* attributes, const int32_t* tgt_offsets, const uint8_t* has_attr,
                          const int32_t* match_t, int B, int Q, int A, double* partials, int64_t* counts, unsigned int* ticket,
                          float* loss, int64_t* totals, void* stream) {
    if (!attr_logits || !attributes || !tgt_offsets || !has_attr || !match_t || !partials || !counts || !ticket || !loss || !totals)
        return GRIT_ERR_BAD_ARG;
    if (!loss_sizes_ok(B, Q, A)) return GRIT_ERR_BAD_ARG;
    const int chunks = (Q + kRows - 1) / kRows;
    if (hipMemsetAsync(ticket, 0, sizeof(unsigned int), (hipStream_t)stream) != hipSuccess) return GRIT_ERR_LAUNCH;
    hipLaunchKernelGGL(det_attr_fwd_kernel, dim3(B * chunks), dim3(256), 0, (hipStream_t)stream, attr_logits, attributes, tgt_offsets,
                       has_attr, match_t, Q, A, chunks, partials, counts, ticket, loss, totals);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

int grit_det_attr_bwd_f32(const float* attr_logits, const uint8_t* attributes, const int32_t* tgt_offsets, const uint8_t* has_attr,
                          const int32_t* match_t, int B, int Q, int A, const int64_t* totals, const float* upstream, float* dlogits,
                          void* stream) {
    if (!attr_logits || !attributes || !tgt_offsets || !has_attr || !match_t || !totals || !upstream || !dlogits) return GRIT_ERR_BAD_ARG;
    if (!loss_sizes_ok(B, Q, A)) return GRIT_ERR_BAD_ARG;
    const int chunks = (Q + kRows - 1) / kRows;
    hipLaunchKernelGGL(det_attr_bwd_kernel, dim3(B * chunks), dim3(256), 0, (hipStream_t)stream, attr_logits, attributes, tgt_offsets,
                       has_attr, match_t, Q, A, chunks, totals, upstream, dlogits);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

}  // extern "C"
