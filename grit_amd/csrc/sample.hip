// Sampled decoding: one word per row from the tempered, top-k / nucleus truncated word distribution (grit_sample_step_f32, the
// nine steps in include/grit_hip.h).  Everything after the fp32 weight of a word is integer arithmetic on uint64 weights, so the
// result is a function of the stored bits, the seed, the row and the step: no atomics on global memory, no workspace, one launch.
//
// One 256-thread workgroup per output row.  The row is read once into LDS (64 KiB at GRIT_SAMPLE_MAX_V) while its maximum is
// reduced; every later pass walks LDS.  Thread t owns the CONTIGUOUS indices [t * per, (t + 1) * per) with `per` odd, so that the
// 64 lanes of a wave hit 32 banks conflict-free (stride per mod 32 is odd) and a block scan of per-thread sums is a scan in index
// order -- which is what step 8 asks for.
//   plain (top_k = 0, top_p = 1): load + max, per-thread weight sums, one block scan, the owner of the target walks its chunk.
//   truncated: the kept set is a prefix of the order (log-prob descending, index ascending), i.e. "every word whose order key is
//     above u*, and the first c words of the group equal to u*".  (u*, c) comes from an 8-bit radix select over the order key, as in
//     det_topk_chunk_kernel (deteval.hip), with a count and a uint64 weight histogram per digit: by count for top-k (which also
//     yields S_K), then by weight for the nucleus inside the top-k set.  All words of a tie group have one weight, so the number
//     kept inside the boundary group is a division, and "the first c by index" is one more block scan (of tie counts).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grit_hip.h"

// the weight of a word is specified operation by operation: no fused multiply-adds
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;

__device__ __forceinline__ uint32_t order_key(float x) {  // larger log-prob <=> larger key; -0.0 and +0.0 share a key
    const uint32_t b = __float_as_uint(x + 0.f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float key_value(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// steps 2-4: trunc(P(f) * 2^(40 + k)) with t = k + f
__device__ __forceinline__ uint64_t word_weight(float lp, float m, float inv_t) {
    const float t = ((lp - m) * inv_t) * __uint_as_float(0x3FB8AA3Bu);
    if (!(t >= -42.f)) return 0;  // -inf, NaN, and 40 + k < -1 with room to spare for the conversion below
    const float fl = floorf(t);
    int e = 40 + (int)fl;
    if (e < -1) return 0;
    e = e > 40 ? 40 : e;  // t > 0 needs a NaN or +inf in the row: keep the shift in range
    const float f = t - fl;
    float p = __uint_as_float(0x3962A320u);
    p = p * f + __uint_as_float(0x3AA36993u);
    p = p * f + __uint_as_float(0x3C1E8620u);
    p = p * f + __uint_as_float(0x3D634478u);
    p = p * f + __uint_as_float(0x3E75FEADu);
    p = p * f + __uint_as_float(0x3F317216u);
    p = p * f + 1.0f;
    const uint64_t mant = (uint64_t)(p * 8388608.f);  // p in [1, 2]: p * 2^23 is an integer, exactly
    const int sh = e - 23;
    return sh >= 0 ? mant << sh : mant >> -sh;
}

struct Scratch {
    uint32_t hist_c[256];
    uint64_t hist_w[256];
    uint64_t wave_sum[kWaves];
    float wave_max[kWaves];
    // what the wave that searches the histogram found
    uint32_t bin, bin_c, above_c;
    uint64_t above_w;
};

// exclusive prefix of v over the threads of the workgroup, and the total
__device__ __forceinline__ uint64_t block_scan(uint64_t v, Scratch& s, uint64_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(incl, d, 64);
        if (lane >= d) incl += o;
    }
    __syncthreads();  // the previous user of wave_sum is done
    if (lane == 63) s.wave_sum[w] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int q = 0; q < kWaves; ++q) {
        const uint64_t x = s.wave_sum[q];
        if (q < w) before += x;
        all += x;
    }
    total = all;
    return before + incl - v;
}

struct Boundary {  // the kept set: key > u, and the first c (by index) of the words whose key equals u
    uint32_t u, c;
};

struct Selected {
    uint32_t u, group_c, above_c;  // the key at the boundary, how many words have it, how many are above it
    uint64_t above_w;              // the weight above it
};

// The key u with metric(key > u) < target <= metric(key >= u), metric = word count (kByWeight = false) or weight sum.  With
// `limited` only the words inside `limit` take part.  Four passes of eight key bits, most significant first.
template <bool kByWeight>
__device__ Selected radix_select(const float* row, int begin, int end, float m, float inv_t, uint64_t target, bool limited,
                                 Boundary limit, uint64_t limit_w, Scratch& s) {
    const int tid = threadIdx.x;
    uint32_t prefix = 0, above_c = 0, group_c = 0;
    uint64_t above_w = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        s.hist_c[tid] = 0;
        s.hist_w[tid] = 0;
        __syncthreads();
        // consecutive words of a thread mostly share a digit (log-probs span a few binades): add a run at a time
        int run_bin = -1;
        uint32_t run_c = 0;
        uint64_t run_w = 0;
        for (int i = begin; i < end; ++i) {
            const float x = row[i];
            const uint32_t u = order_key(x);
            if (shift < 24 && (u >> (shift + 8)) != prefix) continue;
            if (limited && u <= limit.u) continue;  // below the limit: out; its boundary group is added once, below
            const int bin = (u >> shift) & 255;
            if (bin != run_bin) {
                if (run_c) { atomicAdd(&s.hist_c[run_bin], run_c); atomicAdd((unsigned long long*)&s.hist_w[run_bin], (unsigned long long)run_w); }
                run_bin = bin; run_c = 0; run_w = 0;
            }
            ++run_c;
            run_w += word_weight(x, m, inv_t);
        }
        if (run_c) { atomicAdd(&s.hist_c[run_bin], run_c); atomicAdd((unsigned long long*)&s.hist_w[run_bin], (unsigned long long)run_w); }
        if (limited && tid == 0 && (shift == 24 || (limit.u >> (shift + 8)) == prefix)) {
            const int bin = (limit.u >> shift) & 255;
            atomicAdd(&s.hist_c[bin], limit.c);
            atomicAdd((unsigned long long*)&s.hist_w[bin], (unsigned long long)(limit.c * limit_w));
        }
        __syncthreads();
        if (tid < 64) {  // lane l looks at the bins 255 - 4l .. 252 - 4l, highest first
            uint32_t c[4], lane_c = 0;
            uint64_t w[4], lane_w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[j] = s.hist_c[255 - 4 * tid - j];
                w[j] = s.hist_w[255 - 4 * tid - j];
                lane_c += c[j];
                lane_w += w[j];
            }
            uint64_t incl_w = lane_w;
            uint32_t incl_c = lane_c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint64_t ow = __shfl_up(incl_w, d, 64);
                const uint32_t oc = __shfl_up(incl_c, d, 64);
                if (tid >= d) { incl_w += ow; incl_c += oc; }
            }
            uint32_t run_above_c = above_c + (incl_c - lane_c);
            uint64_t run_above_w = above_w + (incl_w - lane_w);
            int hit = -1;
            uint32_t hit_c = 0, hit_above_c = 0;
            uint64_t hit_above_w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint64_t reached = kByWeight ? run_above_w + w[j] : (uint64_t)run_above_c + c[j];
                const bool last = tid == 63 && j == 3;  // cannot be needed inside the contract: target <= the total
                if (hit < 0 && (reached >= target || last)) {
                    hit = 255 - 4 * tid - j; hit_c = c[j]; hit_above_c = run_above_c; hit_above_w = run_above_w;
                }
                run_above_c += c[j];
                run_above_w += w[j];
            }
            const unsigned long long found = __ballot(hit >= 0);
            if (tid == __ffsll((long long)found) - 1) {
                s.bin = hit; s.bin_c = hit_c; s.above_c = hit_above_c; s.above_w = hit_above_w;
            }
        }
        __syncthreads();
        prefix = (prefix << 8) | s.bin;
        above_c = s.above_c;
        above_w = s.above_w;
        group_c = s.bin_c;
    }
    Selected r;
    r.u = prefix; r.group_c = group_c; r.above_c = above_c; r.above_w = above_w;
    return r;
}

template <bool kTruncated>  // false: top_k = 0 and top_p = 1, no select pass is compiled in
__global__ __launch_bounds__(kThreads)
void sample_step_kernel(const float* __restrict__ logp, long ld, int fan, int V, const int64_t* __restrict__ prev_words,
                        const float* __restrict__ alive_in, int eos, int fill, float inv_t, int top_k, unsigned long long top_p_q32,
                        const uint64_t* __restrict__ seed_dev, int step, int64_t* __restrict__ words, float* __restrict__ picked,
                        float* __restrict__ alive_out) {
    __shared__ float row[GRIT_SAMPLE_MAX_V];
    __shared__ Scratch s;
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (prev_words) {  // step 0
        const float alive = alive_in[r] * (prev_words[r] != (int64_t)eos ? 1.f : 0.f);
        if (alive == 0.f) {
            if (tid == 0) { words[r] = fill; picked[r] = 0.f; alive_out[r] = 0.f; }
            return;
        }
    }
    // step 1, while the row moves to LDS: 16-byte loads where the row allows it
    const float* src = logp + (size_t)(r / fan) * ld;
    float m = -INFINITY;
    {
        const int head = (int)(((16 - ((uintptr_t)src & 15)) & 15) >> 2);
        const int lead = head < V ? head : V;
        if (tid < lead) { const float x = src[tid]; row[tid] = x; m = fmaxf(m, x); }
        const int n4 = (V - lead) >> 2;
        const float4* src4 = reinterpret_cast<const float4*>(src + lead);
        for (int i = tid; i < n4; i += kThreads) {
            const float4 x = src4[i];
            const int at = lead + 4 * i;
            row[at] = x.x; row[at + 1] = x.y; row[at + 2] = x.z; row[at + 3] = x.w;
            m = fmaxf(fmaxf(m, x.x), fmaxf(x.y, fmaxf(x.z, x.w)));
        }
        for (int i = lead + 4 * n4 + tid; i < V; i += kThreads) { const float x = src[i]; row[i] = x; m = fmaxf(m, x); }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    if (lane == 0) s.wave_max[wave] = m;
    __syncthreads();
    m = s.wave_max[0];
#pragma unroll
    for (int q = 1; q < kWaves; ++q) m = fmaxf(m, s.wave_max[q]);

    const int per = ((V + kThreads - 1) / kThreads) | 1;
    const int begin = min(V, tid * per), end = min(V, begin + per);

    // steps 5 and 6
    const int K = top_k > 0 && top_k < V ? top_k : V;
    const bool by_k = K < V, by_p = top_p_q32 < (1ull << 32);
    Boundary kept;
    kept.u = 0; kept.c = 0;
    if (kTruncated) {
        uint64_t S_K, kept_w = 0;
        if (by_k) {
            const Selected a = radix_select<false>(row, begin, end, m, inv_t, (uint64_t)K, false, kept, 0, s);
            kept.u = a.u;
            kept.c = (uint32_t)K - a.above_c;
            kept_w = word_weight(key_value(a.u), m, inv_t);
            S_K = a.above_w + kept.c * kept_w;
        } else {
            uint64_t sum = 0;
            for (int i = begin; i < end; ++i) sum += word_weight(row[i], m, inv_t);
            block_scan(sum, s, S_K);
        }
        if (by_p) {
            const uint64_t hi = __umul64hi(top_p_q32, S_K), lo = top_p_q32 * S_K;
            uint64_t need = (hi << 32) | (lo >> 32);
            need = need < 1 ? 1 : need;
            const Boundary top = kept;
            const Selected a = radix_select<true>(row, begin, end, m, inv_t, need, by_k, top, kept_w, s);
            const uint64_t w = word_weight(key_value(a.u), m, inv_t);
            const uint32_t have = by_k && a.u == top.u ? top.c : a.group_c;
            const uint64_t missing = need > a.above_w ? need - a.above_w : 1;
            uint64_t c = w ? (missing + w - 1) / w : have;
            c = c > have ? have : c;
            kept.u = a.u;
            kept.c = (uint32_t)(c < 1 ? 1 : c);
        }
    }
    constexpr bool truncated = kTruncated;

    // "the first c of the boundary group by index": how many of the group lie before this thread's words
    uint64_t group_before = 0;
    if (truncated) {
        uint64_t mine = 0, all;
        for (int i = begin; i < end; ++i) mine += order_key(row[i]) == kept.u;
        group_before = block_scan(mine, s, all);
    }
    // steps 7 and 8: kept weights summed in index order
    uint64_t sum = 0;
    {
        uint64_t seen = group_before;
        for (int i = begin; i < end; ++i) {
            const float x = row[i];
            const uint32_t u = order_key(x);
            const bool in = !truncated || u > kept.u || (u == kept.u && seen++ < kept.c);
            sum += in ? word_weight(x, m, inv_t) : 0;
        }
    }
    uint64_t S;
    const uint64_t before = block_scan(sum, s, S);
    if (S == 0) {  // no finite entry: outside the contract
        if (tid == 0) { words[r] = 0; picked[r] = row[0]; alive_out[r] = 1.f; }
        return;
    }
    uint64_t x = *seed_dev + 0x9E3779B97F4A7C15ull * ((uint64_t)r * 4096ull + (uint64_t)step + 1ull);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    const uint64_t target = __umul64hi(x, S);
    if (before <= target && target < before + sum) {  // exactly one thread
        uint64_t seen = group_before, acc = before;
        int word = begin;
        for (int i = begin; i < end; ++i) {
            const float v = row[i];
            const uint32_t u = order_key(v);
            const bool in = !truncated || u > kept.u || (u == kept.u && seen++ < kept.c);
            acc += in ? word_weight(v, m, inv_t) : 0;
            if (acc > target) { word = i; break; }
        }
        words[r] = word;
        picked[r] = row[word];
        alive_out[r] = 1.f;
    }
}

}  // namespace

extern "C" int grit_sample_step_f32(const float* logp, long ld, int rows, int fan, int V, const int64_t* prev_words,
                                    const float* alive_in, int eos, int fill, float inv_temperature, int top_k,
                                    unsigned long long top_p_q32, const uint64_t* seed_dev, int step, int64_t* words, float* picked,
                                    float* alive_out, void* stream) {
    if (!logp || !seed_dev || !words || !picked || !alive_out || rows <= 0 || fan <= 0 || V <= 0 || ld < V || rows % fan != 0 ||
        (prev_words == nullptr) != (alive_in == nullptr) || step < 0 || step >= 4096 || top_k < 0 || top_p_q32 < 1 ||
        top_p_q32 > (1ull << 32) || !(inv_temperature > 0.f) || !(inv_temperature <= 3.402823466e38f))
        return GRIT_ERR_BAD_ARG;
    if (V > GRIT_SAMPLE_MAX_V) return GRIT_ERR_UNSUPPORTED;
    const bool truncated = (top_k > 0 && top_k < V) || top_p_q32 < (1ull << 32);
    hipLaunchKernelGGL(truncated ? sample_step_kernel<true> : sample_step_kernel<false>, dim3(rows), dim3(kThreads), 0,
                       (hipStream_t)stream, logp, ld, fan, V, prev_words, alive_in, eos, fill, inv_temperature, top_k, top_p_q32,
                       seed_dev, step, words, picked, alive_out);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}
