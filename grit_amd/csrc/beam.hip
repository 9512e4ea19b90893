// Beam-search candidate selection: the `k` best of every row of a [rows, n] float32 matrix, best first.
//
// Replaces what davidnvq/grit models/caption/transformer.py:184-188 (`select`) does with a full descending torch.sort over
// beam * vocabulary = 51 005 candidates per image and step -- and the torch.topk this build used in round 1, whose multi-block
// radix path cannot be replayed from a captured HIP graph on this stack (memory access fault on the second replay once eager
// allocations happen in between, tools/micro/dbg_decode.py topk).  One workgroup per row: every thread keeps the k best of its
// strided share in registers (sorted insertion), the 256 sorted lists are merged by k rounds of a workgroup arg-max over the list
// heads.  Order: value descending; equal values by ascending index (torch leaves the order of ties unspecified); NaN ranks above
// every number, as in torch.  HBM-bound: the row is read once, 16 bytes per lane.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/grit_hip.h"

// No fused multiply-adds anywhere in this file: the ensemble step's `score + mean * factor` must round twice, as torch's
// separate mean and add kernels do (the single-map arithmetic has no product next to a sum, so it is unaffected).
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256, kMaxK = 8;

__device__ __forceinline__ bool better(float a, int ia, float b, int ib) {
    const bool an = a != a, bn = b != b;
    if (an || bn) return an && (!bn || ia < ib);
    return a > b || (a == b && ia < ib);
}

__global__ __launch_bounds__(kThreads)
void topk_rows(const float* __restrict__ x, long ld, int n, int k, int64_t* __restrict__ idx_out, float* __restrict__ val_out) {
    __shared__ float sv[kThreads];
    __shared__ int si[kThreads];
    __shared__ int sw[kThreads];
    const float* row = x + (size_t)blockIdx.x * ld;
    const int tid = threadIdx.x;
    float bv[kMaxK];
    int bi[kMaxK];
#pragma unroll
    for (int j = 0; j < kMaxK; ++j) { bv[j] = -INFINITY; bi[j] = 0x7fffffff; }
    auto push = [&](float v, int i) {
        if (!better(v, i, bv[kMaxK - 1], bi[kMaxK - 1])) return;
        bv[kMaxK - 1] = v; bi[kMaxK - 1] = i;
#pragma unroll
        for (int j = kMaxK - 1; j > 0; --j)
            if (better(bv[j], bi[j], bv[j - 1], bi[j - 1])) {
                const float tv = bv[j]; bv[j] = bv[j - 1]; bv[j - 1] = tv;
                const int ti = bi[j]; bi[j] = bi[j - 1]; bi[j - 1] = ti;
            }
    };
    // 16-byte loads where the row allows it
    const int head = (int)(((16 - ((uintptr_t)row & 15)) & 15) >> 2);
    const int lead = head < n ? head : n;
    if (tid < lead) push(row[tid], tid);
    const int n4 = (n - lead) >> 2;
    const float4* row4 = reinterpret_cast<const float4*>(row + lead);
    for (int i = tid; i < n4; i += kThreads) {
        const float4 v = row4[i];
        const int base = lead + 4 * i;
        push(v.x, base); push(v.y, base + 1); push(v.z, base + 2); push(v.w, base + 3);
    }
    for (int i = lead + 4 * n4 + tid; i < n; i += kThreads) push(row[i], i);
    // merge: k rounds of arg-max over the heads of the per-thread sorted lists
    int headp = 0;
    for (int r = 0; r < k; ++r) {
        float v = -INFINITY; int i = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < kMaxK; ++j)
            if (j == headp) { v = bv[j]; i = bi[j]; }
        sv[tid] = v; si[tid] = i; sw[tid] = tid;
        __syncthreads();
        for (int s = kThreads / 2; s > 0; s >>= 1) {
            if (tid < s && better(sv[tid + s], si[tid + s], sv[tid], si[tid])) {
                sv[tid] = sv[tid + s]; si[tid] = si[tid + s]; sw[tid] = sw[tid + s];
            }
            __syncthreads();
        }
        const int winner = sw[0];
        if (tid == 0) {
            idx_out[(size_t)blockIdx.x * k + r] = si[0];
            val_out[(size_t)blockIdx.x * k + r] = sv[0];
        }
        if (tid == winner) ++headp;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// One beam-search step after the word log-probabilities (transformer.py:204-254 `iter`): candidate scores, the k best of
// beam x vocabulary per image, and the per-beam state that moves with the survivors -- two launches instead of ~25.
//
//   alive[b][j]   = first_step ? 1 : seq_mask[b][j] * (prev_words[b][j] != eos)                              (:212-214)
//   cand[b][j][v] = alive ? seq_logprob[b][j] + logp[b][j][v] : (v == 0 ? seq_logprob[b][j] : -999)          (:210,215-218)
//   top-k of cand[b] flattened over (j, v), value descending / index ascending                               (:184-188)
//   sel_beam = index / V, sel_word = index % V, new score = value, new alive = alive[sel_beam],              (:221-233)
//   picked   = logp[b][sel_beam][sel_word] * alive[sel_beam]                                                 (:238-240)
//
// The arithmetic is the reference's (one fp32 add per candidate; the masked blend `m*c + f*(1-m)` of :218 returns c or f
// exactly for m in {1, 0}), so scores and order are bit-identical to the composed form.  Stage 1: a workgroup per
// (image, beam row, part of the vocabulary) reduces its slice to k sorted candidates; stage 2: one wave per image merges them.
constexpr int kBeamThreads = 256;

__device__ __forceinline__ void wave_best(float& v, int& i, int& o) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const float ov = __shfl_xor(v, s, 64);
        const int oi = __shfl_xor(i, s, 64), oo = __shfl_xor(o, s, 64);
        if (better(ov, oi, v, i)) { v = ov; i = oi; o = oo; }
    }
}

// Where the word log-probabilities come from.  OneMap: a single [rows, ld] map (grit_beam_step_f32).  MeanMaps: the average of
// n <= 8 such maps (grit_beam_step_mean_f32), formed in registers exactly as torch.stack(maps).mean(0) forms it on the device:
// ATen's MeanOps reduction over the stacked dimension runs in ONE thread per output with four accumulators (Reduce.cuh
// thread_reduce_impl, vt0 = 4: map m goes to accumulator m % 4, each starting from 0), combined as ((a0 + a1) + a2) + a3 and
// projected by a MULTIPLY with factor = float(outputs) / float(inputs) (ReduceMomentKernel.cu mean_kernel_impl).
constexpr int kMaxMaps = 8;
struct MapTable { const float* p[kMaxMaps]; };  // by value in the kernel arguments: nothing to upload, nothing to keep alive

struct OneMap {
    static constexpr bool kBans = false, kForced = false;
    const float* p;
    __device__ __forceinline__ float at(size_t i) const { return p[i]; }
    __device__ __forceinline__ bool aligned16(size_t i) const { return (((uintptr_t)(p + i)) & 15) == 0; }
    __device__ __forceinline__ float4 at4(size_t i) const { return *reinterpret_cast<const float4*>(p + i); }
};

struct MeanMaps {
    static constexpr bool kBans = false, kForced = false;
    MapTable t;
    int n;
    float factor;
    __device__ __forceinline__ float at(size_t i) const {
        float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < kMaxMaps; ++m)
            if (m < n) a[m & 3] = a[m & 3] + t.p[m][i];
        return (((a[0] + a[1]) + a[2]) + a[3]) * factor;
    }
    __device__ __forceinline__ bool aligned16(size_t i) const {
        uintptr_t bits = 0;
#pragma unroll
        for (int m = 0; m < kMaxMaps; ++m)
            if (m < n) bits |= (uintptr_t)(t.p[m] + i);
        return (bits & 15) == 0;
    }
    __device__ __forceinline__ float4 at4(size_t i) const {
        float4 a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int m = 0; m < kMaxMaps; ++m)
            if (m < n) {
                const float4 x = *reinterpret_cast<const float4*>(t.p[m] + i);
                float4& s = a[m & 3];
                s.x = s.x + x.x; s.y = s.y + x.y; s.z = s.z + x.z; s.w = s.w + x.w;
            }
        float4 r;
        r.x = (((a[0].x + a[1].x) + a[2].x) + a[3].x) * factor;
        r.y = (((a[0].y + a[1].y) + a[2].y) + a[3].y) * factor;
        r.z = (((a[0].z + a[1].z) + a[2].z) + a[3].z) * factor;
        r.w = (((a[0].w + a[1].w) + a[2].w) + a[3].w) * factor;
        return r;
    }
};

// The constrained step (grit_beam_step_con_f32): a source of word log-probabilities plus the rules that ban words per beam.  All of
// it travels by value in the kernel arguments.  Only stage 1 reads the rules; stage 2 runs on the plain source.
constexpr int kMaxHistory = GRIT_BEAM_MAX_HISTORY, kMaxSuppress = GRIT_BEAM_MAX_SUPPRESS, kMaxSlice = GRIT_BEAM_MAX_SLICE;
struct Bans {
    const int64_t* hist;  // [rows, t], row stride hist_ld
    long hist_ld;
    int t, ngram, repeat_word, eos_word /* -1: <eos> allowed */, n_sup;
    int sup[kMaxSuppress];
};

template <class Base>
struct Banned : Base {
    static constexpr bool kBans = true;
    Bans bans;
};

// The step with forced words (grit_beam_step_forced_f32): the constrained source plus the sets of forced words per image and the
// mask of met sets per beam row.  Stage 1 reads them for one more ban: <eos> while a row has not met every set.
constexpr int kMaxSets = GRIT_BEAM_MAX_FORCED_SETS, kMaxWords = GRIT_BEAM_MAX_FORCED_WORDS;
struct ForcedSets {
    const int64_t* words;  // [B, C, W], -1 = padding
    const int* met;        // [rows] or NULL: every row starts from the image's empty sets
    int C, W;
};

template <class Base>
struct Forced : Banned<Base> {
    static constexpr bool kForced = true;
    ForcedSets forced;
};

__device__ __forceinline__ int met_of_row(const ForcedSets& f, int b, int row_id) {
    if (f.met) return f.met[row_id];
    const int64_t* words = f.words + (size_t)b * f.C * f.W;
    int met = 0;
    for (int c = 0; c < f.C; ++c) {
        bool any = false;
        for (int q = 0; q < f.W; ++q) any = any || words[c * f.W + q] >= 0;
        if (!any) met |= 1 << c;
    }
    return met;
}

// The banned words of one live beam row as a bitmap over the workgroup's vocabulary slice [v0, v1): a thread per history
// position finds the n-gram continuations, further threads add the fixed rules.  The caller synchronises afterwards.
__device__ __forceinline__ void mark_bans(const Bans& c, int row_id, int v0, int v1, int64_t* hist, unsigned* bits) {
    const int tid = threadIdx.x;
    for (int w = tid; w < (v1 - v0 + 31) >> 5; w += kBeamThreads) bits[w] = 0u;
    if (tid < c.t) hist[tid] = c.hist[(size_t)row_id * c.hist_ld + tid];
    __syncthreads();
    auto ban = [&](int64_t word) {
        if (word >= v0 && word < v1) atomicOr(&bits[(int)(word - v0) >> 5], 1u << ((int)(word - v0) & 31));  // LDS
    };
    const int n = c.ngram, t = c.t;
    if (n >= 1 && tid <= t - n) {  // the n - 1 words from position tid against the last n - 1
        bool same = true;
        for (int q = 0; q < n - 1; ++q) same = same && hist[tid + q] == hist[t - n + 1 + q];
        if (same) ban(hist[tid + n - 1]);
    }
    if (tid >= 64 && tid < 64 + c.n_sup) ban(c.sup[tid - 64]);
    if (tid == 128 && c.repeat_word && t >= 1) ban(hist[t - 1]);
    if (tid == 129 && c.eos_word >= 0) ban(c.eos_word);
}

template <int KL, class Src>  // per-thread list length: k <= KL <= kMaxK (5 for the usual beam of 5: 40 % fewer compare-swaps per insertion)
__global__ __launch_bounds__(kBeamThreads)
void beam_partial(Src logp, long ld, const float* __restrict__ seq_lp, const float* __restrict__ seq_mask,
                  const int64_t* __restrict__ prev_words, int eos, int first_step, int cur, int V, int k, int parts,
                  float* __restrict__ ws_val, int* __restrict__ ws_idx) {
    __shared__ float sv[2][kBeamThreads / 64];
    __shared__ int si[2][kBeamThreads / 64];
    __shared__ int so[2][kBeamThreads / 64];
    const int part = blockIdx.x, j = blockIdx.y, b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int row_id = b * cur + j;
    const float base = seq_lp[row_id];
    bool alive = true;
    if (!first_step) alive = (seq_mask[row_id] * (prev_words[row_id] != (int64_t)eos ? 1.f : 0.f)) != 0.f;
    const size_t row = (size_t)row_id * ld;
    const int seg = ((V + parts - 1) / parts + 3) & ~3;
    const int v0 = part * seg, v1 = min(V, v0 + seg);
    float bv[KL];
    int bi[KL];
#pragma unroll
    for (int q = 0; q < KL; ++q) { bv[q] = -INFINITY; bi[q] = 0x7fffffff; }
    auto push = [&](float v, int i) {
        if (!better(v, i, bv[KL - 1], bi[KL - 1])) return;
        bv[KL - 1] = v; bi[KL - 1] = i;
#pragma unroll
        for (int q = KL - 1; q > 0; --q)
            if (better(bv[q], bi[q], bv[q - 1], bi[q - 1])) {
                const float tv = bv[q]; bv[q] = bv[q - 1]; bv[q - 1] = tv;
                const int ti = bi[q]; bi[q] = bi[q - 1]; bi[q - 1] = ti;
            }
    };
    const int flat0 = j * V;
    if constexpr (Src::kBans) {
        // a live beam under constraints: the slice's banned words score -inf and stay candidates with their own index (a finished
        // beam has no bans and takes the branch below)
        __shared__ int64_t hist[kMaxHistory];
        __shared__ unsigned bits[kMaxSlice / 32];
        if (alive && v0 < v1) {  // uniform over the workgroup
            mark_bans(logp.bans, row_id, v0, v1, hist, bits);
            if constexpr (Src::kForced) {  // a row that still owes a forced word may not end
                if (tid == 130 && eos >= v0 && eos < v1 && met_of_row(logp.forced, b, row_id) != (1 << logp.forced.C) - 1)
                    atomicOr(&bits[(eos - v0) >> 5], 1u << ((eos - v0) & 31));  // LDS
            }
            __syncthreads();
            auto score = [&](float x, unsigned banned) { return banned ? -INFINITY : base + x; };
            if (logp.aligned16(row + v0)) {
                const int n4 = (v1 - v0) >> 2;
                for (int i = tid; i < n4; i += kBeamThreads) {
                    const float4 t = logp.at4(row + v0 + 4 * i);
                    const int e = flat0 + v0 + 4 * i;
                    const unsigned m = bits[(4 * i) >> 5] >> ((4 * i) & 31);  // four neighbours share a bitmap word
                    push(score(t.x, m & 1u), e); push(score(t.y, m & 2u), e + 1);
                    push(score(t.z, m & 4u), e + 2); push(score(t.w, m & 8u), e + 3);
                }
                for (int v = v0 + 4 * n4 + tid; v < v1; v += kBeamThreads)
                    push(score(logp.at(row + v), (bits[(v - v0) >> 5] >> ((v - v0) & 31)) & 1u), flat0 + v);
            } else {
                for (int v = v0 + tid; v < v1; v += kBeamThreads)
                    push(score(logp.at(row + v), (bits[(v - v0) >> 5] >> ((v - v0) & 31)) & 1u), flat0 + v);
            }
        }
    }
    if (alive && !Src::kBans) {
        const bool vec = logp.aligned16(row + v0);
        if (vec) {
            const int n4 = (v1 - v0) >> 2;
            for (int i = tid; i < n4; i += kBeamThreads) {
                const float4 t = logp.at4(row + v0 + 4 * i);
                const int e = flat0 + v0 + 4 * i;
                push(base + t.x, e); push(base + t.y, e + 1); push(base + t.z, e + 2); push(base + t.w, e + 3);
            }
            for (int v = v0 + 4 * n4 + tid; v < v1; v += kBeamThreads) push(base + logp.at(row + v), flat0 + v);
        } else {
            for (int v = v0 + tid; v < v1; v += kBeamThreads) push(base + logp.at(row + v), flat0 + v);
        }
    } else if (!alive) {
        // a finished beam survives only through vocabulary index 0; the other entries all score -999 (ties by index)
        const int v = v0 + tid;  // the k <= 8 best of the slice are among its first entries
        if (v < v1) push(v == 0 ? base : -999.f, flat0 + v);
    }
    // merge the 256 sorted lists: k rounds of (wave arg-max over the list heads, then the best of the 4 waves)
    int headp = 0;
    const int out = ((b * cur + j) * parts + part) * kMaxK;
    for (int r = 0; r < k; ++r) {
        float v = -INFINITY; int i = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < KL; ++q)
            if (q == headp) { v = bv[q]; i = bi[q]; }
        int o = tid;
        wave_best(v, i, o);
        const int buf = r & 1;
        if (lane == 0) { sv[buf][w] = v; si[buf][w] = i; so[buf][w] = o; }
        __syncthreads();
        float gv = sv[buf][0]; int gi = si[buf][0], go = so[buf][0];
#pragma unroll
        for (int q = 1; q < kBeamThreads / 64; ++q)
            if (better(sv[buf][q], si[buf][q], gv, gi)) { gv = sv[buf][q]; gi = si[buf][q]; go = so[buf][q]; }
        if (tid == 0) { ws_val[out + r] = gv; ws_idx[out + r] = gi; }
        if (tid == go) ++headp;
    }
}

template <class Src>
__global__ __launch_bounds__(64)
void beam_merge(Src logp, long ld, const float* __restrict__ seq_mask, const int64_t* __restrict__ prev_words,
                int eos, int first_step, int cur, int V, int k, int parts, const float* __restrict__ ws_val,
                const int* __restrict__ ws_idx, int64_t* __restrict__ sel_beam, int64_t* __restrict__ sel_word,
                float* __restrict__ new_lp, float* __restrict__ new_mask, float* __restrict__ picked) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int groups = cur * parts, n = groups * k;  // <= 128 candidates, two per lane
    float v[2]; int i[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = lane + 64 * h;
        v[h] = -INFINITY; i[h] = 0x7fffffff;
        if (c < n) {
            const int g = c / k, r = c - g * k;
            v[h] = ws_val[((size_t)b * groups + g) * kMaxK + r];
            i[h] = ws_idx[((size_t)b * groups + g) * kMaxK + r];
        }
    }
    for (int r = 0; r < k; ++r) {
        const int h = better(v[1], i[1], v[0], i[0]) ? 1 : 0;
        float bvv = v[h]; int bii = i[h], o = lane * 2 + h;
        wave_best(bvv, bii, o);
        if (o == lane * 2) { v[0] = -INFINITY; i[0] = 0x7fffffff; }
        if (o == lane * 2 + 1) { v[1] = -INFINITY; i[1] = 0x7fffffff; }
        if (lane == 0) {
            const int jb = bii / V, word = bii - jb * V;
            const int row_id = b * cur + jb;
            float alive = 1.f;
            if (!first_step) alive = seq_mask[row_id] * (prev_words[row_id] != (int64_t)eos ? 1.f : 0.f);
            const size_t at = (size_t)b * k + r;
            sel_beam[at] = jb; sel_word[at] = word;
            new_lp[at] = bvv; new_mask[at] = alive;
            picked[at] = logp.at((size_t)row_id * ld + word) * alive;
        }
    }
}

// Stage 2 of the diverse step (grit_beam_step_div_f32): the groups of a step are resolved one after the other on the <= 128
// candidates that stage 1 left, one wave per image.  A group pays `diversity` per earlier selection of the same word in this step,
// and the penalty only lowers candidates -- in one source row at most |P| <= k - g of them, P being the words picked so far -- so
// the g best penalised candidates of a row are among its k best unpenalised ones, which is what stage 1 kept (ties included: a
// candidate outside them has k better ones, of which g stay unpenalised and so stay better).  Only the candidates that the penalty
// touches (word in P, live row, finite score) are scored again, from the source and the running score, so the mean of an ensemble
// is formed as in stage 1; all the others keep stage 1's value, which is the penalised one for a count of 0.  The picks of the
// step sit in registers at their output position (-1: picked from a finished row, which counts nothing).
template <class Src>
__global__ __launch_bounds__(64)
void beam_merge_groups(Src logp, long ld, const float* __restrict__ seq_lp, const float* __restrict__ seq_mask,
                       const int64_t* __restrict__ prev_words, int eos, int first_step, int cur, int V, int k, int parts, int G,
                       float diversity, const float* __restrict__ ws_val, const int* __restrict__ ws_idx,
                       int64_t* __restrict__ sel_beam, int64_t* __restrict__ sel_word, float* __restrict__ new_lp,
                       float* __restrict__ new_mask, float* __restrict__ picked) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int lists = cur * parts, n = lists * k, g = k / G;  // <= 128 candidates, two per lane
    constexpr int kNone = 0x7fffffff;
    auto alive_of = [&](int row_id) {
        return first_step ? 1.f : seq_mask[row_id] * (prev_words[row_id] != (int64_t)eos ? 1.f : 0.f);
    };
    float v[2]; int i[2], row[2], word[2]; bool live[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int c = lane + 64 * h;
        v[h] = -INFINITY; i[h] = kNone; row[h] = -1; word[h] = -1; live[h] = false;
        if (c < n) {
            const int l = c / k, r = c - l * k;
            v[h] = ws_val[((size_t)b * lists + l) * kMaxK + r];
            i[h] = ws_idx[((size_t)b * lists + l) * kMaxK + r];
            if (i[h] != kNone) {  // a slice shorter than k leaves empty entries
                row[h] = i[h] / V; word[h] = i[h] - row[h] * V;
                live[h] = alive_of(b * cur + row[h]) != 0.f;
            }
        }
    }
    int pw[kMaxK];
#pragma unroll
    for (int q = 0; q < kMaxK; ++q) pw[q] = -1;
    for (int grp = 0; grp < G; ++grp) {
        const int done = grp * g;                                // the picks of the earlier groups
        const int r0 = cur == 1 ? 0 : done, r1 = cur == 1 ? 1 : done + g;  // this group's source rows
        float pv[2]; int pi[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const bool mine = row[h] >= r0 && row[h] < r1;
            pv[h] = mine ? v[h] : -INFINITY; pi[h] = mine ? i[h] : kNone;
            if (mine && live[h]) {
                int count = 0;
#pragma unroll
                for (int q = 0; q < kMaxK; ++q) count += (q < done && pw[q] == word[h]) ? 1 : 0;
                if (count > 0 && v[h] > -INFINITY && v[h] < INFINITY) {
                    const size_t row_id = (size_t)(b * cur + row[h]);
                    pv[h] = __fadd_rn(seq_lp[row_id], __fsub_rn(logp.at(row_id * ld + word[h]), __fmul_rn(diversity, (float)count)));
                }
            }
        }
        for (int r = 0; r < g; ++r) {
            const bool second = better(pv[1], pi[1], pv[0], pi[0]);
            float bvv = second ? pv[1] : pv[0]; int bii = second ? pi[1] : pi[0], o = lane * 2 + (second ? 1 : 0);
            wave_best(bvv, bii, o);
            if (o == lane * 2) { pv[0] = -INFINITY; pi[0] = kNone; }
            if (o == lane * 2 + 1) { pv[1] = -INFINITY; pi[1] = kNone; }
            int jb = r0, w = 0;  // (fewer than g candidates cannot happen with V >= k; never index with an empty entry)
            if (bii != kNone) { jb = bii / V; w = bii - jb * V; }
            const int row_id = b * cur + jb;
            const float alive = alive_of(row_id);
            const int pos = done + r;
#pragma unroll
            for (int q = 0; q < kMaxK; ++q)
                if (q == pos) pw[q] = alive != 0.f ? w : -1;
            if (lane == 0) {
                const size_t at = (size_t)b * k + pos;
                sel_beam[at] = jb; sel_word[at] = w;
                new_lp[at] = bvv; new_mask[at] = alive;
                picked[at] = logp.at((size_t)row_id * ld + w) * alive;
            }
        }
    }
}

// Stage 2 of the step with forced words (grit_beam_step_forced_f32): one workgroup per image, every candidate of the image in LDS.
// Row j owns the slots [j * per, (j + 1) * per), per = k + C * W: first its k best candidates out of stage 1's lists (a finished
// row: its word-0 candidate alone), then one slot per forced word.  A thread per history position finds the n-gram continuations
// of a row as mark_bans does; a thread per slot then tests its forced word against them and the fixed rules, drops the word when an
// earlier slot of the row holds it already, and banks the candidate.  The round-robin over the banks is a sort by (rank inside
// the bank, bank descending): both are counted, a thread per candidate, and the k first store the outputs at their position.  The
// counting loops compare one integer per candidate (the order of `better` as a 64-bit key; rank and bank as one int), so that
// their LDS reads do not wait for one another.
constexpr int kMaxForcedCand = kMaxK * (kMaxK + kMaxSets * kMaxWords);  // 320

template <class Src>
__global__ __launch_bounds__(kBeamThreads)
void beam_forced_select(Src logp, long ld, Bans bans, ForcedSets f, const float* __restrict__ seq_lp,
                        const float* __restrict__ seq_mask, const int64_t* __restrict__ prev_words, int eos, int first_step, int cur,
                        int V, int k, int parts, const float* __restrict__ ws_val, const int* __restrict__ ws_idx,
                        int64_t* __restrict__ sel_beam, int64_t* __restrict__ sel_word, float* __restrict__ new_lp,
                        float* __restrict__ new_mask, float* __restrict__ picked, int* __restrict__ new_met) {
    constexpr int kNone = 0x7fffffff, kInvalid = -2;
    __shared__ float c_score[kMaxForcedCand];
    __shared__ int c_key[kMaxForcedCand], c_met[kMaxForcedCand], c_bank[kMaxForcedCand], c_slot[kMaxForcedCand];
    __shared__ uint64_t c_ord[kMaxForcedCand];
    __shared__ unsigned char c_valid[kMaxForcedCand];
    __shared__ int64_t s_fw[kMaxSets * kMaxWords];
    __shared__ int64_t s_hist[kMaxK][kMaxHistory], s_next[kMaxK][kMaxHistory];
    __shared__ float s_alive[kMaxK], s_base[kMaxK];
    __shared__ int s_met[kMaxK];
    __shared__ float w_val[128];
    __shared__ int w_idx[128];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int CW = f.C * f.W, per = k + CW, N = cur * per, full = (1 << f.C) - 1;
    const int t = bans.t, n = bans.ngram, lists = parts * k, n_ws = cur * lists;  // n_ws <= 128

    if (tid < CW) s_fw[tid] = f.words[(size_t)b * CW + tid];
    if (tid >= 64 && tid < 64 + cur) {
        const int j = tid - 64, row_id = b * cur + j;
        s_alive[j] = first_step ? 1.f : seq_mask[row_id] * (prev_words[row_id] != (int64_t)eos ? 1.f : 0.f);
        s_base[j] = seq_lp[row_id];
        s_met[j] = met_of_row(f, b, row_id);
    }
    for (int e = tid; e < n_ws; e += kBeamThreads) {  // entry r of list l of row j
        const int l = e / k, r = e - l * k;
        w_val[e] = ws_val[((size_t)b * cur * parts + l) * kMaxK + r];
        w_idx[e] = ws_idx[((size_t)b * cur * parts + l) * kMaxK + r];
    }
    for (int e = tid; e < cur * t; e += kBeamThreads) {
        const int j = e / t, p = e - j * t;
        s_hist[j][p] = bans.hist[(size_t)(b * cur + j) * bans.hist_ld + p];
    }
    for (int c = tid; c < N; c += kBeamThreads) { c_valid[c] = 0; c_bank[c] = kInvalid; }
    __syncthreads();

    // the word that each history position bans by the n-gram rule (-1: none)
    for (int e = tid; e < cur * t; e += kBeamThreads) {
        const int j = e / t, p = e - j * t;
        int64_t next = -1;
        if (n >= 1 && p <= t - n) {
            bool same = true;
            for (int q = 0; q < n - 1; ++q) same = same && s_hist[j][p + q] == s_hist[j][t - n + 1 + q];
            if (same) next = s_hist[j][p + n - 1];
        }
        s_next[j][p] = next;
    }
    // A: the k best of a live row among the entries that stage 1 left for it, each at the slot of its rank
    for (int e = tid; e < n_ws; e += kBeamThreads) {
        const int j = e / lists;
        if (s_alive[j] == 0.f || w_idx[e] == kNone) continue;
        int rank = 0;
        for (int o = j * lists; o < (j + 1) * lists; ++o) rank += better(w_val[o], w_idx[o], w_val[e], w_idx[e]) ? 1 : 0;
        if (rank < k) {
            const int c = j * per + rank;
            c_score[c] = w_val[e]; c_key[c] = w_idx[e]; c_valid[c] = 1;
        }
    }
    __syncthreads();
    // A of a finished row, and F: the forced words that the row may still choose
    for (int c = tid; c < N; c += kBeamThreads) {
        const int j = c / per, q = c - j * per;
        const bool live = s_alive[j] != 0.f;
        if (q < k) {
            if (!live && q == 0) { c_score[c] = s_base[j]; c_key[c] = j * V; c_valid[c] = 1; }
            continue;
        }
        const int64_t w = s_fw[q - k];
        const int set = (q - k) / f.W;
        if (!live || w < 0 || w >= V || ((s_met[j] >> set) & 1)) continue;
        bool banned = w == eos && (bans.eos_word >= 0 || s_met[j] != full);
        for (int i = 0; i < bans.n_sup; ++i) banned = banned || w == bans.sup[i];
        if (bans.repeat_word && t >= 1) banned = banned || w == s_hist[j][t - 1];
        for (int p = 0; p < t; ++p) banned = banned || w == s_next[j][p];
        if (banned) continue;
        c_score[c] = s_base[j] + logp.at((size_t)(b * cur + j) * ld + (int)w);
        c_key[c] = j * V + (int)w;
        c_valid[c] = 1;
    }
    __syncthreads();
    // one candidate per (row, word); the sets that the word hits; the bank
    for (int c = tid; c < N; c += kBeamThreads) {
        if (!c_valid[c]) continue;
        const int j = c / per, q = c - j * per;
        bool dup = false;
        if (q >= k)
            for (int o = j * per; o < c; ++o) dup = dup || (c_valid[o] && c_key[o] == c_key[c]);
        if (dup) continue;
        int met = s_met[j];
        if (s_alive[j] != 0.f) {
            const int64_t w = c_key[c] - j * V;
            for (int i = 0; i < CW; ++i)
                if (s_fw[i] == w) met |= 1 << (i / f.W);
        }
        c_met[c] = met;
        c_bank[c] = c_score[c] == -INFINITY ? -1 : __popc((unsigned)met);
        // smaller = earlier under `better`: NaN above every number, value descending (-0 == +0), then the key ascending
        const float v = c_score[c];
        const unsigned bits = __float_as_uint(v == 0.f ? 0.f : v);
        const unsigned descending = v != v ? 0u : ~((bits & 0x80000000u) ? ~bits : (bits | 0x80000000u));
        c_ord[c] = ((uint64_t)descending << 32) | (unsigned)c_key[c];
    }
    __syncthreads();
    for (int c = tid; c < N; c += kBeamThreads) {
        const int bank = c_bank[c];
        int slot = kNone;
        if (bank != kInvalid) {
            const uint64_t mine = c_ord[c];
            int rank = 0;
#pragma unroll 8
            for (int o = 0; o < N; ++o) rank += (c_bank[o] == bank && c_ord[o] < mine) ? 1 : 0;
            slot = (rank << 4) | (kMaxSets - bank);  // round by round, inside a round the high banks first
        }
        c_slot[c] = slot;
    }
    __syncthreads();
    for (int c = tid; c < N; c += kBeamThreads) {
        const int slot = c_slot[c];
        if (slot == kNone) continue;
        int pos = 0;
#pragma unroll 8
        for (int o = 0; o < N; ++o) pos += c_slot[o] < slot ? 1 : 0;
        if (pos >= k) continue;
        const int jb = c_key[c] / V, word = c_key[c] - jb * V;
        const int row_id = b * cur + jb;
        const size_t at = (size_t)b * k + pos;
        sel_beam[at] = jb; sel_word[at] = word;
        new_lp[at] = c_score[c]; new_mask[at] = s_alive[jb];
        picked[at] = logp.at((size_t)row_id * ld + word) * s_alive[jb];
        new_met[at] = c_met[c];
    }
}

}  // namespace

namespace {

// Stage 1 cuts the vocabulary of every beam row into this many slices, a workgroup each.
constexpr int beam_parts(int cur_beam) { return cur_beam == 1 ? 8 : 2; }

}  // namespace

extern "C" long grit_beam_step_workspace(int B, int cur_beam, int k) {
    if (B <= 0 || cur_beam <= 0 || k <= 0) return 0;
    return (long)B * cur_beam * beam_parts(cur_beam) * kMaxK * 8;
}

namespace {

// Stage 1 applies the bans when a rule is set; without one, t and history are not read.  A step with forced words always carries
// them: its stage 2 tests the forced words against the rules.
bool with_bans(const grit_beam_step_args& a) {
    return a.force_words || a.no_repeat_ngram > 0 || a.no_repeat_word || a.ban_eos || a.n_suppress > 0;
}

// GRIT_OK when the step can be launched; the order of the refusals is the one that include/grit_hip.h states.
int beam_check(const grit_beam_step_args& a) {
    const bool bans = with_bans(a), forced = a.force_words != nullptr, grouped = a.groups > 0;
    if (!a.maps || a.n_maps <= 0 || a.B <= 0 || a.cur_beam <= 0 || a.V <= 0 || a.k <= 0 || a.no_repeat_ngram < 0 ||
        a.n_suppress < 0 || a.groups < 0)
        return GRIT_ERR_BAD_ARG;
    if (bans && (a.t < 0 || (a.n_suppress > 0 && !a.suppress) || (a.t > 0 && (!a.history || a.history_ld < a.t)) ||
                 (a.ban_eos && (a.eos < 0 || a.eos >= a.V))))
        return GRIT_ERR_BAD_ARG;
    if (forced && (grouped || a.n_sets < 1 || a.n_words < 1 || !a.new_met)) return GRIT_ERR_BAD_ARG;
    // the limits of the source, the bans, the groups and the forced words
    if (a.n_maps > kMaxMaps || (bans && (a.t > kMaxHistory || a.n_suppress > kMaxSuppress)) ||
        ((grouped || forced) && (a.k > kMaxK || (a.cur_beam != 1 && a.cur_beam != a.k) || a.V < a.k)) ||
        (grouped && (a.k % a.groups != 0 || !(a.diversity >= 0.f && a.diversity < INFINITY))) ||
        (forced && (a.n_sets > kMaxSets || a.n_words > kMaxWords)))
        return GRIT_ERR_UNSUPPORTED;
    if (!a.seq_logprob || !a.workspace || !a.sel_beam || !a.sel_word || !a.new_seq_logprob || !a.new_seq_mask || !a.picked_logprob ||
        a.ld < a.V || (!a.first_step && (!a.seq_mask || !a.prev_words)))
        return GRIT_ERR_BAD_ARG;
    for (int m = 0; m < a.n_maps; ++m)
        if (!a.maps[m]) return GRIT_ERR_BAD_ARG;
    for (int i = 0; bans && i < a.n_suppress; ++i)
        if (a.suppress[i] < 0 || a.suppress[i] >= a.V) return GRIT_ERR_BAD_ARG;
    // the limits of the plain step, and the ban bitmap of a slice
    const int parts = beam_parts(a.cur_beam);
    if (a.k > kMaxK || (long)a.k > (long)a.cur_beam * a.V || a.cur_beam * parts * a.k > 128 || (long)a.cur_beam * a.V > 0x7fffffffL ||
        a.B > 65535 || (bans && (((a.V + parts - 1) / parts + 3) & ~3) > kMaxSlice))
        return GRIT_ERR_UNSUPPORTED;
    return a.workspace_bytes < grit_beam_step_workspace(a.B, a.cur_beam, a.k) ? GRIT_ERR_BAD_ARG : GRIT_OK;
}

Bans beam_bans(const grit_beam_step_args& a) {
    Bans bans{};
    bans.hist = a.history; bans.hist_ld = a.history_ld; bans.t = a.t;
    bans.ngram = a.no_repeat_ngram; bans.repeat_word = a.no_repeat_word != 0; bans.eos_word = a.ban_eos ? a.eos : -1;
    bans.n_sup = a.n_suppress;
    for (int i = 0; i < a.n_suppress; ++i) bans.sup[i] = a.suppress[i];
    return bans;
}

MeanMaps beam_mean(const grit_beam_step_args& a) {
    MeanMaps src{};
    for (int m = 0; m < a.n_maps; ++m) src.t.p[m] = a.maps[m];
    src.n = a.n_maps;
    // torch: static_cast<float>(iter.num_output_elements()) / iter.numel() -- float(N) / float(K * N), not 1 / K (they differ once
    // K * N is no longer exact in float)
    const long outputs = (long)a.B * a.cur_beam * a.V;
    src.factor = (float)outputs / (float)(outputs * a.n_maps);
    return src;
}

struct Lists { int parts; float* val; int* idx; };  // what stage 1 leaves in the workspace for stage 2

template <class Part>  // Part: what stage 1 reads, the source itself, Banned<Src> or Forced<Src>
Lists beam_stage1(const Part& part, const grit_beam_step_args& a, hipStream_t stream) {
    const int parts = beam_parts(a.cur_beam);
    float* ws_val = reinterpret_cast<float*>(a.workspace);
    int* ws_idx = reinterpret_cast<int*>(ws_val + (size_t)a.B * a.cur_beam * parts * kMaxK);
    const auto kernel = a.k <= 5 ? beam_partial<5, Part> : beam_partial<kMaxK, Part>;
    hipLaunchKernelGGL(kernel, dim3(parts, a.cur_beam, a.B), dim3(kBeamThreads), 0, stream, part, a.ld, a.seq_logprob, a.seq_mask,
                       a.prev_words, a.eos, a.first_step, a.cur_beam, a.V, a.k, parts, ws_val, ws_idx);
    return {parts, ws_val, ws_idx};
}

// The two launches of a step whose stage 1 reads Part = Src (plain), Banned<Src> or Forced<Src>; stage 2 reads the plain source.
template <class Part, class Src>
int beam_step(const Src& src, const grit_beam_step_args& a, hipStream_t stream) {
    Part part;
    static_cast<Src&>(part) = src;
    if constexpr (Part::kBans) part.bans = beam_bans(a);
    if constexpr (Part::kForced) part.forced = ForcedSets{a.force_words, a.met_in, a.n_sets, a.n_words};
    const Lists l = beam_stage1(part, a, stream);
    if constexpr (Part::kForced)
        hipLaunchKernelGGL(beam_forced_select<Src>, dim3(a.B), dim3(kBeamThreads), 0, stream, src, a.ld, part.bans, part.forced,
                           a.seq_logprob, a.seq_mask, a.prev_words, a.eos, a.first_step, a.cur_beam, a.V, a.k, l.parts, l.val, l.idx,
                           a.sel_beam, a.sel_word, a.new_seq_logprob, a.new_seq_mask, a.picked_logprob, a.new_met);
    else if (a.groups > 0)
        hipLaunchKernelGGL(beam_merge_groups<Src>, dim3(a.B), dim3(64), 0, stream, src, a.ld, a.seq_logprob, a.seq_mask, a.prev_words,
                           a.eos, a.first_step, a.cur_beam, a.V, a.k, l.parts, a.groups, a.diversity, l.val, l.idx, a.sel_beam, a.sel_word,
                           a.new_seq_logprob, a.new_seq_mask, a.picked_logprob);
    else
        hipLaunchKernelGGL(beam_merge<Src>, dim3(a.B), dim3(64), 0, stream, src, a.ld, a.seq_mask, a.prev_words, a.eos, a.first_step,
                           a.cur_beam, a.V, a.k, l.parts, l.val, l.idx, a.sel_beam, a.sel_word, a.new_seq_logprob, a.new_seq_mask,
                           a.picked_logprob);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

}  // namespace

extern "C" int grit_beam_step(const grit_beam_step_args* args, void* stream) {
    if (!args) return GRIT_ERR_BAD_ARG;
    const grit_beam_step_args& a = *args;
    const int status = beam_check(a);
    if (status != GRIT_OK) return status;
    hipStream_t s = (hipStream_t)stream;
    const bool one = a.n_maps == 1;
    const OneMap map{a.maps[0]};
    const MeanMaps mean = beam_mean(a);
    if (!with_bans(a)) return one ? beam_step<OneMap>(map, a, s) : beam_step<MeanMaps>(mean, a, s);
    if (!a.force_words) return one ? beam_step<Banned<OneMap>>(map, a, s) : beam_step<Banned<MeanMaps>>(mean, a, s);
    return one ? beam_step<Forced<OneMap>>(map, a, s) : beam_step<Forced<MeanMaps>>(mean, a, s);
}


extern "C" int grit_topk_rows_f32(const float* x, long ld, int rows, int n, int k, int64_t* idx_out, float* val_out, void* stream) {
    if (!x || !idx_out || !val_out || rows <= 0 || n <= 0 || k <= 0) return GRIT_ERR_BAD_ARG;
    if (k > kMaxK || k > n) return GRIT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(topk_rows, dim3(rows), dim3(kThreads), 0, (hipStream_t)stream, x, ld, n, k, idx_out, val_out);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}
