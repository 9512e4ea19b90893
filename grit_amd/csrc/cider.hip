// CIDEr-D reward of self-critical training on the device: generated token ids in, one score per hypothesis row out, one launch,
// no host involvement.
//
// Stands for davidnvq/grit engine/caption_engine.py:433-438 (text_field.decode -> PTBTokenizer.tokenize -> cider.compute_score)
// and datasets/caption/metrics/cider/cider_scorer.py (counts2vec / sim / compute_cider), in the arrangement of this build's
// datasets/caption/metrics/cider.py (_Vec, Cider._similarity, Cider.compute_score).  Everything that does not depend on the
// hypothesis is packed once on the host (grit_amd/ops/cider.py): the per-word expansion of the tokenizer, the corpus idf as a
// trie flattened into sorted arrays, and the cooked tf-idf vectors of every image's references.
//
// One workgroup per hypothesis row, float64 throughout.  Every sum runs sequentially in the order the host's dictionaries are
// walked (n-grams by first occurrence, orders 1..4, references in list order), with no fused multiply-add and no atomics, so a
// row's result does not depend on the launch and differs from the host's only where libm differs (exp, sqrt).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/grit_hip.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTok = GRIT_CIDER_MAX_TOKENS;  // expanded tokens of one row: one thread per position
constexpr int kMaxT = GRIT_CIDER_MAX_TOKENS;    // words of one row
constexpr int kOrders = 4;

struct Tuple { int t[kOrders]; };

// position of `key` in keys[lo, hi) (sorted, unique), or -1
__device__ __forceinline__ long find_key(const uint64_t* __restrict__ keys, long lo, long hi, uint64_t key) {
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        const uint64_t k = keys[mid];
        if (k == key) return mid;
        if (k < key) lo = mid + 1; else hi = mid;
    }
    return -1;
}

__global__ __launch_bounds__(kThreads)
void cider_reward(const int64_t* __restrict__ tokens, int T, const int32_t* __restrict__ slots, int beam, grit_cider_tables tab,
                  float* __restrict__ out32, double* __restrict__ out64) {
    __shared__ int s_word[kMaxT];              // word id, or -1 at and after the cut
    __shared__ int s_meta[kMaxT];
    __shared__ int s_tok[kMaxTok + kOrders];   // expanded tokens, -1 behind the end
    __shared__ double s_w[kOrders][kMaxTok];   // tf * idf at the first occurrence of an n-gram, 0 elsewhere
    __shared__ double s_term[kOrders][kMaxTok];
    __shared__ double s_norm[kOrders];
    __shared__ double s_val[kOrders];

    const int tid = threadIdx.x;
    const int row = blockIdx.x;
    const int64_t* trow = tokens + (size_t)row * T;

    // ---- 1. words up to the first EOS, their expansion -------------------------------------------------------------------
    if (tid < T) {
        const int64_t w = trow[tid];
        const bool known = w >= 0 && w < tab.vocab;  // an id outside the vocabulary is reported below, not looked up
        s_word[tid] = known ? (int)w : -1;
        s_meta[tid] = known ? tab.word_meta[w] : 0;
    }
    const int slot = slots[row / beam];
    __syncthreads();
    int cut = T;
    for (int t = T - 1; t >= 0; --t)
        if (s_meta[t] & GRIT_CIDER_META_EOS) cut = t;
    // an id outside the vocabulary BEFORE the cut (the host would raise), or an unknown slot: NaN, never a wrong number
    bool bad = slot < 0 || slot >= tab.n_slots;
    for (int t = 0; t < cut; ++t) bad = bad || s_word[t] < 0;
    if (bad) {
        if (tid == 0) {
            out32[row] = __builtin_nanf("");
            if (out64) out64[row] = __builtin_nan("");
        }
        return;
    }
    int last = -1;  // the last word that is not whitespace-only: it alone is tokenised as the end of the sentence
    for (int t = 0; t < cut; ++t)
        if (!(s_meta[t] & GRIT_CIDER_META_BLANK)) last = t;
    int offset = 0, L = 0;
    for (int t = 0; t < cut; ++t) {
        const int m = s_meta[t];
        const int c = min(t == last ? (m >> GRIT_CIDER_META_FIN_SHIFT) & 15 : m & 15, tab.width);
        if (t < tid) offset += c;
        L += c;
    }
    if (tid < cut) {
        const int m = s_meta[tid];
        const bool fin = tid == last;
        const int c = min(fin ? (m >> GRIT_CIDER_META_FIN_SHIFT) & 15 : m & 15, tab.width);
        const int32_t* e = tab.expansion + ((size_t)s_word[tid] * 2 + (fin ? 1 : 0)) * tab.width;
        for (int j = 0; j < c; ++j) s_tok[offset + j] = e[j];
    }
    if (tid < kOrders) s_tok[L + tid] = -1;
    __syncthreads();

    // ---- 2. + 3. term frequency at the first occurrence, idf chained by order, weight ------------------------------------
    if (tid < L) {
        Tuple me;
#pragma unroll
        for (int k = 0; k < kOrders; ++k) me.t[k] = s_tok[tid + k];
        int tf[kOrders] = {0, 0, 0, 0};
        bool first[kOrders] = {true, true, true, true};
        for (int j = 0; j < L; ++j) {
            bool same = true;
#pragma unroll
            for (int k = 0; k < kOrders; ++k) {
                same = same && s_tok[j + k] == me.t[k];
                if (same && j + k < L) {  // (a tuple that runs behind the end compares -1 == -1: excluded by the bound)
                    ++tf[k];
                    if (j < tid) first[k] = false;
                }
            }
        }
        long node = 0;
#pragma unroll
        for (int k = 0; k < kOrders; ++k) {
            double w = 0.0;
            if (tid + k < L) {
                if (node >= 0) {
                    const long at = find_key(tab.idf_key, tab.idf_start[k], tab.idf_start[k + 1],
                                             ((uint64_t)node << 32) | (uint32_t)me.t[k]);
                    node = at < 0 ? -1 : at - tab.idf_start[k];
                    if (at >= 0 && first[k]) w = (double)tf[k] * tab.idf_val[at];
                }
                if (node < 0 && first[k]) w = (double)tf[k] * tab.log_corpus;  // unseen: document frequency 1
            }
            s_w[k][tid] = w;
        }
    }
    __syncthreads();
    if (tid < kOrders) {
        double sq = 0.0;
        for (int i = 0; i + tid < L; ++i) {
            const double w = s_w[tid][i];
            sq += w * w;
        }
        s_norm[tid] = sqrt(sq);
    }
    __syncthreads();

    // ---- 4. clipped similarity against every reference of the image ------------------------------------------------------
    const int r0 = tab.slot_ref_start[slot], r1 = tab.slot_ref_start[slot + 1];
    const int len_h = L > 0 ? L - 1 : 0;  // sentence length in bigram occurrences
    double total = 0.0;                   // thread 0 only
    for (int r = r0; r < r1; ++r) {
        for (int item = tid; item < kOrders * L; item += kThreads) {
            const int k = item / L, i = item - k * L;
            double term = 0.0;
            const double wh = s_w[k][i];
            if (i + k < L && wh != 0.0) {
                const int e0 = tab.ref_ent_start[r * kOrders + k], e1 = tab.ref_ent_start[r * kOrders + k + 1];
                const int a = s_tok[i], b = k > 0 ? s_tok[i + 1] : -1, c = k > 1 ? s_tok[i + 2] : -1, d = k > 2 ? s_tok[i + 3] : -1;
                for (int e = e0; e < e1; ++e) {
                    const int4 q = static_cast<const int4*>(tab.ent_tok)[e];
                    if (q.x == a && q.y == b && q.z == c && q.w == d) {
                        const double wr = tab.ent_w[e];
                        term = (wh < wr ? wh : wr) * wr;
                    }
                }
            }
            s_term[k][i] = term;
        }
        __syncthreads();
        if (tid < kOrders) {
            double val = 0.0;
            for (int i = 0; i + tid < L; ++i) val += s_term[tid][i];
            const double nr = tab.ref_norm[(size_t)r * kOrders + tid];
            if (s_norm[tid] != 0.0 && nr != 0.0) val /= s_norm[tid] * nr;
            s_val[tid] = val;
        }
        __syncthreads();
        if (tid == 0) {
            const double delta = (double)(len_h - tab.ref_len[r]);
            const double penalty = exp(-(delta * delta) / (2.0 * (tab.sigma * tab.sigma)));
            double sim = 0.0;
            for (int k = 0; k < kOrders; ++k) sim += s_val[k] * penalty;
            total += sim / (double)kOrders;
        }
        // s_term / s_val of the next reference are written only after the barrier that follows its matching loop
    }
    if (tid == 0) {
        const double score = r1 > r0 ? total / (double)(r1 - r0) * 10.0 : 0.0;
        out32[row] = (float)score;
        if (out64) out64[row] = score;
    }
}

}  // namespace

extern "C" int grit_cider_reward(const int64_t* tokens, int rows, int T, const int32_t* slots, int beam,
                                 const grit_cider_tables* tab, float* out32, double* out64, void* stream) {
    if (!tokens || !slots || !tab || !out32 || rows <= 0 || T <= 0 || beam <= 0 || rows % beam != 0) return GRIT_ERR_BAD_ARG;
    if (!tab->expansion || !tab->word_meta || !tab->idf_key || !tab->idf_val || !tab->slot_ref_start || !tab->ref_ent_start ||
        !tab->ent_tok || !tab->ent_w || !tab->ref_norm || !tab->ref_len || tab->vocab <= 0 || tab->n_slots <= 0 ||
        tab->width <= 0 || !(tab->sigma > 0.0))
        return GRIT_ERR_BAD_ARG;
    for (int k = 0; k < 4; ++k)
        if (tab->idf_start[k] < 0 || tab->idf_start[k + 1] < tab->idf_start[k]) return GRIT_ERR_BAD_ARG;
    if (tab->width > GRIT_CIDER_MAX_EXPANSION || (long)T * tab->width > GRIT_CIDER_MAX_TOKENS) return GRIT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(cider_reward, dim3(rows), dim3(kThreads), 0, (hipStream_t)stream, tokens, T, slots, beam, *tab, out32,
                       out64);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}
