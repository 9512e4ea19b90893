// What the caption kernels share (cider.hip: the self-critical reward; caption_scores.hip: the evaluation's BLEU / ROUGE-L /
// CIDEr): a row of word ids -> tokenizer tokens, the tf-idf weights of the hypothesis, and the walk over the cooked references.
// One workgroup of kThreads per hypothesis row; every function here is called by all of its threads.
//
// float64 throughout, every sum sequential in the order the host's dictionaries are walked (n-grams by first occurrence, orders
// 1..4, references in list order), no fused multiply-add, no atomics.
#ifndef GRIT_CIDER_INTERNAL_H
#define GRIT_CIDER_INTERNAL_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/grit_hip.h"

#pragma clang fp contract(off)

namespace grit_cider {

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

// The words of one row up to the first <eos> and their expansion into s_tok[0, L), -1 in the kOrders places behind.  With
// `collapse` every word id equal to its predecessor is dropped first (the evaluation's itertools.groupby).  Returns L, or -1 when
// an id in front of the cut lies outside the vocabulary (the host would raise): the caller reports it, never a wrong number.
// s_word / s_meta: kMaxT ints, s_tok: kMaxTok + kOrders ints.
__device__ __forceinline__ int expand_row(const int64_t* __restrict__ trow, int T, const grit_cider_tables& tab, bool collapse,
                                          int* s_word, int* s_meta, int* s_tok) {
    const int tid = threadIdx.x;
    if (tid < T) {
        const int64_t w = trow[tid];
        const bool known = w >= 0 && w < tab.vocab;  // an id outside the vocabulary is reported below, not looked up
        s_word[tid] = known ? (int)w : -1;
        s_meta[tid] = known ? tab.word_meta[w] : 0;
    }
    __syncthreads();
    int cut = T;
    for (int t = T - 1; t >= 0; --t)
        if (s_meta[t] & GRIT_CIDER_META_EOS) cut = t;
    bool bad = false;
    for (int t = 0; t < cut; ++t) bad = bad || s_word[t] < 0;
    if (bad) return -1;
    auto kept = [&](int t) { return !collapse || t == 0 || s_word[t] != s_word[t - 1]; };
    int last = -1;  // the last word that is not whitespace-only: it alone is tokenised as the end of the sentence
    for (int t = 0; t < cut; ++t)
        if (kept(t) && !(s_meta[t] & GRIT_CIDER_META_BLANK)) last = t;
    int offset = 0, L = 0;
    for (int t = 0; t < cut; ++t) {
        const int m = s_meta[t];
        const int c = kept(t) ? min(t == last ? (m >> GRIT_CIDER_META_FIN_SHIFT) & 15 : m & 15, tab.width) : 0;
        if (t < tid) offset += c;
        L += c;
    }
    if (tid < cut && kept(tid)) {
        const int m = s_meta[tid];
        const bool fin = tid == last;
        const int c = min(fin ? (m >> GRIT_CIDER_META_FIN_SHIFT) & 15 : m & 15, tab.width);
        const int32_t* e = tab.expansion + ((size_t)s_word[tid] * 2 + (fin ? 1 : 0)) * tab.width;
        for (int j = 0; j < c; ++j) s_tok[offset + j] = e[j];
    }
    if (tid < kOrders) s_tok[L + tid] = -1;
    __syncthreads();
    return L;
}

// Term frequency at the first occurrence of every n-gram of the hypothesis, idf chained by order: s_w[k][i] = tf * idf at the first
// occurrence of the (k+1)-gram that starts at i, 0 elsewhere; s_norm[k].  With kTf also s_tf[k][i] = that tf, 0 elsewhere.
template <bool kTf>
__device__ __forceinline__ void hypothesis_weights(const grit_cider_tables& tab, int L, const int* s_tok, double (*s_w)[kMaxTok],
                                                   double* s_norm, int (*s_tf)[kMaxTok]) {
    const int tid = threadIdx.x;
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
            if (kTf) s_tf[k][tid] = tid + k < L && first[k] ? tf[k] : 0;
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
}

// Clipped similarity against the references [r0, r1) of the image: the CIDEr-D score of the row, valid in thread 0.
// With kBleu the same walk over a reference's entries also takes the raw term frequency next to each entry (ent_tf):
// s_best[k][i] = max over the references of the count of the n-gram whose first occurrence is at i (the caller zeroes it), so
// each entry list is read once for both metrics.  The walk then covers every first occurrence, also one of weight 0 (idf 0),
// whose CIDEr term is 0 either way.
template <bool kBleu>
__device__ __forceinline__ double score_against_references(const grit_cider_tables& tab, int r0, int r1, int L, const int* s_tok,
                                                           double (*s_w)[kMaxTok], double (*s_term)[kMaxTok], const double* s_norm,
                                                           double* s_val, const int (*s_tf)[kMaxTok], int (*s_best)[kMaxTok],
                                                           const int32_t* __restrict__ ent_tf) {
    const int tid = threadIdx.x;
    const int len_h = L > 0 ? L - 1 : 0;  // sentence length in bigram occurrences
    double total = 0.0;                   // thread 0 only
    for (int r = r0; r < r1; ++r) {
        for (int item = tid; item < kOrders * L; item += kThreads) {
            const int k = item / L, i = item - k * L;
            double term = 0.0;
            const double wh = s_w[k][i];
            if (kBleu ? s_tf[k][i] > 0 : (i + k < L && wh != 0.0)) {
                const int e0 = tab.ref_ent_start[r * kOrders + k], e1 = tab.ref_ent_start[r * kOrders + k + 1];
                const int a = s_tok[i], b = k > 0 ? s_tok[i + 1] : -1, c = k > 1 ? s_tok[i + 2] : -1, d = k > 2 ? s_tok[i + 3] : -1;
                for (int e = e0; e < e1; ++e) {
                    const int4 q = static_cast<const int4*>(tab.ent_tok)[e];
                    if (q.x == a && q.y == b && q.z == c && q.w == d) {
                        const double wr = tab.ent_w[e];
                        if (!kBleu || wh != 0.0) term = (wh < wr ? wh : wr) * wr;
                        if (kBleu) s_best[k][i] = max(s_best[k][i], ent_tf[e]);  // (an item stays with its thread over r)
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
    return r1 > r0 ? total / (double)(r1 - r0) * 10.0 : 0.0;
}

// the checks on the tables that both entry points make
inline int check_tables(const grit_cider_tables* tab, int T) {
    if (!tab->expansion || !tab->word_meta || !tab->idf_key || !tab->idf_val || !tab->slot_ref_start || !tab->ref_ent_start ||
        !tab->ent_tok || !tab->ent_w || !tab->ref_norm || !tab->ref_len || tab->vocab <= 0 || tab->n_slots <= 0 ||
        tab->width <= 0 || !(tab->sigma > 0.0))
        return GRIT_ERR_BAD_ARG;
    for (int k = 0; k < 4; ++k)
        if (tab->idf_start[k] < 0 || tab->idf_start[k + 1] < tab->idf_start[k]) return GRIT_ERR_BAD_ARG;
    if (tab->width > GRIT_CIDER_MAX_EXPANSION || (long)T * tab->width > GRIT_CIDER_MAX_TOKENS) return GRIT_ERR_UNSUPPORTED;
    return GRIT_OK;
}

}  // namespace grit_cider
#endif  // GRIT_CIDER_INTERNAL_H
