// The evaluation's caption scores on the device: generated token ids in, per hypothesis row the ten BLEU integers, ROUGE-L and
// CIDEr-D out, one launch, no host involvement.
//
// Stands for davidnvq/grit engine/caption_engine.py:165-190 (text_field.decode -> itertools.groupby -> PTBTokenizer.tokenize ->
// metrics.compute_scores) and datasets/caption/metrics/{bleu/bleu_scorer.py (cook_refs, cook_test), rouge/rouge.py (my_lcs,
// calc_score), cider/cider_scorer.py}, in the arrangement of this build's datasets/caption/metrics/{bleu,rouge,cider}.py.
// Everything that does not depend on the hypothesis is packed once on the host (grit_amd/ops/caption_scores.py on top of
// grit_amd/ops/cider.py).  The corpus formulas (sums of the integers, means) stay on the host: they are a few scalars.
//
// One workgroup per hypothesis row.  The row's words are cut, collapsed and expanded, its n-gram weights formed and the cooked
// references walked by the code the self-critical reward uses (cider_internal.h); the walk also collects the clipped counts of
// BLEU.  ROUGE-L is an integer longest-common-subsequence table per reference, swept by anti-diagonals with one thread per
// hypothesis token, then the host's float64 expression in the host's order.  No atomics, nothing depends on the launch geometry.
#include "cider_internal.h"

#pragma clang fp contract(off)

namespace {

using namespace grit_cider;

__global__ __launch_bounds__(kThreads)
void caption_scores(const int64_t* __restrict__ tokens, int T, const int32_t* __restrict__ slots, int collapse,
                    grit_cider_tables tab, grit_score_tables ext, int32_t* __restrict__ comps, double* __restrict__ rouge,
                    double* __restrict__ cider) {
    __shared__ int s_word[kMaxT];
    __shared__ int s_meta[kMaxT];
    __shared__ int s_tok[kMaxTok + kOrders];
    __shared__ double s_w[kOrders][kMaxTok];
    __shared__ double s_term[kOrders][kMaxTok];
    __shared__ double s_norm[kOrders];
    __shared__ double s_val[kOrders];
    __shared__ int s_tf[kOrders][kMaxTok];    // count of an n-gram in the hypothesis at its first occurrence, 0 elsewhere
    __shared__ int s_best[kOrders][kMaxTok];  // the largest count of that n-gram in any one reference
    __shared__ int s_correct[kOrders];
    __shared__ int s_diag[3][kMaxTok + 1];    // three anti-diagonals of the subsequence table, [i + 1] = hypothesis position i
    __shared__ int s_lcs;

    const int tid = threadIdx.x;
    const int row = blockIdx.x;

    // ---- 1. + 2. words up to the first EOS, repeated words dropped, their expansion --------------------------------------
    const int slot = slots[row];
    for (int i = tid; i < kOrders * kMaxTok; i += kThreads) (&s_best[0][0])[i] = 0;  // (barriers follow in expand_row)
    const int L = expand_row(tokens + (size_t)row * T, T, tab, collapse != 0, s_word, s_meta, s_tok);
    if (L < 0 || slot < 0 || slot >= tab.n_slots) {  // NaN / -1, never a wrong number
        if (tid < GRIT_SCORE_COMPONENTS) comps[(size_t)row * GRIT_SCORE_COMPONENTS + tid] = -1;
        if (tid == 0) {
            rouge[row] = __builtin_nan("");
            cider[row] = __builtin_nan("");
        }
        return;
    }
    const int r0 = tab.slot_ref_start[slot], r1 = tab.slot_ref_start[slot + 1];

    // ---- 3. + 5. CIDEr-D, and on the same walk over the references' entries the clipped counts of BLEU -------------------
    hypothesis_weights<true>(tab, L, s_tok, s_w, s_norm, s_tf);
    const double score = score_against_references<true>(tab, r0, r1, L, s_tok, s_w, s_term, s_norm, s_val, s_tf, s_best, ext.ent_tf);
    __syncthreads();
    if (tid < kOrders) {
        int c = 0;
        for (int i = 0; i + tid < L; ++i) c += min(s_tf[tid][i], s_best[tid][i]);
        s_correct[tid] = c;
    }
    if (L == 0 && tid == 0) s_tok[0] = ext.empty_tok;  // ROUGE splits at single spaces: the empty string is one empty token
    __syncthreads();

    // ---- 4. ROUGE-L: the subsequence table of the hypothesis against each reference --------------------------------------
    const int Lh = L > 0 ? L : 1;
    const int mine = tid < Lh ? s_tok[tid] : -1;
    double prec_max = 0.0, rec_max = 0.0;  // thread 0 only
    int reflen = 0, gap = 0x7fffffff;      // thread 0 only: the reference word count closest to the hypothesis', ties to the shorter
    for (int r = r0; r < r1; ++r) {
        const int q0 = ext.seq_start[r], Lr = ext.seq_start[r + 1] - q0;
        for (int i = tid; i < 3 * (kMaxTok + 1); i += kThreads) (&s_diag[0][0])[i] = 0;
        if (tid == 0) s_lcs = 0;
        __syncthreads();
        // cell (i, j) = hypothesis token i against reference token j lies on diagonal d = i + j; thread i keeps the cell to its
        // left, thread i - 1 left the cell above on diagonal d - 1 and the one above-left on diagonal d - 2
        int left = 0;
        const int n_diag = Lr > 0 ? Lh + Lr - 1 : 0;
        for (int d = 0; d < n_diag; ++d) {
            int* cur = s_diag[d % 3];
            const int* prev1 = s_diag[(d + 2) % 3];
            const int* prev2 = s_diag[(d + 1) % 3];
            const int j = d - tid;
            if (tid < Lh) {
                int v = 0;
                if (j >= 0 && j < Lr) {
                    v = ext.seq_tok[q0 + j] == mine ? prev2[tid] + 1 : max(prev1[tid], left);
                    left = v;
                }
                cur[tid + 1] = v;
            }
            __syncthreads();
        }
        if (tid == Lh - 1) s_lcs = left;
        __syncthreads();
        if (tid == 0) {
            const int lcs = s_lcs;
            const double p = lcs / (double)Lh;
            const double q = Lr > 0 ? lcs / (double)Lr : 0.0;
            if (p > prec_max) prec_max = p;
            if (q > rec_max) rec_max = q;
            const int words = ext.ref_words[r];
            const int g = words > L ? words - L : L - words;
            if (g < gap || (g == gap && words < reflen)) {
                gap = g;
                reflen = words;
            }
        }
        // s_lcs and s_diag of the next reference are written only after the barrier above
    }

    if (tid < kOrders) {
        int32_t* out = comps + (size_t)row * GRIT_SCORE_COMPONENTS;
        out[2 + tid] = L > tid ? L - tid : 0;
        out[2 + kOrders + tid] = s_correct[tid];
    }
    if (tid == 0) {
        comps[(size_t)row * GRIT_SCORE_COMPONENTS] = L;
        comps[(size_t)row * GRIT_SCORE_COMPONENTS + 1] = reflen;
        double f = 0.0;
        if (prec_max != 0.0 && rec_max != 0.0) f = ((1.0 + ext.beta2) * prec_max * rec_max) / (rec_max + ext.beta2 * prec_max);
        rouge[row] = f;
        cider[row] = score;
    }
}

}  // namespace

extern "C" int grit_caption_scores(const int64_t* tokens, int rows, int T, const int32_t* slots, int collapse,
                                   const grit_cider_tables* tab, const grit_score_tables* ext, int32_t* comps, double* rouge,
                                   double* cider, void* stream) {
    if (!tokens || !slots || !tab || !ext || !comps || !rouge || !cider || rows <= 0 || T <= 0) return GRIT_ERR_BAD_ARG;
    if (!ext->ent_tf || !ext->ref_words || !ext->seq_start || !ext->seq_tok || !(ext->beta2 > 0.0)) return GRIT_ERR_BAD_ARG;
    const int st = check_tables(tab, T);
    if (st != GRIT_OK) return st;
    hipLaunchKernelGGL(caption_scores, dim3(rows), dim3(kThreads), 0, (hipStream_t)stream, tokens, T, slots, collapse, *tab, *ext,
                       comps, rouge, cider);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}
