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
#include "cider_internal.h"

#pragma clang fp contract(off)

namespace {

using namespace grit_cider;  // the steps themselves: cider_internal.h, shared with caption_scores.hip

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

    // ---- 1. words up to the first EOS, their expansion -------------------------------------------------------------------
    const int slot = slots[row / beam];
    const int L = expand_row(tokens + (size_t)row * T, T, tab, false, s_word, s_meta, s_tok);
    // an id outside the vocabulary BEFORE the cut (the host would raise), or an unknown slot: NaN, never a wrong number
    if (L < 0 || slot < 0 || slot >= tab.n_slots) {
        if (tid == 0) {
            out32[row] = __builtin_nanf("");
            if (out64) out64[row] = __builtin_nan("");
        }
        return;
    }

    // ---- 2. + 3. term frequency at the first occurrence, idf chained by order, weight ------------------------------------
    hypothesis_weights<false>(tab, L, s_tok, s_w, s_norm, nullptr);

    // ---- 4. clipped similarity against every reference of the image ------------------------------------------------------
    const double score = score_against_references<false>(tab, tab.slot_ref_start[slot], tab.slot_ref_start[slot + 1], L, s_tok, s_w,
                                                         s_term, s_norm, s_val, nullptr, nullptr, nullptr);
    if (tid == 0) {
        out32[row] = (float)score;
        if (out64) out64[row] = score;
    }
}

}  // namespace

extern "C" int grit_cider_reward(const int64_t* tokens, int rows, int T, const int32_t* slots, int beam,
                                 const grit_cider_tables* tab, float* out32, double* out64, void* stream) {
    if (!tokens || !slots || !tab || !out32 || rows <= 0 || T <= 0 || beam <= 0 || rows % beam != 0) return GRIT_ERR_BAD_ARG;
    const int st = check_tables(tab, T);
    if (st != GRIT_OK) return st;
    hipLaunchKernelGGL(cider_reward, dim3(rows), dim3(kThreads), 0, (hipStream_t)stream, tokens, T, slots, beam, *tab, out32,
                       out64);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}
