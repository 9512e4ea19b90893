// Consensus (minimum-Bayes-risk) reranking under CIDEr-D on the device: the n candidate captions of an image in, the pairwise
// similarity matrix, every candidate's consensus score and the index of the best one out.  Host form: grit_amd/ops/consensus.py.
//
// Nothing in the reference stands behind this; the steps are those of cider.hip.  A candidate as a reference has the vector it has
// as a hypothesis, so both sides of a pair come from expand_row + hypothesis_weights (cider_internal.h) and nothing is cooked on
// the host.
//
// Two launches:
//   consensus_cook    one workgroup of kThreads per row, as the reward: tokens, tf-idf weights at first occurrences, norms and L of
//                     the row go to the workspace (only the first L entries are written, and only they are read);
//   consensus_score   one workgroup per IMAGE.  The selection needs every score of the image, and there are neither atomics nor a
//                     third launch to gather them, so the image is the unit.  Its kScoreThreads / 64 waves share the n * (n - 1)
//                     ordered pairs; a wave owns a pair and walks the four orders itself.
// float64 throughout, every sum sequential in the host's order (n-grams by first occurrence, orders 1..4, candidates ascending), no
// fused multiply-add, no atomics: the result does not depend on which wave took which pair.
#include "cider_internal.h"

#pragma clang fp contract(off)

namespace {

using namespace grit_cider;

constexpr int kMaxCand = GRIT_CONSENSUS_MAX_CANDIDATES;
constexpr int kTokStride = kMaxTok + kOrders;  // a row's tokens and the -1 behind them
constexpr int kScoreThreads = 1024;
constexpr int kWave = 64;

// The workspace, array by array over all rows (doubles first: the base is aligned as hipMalloc aligns it).
struct Workspace {
    double* w;      // [rows][kOrders][kMaxTok]
    double* norm;   // [rows][kOrders]
    int32_t* tok;   // [rows][kTokStride]
    int32_t* len;   // [rows]  L, or -1: an id outside the vocabulary in front of <eos>
};

inline size_t workspace_bytes(size_t rows) {
    return rows * ((size_t)kOrders * kMaxTok * sizeof(double) + kOrders * sizeof(double) + kTokStride * sizeof(int32_t) +
                   sizeof(int32_t));
}

inline Workspace carve(void* base, size_t rows) {
    Workspace ws;
    ws.w = static_cast<double*>(base);
    ws.norm = ws.w + rows * kOrders * kMaxTok;
    ws.tok = reinterpret_cast<int32_t*>(ws.norm + rows * kOrders);
    ws.len = ws.tok + rows * kTokStride;
    return ws;
}

__global__ __launch_bounds__(kThreads)
void consensus_cook(const int64_t* __restrict__ tokens, int T, int collapse, grit_cider_tables tab, Workspace ws) {
    __shared__ int s_word[kMaxT];
    __shared__ int s_meta[kMaxT];
    __shared__ int s_tok[kTokStride];
    __shared__ double s_w[kOrders][kMaxTok];
    __shared__ double s_norm[kOrders];

    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const int L = expand_row(tokens + row * T, T, tab, collapse != 0, s_word, s_meta, s_tok);
    if (L < 0) {
        if (tid == 0) ws.len[row] = -1;
        return;
    }
    hypothesis_weights<false>(tab, L, s_tok, s_w, s_norm, nullptr);
    if (tid < L) {
#pragma unroll
        for (int k = 0; k < kOrders; ++k) ws.w[(row * kOrders + k) * kMaxTok + tid] = s_w[k][tid];
    }
    for (int t = tid; t < L + kOrders; t += kThreads) ws.tok[row * kTokStride + t] = s_tok[t];
    if (tid < kOrders) ws.norm[row * kOrders + tid] = s_norm[tid];
    if (tid == 0) ws.len[row] = L;
}

__global__ __launch_bounds__(kScoreThreads)
void consensus_score(int n, double sigma, Workspace ws, double* __restrict__ sim64, double* __restrict__ score64,
                     float* __restrict__ score32, int32_t* __restrict__ best, int32_t* __restrict__ bad) {
    __shared__ int s_tok[kMaxCand * kTokStride];
    __shared__ double s_norm[kMaxCand][kOrders];
    __shared__ double s_sim[kMaxCand][kMaxCand];
    __shared__ double s_score[kMaxCand];
    __shared__ int s_len[kMaxCand];

    const int tid = threadIdx.x;
    const size_t image = blockIdx.x;
    const size_t row0 = image * n;

    if (tid < n) s_len[tid] = ws.len[row0 + tid];
    __syncthreads();
    bool any_bad = false;
    for (int c = 0; c < n; ++c) any_bad = any_bad || s_len[c] < 0;
    if (any_bad) {  // (the same decision in every thread)
        const double nan = __builtin_nan("");
        if (sim64)
            for (int e = tid; e < n * n; e += kScoreThreads) sim64[image * n * n + e] = nan;
        if (tid < n) {
            score64[row0 + tid] = nan;
            if (score32) score32[row0 + tid] = __builtin_nanf("");
        }
        if (tid == 0) {
            best[image] = 0;
            bad[image] = 1;
        }
        return;
    }
    for (int e = tid; e < n * kTokStride; e += kScoreThreads) {
        const int c = e / kTokStride, p = e - c * kTokStride;
        if (p < s_len[c] + kOrders) s_tok[e] = ws.tok[row0 * kTokStride + e];
    }
    if (tid < n * kOrders) s_norm[tid / kOrders][tid % kOrders] = ws.norm[row0 * kOrders + tid];
    __syncthreads();

    // ---- the pairs: hypothesis i against reference j ---------------------------------------------------------------------
    const int lane = tid % kWave;
    for (int pair = tid / kWave; pair < n * n; pair += kScoreThreads / kWave) {  // (uniform in the wave)
        const int i = pair / n, j = pair - i * n;
        if (i == j) {
            if (lane == 0) s_sim[i][j] = 0.0;
            continue;
        }
        const int Li = s_len[i], Lj = s_len[j];
        const int* ti = s_tok + i * kTokStride;
        const int* tj = s_tok + j * kTokStride;
        const double* wi = ws.w + (row0 + i) * kOrders * kMaxTok;
        const double* wj = ws.w + (row0 + j) * kOrders * kMaxTok;
        const double delta = (double)((Li > 0 ? Li - 1 : 0) - (Lj > 0 ? Lj - 1 : 0));  // lengths in bigram occurrences
        const double penalty = exp(-(delta * delta) / (2.0 * (sigma * sigma)));
        double sim = 0.0;
        for (int k = 0; k < kOrders; ++k) {
            double val = 0.0;
            for (int base = 0; base + k < Li; base += kWave) {
                // the lane's n-gram of i: a first occurrence carries a weight; it meets the first occurrence in j, which carries j's
                const int p = base + lane;
                double term = 0.0;
                if (p + k < Li) {
                    const double wh = wi[k * kMaxTok + p];
                    if (wh != 0.0) {
                        for (int q = 0; q + k < Lj; ++q) {
                            bool same = true;
                            for (int m = 0; m <= k; ++m) same = same && tj[q + m] == ti[p + m];
                            if (same) {
                                const double wr = wj[k * kMaxTok + q];
                                term = (wh < wr ? wh : wr) * wr;
                                break;
                            }
                        }
                    }
                }
                // in the order of the positions; a position without a term adds 0.0, which changes nothing
                const int live = min(kWave, Li - k - base);
                for (int l = 0; l < live; ++l) val += __shfl(term, l, kWave);
            }
            const double ni = s_norm[i][k], nj = s_norm[j][k];
            if (ni != 0.0 && nj != 0.0) val /= ni * nj;
            sim += val * penalty;
        }
        if (lane == 0) s_sim[i][j] = sim / (double)kOrders;
    }
    __syncthreads();

    // ---- consensus score of every candidate, then the first maximum ------------------------------------------------------
    if (sim64)
        for (int e = tid; e < n * n; e += kScoreThreads) sim64[image * n * n + e] = s_sim[e / n][e % n];
    if (tid < n) {
        double total = 0.0;
        for (int j = 0; j < n; ++j)
            if (j != tid) total += s_sim[tid][j];
        const double score = n > 1 ? total / (double)(n - 1) * 10.0 : 0.0;
        s_score[tid] = score;
        score64[row0 + tid] = score;
        if (score32) score32[row0 + tid] = (float)score;
    }
    __syncthreads();
    if (tid == 0) {
        int arg = 0;
        for (int c = 1; c < n; ++c)
            if (s_score[c] > s_score[arg]) arg = c;
        best[image] = arg;
        bad[image] = 0;
    }
}

// what this entry point reads of the tables: no reference slots are needed
int check_consensus(const grit_cider_tables* tab, int images, int n, int T) {
    if (!tab || images <= 0 || n <= 0 || T <= 0) return GRIT_ERR_BAD_ARG;
    if (!tab->expansion || !tab->word_meta || !tab->idf_key || !tab->idf_val || tab->vocab <= 0 || tab->width <= 0 ||
        !(tab->sigma > 0.0) || tab->log_corpus != tab->log_corpus)
        return GRIT_ERR_BAD_ARG;
    for (int k = 0; k < 4; ++k)
        if (tab->idf_start[k] < 0 || tab->idf_start[k + 1] < tab->idf_start[k]) return GRIT_ERR_BAD_ARG;
    if ((long)images * n > 0x7fffffffL) return GRIT_ERR_BAD_ARG;
    if (n > kMaxCand || tab->width > GRIT_CIDER_MAX_EXPANSION || (long)T * tab->width > GRIT_CIDER_MAX_TOKENS)
        return GRIT_ERR_UNSUPPORTED;
    return GRIT_OK;
}

}  // namespace

extern "C" long grit_cider_consensus_workspace(int images, int n, int T) {
    // (T does not enter: a row is stored at its limit, GRIT_CIDER_MAX_TOKENS, whatever T is; the argument keeps the form open)
    if (images <= 0 || n <= 0 || T <= 0 || n > kMaxCand || (long)images * n > 0x7fffffffL) return 0;
    return (long)workspace_bytes((size_t)images * n);
}

extern "C" int grit_cider_consensus(const int64_t* tokens, int images, int n, int T, int collapse, const grit_cider_tables* tab,
                                    double* sim64, double* score64, float* score32, int32_t* best, int32_t* bad, void* workspace,
                                    void* stream) {
    if (!tokens || !score64 || !best || !bad || !workspace) return GRIT_ERR_BAD_ARG;
    const int st = check_consensus(tab, images, n, T);
    if (st != GRIT_OK) return st;
    const size_t rows = (size_t)images * n;
    const Workspace ws = carve(workspace, rows);
    hipLaunchKernelGGL(consensus_cook, dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, tokens, T, collapse, *tab, ws);
    if (hipGetLastError() != hipSuccess) return GRIT_ERR_LAUNCH;
    hipLaunchKernelGGL(consensus_score, dim3((unsigned)images), dim3(kScoreThreads), 0, (hipStream_t)stream, n, tab->sigma, ws,
                       sim64, score64, score32, best, bad);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}
