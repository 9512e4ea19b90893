// Detector training losses (include/grit_hip.h, "Detector set criterion"): the Hungarian matcher's cost matrix and its optimal
// assignment for every (output layer, image) pair in one launch, and the set criterion's forward and backward over all layers
// in one launch each.  fp32 in and out; dual variables, path lengths and every sum in float64.
//
// Solver: shortest augmenting paths over the smaller side of the rectangular problem (Jonker-Volgenant as stated by Crouse,
// "On implementing 2D rectangular assignment algorithms", 2016 -- the algorithm scipy.optimize.linear_sum_assignment runs), ONE
// wave per problem.  Lane l owns the columns j = l, l + 64, ...: their reduced path lengths, predecessor and "scanned" flag are
// only ever touched by the owner inside the search loop, so that loop has no barrier at all -- the only exchange is the
// (value, column) min-reduction over the lanes.  The reduced cost is evaluated in scipy's own order, ((minVal + c) - u) - v, in
// double on the fp32 costs as stored, so on a problem with a unique optimum the assignment equals scipy's.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/grit_hip.h"

namespace {

constexpr int kSide = GRIT_DET_MAX_SIDE;
constexpr int kWave = 64;
constexpr int kRows = GRIT_DET_LOSS_ROWS;
constexpr int kFields = GRIT_DET_LOSS_FIELDS;
constexpr int kAssigned = 1 << 16;  // key bit above every column index (kSide <= 65536)

struct LsaState {
    double u[kSide];         // duals of the rows (the smaller side)
    double v[kSide];         // duals of the columns
    double shortest[kSide];  // reduced length of the shortest path found to each column
    int path[kSide];         // its predecessor row
    int row4col[kSide];
    int col4row[kSide];
    unsigned char scanned[kSide];
};

// One wave (a 64-thread workgroup).  The cost of (query q, target t) is C[q * qs + t * ts]; match_q [T] <- query of each target or
// -1, match_t [Q] (may be null) <- target of each query or -1.  A problem with a non-finite entry that leaves no finite augmenting
// path gets -1 everywhere.  The column scan walks the LARGER side; with T <= Q its loads are ts floats apart.  A transposed copy
// that makes them contiguous was measured and is not kept: the matrices live in L2 and the launch got 7 % slower.
__device__ void lsa_solve(const float* __restrict__ C, long qs, long ts, int Q, int T, int32_t* __restrict__ match_q,
                          int32_t* __restrict__ match_t, LsaState& s) {
    const int lane = threadIdx.x;
    for (int t = lane; t < T; t += kWave) match_q[t] = -1;
    if (match_t)
        for (int q = lane; q < Q; q += kWave) match_t[q] = -1;
    const bool rows_are_targets = T <= Q;
    const int n = rows_are_targets ? T : Q;  // rows: the smaller side
    const int m = rows_are_targets ? Q : T;  // columns
    const long rs = rows_are_targets ? ts : qs, cs = rows_are_targets ? qs : ts;
    for (int j = lane; j < m; j += kWave) {
        s.v[j] = 0.0;
        s.row4col[j] = -1;
    }
    for (int i = lane; i < n; i += kWave) {
        s.u[i] = 0.0;
        s.col4row[i] = -1;
    }
    __syncthreads();
    bool feasible = true;
    for (int cur = 0; cur < n && feasible; ++cur) {
        for (int j = lane; j < m; j += kWave) {
            s.shortest[j] = INFINITY;
            s.scanned[j] = 0;
        }
        double min_val = 0.0;
        int i = cur, sink = -1;
        while (sink < 0) {
            const double ui = s.u[i];
            const float* row = C + i * rs;
            double best = INFINITY;
            int key = INT_MAX;
            for (int j = lane; j < m; j += kWave) {
                if (s.scanned[j]) continue;
                const double r = min_val + (double)row[j * cs] - ui - s.v[j];
                double sh = s.shortest[j];
                if (r < sh) {
                    sh = r;
                    s.shortest[j] = r;
                    s.path[j] = i;
                }
                // among equal lengths an unassigned column ends the search at once; then the lowest index, so the choice is a
                // function of the data alone
                const int k = j | (s.row4col[j] >= 0 ? kAssigned : 0);
                if (sh < INFINITY && (sh < best || (sh == best && k < key))) {
                    best = sh;
                    key = k;
                }
            }
            for (int off = kWave / 2; off > 0; off >>= 1) {
                const double ob = __shfl_xor(best, off, kWave);
                const int ok = __shfl_xor(key, off, kWave);
                if (ob < best || (ob == best && ok < key)) {
                    best = ob;
                    key = ok;
                }
            }
            if (key == INT_MAX) {  // every remaining column is at infinite (or NaN) distance
                feasible = false;
                break;
            }
            min_val = best;
            const int j = key & (kAssigned - 1);
            if (lane == (j & (kWave - 1))) s.scanned[j] = 1;
            if (key & kAssigned)
                i = s.row4col[j];
            else
                sink = j;
        }
        if (!feasible) break;
        // duals: every scanned column but the sink is assigned, to a row the search went through
        for (int j = lane; j < m; j += kWave) {
            if (!s.scanned[j]) continue;
            const double d = min_val - s.shortest[j];
            const int r = s.row4col[j];
            if (r >= 0) s.u[r] += d;
            s.v[j] -= d;
        }
        if (lane == 0) s.u[cur] += min_val;
        __syncthreads();
        if (lane == 0) {  // augment along the predecessors
            int j = sink;
            for (int guard = 0; guard <= n; ++guard) {
                const int r = s.path[j];
                s.row4col[j] = r;
                const int next = s.col4row[r];
                s.col4row[r] = j;
                j = next;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }
    if (!feasible) return;
    for (int i = lane; i < n; i += kWave) {
        const int j = s.col4row[i];
        const int t = rows_are_targets ? i : j, q = rows_are_targets ? j : i;
        match_q[t] = q;
        if (match_t) match_t[q] = t;
    }
}

__device__ inline void fill_unmatched(int32_t* match_q, int Tmax, int32_t* match_t, int Q) {
    for (int t = threadIdx.x; t < Tmax; t += kWave) match_q[t] = -1;
    if (match_t)
        for (int q = threadIdx.x; q < Q; q += kWave) match_t[q] = -1;
}

__global__ __launch_bounds__(kWave) void lsa_kernel(const float* __restrict__ cost, const int32_t* __restrict__ counts,
                                                    const int32_t* __restrict__ rows, int Q, long ld, int Tmax,
                                                    int32_t* __restrict__ match_q, int32_t* __restrict__ match_t) {
    __shared__ LsaState s;
    const long p = blockIdx.x;
    const int T = counts[p], Qp = rows ? rows[p] : Q;
    int32_t* mq = match_q + p * Tmax;
    int32_t* mt = match_t ? match_t + p * Q : nullptr;
    if (T < 0 || T > Tmax || T > ld || Qp < 0 || Qp > Q) {
        fill_unmatched(mq, Tmax, mt, Q);
        return;
    }
    for (int t = T + threadIdx.x; t < Tmax; t += kWave) mq[t] = -1;
    if (mt)
        for (int q = Qp + threadIdx.x; q < Q; q += kWave) mt[q] = -1;
    lsa_solve(cost + p * Q * ld, ld, 1, Qp, T, mq, mt, s);
}

// The matcher's cost of one (query, target) pair in fp32, operation by operation as the composition of elementwise ops states it
// (no contraction into fused multiply-adds: the result then differs from that composition only by the ulps of expf / logf).
__device__ inline float pair_cost(float logit, const float* __restrict__ qb, const float* __restrict__ tb, float w_class, float w_bbox,
                                  float w_giou) {
#pragma clang fp contract(off)
    const float p = 1.0f / (1.0f + expf(-logit));
    const float neg = 0.75f * (p * p) * (-logf(1.0f - p + 1e-8f));
    const float pos = 0.25f * ((1.0f - p) * (1.0f - p)) * (-logf(p + 1e-8f));
    const float cls = pos - neg;
    const float l1 = fabsf(qb[0] - tb[0]) + fabsf(qb[1] - tb[1]) + fabsf(qb[2] - tb[2]) + fabsf(qb[3] - tb[3]);
    const float ax0 = qb[0] - 0.5f * qb[2], ay0 = qb[1] - 0.5f * qb[3], ax1 = qb[0] + 0.5f * qb[2], ay1 = qb[1] + 0.5f * qb[3];
    const float bx0 = tb[0] - 0.5f * tb[2], by0 = tb[1] - 0.5f * tb[3], bx1 = tb[0] + 0.5f * tb[2], by1 = tb[1] + 0.5f * tb[3];
    const float area_a = (ax1 - ax0) * (ay1 - ay0), area_b = (bx1 - bx0) * (by1 - by0);
    const float iw = fmaxf(fminf(ax1, bx1) - fmaxf(ax0, bx0), 0.0f), ih = fmaxf(fminf(ay1, by1) - fmaxf(ay0, by0), 0.0f);
    const float inter = iw * ih;
    const float uni = area_a + area_b - inter;
    const float iou = inter / uni;
    const float ew = fmaxf(fmaxf(ax1, bx1) - fminf(ax0, bx0), 0.0f), eh = fmaxf(fmaxf(ay1, by1) - fminf(ay0, by0), 0.0f);
    const float hull = ew * eh;
    const float giou = iou - (hull - uni) / hull;
    return w_bbox * l1 + w_class * cls + w_giou * (-giou);
}

__global__ __launch_bounds__(kWave) void det_match_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                          const int64_t* __restrict__ tgt_labels, const float* __restrict__ tgt_boxes,
                                                          const int32_t* __restrict__ tgt_offsets, int B, int Q, int K, int Tmax,
                                                          float w_class, float w_bbox, float w_giou, float* __restrict__ cost, long ld,
                                                          int32_t* __restrict__ match_q, int32_t* __restrict__ match_t) {
    __shared__ LsaState s;
    const long p = blockIdx.x;  // = layer * B + image
    const int b = (int)(p % B);
    const int first = tgt_offsets[b], T = tgt_offsets[b + 1] - first;
    int32_t* mq = match_q + p * Tmax;
    int32_t* mt = match_t + p * Q;
    if (first < 0 || T < 0 || T > Tmax) {
        fill_unmatched(mq, Tmax, mt, Q);
        return;
    }
    for (int t = T + threadIdx.x; t < Tmax; t += kWave) mq[t] = -1;
    float* C = cost + p * Q * ld;
    const float* x = logits + p * Q * K;
    const float* qb = boxes + p * Q * 4;
    const int total = Q * T;
    for (int e = threadIdx.x; e < total; e += kWave) {
        const int q = e / T, t = e - q * T;
        const int64_t label = tgt_labels[first + t];
        float c = NAN;  // a label outside [0, K) poisons its column: the problem comes back unmatched instead of reading out of bounds
        if (label >= 0 && label < K) c = pair_cost(x[(long)q * K + label], qb + q * 4, tgt_boxes + (long)(first + t) * 4, w_class, w_bbox, w_giou);
        C[q * ld + t] = c;
    }
    __syncthreads();
    lsa_solve(C, ld, 1, Q, T, mq, mt, s);
}

// ---- criterion -----------------------------------------------------------------------------------------------------------------

__device__ inline double wave_sum(double v) {
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// Sum over the 256 threads of a block, returned to every thread.  `sh` holds 4 doubles.
__device__ inline double block_sum(double v, double* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

struct Focal {
    float p, q, sp_pos, sp_neg;  // sigmoid(x), 1 - sigmoid(x), softplus(x), softplus(-x): none of them by cancellation
};

__device__ inline Focal focal_terms(float x) {
    const float e = expf(-fabsf(x));
    const float inv = 1.0f / (1.0f + e);
    const float l = log1pf(e);
    Focal f;
    f.p = x >= 0.0f ? inv : e * inv;
    f.q = x >= 0.0f ? e * inv : inv;
    f.sp_pos = fmaxf(x, 0.0f) + l;
    f.sp_neg = fmaxf(-x, 0.0f) + l;
    return f;
}

// L1 and 1 - GIoU of a matched pair (cxcywh) in double, and optionally their gradients with respect to the predicted box.  The
// derivative of min / max at a tie is split evenly and the clamp passes it at zero, as autograd does.
__device__ inline void box_pair(const float* __restrict__ qb, const float* __restrict__ tb, double& l1, double& gl, double* d_l1,
                                double* d_gl) {
    const double a[4] = {(double)qb[0], (double)qb[1], (double)qb[2], (double)qb[3]};
    const double g[4] = {(double)tb[0], (double)tb[1], (double)tb[2], (double)tb[3]};
    l1 = fabs(a[0] - g[0]) + fabs(a[1] - g[1]) + fabs(a[2] - g[2]) + fabs(a[3] - g[3]);
    const double a0[2] = {a[0] - 0.5 * a[2], a[1] - 0.5 * a[3]}, a1[2] = {a[0] + 0.5 * a[2], a[1] + 0.5 * a[3]};
    const double b0[2] = {g[0] - 0.5 * g[2], g[1] - 0.5 * g[3]}, b1[2] = {g[0] + 0.5 * g[2], g[1] + 0.5 * g[3]};
    const double area_a = (a1[0] - a0[0]) * (a1[1] - a0[1]), area_b = (b1[0] - b0[0]) * (b1[1] - b0[1]);
    double iw[2], ew[2];
    for (int d = 0; d < 2; ++d) {
        iw[d] = fmax(fmin(a1[d], b1[d]) - fmax(a0[d], b0[d]), 0.0);
        ew[d] = fmax(fmax(a1[d], b1[d]) - fmin(a0[d], b0[d]), 0.0);
    }
    const double inter = iw[0] * iw[1], uni = area_a + area_b - inter, hull = ew[0] * ew[1];
    gl = 1.0 - (inter / uni - (hull - uni) / hull);
    if (!d_l1) return;
    for (int c = 0; c < 4; ++c) d_l1[c] = a[c] > g[c] ? 1.0 : (a[c] < g[c] ? -1.0 : 0.0);
    // giou = inter / uni - 1 + uni / hull
    const double g_uni = -inter / (uni * uni) + 1.0 / hull;
    const double g_inter = 1.0 / uni - g_uni;  // uni = area_a + area_b - inter
    const double g_hull = -uni / (hull * hull);
    double g0[2], g1[2];  // d giou / d a0[d], d a1[d]
    for (int d = 0; d < 2; ++d) {
        const int o = 1 - d;
        const double side_o = a1[o] - a0[o];
        double lo = -g_uni * side_o, hi = g_uni * side_o;  // through area_a
        const double raw_i = fmin(a1[d], b1[d]) - fmax(a0[d], b0[d]);
        if (raw_i >= 0.0) {
            const double gi = g_inter * iw[o];
            hi += gi * (a1[d] < b1[d] ? 1.0 : (a1[d] == b1[d] ? 0.5 : 0.0));
            lo -= gi * (a0[d] > b0[d] ? 1.0 : (a0[d] == b0[d] ? 0.5 : 0.0));
        }
        const double raw_e = fmax(a1[d], b1[d]) - fmin(a0[d], b0[d]);
        if (raw_e >= 0.0) {
            const double ge = g_hull * ew[o];
            hi += ge * (a1[d] > b1[d] ? 1.0 : (a1[d] == b1[d] ? 0.5 : 0.0));
            lo -= ge * (a0[d] < b0[d] ? 1.0 : (a0[d] == b0[d] ? 0.5 : 0.0));
        }
        g0[d] = lo;
        g1[d] = hi;
    }
    // loss = 1 - giou; a0 = c - s / 2, a1 = c + s / 2
    d_gl[0] = -(g0[0] + g1[0]);
    d_gl[1] = -(g0[1] + g1[1]);
    d_gl[2] = -0.5 * (g1[0] - g0[0]);
    d_gl[3] = -0.5 * (g1[1] - g0[1]);
}

// Block (layer, image, chunk of kRows queries), one wave per query row.  partials [blocks, 8] = focal sum, L1 sum, (1 - GIoU) sum,
// rows whose argmax is not the last class, matched rows whose argmax is their label, matched rows.  The block that takes the last
// ticket reduces the partials per layer and writes out [L, kFields].  The entry point zeroes the ticket in front of every launch.
__global__ __launch_bounds__(256) void det_loss_fwd_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                           const int64_t* __restrict__ tgt_labels, const float* __restrict__ tgt_boxes,
                                                           const int32_t* __restrict__ tgt_offsets, const int32_t* __restrict__ match_t,
                                                           int L, int B, int Q, int K, int chunks, float alpha,
                                                           const float* __restrict__ num_boxes, double* partials, unsigned int* ticket,
                                                           float* __restrict__ out) {
    __shared__ double red[4][6];
    __shared__ double sum4[4];
    __shared__ int is_last;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const long p = blockIdx.x / chunks;
    const int chunk = blockIdx.x - (int)p * chunks, b = (int)(p % B);
    const int first = tgt_offsets[b], T = tgt_offsets[b + 1] - first;
    const int q_end = min(Q, (chunk + 1) * kRows);
    double focal = 0.0, l1 = 0.0, gl = 0.0, card = 0.0, correct = 0.0, matched = 0.0;
    for (int q = chunk * kRows + wave; q < q_end; q += 4) {
        const int t = match_t[p * Q + q];
        const bool hit = t >= 0 && t < T;
        const int64_t label = hit ? tgt_labels[first + t] : -1;
        const float* x = logits + (p * Q + q) * K;
        float top = -INFINITY;
        int arg = INT_MAX;
        for (int k = lane; k < K; k += kWave) {
            const float xv = x[k];
            const Focal f = focal_terms(xv);
            focal += k == label ? alpha * (f.sp_neg * (f.q * f.q)) : (1.0f - alpha) * (f.sp_pos * (f.p * f.p));
            if (xv > top) {
                top = xv;
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
        if (lane == 0) {
            card += arg != K - 1;
            if (hit) {
                matched += 1.0;
                correct += arg == label;
                double a, c;
                box_pair(boxes + (p * Q + q) * 4, tgt_boxes + (long)(first + t) * 4, a, c, nullptr, nullptr);
                l1 += a;
                gl += c;
            }
        }
    }
    focal = wave_sum(focal);
    if (lane == 0) {
        red[wave][0] = focal, red[wave][1] = l1, red[wave][2] = gl;
        red[wave][3] = card, red[wave][4] = correct, red[wave][5] = matched;
    }
    __syncthreads();
    if (threadIdx.x < 6)
        partials[(long)blockIdx.x * 8 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) is_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    const volatile double* part = partials;
    const double nb = (double)num_boxes[0];
    for (int l = 0; l < L; ++l) {
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int img = threadIdx.x; img < B; img += 256) {
            double count = 0.0;
            for (int c = 0; c < chunks; ++c) {
                const volatile double* row = part + ((long)(l * B + img) * chunks + c) * 8;
                acc[0] += row[0], acc[1] += row[1], acc[2] += row[2], count += row[3], acc[4] += row[4], acc[5] += row[5];
            }
            acc[3] += fabs(count - (double)(tgt_offsets[img + 1] - tgt_offsets[img]));
        }
        for (int f = 0; f < 6; ++f) acc[f] = block_sum(acc[f], sum4);
        if (threadIdx.x == 0) {
            float* o = out + l * kFields;
            o[0] = (float)(acc[0] / nb);
            o[1] = (float)(acc[1] / nb);
            o[2] = (float)(acc[2] / nb);
            o[3] = (float)(acc[3] / (double)B);
            o[4] = acc[5] > 0.0 ? 100.0f - (float)acc[4] * (100.0f / (float)acc[5]) : 100.0f;
            for (int f = 5; f < kFields; ++f) o[f] = 0.0f;
        }
    }
}

// Same blocks and rows as the forward.  coef [L, ldc]: the upstream gradient of out[l][0..2] (loss_ce, loss_bbox, loss_giou).
__global__ __launch_bounds__(256) void det_loss_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ boxes,
                                                           const int64_t* __restrict__ tgt_labels, const float* __restrict__ tgt_boxes,
                                                           const int32_t* __restrict__ tgt_offsets, const int32_t* __restrict__ match_t,
                                                           int B, int Q, int K, int chunks, float alpha, const float* __restrict__ num_boxes,
                                                           const float* __restrict__ coef, int ldc, float* __restrict__ dlogits,
                                                           float* __restrict__ dboxes) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const long p = blockIdx.x / chunks;
    const int chunk = blockIdx.x - (int)p * chunks, b = (int)(p % B), l = (int)(p / B);
    const int first = tgt_offsets[b], T = tgt_offsets[b + 1] - first;
    const int q_end = min(Q, (chunk + 1) * kRows);
    const float nb = num_boxes[0];
    const float s_ce = coef[l * ldc] / nb;
    const double s_l1 = (double)coef[l * ldc + 1] / (double)nb, s_gl = (double)coef[l * ldc + 2] / (double)nb;
    for (int q = chunk * kRows + wave; q < q_end; q += 4) {
        const int t = match_t[p * Q + q];
        const bool hit = t >= 0 && t < T;
        const int64_t label = hit ? tgt_labels[first + t] : -1;
        const float* x = logits + (p * Q + q) * K;
        float* dx = dlogits + (p * Q + q) * K;
        for (int k = lane; k < K; k += kWave) {
            const Focal f = focal_terms(x[k]);
            const float d = k == label ? -alpha * (f.q * f.q) * (f.q + 2.0f * f.sp_neg * f.p)
                                       : (1.0f - alpha) * (f.p * f.p) * (f.p + 2.0f * f.sp_pos * f.q);
            dx[k] = s_ce * d;
        }
        if (lane == 0) {
            float* db = dboxes + (p * Q + q) * 4;
            if (hit) {
                double a, c, d_l1[4], d_gl[4];
                box_pair(boxes + (p * Q + q) * 4, tgt_boxes + (long)(first + t) * 4, a, c, d_l1, d_gl);
                for (int i = 0; i < 4; ++i) db[i] = (float)(s_l1 * d_l1[i] + s_gl * d_gl[i]);
            } else {
                db[0] = db[1] = db[2] = db[3] = 0.0f;
            }
        }
    }
}

bool sizes_ok(int L, int B, int Q, int K) {
    if (L <= 0 || B <= 0 || Q <= 0 || K <= 0) return false;
    return (double)L * B * Q * (double)K < 9.0e15 && (long)L * B * ((Q + kRows - 1) / kRows) < INT_MAX;
}

}  // namespace

extern "C" {

int grit_lsa_f32(const float* cost, const int32_t* counts, const int32_t* rows, int P, int Q, int ld, int Tmax, int32_t* match_q,
                 int32_t* match_t, void* stream) {
    if (!cost || !counts || !match_q || P <= 0 || Q <= 0 || Tmax <= 0 || ld < Tmax) return GRIT_ERR_BAD_ARG;
    if (Q > kSide || Tmax > kSide) return GRIT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(lsa_kernel, dim3(P), dim3(kWave), 0, (hipStream_t)stream, cost, counts, rows, Q, (long)ld, Tmax, match_q,
                       match_t);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

int grit_det_match_f32(const float* logits, const float* boxes, const int64_t* tgt_labels, const float* tgt_boxes,
                       const int32_t* tgt_offsets, int L, int B, int Q, int K, int Tmax, float w_class, float w_bbox, float w_giou,
                       float* cost, int ld, int32_t* match_q, int32_t* match_t, void* stream) {
    if (!logits || !boxes || !tgt_labels || !tgt_boxes || !tgt_offsets || !cost || !match_q || !match_t) return GRIT_ERR_BAD_ARG;
    if (!sizes_ok(L, B, Q, K) || Tmax <= 0 || ld < Tmax) return GRIT_ERR_BAD_ARG;
    if (Q > kSide || Tmax > kSide) return GRIT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(det_match_kernel, dim3(L * B), dim3(kWave), 0, (hipStream_t)stream, logits, boxes, tgt_labels, tgt_boxes,
                       tgt_offsets, B, Q, K, Tmax, w_class, w_bbox, w_giou, cost, (long)ld, match_q, match_t);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

int grit_det_loss_fwd_f32(const float* logits, const float* boxes, const int64_t* tgt_labels, const float* tgt_boxes,
                          const int32_t* tgt_offsets, const int32_t* match_t, int L, int B, int Q, int K, float alpha,
                          const float* num_boxes, double* partials, unsigned int* ticket, float* out, void* stream) {
    if (!logits || !boxes || !tgt_labels || !tgt_boxes || !tgt_offsets || !match_t || !num_boxes || !partials || !ticket || !out)
        return GRIT_ERR_BAD_ARG;
    if (!sizes_ok(L, B, Q, K)) return GRIT_ERR_BAD_ARG;
    const int chunks = (Q + kRows - 1) / kRows;
    if (hipMemsetAsync(ticket, 0, sizeof(unsigned int), (hipStream_t)stream) != hipSuccess) return GRIT_ERR_LAUNCH;
    hipLaunchKernelGGL(det_loss_fwd_kernel, dim3(L * B * chunks), dim3(256), 0, (hipStream_t)stream, logits, boxes, tgt_labels, tgt_boxes,
                       tgt_offsets, match_t, L, B, Q, K, chunks, alpha, num_boxes, partials, ticket, out);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

int grit_det_loss_bwd_f32(const float* logits, const float* boxes, const int64_t* tgt_labels, const float* tgt_boxes,
                          const int32_t* tgt_offsets, const int32_t* match_t, int L, int B, int Q, int K, float alpha,
                          const float* num_boxes, const float* coef, int ldc, float* dlogits, float* dboxes, void* stream) {
    if (!logits || !boxes || !tgt_labels || !tgt_boxes || !tgt_offsets || !match_t || !num_boxes || !coef || !dlogits || !dboxes)
        return GRIT_ERR_BAD_ARG;
    if (!sizes_ok(L, B, Q, K) || ldc < 3) return GRIT_ERR_BAD_ARG;
    const int chunks = (Q + kRows - 1) / kRows;
    hipLaunchKernelGGL(det_loss_bwd_kernel, dim3(L * B * chunks), dim3(256), 0, (hipStream_t)stream, logits, boxes, tgt_labels, tgt_boxes,
                       tgt_offsets, match_t, B, Q, K, chunks, alpha, num_boxes, coef, ldc, dlogits, dboxes);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

}  // extern "C"
