// Detector evaluation (include/grit_hip.h, "Detector evaluation"): the selection of an image's best detections out of its
// [Q, K] logit map, and the per-image matching of detections to ground truth of the COCO box protocol.
//
// Selection.  The order wanted -- logit descending, flat index ascending -- is the descending order of ONE 64-bit key per element:
// the order-preserving integer image of the float in the high word, the complement of the index in the low word.  All keys of an
// image are distinct, so "the N best" is a set and every stage may emit it in any order; only the last one sorts.
//   stage 1  a workgroup per (chunk, image): radix select, 8 bits a pass, finds the chunk's N-th largest float image `thr` and
//            how many elements equal to it belong to the N best; everything above goes out through an LDS counter, the equal
//            ones in index order (a ballot prefix over tiles of 256), which is only walked when not all of them are wanted.
//   stage 2  a workgroup per image: bitonic sort of the <= 40 x 100 candidates in LDS, then logits, indices and boxes of the first N.
// Matching.  A workgroup per image.  A work item is (first detection of a category, area range, threshold): it walks that
// category's detections in order and, for each, the category's ground truths -- the regular ones first, the ignored ones after
// them, which is the stable "ignored last" order without a sort.  IoUs are computed on the fly (a [100, 512] float64 table does
// not fit in LDS).  "Ground truth g is taken at (range a, threshold t)" is bit t of an LDS word per (a, g): a bit has one writer.
// The Visual Genome protocol's matching (grit_det_voc_img, one threshold, no ignored rows) is described at its kernel below.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/grit_hip.h"

namespace {

constexpr int kTop = GRIT_DET_TOPK;
constexpr int kMaxChunks = GRIT_DET_TOPK_CHUNKS;
constexpr int kChunk = 8192;  // elements of a chunk at and below which its float images are kept in LDS after the first read
constexpr int kSortMax = 4096;  // >= kMaxChunks * kTop, a power of two
constexpr int kThreads = 256;
constexpr int kMergeThreads = 1024;  // one workgroup per image sorts and every step ends in a barrier: 256 threads took 158 us
constexpr int kWave = 64;
constexpr int kSide = GRIT_DET_MAX_SIDE;
constexpr int kMaxThr = 16;
constexpr int kMaxRng = 4;

static_assert(kMaxChunks * kTop <= kSortMax, "the merge sorts every candidate of an image in one LDS array");

__device__ inline uint32_t float_image(float x) {
    const uint32_t u = __float_as_uint(x);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ inline float image_float(uint32_t k) { return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }

__device__ inline uint64_t sort_key(uint32_t image, uint32_t index) { return ((uint64_t)image << 32) | (uint32_t)~index; }

__global__ __launch_bounds__(kThreads) void det_topk_chunk_kernel(const float* __restrict__ logits, int n, int chunk_len, int chunks,
                                                                  int N, uint64_t* __restrict__ cand) {
    __shared__ uint32_t s_image[kChunk];
    __shared__ unsigned int hist[256];
    __shared__ unsigned int wave_count[kThreads / kWave];
    __shared__ unsigned int s_prefix, s_remaining, s_equal, s_slot;
    const int chunk = blockIdx.x, b = blockIdx.y;
    const float* x = logits + (long)b * n;
    const long lo = (long)chunk * chunk_len;
    const int len = lo < n ? (int)min((long)chunk_len, (long)n - lo) : 0;
    uint64_t* out = cand + ((long)b * chunks + chunk) * N;
    if (len <= N) {  // the whole chunk; key 0 is below every real key (the low word of a real key has bit 31 set)
        for (int i = threadIdx.x; i < N; i += kThreads) out[i] = i < len ? sort_key(float_image(x[lo + i]), (uint32_t)(lo + i)) : 0;
        return;
    }
    const bool cached = len <= kChunk;
    if (cached)
        for (int i = threadIdx.x; i < len; i += kThreads) s_image[i] = float_image(x[lo + i]);
    auto image_at = [&](int i) { return cached ? s_image[i] : float_image(x[lo + i]); };
    uint32_t prefix = 0, remaining = N;
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;
        __syncthreads();
        const uint32_t high = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
        // logits of one map share sign and exponent: in the first pass nearly every element has the same digit, and 64 lanes
        // adding to one LDS word take 64 turns.  A thread therefore counts runs of equal digits and adds a run at a time.
        uint32_t run_digit = 0, run = 0;
        for (int i = threadIdx.x; i < len; i += kThreads) {
            const uint32_t k = image_at(i);
            if ((k & high) != prefix) continue;
            const uint32_t d = (k >> shift) & 255u;
            if (d != run_digit && run) {
                atomicAdd(&hist[run_digit], run);
                run = 0;
            }
            run_digit = d;
            ++run;
        }
        if (run) atomicAdd(&hist[run_digit], run);
        __syncthreads();
        if (threadIdx.x < kWave) {  // the digit that holds the `remaining`-th largest of the elements under the prefix
            const int lane = threadIdx.x;  // owns the digits 4 lane .. 4 lane + 3
            const uint32_t h0 = hist[4 * lane], h1 = hist[4 * lane + 1], h2 = hist[4 * lane + 2], h3 = hist[4 * lane + 3];
            const uint32_t own = h0 + h1 + h2 + h3;
            uint32_t suffix = own;  // own + the counts of every higher lane
            for (int off = 1; off < kWave; off <<= 1) {
                const uint32_t o = __shfl_down(suffix, off, kWave);
                if (lane + off < kWave) suffix += o;
            }
            uint32_t above = suffix - own;
            if (above < remaining && remaining <= suffix) {  // exactly one lane: the elements under the prefix are >= remaining
                int d = 3;
                uint32_t h = h3;
                if (above + h3 < remaining) {
                    above += h3, d = 2, h = h2;
                    if (above + h2 < remaining) {
                        above += h2, d = 1, h = h1;
                        if (above + h1 < remaining) above += h1, d = 0, h = h0;
                    }
                }
                s_prefix = prefix | ((uint32_t)(4 * lane + d) << shift);
                s_remaining = remaining - above;
                s_equal = h;
            }
            if (lane == 0) s_slot = 0;
        }
        __syncthreads();
        prefix = s_prefix;
        remaining = s_remaining;
    }
    const uint32_t thr = prefix, above = N - remaining;  // `above` elements are larger, `remaining` of the s_equal equal ones are wanted
    const bool all_equal_wanted = s_equal == remaining;
    for (int i = threadIdx.x; i < len; i += kThreads) {
        const uint32_t k = image_at(i);
        if (k > thr || (all_equal_wanted && k == thr)) {
            const unsigned int slot = atomicAdd(&s_slot, 1u);
            if (slot < (unsigned int)N) out[slot] = sort_key(k, (uint32_t)(lo + i));
        }
    }
    if (all_equal_wanted) return;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    uint32_t taken = 0;  // the same in every thread
    for (int first = 0; first < len && taken < remaining; first += kThreads) {
        const int i = first + threadIdx.x;
        const bool equal = i < len && image_at(i) == thr;
        const unsigned long long votes = __ballot(equal);
        if (lane == 0) wave_count[wave] = (unsigned int)__popcll(votes);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < kThreads / kWave; ++w) {
            const uint32_t c = wave_count[w];
            before += w < wave ? c : 0u;
            total += c;
        }
        const uint32_t rank = taken + before + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
        if (equal && rank < remaining) out[above + rank] = sort_key(thr, (uint32_t)(lo + i));
        taken += total;
        __syncthreads();
    }
}

// The composition's fp32 arithmetic, operation for operation: (centre -/+ 0.5 * size) * extent.
__device__ inline void corner_box(const float* __restrict__ box, float height, float width, float* __restrict__ out) {
#pragma clang fp contract(off)
    const float cx = box[0], cy = box[1], w = box[2], h = box[3];
    out[0] = (cx - 0.5f * w) * width;
    out[1] = (cy - 0.5f * h) * height;
    out[2] = (cx + 0.5f * w) * width;
    out[3] = (cy + 0.5f * h) * height;
}

__global__ __launch_bounds__(kMergeThreads) void det_topk_merge_kernel(const uint64_t* __restrict__ cand, int count, int padded, int N,
                                                                  const float* __restrict__ boxes, const float* __restrict__ sizes, int Q,
                                                                  int K, float* __restrict__ top_logit, int32_t* __restrict__ top_index,
                                                                  float* __restrict__ out_boxes) {
    __shared__ uint64_t keys[kSortMax];
    const long b = blockIdx.x;
    for (int i = threadIdx.x; i < padded; i += kMergeThreads) keys[i] = i < count ? cand[b * count + i] : 0;
    __syncthreads();
    for (int k = 2; k <= padded; k <<= 1) {  // bitonic, descending
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < padded; i += kMergeThreads) {
                const int p = i ^ j;
                if (p > i) {
                    const uint64_t a = keys[i], c = keys[p];
                    if (((i & k) == 0) ? a < c : a > c) {
                        keys[i] = c;
                        keys[p] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int r = threadIdx.x; r < N; r += kMergeThreads) {
        const uint64_t key = keys[r];
        const uint32_t index = ~(uint32_t)key;
        const int q = min((int)(index / (uint32_t)K), Q - 1);  // a real key's index is below Q * K; the clamp is for key 0 only
        top_logit[b * N + r] = image_float((uint32_t)(key >> 32));
        top_index[b * N + r] = (int32_t)index;
        corner_box(boxes + (b * Q + q) * 4, sizes[b * 2], sizes[b * 2 + 1], out_boxes + (b * N + r) * 4);
    }
}

// ---- per-image evaluation ---------------------------------------------------------------------------------------------------------

// Box IoU of the COCO API (bbIou) on (x, y, w, h) boxes, in its order of operations.
__device__ inline double box_iou(const double* __restrict__ d, const double* __restrict__ g, bool crowd) {
#pragma clang fp contract(off)
    double w = fmin(d[2] + d[0], g[2] + g[0]) - fmax(d[0], g[0]);
    if (w <= 0.0) w = 0.0;
    double h = fmin(d[3] + d[1], g[3] + g[1]) - fmax(d[1], g[1]);
    if (h <= 0.0) h = 0.0;
    const double i = w * h;
    const double u = crowd ? d[2] * d[3] : d[2] * d[3] + g[2] * g[3] - i;
    return i / u;
}

__global__ __launch_bounds__(kThreads) void det_eval_img_kernel(const float* __restrict__ scores, const int64_t* __restrict__ labels,
                                                                const float* __restrict__ boxes, const int32_t* __restrict__ slot, int N,
                                                                grit_det_gt gt, const double* __restrict__ iou_thr, int T,
                                                                const double* __restrict__ area_rng, int A, uint32_t* __restrict__ rec_flags,
                                                                int32_t* __restrict__ rec_rank, float* __restrict__ rec_score,
                                                                int32_t* __restrict__ rec_label, uint8_t* __restrict__ seen) {
    __shared__ double s_box[kTop][4];
    __shared__ double s_thr[kMaxThr], s_rng[kMaxRng][2];
    __shared__ int s_label[kTop], s_rank[kTop], s_gt_first[kTop], s_gt_end[kTop];
    __shared__ unsigned int s_flags[kTop][kMaxRng];
    __shared__ unsigned int s_taken[kMaxRng][kSide];
    const long b = blockIdx.x;
    const int img = slot[b];
    if (img < 0 || img >= gt.n_img) return;
    const int first = gt.img_off[img], G = gt.img_off[img + 1] - first;
    if (first < 0 || G < 0 || G > kSide) return;
    for (int n = threadIdx.x; n < N; n += kThreads) {
#pragma clang fp contract(off)
        const int64_t label = labels[b * N + n];
        s_label[n] = label >= 0 && label < gt.n_cat && gt.cat_valid[label] ? (int)label : -1;
        const float* c = boxes + (b * N + n) * 4;
        s_box[n][0] = (double)c[0];
        s_box[n][1] = (double)c[1];
        s_box[n][2] = (double)(c[2] - c[0]);
        s_box[n][3] = (double)(c[3] - c[1]);
        for (int a = 0; a < kMaxRng; ++a) s_flags[n][a] = 0;
    }
    for (int i = threadIdx.x; i < kMaxRng * kSide; i += kThreads) (&s_taken[0][0])[i] = 0;
    if (threadIdx.x < T) s_thr[threadIdx.x] = fmin(iou_thr[threadIdx.x], 1.0 - 1e-10);
    if (threadIdx.x < 2 * A) (&s_rng[0][0])[threadIdx.x] = area_rng[threadIdx.x];
    __syncthreads();
    for (int n = threadIdx.x; n < N; n += kThreads) {
        const int label = s_label[n];
        int rank = -1, lo = 0, hi = 0;
        if (label >= 0) {
            rank = 0;
            for (int m = 0; m < n; ++m) rank += s_label[m] == label;
            const int32_t* cat = gt.cat + first;  // sorted within the image
            int l = 0, r = G;
            while (l < r) {
                const int mid = (l + r) >> 1;
                if (cat[mid] < label) l = mid + 1; else r = mid;
            }
            lo = l;
            r = G;
            while (l < r) {
                const int mid = (l + r) >> 1;
                if (cat[mid] <= label) l = mid + 1; else r = mid;
            }
            hi = l;
        }
        s_rank[n] = rank;
        s_gt_first[n] = lo;
        s_gt_end[n] = hi;
    }
    __syncthreads();
    const int items = N * A * T;
    for (int item = threadIdx.x; item < items; item += kThreads) {
        const int t = item % T, a = (item / T) % A, n = item / (T * A);
        if (s_rank[n] != 0) continue;  // the first detection of a category carries the category
        const int label = s_label[n], g_first = s_gt_first[n], g_end = s_gt_end[n];
        const double area_lo = s_rng[a][0], area_hi = s_rng[a][1], thr = s_thr[t];
        const unsigned int bit = 1u << t;
        for (int m = n; m < N; ++m) {
            if (s_label[m] != label) continue;
            const double* d = s_box[m];
            double best = thr;
            int match = -1;
            bool match_ignored = false;
            for (int g = g_first; g < g_end; ++g) {  // the regular ground truths: a taken one is skipped
                const double ga = gt.area[first + g];
                if (gt.crowd[first + g] || ga < area_lo || ga > area_hi) continue;
                if (s_taken[a][g] & bit) continue;
                const double iou = box_iou(d, gt.box + (long)(first + g) * 4, false);
                if (iou < best) continue;
                best = iou;
                match = g;
            }
            if (match < 0) {  // the walk goes on into the ignored ones only while nothing regular is held
                for (int g = g_first; g < g_end; ++g) {
                    const double ga = gt.area[first + g];
                    const bool crowd = gt.crowd[first + g] != 0;
                    if (!(crowd || ga < area_lo || ga > area_hi)) continue;
                    if ((s_taken[a][g] & bit) && !crowd) continue;
                    const double iou = box_iou(d, gt.box + (long)(first + g) * 4, crowd);
                    if (iou < best) continue;
                    best = iou;
                    match = g;
                    match_ignored = true;
                }
            }
            if (match >= 0) {
                atomicOr(&s_taken[a][match], bit);
                atomicOr(&s_flags[m][a], match_ignored ? bit | (bit << 16) : bit);
            } else {
                const double area = d[2] * d[3];
                if (area < area_lo || area > area_hi) atomicOr(&s_flags[m][a], bit << 16);
            }
        }
    }
    __syncthreads();
    for (int n = threadIdx.x; n < N; n += kThreads) {
        const long row = (long)img * N + n;
        rec_rank[row] = s_rank[n];
        rec_score[row] = scores[b * N + n];
        rec_label[row] = (int32_t)labels[b * N + n];
        for (int a = 0; a < A; ++a) rec_flags[row * A + a] = s_flags[n][a];
    }
    if (threadIdx.x == 0) seen[img] = 1;
}

// ---- per-image matching of the Visual Genome protocol (PASCAL VOC at one threshold) --------------------------------------------

// Overlap of a detection's corners d and a ground-truth row g (x, y, w, h), both with the protocol's +1 pixel convention.
__device__ inline double voc_overlap(const double* __restrict__ d, const double* __restrict__ g) {
#pragma clang fp contract(off)
    const double g2 = g[0] + g[2], g3 = g[1] + g[3];
    const double iw = fmax(fmin(g2, d[2]) - fmax(g[0], d[0]) + 1.0, 0.0);
    const double ih = fmax(fmin(g3, d[3]) - fmax(g[1], d[1]) + 1.0, 0.0);
    const double inters = iw * ih;
    const double uni = (d[2] - d[0] + 1.0) * (d[3] - d[1] + 1.0) + (g2 - g[0] + 1.0) * (g3 - g[1] + 1.0) - inters;
    return inters / uni;
}

// A thread per detection finds (ovmax, jmax) over its class's rows -- independent of every other detection.  "True positive or
// duplicate" is then whether an earlier detection of the class holds the same row above the threshold: a first-occurrence test on
// the LDS copies, no state carried from detection to detection.
__global__ __launch_bounds__(kThreads) void det_voc_img_kernel(const float* __restrict__ scores, const int64_t* __restrict__ labels,
                                                               const float* __restrict__ boxes, const int32_t* __restrict__ slot, int N,
                                                               grit_det_gt gt, double thr, uint8_t* __restrict__ rec_flag,
                                                               int32_t* __restrict__ rec_gt, double* __restrict__ rec_iou,
                                                               float* __restrict__ rec_score, int32_t* __restrict__ rec_label,
                                                               uint8_t* __restrict__ seen) {
    __shared__ double s_ov[kTop];
    __shared__ int s_label[kTop], s_j[kTop];
    const long b = blockIdx.x;
    const int img = slot[b];
    if (img < 0 || img >= gt.n_img) return;
    const int first = gt.img_off[img], G = gt.img_off[img + 1] - first;
    if (first < 0 || G < 0 || G > kSide) return;
    for (int n = threadIdx.x; n < N; n += kThreads) {
        const int64_t wide = labels[b * N + n];
        const int label = wide >= 0 && wide < gt.n_cat && gt.cat_valid[wide] ? (int)wide : -1;
        double ovmax = -INFINITY;
        int jmax = -1;
        if (label >= 0) {
            const int32_t* cat = gt.cat + first;  // sorted within the image
            int l = 0, r = G;
            while (l < r) {
                const int mid = (l + r) >> 1;
                if (cat[mid] < label) l = mid + 1; else r = mid;
            }
            const float* c = boxes + (b * N + n) * 4;
            const double d[4] = {(double)c[0], (double)c[1], (double)c[2], (double)c[3]};
            for (int g = l; g < G && cat[g] == label; ++g) {
                const double ov = voc_overlap(d, gt.box + (long)(first + g) * 4);
                if (ov > ovmax) {  // strictly: the first row of the largest overlap stays
                    ovmax = ov;
                    jmax = g;
                }
            }
        }
        s_label[n] = label;
        s_ov[n] = ovmax;
        s_j[n] = jmax;
    }
    __syncthreads();
    for (int n = threadIdx.x; n < N; n += kThreads) {
        const int label = s_label[n], jmax = s_j[n];
        const double ovmax = s_ov[n];
        int flag = 0;
        if (label >= 0) {
            flag = 2;
            if (ovmax > thr) {
                flag = 1;
                for (int m = 0; m < n; ++m)
                    if (s_label[m] == label && s_j[m] == jmax && s_ov[m] > thr) flag = 3;
            }
        }
        const long row = (long)img * N + n;
        rec_flag[row] = (uint8_t)flag;
        rec_gt[row] = jmax;
        rec_iou[row] = ovmax;
        rec_score[row] = scores[b * N + n];
        rec_label[row] = (int32_t)labels[b * N + n];
    }
    if (threadIdx.x == 0) seen[img] = 1;
}

}  // namespace

extern "C" {

int grit_det_topk_f32(const float* logits, const float* boxes, const float* sizes, int B, int Q, int K, uint64_t* work,
                      float* top_logit, int32_t* top_index, float* out_boxes, void* stream) {
    if (!logits || !boxes || !sizes || !work || !top_logit || !top_index || !out_boxes) return GRIT_ERR_BAD_ARG;
    if (B <= 0 || B > 65535 || Q <= 0 || K <= 0 || (long)Q * K >= (1L << 31)) return GRIT_ERR_BAD_ARG;
    const int n = Q * K, N = n < kTop ? n : kTop;
    int chunks = (n + kChunk - 1) / kChunk;
    if (chunks > kMaxChunks) chunks = kMaxChunks;
    const int chunk_len = (int)(((long)n + chunks - 1) / chunks);
    const int count = chunks * N;
    int padded = 1;
    while (padded < count) padded <<= 1;
    hipLaunchKernelGGL(det_topk_chunk_kernel, dim3(chunks, B), dim3(kThreads), 0, (hipStream_t)stream, logits, n, chunk_len, chunks, N,
                       work);
    hipLaunchKernelGGL(det_topk_merge_kernel, dim3(B), dim3(kMergeThreads), 0, (hipStream_t)stream, (const uint64_t*)work, count, padded, N,
                       boxes, sizes, Q, K, top_logit, top_index, out_boxes);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

int grit_det_eval_img(const float* scores, const int64_t* labels, const float* boxes, const int32_t* slot, int B, int N,
                      const grit_det_gt* gt, const double* iou_thr, int T, const double* area_rng, int A, uint32_t* rec_flags,
                      int32_t* rec_rank, float* rec_score, int32_t* rec_label, uint8_t* seen, void* stream) {
    if (!scores || !labels || !boxes || !slot || !gt || !iou_thr || !area_rng || !rec_flags || !rec_rank || !rec_score || !rec_label || !seen)
        return GRIT_ERR_BAD_ARG;
    if (!gt->img_off || !gt->box || !gt->area || !gt->cat || !gt->crowd || !gt->cat_valid || gt->n_img <= 0 || gt->n_cat <= 0)
        return GRIT_ERR_BAD_ARG;
    if (B <= 0 || N <= 0 || N > kTop || T <= 0 || T > kMaxThr || A <= 0 || A > kMaxRng) return GRIT_ERR_BAD_ARG;
    if (gt->max_per_img > kSide) return GRIT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(det_eval_img_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, scores, labels, boxes, slot, N, *gt, iou_thr,
                       T, area_rng, A, rec_flags, rec_rank, rec_score, rec_label, seen);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

int grit_det_voc_img(const float* scores, const int64_t* labels, const float* boxes, const int32_t* slot, int B, int N,
                     const grit_det_gt* gt, double iou_thr, uint8_t* rec_flag, int32_t* rec_gt, double* rec_iou, float* rec_score,
                     int32_t* rec_label, uint8_t* seen, void* stream) {
    if (!scores || !labels || !boxes || !slot || !gt || !rec_flag || !rec_gt || !rec_iou || !rec_score || !rec_label || !seen)
        return GRIT_ERR_BAD_ARG;
    if (!gt->img_off || !gt->box || !gt->cat || !gt->cat_valid || gt->n_img <= 0 || gt->n_cat <= 0) return GRIT_ERR_BAD_ARG;
    if (B <= 0 || N <= 0 || N > kTop || iou_thr != iou_thr) return GRIT_ERR_BAD_ARG;
    if (gt->max_per_img > kSide) return GRIT_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(det_voc_img_kernel, dim3(B), dim3(kThreads), 0, (hipStream_t)stream, scores, labels, boxes, slot, N, *gt, iou_thr,
                       rec_flag, rec_gt, rec_iou, rec_score, rec_label, seen);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

}  // extern "C"
