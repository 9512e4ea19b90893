// Detector pre-training on the flat bf16-compute / fp32-master layout (grit_amd/amp.py): the two streaming kernels the step around
// the device matcher and criterion needs (reference train_detector.py:24-89, engine/det_solver.py:108).
//
// grit_grad_norm_flat: the global L2 norm of the gradients as they lie in the flat buckets (the sum over the ranks), and from it the
//   factor torch.nn.utils.clip_grad_norm_ would multiply every gradient by -- on the device, never read back:
//     total_norm = float(grad_scale * sqrt(sum g^2))          squares and sums in float64
//     clip_coef  = min(1, max_norm / (total_norm + 1e-6))     fp32, torch's expression (a NaN stays a NaN)
//     clip_scale = grad_scale * clip_coef                     what grit_adamw_flat_dev multiplies every gradient element by
//   One pass over 2 B (bf16) per parameter with 16-byte loads.  Every thread owns a fixed set of elements and adds them in a fixed
//   order, a workgroup reduces in a fixed order to ONE float64 partial, and the workgroup that takes the last ticket adds the
//   partials in index order: the result does not depend on the order in which workgroups ran, two calls give identical bits.
//
// grit_adamw_flat_dev: adam_flat (adam_flat.h) behind p <- p * (1 - lr * weight_decay), with the gradient factor taken from the clip cell.
#include "adam_flat.h"

namespace {

struct NormTable {
    grit_norm_range r[GRIT_NORM_MAX_RANGES];
};

__device__ __forceinline__ double add_sq(double acc, float x) {
    const double d = (double)x;
    return fma(d, d, acc);
}
__device__ __forceinline__ double add_sq_bf16x2(double acc, unsigned int u) {
    return add_sq(add_sq(acc, __uint_as_float(u << 16)), __uint_as_float(u & 0xffff0000u));
}

// One 16-byte unit: 8 bf16 or 4 fp32 elements.
template <bool BF16> __device__ __forceinline__ double add_sq_unit(double acc, const uint4* q) {
    const uint4 u = *q;
    if constexpr (BF16) {
        return add_sq_bf16x2(add_sq_bf16x2(add_sq_bf16x2(add_sq_bf16x2(acc, u.x), u.y), u.z), u.w);
    } else {
        return add_sq(add_sq(add_sq(add_sq(acc, __uint_as_float(u.x)), __uint_as_float(u.y)), __uint_as_float(u.z)),
                      __uint_as_float(u.w));
    }
}

// Workgroup b of launch l writes partials[row_base + b].  finalize != 0 (the last launch of a call): the workgroup that takes the
// last ticket adds partials[0 .. total_rows) -- the rows of the earlier launches of the chain are complete, the stream orders them.
template <bool BF16>
__global__ __launch_bounds__(256)
void grad_norm_flat(const NormTable tab, int n_ranges, int row_base, int total_rows, int finalize, float grad_scale, float max_norm,
                    double* partials, unsigned int* ticket, float* __restrict__ out) {
    __shared__ double red[256];
    __shared__ int is_last;
    const long stride = (long)gridDim.x * 256;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    double acc0 = 0.0, acc1 = 0.0;
    for (int r = 0; r < n_ranges; ++r) {
        const char* base = (const char*)tab.r[r].grad;
        long units = tab.r[r].n / (BF16 ? 8 : 4);
        if constexpr (BF16) {
            // quads of bf16 are 8-byte aligned: a range that starts on an odd quad gives up its first one, a range that then holds an
            // odd number of quads its last one; thread 0 of the grid takes them with 8-byte loads
            const long n4 = tab.r[r].n / 4;
            const long head = ((uintptr_t)base & 8) ? 1 : 0;
            units = (n4 - head) >> 1;
            if (gid == 0) {
                if (head) {
                    const uint2 u = *reinterpret_cast<const uint2*>(base);
                    acc1 = add_sq_bf16x2(add_sq_bf16x2(acc1, u.x), u.y);
                }
                if ((n4 - head) & 1) {
                    const uint2 u = *reinterpret_cast<const uint2*>(base + 8 * (n4 - 1));
                    acc1 = add_sq_bf16x2(add_sq_bf16x2(acc1, u.x), u.y);
                }
            }
            base += 8 * head;
        }
        const uint4* q = reinterpret_cast<const uint4*>(base);
        long i = gid;
        for (; i + stride < units; i += 2 * stride) {  // two 16-byte loads in flight per thread and trip
            const uint4* q0 = q + i;
            const uint4* q1 = q + i + stride;
            const double a = add_sq_unit<BF16>(0.0, q0);
            const double b = add_sq_unit<BF16>(0.0, q1);
            acc0 += a;
            acc1 += b;
        }
        if (i < units) acc0 = add_sq_unit<BF16>(acc0, q + i);
    }
    // workgroup sum in a fixed order: a tree over the 256 threads
    red[threadIdx.x] = acc0 + acc1;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[row_base + blockIdx.x] = red[0];
    if (!finalize) return;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) is_last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    // thread t adds its contiguous share of the rows in index order, thread 0 then adds the 256 shares in index order
    const volatile double* part = partials;
    const int per = (total_rows + 255) / 256;
    double s = 0.0;
    for (int k = threadIdx.x * per; k < (threadIdx.x + 1) * per && k < total_rows; ++k) s += part[k];
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum = 0.0;
        for (int t = 0; t < 256; ++t) sum += red[t];
        const float total = (float)((double)grad_scale * sqrt(sum));
        const float q = max_norm / (total + 1e-6f);
        const float coef = q > 1.0f ? 1.0f : q;  // torch.clamp(max = 1): a NaN stays
        out[0] = total;
        out[1] = grad_scale * coef;
        out[2] = coef;
    }
}

}  // namespace

extern "C" int grit_grad_norm_flat(const grit_norm_range* ranges, int n_ranges, int grad_is_bf16, float grad_scale, float max_norm,
                                   double* partials, unsigned int* ticket, float* out, void* stream) {
    if (!ranges || n_ranges <= 0 || !partials || !ticket || !out || !(max_norm >= 0.f)) return GRIT_ERR_BAD_ARG;
    for (int r = 0; r < n_ranges; ++r)
        if (!ranges[r].grad || ranges[r].n <= 0) return GRIT_ERR_BAD_ARG;
    for (int r = 0; r < n_ranges; ++r)
        if (ranges[r].n % 4 != 0 || ((uintptr_t)ranges[r].grad % (grad_is_bf16 ? 8 : 16)) != 0) return GRIT_ERR_UNSUPPORTED;
    const int launches = (n_ranges + GRIT_NORM_MAX_RANGES - 1) / GRIT_NORM_MAX_RANGES;
    // the grid of every launch first: the last one is told how many rows the chain wrote
    int total_rows = 0;
    for (int l = 0; l < launches; ++l) {
        const int first = l * GRIT_NORM_MAX_RANGES;
        const int count = n_ranges - first < GRIT_NORM_MAX_RANGES ? n_ranges - first : GRIT_NORM_MAX_RANGES;
        long longest = 0;
        for (int r = 0; r < count; ++r) {
            const long units = (ranges[first + r].n + (grad_is_bf16 ? 7 : 3)) / (grad_is_bf16 ? 8 : 4);
            if (units > longest) longest = units;
        }
        long blocks = (longest + 255) / 256;
        if (blocks > GRIT_NORM_BLOCK_CAP) blocks = GRIT_NORM_BLOCK_CAP;
        total_rows += (int)blocks;
    }
    if (hipMemsetAsync(ticket, 0, sizeof(unsigned int), (hipStream_t)stream) != hipSuccess) return GRIT_ERR_LAUNCH;
    int row_base = 0;
    for (int l = 0; l < launches; ++l) {
        const int first = l * GRIT_NORM_MAX_RANGES;
        const int count = n_ranges - first < GRIT_NORM_MAX_RANGES ? n_ranges - first : GRIT_NORM_MAX_RANGES;
        NormTable tab;
        long longest = 0;
        for (int r = 0; r < GRIT_NORM_MAX_RANGES; ++r) {
            tab.r[r].grad = r < count ? ranges[first + r].grad : nullptr;
            tab.r[r].n = r < count ? ranges[first + r].n : 0;
            const long units = (tab.r[r].n + (grad_is_bf16 ? 7 : 3)) / (grad_is_bf16 ? 8 : 4);
            if (units > longest) longest = units;
        }
        long blocks = (longest + 255) / 256;
        if (blocks > GRIT_NORM_BLOCK_CAP) blocks = GRIT_NORM_BLOCK_CAP;
        const int finalize = l == launches - 1;
        if (grad_is_bf16)
            hipLaunchKernelGGL(grad_norm_flat<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tab, count, row_base,
                               total_rows, finalize, grad_scale, max_norm, partials, ticket, out);
        else
            hipLaunchKernelGGL(grad_norm_flat<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tab, count, row_base,
                               total_rows, finalize, grad_scale, max_norm, partials, ticket, out);
        if (hipGetLastError() != hipSuccess) return GRIT_ERR_LAUNCH;
        row_base += (int)blocks;
    }
    return GRIT_OK;
}

extern "C" int grit_adamw_flat_dev(float* param, const void* grad, int grad_is_bf16, float* exp_avg, float* exp_avg_sq,
                                   void* compute_bf16, long n, float beta1, float beta2, float eps, float grad_scale,
                                   const float* hyper, const float* clip_scale, void* stream) {
    if (!hyper || ((uintptr_t)hyper % 16) || ((uintptr_t)clip_scale % 4)) return GRIT_ERR_BAD_ARG;
    return adam_launch<true>(param, grad, grad_is_bf16, exp_avg, exp_avg_sq, compute_bf16, n, 0.f, beta1, beta2, eps, 1.f, 1.f,
                             grad_scale, hyper, clip_scale, stream);
}
