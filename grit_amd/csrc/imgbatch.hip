// Image side of the batch contract on the device: decoded RGB uint8 images of different sizes ->
//   Pillow-exact bicubic resize -> ToTensor (/255) -> Normalize ((x - mean) / std) -> zero-padded [B,3,H,W] f32 + mask.
// Replaces the per-image host chain of the reference (datasets/caption/transforms/utils.py:4-45,
// transforms/__init__.py:6-32, engine/utils.py:278-295) by two launches per batch.
//
// Arithmetic is Pillow's (src/libImaging/Resample.c, 8 bits per channel): per axis a table of (first tap, tap count,
// taps in 22-bit fixed point) built in double precision on the host (grit_resample_taps_bicubic below), a horizontal
// pass into a uint8 intermediate, a vertical pass, each output = clamp((2^21 + sum tap * pixel) >> 22).  All integer,
// so the result is bit-identical to Image.resize(..., BICUBIC); the float stage is a 3 x 256 lookup table computed by
// the caller with the framework's own float ops.
//
// Both kernels are byte streams: pass 1 reads 3*h*w and writes 3*h*ow bytes per image, pass 2 reads 3*h*ow and writes
// 13*H*W (three f32 planes + the mask).  Tap tables are a few KB per image and stay in L2.  The intermediate keeps
// dword-aligned rows (pitch = 3*ow rounded up to 4) so that pass 2 reads it four bytes at a time.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/grit_hip.h"

namespace {

constexpr int kPrecisionBits = 22;

struct ImageDesc {  // one row of the int64 descriptor table, see grit_hip.h
    int64_t src_off, src_h, src_w, dst_h, dst_w, kx, ky, xb_off, xt_off, yb_off, yt_off, tmp_off;
};
static_assert(sizeof(ImageDesc) == GRIT_IMAGE_DESC_FIELDS * sizeof(int64_t), "descriptor layout");

constexpr int kRows = 4;  // source rows per thread in the horizontal pass

__host__ __device__ __forceinline__ int tmp_pitch(int dst_w) { return (3 * dst_w + 3) & ~3; }  // bytes, dword-aligned rows

__device__ __forceinline__ uint8_t clip8(int v) {
    v >>= kPrecisionBits;
    return (uint8_t)min(max(v, 0), 255);
}

// pass 1, generic: one thread per output byte (pixel x, channel c) of one source row; any tap count
__global__ __launch_bounds__(256)
void resample_rows_any(const uint8_t* __restrict__ src, const ImageDesc* __restrict__ desc,
                       const int32_t* __restrict__ tables, uint8_t* __restrict__ tmp) {
    const ImageDesc d = desc[blockIdx.z];
    const int y = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;  // byte within the output row
    const int ow = (int)d.dst_w, w = (int)d.src_w;
    if (y >= d.src_h || j >= ow * 3) return;
    const int xx = j / 3, c = j - xx * 3;
    const int2 b = *reinterpret_cast<const int2*>(tables + d.xb_off + 2 * xx);
    const int32_t* __restrict__ k = tables + d.xt_off + (int64_t)xx * d.kx;
    const uint8_t* __restrict__ p = src + d.src_off + ((int64_t)y * w + b.x) * 3 + c;
    int ss = 1 << (kPrecisionBits - 1);
    for (int x = 0; x < b.y; ++x) ss += (int)p[3 * x] * k[x];
    tmp[d.tmp_off + (int64_t)y * tmp_pitch(ow) + j] = clip8(ss);
}

// pass 1, up to K taps (K = 7 covers every scale <= 1.25 incl. all upscaling, K = 9 scales <= 2, K = 13 scales <= 3): one thread per output
// pixel and kRows consecutive source rows.  The taps (shared by the rows) sit in registers; the 3*K source bytes of a
// pixel-row are fetched as aligned dwords and shifted into place (v_alignbyte) instead of 3*K byte loads.  Bytes read
// beyond the tap count meet zero taps; the caller pads the blob so that they stay readable.
template <int K>
__global__ __launch_bounds__(256)
void resample_rows_k(const uint8_t* __restrict__ src, const ImageDesc* __restrict__ desc,
                     const int32_t* __restrict__ tables, uint8_t* __restrict__ tmp) {
    constexpr int kWords = (3 * K + 3) / 4;  // realigned dwords holding the 3*K bytes
    __shared__ uint32_t packed[4][kRows][48];  // per wave: the 64 pixels x 3 bytes of each row, re-read as 48 dwords
    const ImageDesc d = desc[blockIdx.z];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x_wave = blockIdx.x * 256 + wave * 64;  // first output pixel of this wave
    const int y0 = blockIdx.y * kRows;
    const int ow = (int)d.dst_w, w = (int)d.src_w, h = (int)d.src_h, kx = (int)d.kx;
    if (y0 >= h || x_wave >= ow) return;  // wave-uniform
    const int xx = min(x_wave + lane, ow - 1);  // lanes past the row end repeat the last pixel; their bytes are not stored
    const int first = tables[d.xb_off + 2 * xx];
    const int32_t* __restrict__ k = tables + d.xt_off + (int64_t)xx * kx;
    int tap[K];
#pragma unroll
    for (int t = 0; t < K; ++t) tap[t] = t < kx ? k[t] : 0;  // table rows are zero past the tap count
    const int pitch = tmp_pitch(ow);
    uint8_t* __restrict__ staged = reinterpret_cast<uint8_t*>(&packed[wave][0][0]);
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int y = min(y0 + r, h - 1);
        const int64_t a = d.src_off + ((int64_t)y * w + first) * 3;
        const uint32_t* __restrict__ q = reinterpret_cast<const uint32_t*>(src + (a & ~(int64_t)3));
        const uint32_t shift = (uint32_t)(a & 3);
        uint32_t raw[kWords + 1], word[kWords];
#pragma unroll
        for (int i = 0; i <= kWords; ++i) raw[i] = q[i];
#pragma unroll
        for (int i = 0; i < kWords; ++i) word[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], shift);
        int s[3] = {1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1)};
#pragma unroll
        for (int t = 0; t < K; ++t)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int j = 3 * t + c;
                s[c] += __mul24((int)((word[j >> 2] >> (8 * (j & 3))) & 0xffu), tap[t]);
            }
        uint8_t* __restrict__ o = staged + r * 192 + 3 * lane;
        o[0] = clip8(s[0]); o[1] = clip8(s[1]); o[2] = clip8(s[2]);
    }
    // the wave's own LDS rows: no barrier needed beyond the wave's program order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int byte0 = 3 * x_wave + 4 * lane;  // byte of the output row this lane's dword starts at (x_wave*3 % 4 == 0)
    if (lane < 48 && byte0 < pitch) {
#pragma unroll
        for (int r = 0; r < kRows; ++r)
            if (y0 + r < h)
                *reinterpret_cast<uint32_t*>(tmp + d.tmp_off + (int64_t)(y0 + r) * pitch + byte0) = packed[wave][r][lane];
    }
}

// pass 2: one thread per 4 consecutive pixels (12 bytes = 3 aligned dwords of the intermediate row; the taps of a row are
// wave-uniform): vertical taps, lookup, one float4 store per colour plane, 4 mask bytes, zero padding.
__global__ __launch_bounds__(256)
void resample_cols_normalize(const uint8_t* __restrict__ tmp, const ImageDesc* __restrict__ desc,
                             const int32_t* __restrict__ tables, const float* __restrict__ lut, int out_h, int out_w,
                             float* __restrict__ out, uint8_t* __restrict__ mask) {
    __shared__ float table[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += 256) table[i] = lut[i];
    __syncthreads();
    const ImageDesc d = desc[blockIdx.z];
    // Workgroups go to the 8 XCDs round-robin in launch order and every XCD has its own L2.  Neighbouring output rows
    // share most of their source rows, so each XCD gets one contiguous band of rows (gridDim.y is a multiple of 8 when
    // the grid is one workgroup wide) instead of every eighth row -- otherwise each L2 fetches the whole intermediate.
    int yy = blockIdx.y;
    if (gridDim.x == 1) yy = (yy & 7) * (gridDim.y >> 3) + (yy >> 3);
    const int px0 = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (yy >= out_h || px0 >= out_w) return;
    const int ow = (int)d.dst_w, pitch = tmp_pitch(ow);
    int s[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = 1 << (kPrecisionBits - 1);
    const bool inside = yy < d.dst_h && px0 < ow;
    if (inside) {
        const int first = tables[d.yb_off + 2 * yy], count = tables[d.yb_off + 2 * yy + 1];
        const int32_t* __restrict__ k = tables + d.yt_off + (int64_t)yy * d.ky;
        const uint8_t* __restrict__ p = tmp + d.tmp_off + (int64_t)first * pitch + 3 * px0;
        // the last pixels of a row may reach past the pitch: read only the dwords that belong to the row
        const int words = min(3, (pitch - 3 * px0) >> 2);
        for (int y = 0; y < count; ++y) {
            const uint32_t* __restrict__ q = reinterpret_cast<const uint32_t*>(p);
            uint32_t v[3];
            v[0] = q[0];
            v[1] = words > 1 ? q[1] : 0u;
            v[2] = words > 2 ? q[2] : 0u;
            const int t = k[y];
#pragma unroll
            for (int i = 0; i < 12; ++i) s[i] += __mul24((int)((v[i >> 2] >> (8 * (i & 3))) & 0xffu), t);
            p += pitch;
        }
    }
    const int64_t plane = (int64_t)out_h * out_w;
    float* __restrict__ o = out + (int64_t)blockIdx.z * 3 * plane + (int64_t)yy * out_w + px0;
    uint8_t* __restrict__ m = mask + (int64_t)blockIdx.z * plane + (int64_t)yy * out_w + px0;
    float f[3][4];
    uint32_t pad = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool real = inside && px0 + i < ow;
        pad |= real ? 0u : 1u << (8 * i);
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c][i] = real ? table[c * 256 + clip8(s[3 * i + c])] : 0.f;
    }
    if ((out_w & 3) == 0) {  // rows of the planes are 16-byte aligned
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(o + c * plane) = make_float4(f[c][0], f[c][1], f[c][2], f[c][3]);
        *reinterpret_cast<uint32_t*>(m) = pad;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (px0 + i < out_w) {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c * plane + i] = f[c][i];
                m[i] = (uint8_t)(pad >> (8 * i));
            }
    }
}

}  // namespace

#pragma clang fp contract(off)  // host tables must round exactly like Pillow's: no fused multiply-add
static double cubic_weight(double x) {  // bicubic convolution kernel, a = -0.5
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

static double triangle_weight(double x) {  // bilinear
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for a filter of half-width `radius` source pixels at scale 1
static int resample_taps(double (*weight)(double), double radius, int in_size, int out_size, int32_t* bounds, int32_t* taps,
                         long taps_capacity) {
    if (in_size <= 0 || out_size <= 0) return -GRIT_ERR_BAD_ARG;
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = radius * filterscale, inv = 1.0 / filterscale;
    const int ksize = (int)ceil(support) * 2 + 1;
    if (!bounds && !taps) return ksize;
    if (!bounds || !taps || taps_capacity < (long)out_size * ksize) return -GRIT_ERR_BAD_ARG;
    double stack_k[64];
    double* k = ksize <= 64 ? stack_k : new double[ksize];
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int first = (int)(center - support + 0.5);
        if (first < 0) first = 0;
        int last = (int)(center + support + 0.5);
        if (last > in_size) last = in_size;
        const int count = last - first;
        double total = 0.0;
        for (int x = 0; x < count; ++x) {
            k[x] = weight((x + first - center + 0.5) * inv);
            total += k[x];
        }
        int32_t* t = taps + (long)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            double v = 0.0;
            if (x < count) v = total != 0.0 ? k[x] / total : k[x];
            t[x] = v < 0 ? (int)(-0.5 + v * (1 << kPrecisionBits)) : (int)(0.5 + v * (1 << kPrecisionBits));
        }
        bounds[2 * xx] = first;
        bounds[2 * xx + 1] = count;
    }
    if (k != stack_k) delete[] k;
    return ksize;
}

extern "C" int grit_resample_taps_bicubic(int in_size, int out_size, int32_t* bounds, int32_t* taps, long taps_capacity) {
    return resample_taps(cubic_weight, 2.0, in_size, out_size, bounds, taps, taps_capacity);
}

extern "C" int grit_resample_taps_bilinear(int in_size, int out_size, int32_t* bounds, int32_t* taps, long taps_capacity) {
    return resample_taps(triangle_weight, 1.0, in_size, out_size, bounds, taps, taps_capacity);
}

extern "C" int grit_image_batch_fwd(const uint8_t* src, const int64_t* desc, const int32_t* tables, uint8_t* tmp,
                                    const float* lut, int batch, int max_src_h, int max_dst_w, int max_kx, int out_h,
                                    int out_w, float* out, uint8_t* mask, void* stream) {
    if (!src || !desc || !tables || !tmp || !lut || !out || !mask) return GRIT_ERR_BAD_ARG;
    if (batch <= 0 || max_src_h <= 0 || max_dst_w <= 0 || max_kx <= 0 || out_h <= 0 || out_w <= 0 || max_dst_w > out_w)
        return GRIT_ERR_BAD_ARG;
    if (((uintptr_t)src | (uintptr_t)tmp) & 3) return GRIT_ERR_BAD_ARG;
    if (max_src_h > 65535 || out_h > 65535 || batch > 65535) return GRIT_ERR_UNSUPPORTED;
    const ImageDesc* d = reinterpret_cast<const ImageDesc*>(desc);
    const hipStream_t s = (hipStream_t)stream;
    const dim3 pixels((max_dst_w + 255) / 256, (max_src_h + kRows - 1) / kRows, batch);
    if (max_kx <= 7)
        hipLaunchKernelGGL(resample_rows_k<7>, pixels, dim3(256), 0, s, src, d, tables, tmp);
    else if (max_kx <= 9)
        hipLaunchKernelGGL(resample_rows_k<9>, pixels, dim3(256), 0, s, src, d, tables, tmp);
    else if (max_kx <= 13)
        hipLaunchKernelGGL(resample_rows_k<13>, pixels, dim3(256), 0, s, src, d, tables, tmp);
    else
        hipLaunchKernelGGL(resample_rows_any, dim3((max_dst_w * 3 + 255) / 256, max_src_h, batch), dim3(256), 0, s,
                           src, d, tables, tmp);
    const int wide = (out_w + 1023) / 1024;
    hipLaunchKernelGGL(resample_cols_normalize, dim3(wide, wide == 1 ? (out_h + 7) / 8 * 8 : out_h, batch), dim3(256), 0, s,
                       tmp, d, tables, lut, out_h, out_w, out, mask);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------------------------
// RandAugment between the resize and the float stage (reference datasets/caption/transforms/randaug.py:74-104), with
// Pillow's arithmetic on the resized uint8 image: grit_image_batch_aug_fwd.  The vertical pass writes uint8 (dword-aligned
// rows, like the intermediate), up to four stages run over two ping-pong buffers -- every image of the batch takes its
// own operation of that stage from its descriptor row, one launch per stage -- and a last launch applies the lookup
// table, the padding and the mask.  AutoContrast needs the per-channel min / max and Contrast the sum of the grey values
// of the image as it stands before that stage: the launch that WRITES those bytes (the vertical pass or the stage
// before) reduces them per block and the reader reduces the blocks' records: integers, so the order does not matter.
// All byte streams: a stage reads and writes 3 * h * w bytes per image.
namespace {

constexpr int kAugHeader = 4;  // buf_off, op count, two spare
constexpr int kAugStage = 8;   // op, seven parameters
static_assert(kAugHeader + GRIT_IMAGE_AUG_STAGES * kAugStage == GRIT_IMAGE_AUG_FIELDS, "augmentation descriptor layout");

__device__ __forceinline__ uint32_t byte_of(const uint32_t* v, int k) { return (v[k >> 2] >> (8 * (k & 3))) & 0xffu; }

__device__ __forceinline__ uint32_t grey(uint32_t r, uint32_t g, uint32_t b) {  // Pillow's RGB -> L
    return (r * 19595u + g * 38470u + b * 7471u + 0x8000u) >> 16;
}

// Every float expression below must round like Pillow's C / Python's doubles: one rounding per operation, never a fused
// multiply-add.  The contraction pragma is what guarantees it (the __fmul_rn / __dadd_rn family are plain operators in
// the HIP headers and would still be contracted), so it is stated again here, for the device code.
#pragma clang fp contract(off)

// Pillow's ImagingBlend(degenerate, image, alpha) on one byte: fp32 multiply, then fp32 add, each rounded
__device__ __forceinline__ uint32_t blend8(uint32_t d, uint32_t i, float alpha) {
    const float product = alpha * (float)((int)i - (int)d);
    const float t = (float)d + product;
    if (alpha >= 0.f && alpha <= 1.f) return (uint32_t)(int)t;  // between d and i
    return t <= 0.f ? 0u : t >= 255.f ? 255u : (uint32_t)(int)t;
}

__device__ __forceinline__ uint32_t clip8f(float s) { return s <= 0.f ? 0u : s >= 255.f ? 255u : (uint32_t)(int)s; }

// Statistics for AutoContrast (per-channel min / max) and Contrast (sum of the grey values), taken of the image as it
// stands before that stage.  The launch that WRITES those bytes gathers them: every block reduces its own pixels and
// stores one record of 8 words -- [0..2] 255 - min, [3..5] max per channel, [6..7] the 64-bit grey sum -- into its own
// slot of stats[image][stage][block]; the stage that needs them reduces the image's records again.  Integers only, no
// atomics, nothing to zero: a record is read only if the descriptor made every block of the writer store it.
struct Stats {
    uint32_t inv_lo[3], hi[3];
    unsigned long long sum;
};

__device__ __forceinline__ bool needs_stats(int op) { return op == GRIT_AUG_AUTOCONTRAST || op == GRIT_AUG_CONTRAST; }

// block-wide reduction (all 256 threads call it); every thread returns the block's result
__device__ __forceinline__ Stats reduce_block(Stats s, uint32_t (*red)[8]) {
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s.inv_lo[c] = max(s.inv_lo[c], (uint32_t)__shfl_xor((int)s.inv_lo[c], off, 64));
            s.hi[c] = max(s.hi[c], (uint32_t)__shfl_xor((int)s.hi[c], off, 64));
        }
        s.sum += __shfl_xor(s.sum, off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            red[wave][c] = s.inv_lo[c];
            red[wave][3 + c] = s.hi[c];
        }
        red[wave][6] = (uint32_t)s.sum;
        red[wave][7] = (uint32_t)(s.sum >> 32);
    }
    __syncthreads();
    Stats r = {{0u, 0u, 0u}, {0u, 0u, 0u}, 0ull};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            r.inv_lo[c] = max(r.inv_lo[c], red[w][c]);
            r.hi[c] = max(r.hi[c], red[w][3 + c]);
        }
        r.sum += (unsigned long long)red[w][6] | (unsigned long long)red[w][7] << 32;
    }
    __syncthreads();  // red may be used again
    return r;
}

// writer side: v = the thread's 4 pixels, n of them real; rec = this block's record
__device__ __forceinline__ void write_stats(const uint32_t* v, int n, uint32_t* __restrict__ rec, uint32_t (*red)[8]) {
    Stats s = {{0u, 0u, 0u}, {0u, 0u, 0u}, 0ull};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i >= n) continue;
        const uint32_t px[3] = {byte_of(v, 3 * i), byte_of(v, 3 * i + 1), byte_of(v, 3 * i + 2)};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            s.inv_lo[c] = max(s.inv_lo[c], 255u - px[c]);
            s.hi[c] = max(s.hi[c], px[c]);
        }
        s.sum += grey(px[0], px[1], px[2]);
    }
    s = reduce_block(s, red);
    if (threadIdx.x == 0) {
        reinterpret_cast<uint4*>(rec)[0] = make_uint4(s.inv_lo[0], s.inv_lo[1], s.inv_lo[2], s.hi[0]);
        reinterpret_cast<uint4*>(rec)[1] = make_uint4(s.hi[1], s.hi[2], (uint32_t)s.sum, (uint32_t)(s.sum >> 32));
    }
}

// reader side: the image's records -> its statistics, in every thread
__device__ __forceinline__ Stats read_stats(const uint32_t* __restrict__ recs, int nblk, uint32_t (*red)[8]) {
    Stats s = {{0u, 0u, 0u}, {0u, 0u, 0u}, 0ull};
    for (int i = threadIdx.x; i < nblk; i += 256) {
        const uint4 a = reinterpret_cast<const uint4*>(recs)[2 * i], b = reinterpret_cast<const uint4*>(recs)[2 * i + 1];
        s.inv_lo[0] = max(s.inv_lo[0], a.x); s.inv_lo[1] = max(s.inv_lo[1], a.y); s.inv_lo[2] = max(s.inv_lo[2], a.z);
        s.hi[0] = max(s.hi[0], a.w); s.hi[1] = max(s.hi[1], b.x); s.hi[2] = max(s.hi[2], b.y);
        s.sum += (unsigned long long)b.z | (unsigned long long)b.w << 32;
    }
    return reduce_block(s, red);
}

// 4 pixels -> 3 dwords, zero past the row end; stores only the dwords that belong to the row
__device__ __forceinline__ void store_quad(uint8_t* __restrict__ row, int px0, int pitch, const uint32_t* o) {
    uint32_t* __restrict__ q = reinterpret_cast<uint32_t*>(row + 3 * px0);
    const int words = min(3, (pitch - 3 * px0) >> 2);
    q[0] = o[0];
    if (words > 1) q[1] = o[1];
    if (words > 2) q[2] = o[2];
}

__device__ __forceinline__ void load_quad(const uint8_t* __restrict__ row, int px0, int pitch, uint32_t* v) {
    const uint32_t* __restrict__ q = reinterpret_cast<const uint32_t*>(row + 3 * px0);
    const int words = min(3, (pitch - 3 * px0) >> 2);
    v[0] = q[0];
    v[1] = words > 1 ? q[1] : 0u;
    v[2] = words > 2 ? q[2] : 0u;
}

// one thread per 4 pixels of one row; threads of a block run over the rows of the image (row-major quads)
struct Quad { int yy, px0; bool active; };
__device__ __forceinline__ Quad quad_of(int block, int h, int w) {
    const int quads = (w + 3) >> 2;
    const int t = block * 256 + threadIdx.x;
    Quad q;
    q.yy = t / quads;
    q.px0 = 4 * (t - q.yy * quads);
    q.active = q.yy < h;
    return q;
}

// pass 2 of the augmented path: vertical taps -> uint8 rows of work buffer 0 (+ the statistics of the first operation)
__global__ __launch_bounds__(256)
void resample_cols_u8(const uint8_t* __restrict__ tmp, const ImageDesc* __restrict__ desc, const int32_t* __restrict__ tables,
                      const int32_t* __restrict__ aug, uint8_t* __restrict__ work, uint32_t* __restrict__ stats) {
    __shared__ uint32_t red[4][8];
    const ImageDesc d = desc[blockIdx.z];
    const int32_t* __restrict__ a = aug + (int64_t)blockIdx.z * GRIT_IMAGE_AUG_FIELDS;
    // neighbouring rows share their source rows: one contiguous band of blocks per XCD (gridDim.x is a multiple of 8)
    const int block = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const int oh = (int)d.dst_h, ow = (int)d.dst_w, pitch = tmp_pitch(ow);
    const Quad q = quad_of(block, oh, ow);
    uint32_t o[3] = {0u, 0u, 0u};
    if (q.active) {
        int s[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) s[i] = 1 << (kPrecisionBits - 1);
        const int first = tables[d.yb_off + 2 * q.yy], count = tables[d.yb_off + 2 * q.yy + 1];
        const int32_t* __restrict__ k = tables + d.yt_off + (int64_t)q.yy * d.ky;
        const uint8_t* __restrict__ p = tmp + d.tmp_off + (int64_t)first * pitch;
        for (int y = 0; y < count; ++y) {
            uint32_t v[3];
            load_quad(p, q.px0, pitch, v);
            const int t = k[y];
#pragma unroll
            for (int i = 0; i < 12; ++i) s[i] += __mul24((int)byte_of(v, i), t);
            p += pitch;
        }
#pragma unroll
        for (int i = 0; i < 12; ++i)
            if (q.px0 + i / 3 < ow) o[i >> 2] |= (uint32_t)clip8(s[i]) << (8 * (i & 3));
        store_quad(work + a[0] + (int64_t)q.yy * pitch, q.px0, pitch, o);
    }
    if (needs_stats(a[kAugHeader]))  // block-uniform
        write_stats(o, q.active ? min(4, ow - q.px0) : 0,
                    stats + (((int64_t)blockIdx.z * GRIT_IMAGE_AUG_STAGES) * gridDim.x + block) * 8, red);
}

// one 20-byte window of a row around the thread's 12 bytes (byte k of the quad = window byte 4 + k)
__device__ __forceinline__ void load_window(const uint8_t* __restrict__ row, int px0, int pitch, uint32_t* win) {
    load_quad(row, px0, pitch, win + 1);
    const uint32_t* __restrict__ q = reinterpret_cast<const uint32_t*>(row + 3 * px0);
    win[0] = px0 > 0 ? q[-1] : 0u;
    win[4] = 3 * px0 + 16 <= pitch ? q[3] : 0u;
}

// one augmentation stage: in -> out for every image of the batch, each with its own operation (block-uniform)
__global__ __launch_bounds__(256)
void augment_stage(const ImageDesc* __restrict__ desc, const int32_t* __restrict__ aug, const int32_t* __restrict__ tables,
                   const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint32_t* __restrict__ stats, int stage) {
    __shared__ uint8_t lut[3 * 256];
    __shared__ uint32_t red[4][8];
    const ImageDesc d = desc[blockIdx.z];
    const int32_t* __restrict__ a = aug + (int64_t)blockIdx.z * GRIT_IMAGE_AUG_FIELDS;
    const int32_t* __restrict__ p = a + kAugHeader + stage * kAugStage;
    const int n_ops = min(a[1], GRIT_IMAGE_AUG_STAGES);
    if (stage >= n_ops) return;  // this image's plan is shorter (block-uniform): its result stays in buffer n_ops & 1
    const int op = p[0];
    const int next_op = stage + 1 < n_ops ? p[kAugStage] : GRIT_AUG_COPY;
    const int h = (int)d.dst_h, w = (int)d.dst_w, pitch = tmp_pitch(w);
    uint32_t* __restrict__ st = stats + ((int64_t)blockIdx.z * GRIT_IMAGE_AUG_STAGES + stage) * gridDim.x * 8;  // this stage's records
    const uint8_t* __restrict__ src = in + a[0];
    Stats stat = {{0u, 0u, 0u}, {0u, 0u, 0u}, 0ull};
    if (needs_stats(op)) stat = read_stats(st, gridDim.x, red);  // block-uniform
    if (op == GRIT_AUG_AUTOCONTRAST) {  // PIL.ImageOps.autocontrast: per channel a table from (lo, hi), fp64, separate roundings
        for (int i = threadIdx.x; i < 3 * 256; i += 256) {
            const int c = i >> 8, v = i & 255;
            const int lo = 255 - (int)stat.inv_lo[c], hi = (int)stat.hi[c];
            int r = v;
            if (hi > lo) {
                const double scale = 255.0 / (double)(hi - lo);
                const double offset = (double)(-lo) * scale;
                const double scaled = (double)v * scale;
                r = (int)(scaled + offset);
                r = min(max(r, 0), 255);
            }
            lut[i] = (uint8_t)r;
        }
        __syncthreads();
    }
    const Quad q = quad_of(blockIdx.x, h, w);
    uint32_t b[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) b[i] = 0u;
    if (q.active) {
        const int yy = q.yy, px0 = q.px0;
        const uint8_t* __restrict__ row = src + (int64_t)yy * pitch;
        if (op == GRIT_AUG_AFFINE_FIXED || op == GRIT_AUG_AFFINE_TABLE) {  // nearest neighbour, fill 0
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int x = px0 + i;
                int xin = -1, yin = -1;
                if (x < w) {
                    if (op == GRIT_AUG_AFFINE_FIXED) {  // 16.16 fixed point; wraps like the sums of Pillow's int walk
                        xin = (int)((uint32_t)p[3] + (uint32_t)p[1] * (uint32_t)x + (uint32_t)p[2] * (uint32_t)yy) >> 16;
                        yin = (int)((uint32_t)p[6] + (uint32_t)p[4] * (uint32_t)x + (uint32_t)p[5] * (uint32_t)yy) >> 16;
                    } else {  // index tables walked in doubles on the host
                        xin = tables[p[1] + x];
                        yin = tables[p[2] + yy];
                    }
                }
                if (xin >= 0 && xin < w && yin >= 0 && yin < h) {
                    const uint8_t* __restrict__ s = src + (int64_t)yin * pitch + 3 * xin;
                    b[3 * i] = s[0]; b[3 * i + 1] = s[1]; b[3 * i + 2] = s[2];
                }
            }
        } else if (op == GRIT_AUG_SHARPNESS) {  // blend(3 x 3 SMOOTH, image): fp32, no contraction, Pillow's order of sums
            const float alpha = __int_as_float(p[1]);
            const float k1 = (float)(1.0 / 13.0), k5 = (float)(5.0 / 13.0);
            uint32_t mid[5];
            load_window(row, px0, pitch, mid);
            const bool inner_row = h >= 3 && w >= 3 && yy > 0 && yy < h - 1;
            uint32_t up[5] = {0u, 0u, 0u, 0u, 0u}, down[5] = {0u, 0u, 0u, 0u, 0u};  // rows yy - 1 and yy + 1
            if (inner_row) {
                load_window(row - pitch, px0, pitch, up);
                load_window(row + pitch, px0, pitch, down);
            }
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                const int x = px0 + k / 3;
                const uint32_t centre = byte_of(mid, 4 + k);
                uint32_t deg = centre;
                if (inner_row && x > 0 && x < w - 1) {
                    float s = 0.5f;
                    s += ((float)byte_of(down, 1 + k) * k1 + (float)byte_of(down, 4 + k) * k1) + (float)byte_of(down, 7 + k) * k1;
                    s += ((float)byte_of(mid, 1 + k) * k1 + (float)centre * k5) + (float)byte_of(mid, 7 + k) * k1;
                    s += ((float)byte_of(up, 1 + k) * k1 + (float)byte_of(up, 4 + k) * k1) + (float)byte_of(up, 7 + k) * k1;
                    deg = clip8f(s);
                }
                if (x < w) b[k] = blend8(deg, centre, alpha);
            }
        } else {  // point operations on the thread's own 12 bytes
            uint32_t v[3];
            load_quad(row, px0, pitch, v);
            const float alpha = __int_as_float(p[1]);
            uint32_t mean = 0u;
            if (op == GRIT_AUG_CONTRAST) {  // int(sum / count + 0.5) of the grey image
                const unsigned long long sum = stat.sum;
                const unsigned long long count = (unsigned long long)h * (unsigned long long)w;
                mean = (uint32_t)((2ull * sum + count) / (2ull * count));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (px0 + i >= w) continue;
                const uint32_t r = byte_of(v, 3 * i), g = byte_of(v, 3 * i + 1), bl = byte_of(v, 3 * i + 2);
                const uint32_t c3[3] = {r, g, bl};
                const uint32_t l = grey(r, g, bl);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    uint32_t o = c3[c];  // GRIT_AUG_COPY
                    if (op == GRIT_AUG_AUTOCONTRAST) o = lut[c * 256 + c3[c]];
                    else if (op == GRIT_AUG_COLOR) o = blend8(l, c3[c], alpha);
                    else if (op == GRIT_AUG_CONTRAST) o = blend8(mean, c3[c], alpha);
                    else if (op == GRIT_AUG_BRIGHTNESS) o = blend8(0u, c3[c], alpha);
                    b[3 * i + c] = o;
                }
            }
        }
    }
    uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 12; ++i) o[i >> 2] |= b[i] << (8 * (i & 3));
    if (q.active) store_quad(out + a[0] + (int64_t)q.yy * pitch, q.px0, pitch, o);
    if (needs_stats(next_op))  // block-uniform
        write_stats(o, q.active ? min(4, w - q.px0) : 0, st + ((int64_t)gridDim.x + blockIdx.x) * 8, red);
}

// last launch of the augmented path: uint8 rows (of the buffer each image ended in) -> lookup, one float4 store per colour plane, 4 mask bytes, zero padding
__global__ __launch_bounds__(256)
void normalize_pad(const uint8_t* __restrict__ work, long work_bytes, const ImageDesc* __restrict__ desc,
                   const int32_t* __restrict__ aug, const float* __restrict__ lut, int out_h, int out_w,
                   float* __restrict__ out, uint8_t* __restrict__ mask) {
    __shared__ float table[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += 256) table[i] = lut[i];
    __syncthreads();
    const ImageDesc d = desc[blockIdx.z];
    const int yy = blockIdx.y;
    const int px0 = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (px0 >= out_w) return;
    const int ow = (int)d.dst_w, pitch = tmp_pitch(ow);
    const bool inside = yy < d.dst_h && px0 < ow;
    uint32_t v[3] = {0u, 0u, 0u};
    if (inside) {  // an image with k operations ends in buffer k & 1
        const int32_t* __restrict__ a = aug + (int64_t)blockIdx.z * GRIT_IMAGE_AUG_FIELDS;
        load_quad(work + (min(a[1], GRIT_IMAGE_AUG_STAGES) & 1) * work_bytes + a[0] + (int64_t)yy * pitch, px0, pitch, v);
    }
    const int64_t plane = (int64_t)out_h * out_w;
    float* __restrict__ o = out + (int64_t)blockIdx.z * 3 * plane + (int64_t)yy * out_w + px0;
    uint8_t* __restrict__ m = mask + (int64_t)blockIdx.z * plane + (int64_t)yy * out_w + px0;
    float f[3][4];
    uint32_t pad = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool real = inside && px0 + i < ow;
        pad |= real ? 0u : 1u << (8 * i);
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c][i] = real ? table[c * 256 + byte_of(v, 3 * i + c)] : 0.f;
    }
    if ((out_w & 3) == 0) {  // rows of the planes are 16-byte aligned
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(o + c * plane) = make_float4(f[c][0], f[c][1], f[c][2], f[c][3]);
        *reinterpret_cast<uint32_t*>(m) = pad;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (px0 + i < out_w) {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c * plane + i] = f[c][i];
                m[i] = (uint8_t)(pad >> (8 * i));
            }
    }
}

}  // namespace

extern "C" int grit_image_batch_aug_fwd(const uint8_t* src, const int64_t* desc, const int32_t* tables, uint8_t* tmp,
                                        const float* lut, const int32_t* aug, int n_stages, uint8_t* work, long work_bytes,
                                        uint32_t* stats, int batch, int max_src_h, int max_dst_h, int max_dst_w, int max_kx,
                                        int out_h, int out_w, float* out, uint8_t* mask, void* stream) {
    if (!src || !desc || !tables || !tmp || !lut || !aug || !work || !stats || !out || !mask) return GRIT_ERR_BAD_ARG;
    if (batch <= 0 || max_src_h <= 0 || max_dst_h <= 0 || max_dst_w <= 0 || max_kx <= 0 || out_h <= 0 || out_w <= 0 ||
        max_dst_w > out_w || max_dst_h > out_h || n_stages < 0 || n_stages > GRIT_IMAGE_AUG_STAGES || work_bytes <= 0 || (work_bytes & 3))
        return GRIT_ERR_BAD_ARG;
    if (((uintptr_t)src | (uintptr_t)tmp | (uintptr_t)work) & 3 || (uintptr_t)stats & 15) return GRIT_ERR_BAD_ARG;
    if (max_src_h > 65535 || out_h > 65535 || batch > 65535 || max_dst_h > 32767 || max_dst_w > 32767) return GRIT_ERR_UNSUPPORTED;
    const ImageDesc* d = reinterpret_cast<const ImageDesc*>(desc);
    const hipStream_t s = (hipStream_t)stream;
    const dim3 pixels((max_dst_w + 255) / 256, (max_src_h + kRows - 1) / kRows, batch);
    if (max_kx <= 7)
        hipLaunchKernelGGL(resample_rows_k<7>, pixels, dim3(256), 0, s, src, d, tables, tmp);
    else if (max_kx <= 9)
        hipLaunchKernelGGL(resample_rows_k<9>, pixels, dim3(256), 0, s, src, d, tables, tmp);
    else if (max_kx <= 13)
        hipLaunchKernelGGL(resample_rows_k<13>, pixels, dim3(256), 0, s, src, d, tables, tmp);
    else
        hipLaunchKernelGGL(resample_rows_any, dim3((max_dst_w * 3 + 255) / 256, max_src_h, batch), dim3(256), 0, s,
                           src, d, tables, tmp);
    const int blocks = (int)GRIT_IMAGE_AUG_BLOCKS(max_dst_h, max_dst_w);  // the same grid for the writers and readers of `stats`
    hipLaunchKernelGGL(resample_cols_u8, dim3(blocks, 1, batch), dim3(256), 0, s, tmp, d, tables, aug, work, stats);
    for (int i = 0; i < n_stages; ++i)
        hipLaunchKernelGGL(augment_stage, dim3(blocks, 1, batch), dim3(256), 0, s, d, aug, tables,
                           work + (i & 1) * work_bytes, work + ((i + 1) & 1) * work_bytes, stats, i);
    hipLaunchKernelGGL(normalize_pad, dim3((out_w + 1023) / 1024, out_h, batch), dim3(256), 0, s,
                       work, work_bytes, d, aug, lut, out_h, out_w, out, mask);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------------------------------
// The detector's input pipeline (reference datasets/detection/transforms.py:107-223, 240-352: hflip, resize, crop chained on
// PIL images): grit_image_batch_geo_fwd.  An image takes one or two resizes, A then B, each over a source WINDOW: the host
// folds a crop into the window's first byte and height and a horizontal flip into mirrored taps of the next horizontal pass
// (sum_k tap[k] * flipped[first + k] = sum_k tap[count - 1 - k] * row[w - first - count + k], integers), so the kernels see
// neither.  Resize A ends as uint8 rows in the work buffer (dword-aligned rows like the intermediate), resize B reads the blob
// or that buffer and ends in the float stage of grit_image_batch_fwd.  Same arithmetic, same clip8, same lookup table.
namespace {

struct GeoResize {  // see grit_hip.h
    int64_t buf, off, pitch, src_h, dst_h, dst_w, kx, ky, xb_off, xt_off, yb_off, yt_off, tmp_off, out_off;
};
struct GeoDesc {
    int64_t n, spare;
    GeoResize r[2];
};
static_assert(sizeof(GeoDesc) == GRIT_IMAGE_GEO_FIELDS * sizeof(int64_t), "geometry descriptor layout");

// horizontal pass of resize `which` (0 = A, 1 = B), generic: resample_rows_any over a window
__global__ __launch_bounds__(256)
void geo_rows_any(const uint8_t* __restrict__ blob, const uint8_t* __restrict__ work, const GeoDesc* __restrict__ desc,
                  const int32_t* __restrict__ tables, uint8_t* __restrict__ tmp, int which) {
    if (which == 0 && desc[blockIdx.z].n < 2) return;  // one-resize images sit out pass A (block-uniform)
    const GeoResize d = desc[blockIdx.z].r[which];
    const int y = blockIdx.y;
    const int j = blockIdx.x * 256 + threadIdx.x;  // byte within the output row
    const int ow = (int)d.dst_w;
    if (y >= d.src_h || j >= ow * 3) return;
    const int xx = j / 3, c = j - xx * 3;
    const int2 b = *reinterpret_cast<const int2*>(tables + d.xb_off + 2 * xx);
    const int32_t* __restrict__ k = tables + d.xt_off + (int64_t)xx * d.kx;
    const uint8_t* __restrict__ p = (d.buf ? work : blob) + d.off + (int64_t)y * d.pitch + 3 * b.x + c;
    int ss = 1 << (kPrecisionBits - 1);
    for (int x = 0; x < b.y; ++x) ss += (int)p[3 * x] * k[x];
    tmp[d.tmp_off + (int64_t)y * tmp_pitch(ow) + j] = clip8(ss);
}

// horizontal pass of resize `which`, up to K taps: resample_rows_k over a window -- the same aligned-dword fetch and
// v_alignbyte realignment, with the row address taken from the window's first byte and the source's row pitch.  A row reads
// kWords + 1 dwords from its first tap's dword on, whatever the tap count: both source buffers carry GRIT_IMAGE_SRC_PAD
// readable bytes past their end, and a window's first byte is never negative, so the fetch stays inside them.
template <int K>
__global__ __launch_bounds__(256)
void geo_rows_k(const uint8_t* __restrict__ blob, const uint8_t* __restrict__ work, const GeoDesc* __restrict__ desc,
                const int32_t* __restrict__ tables, uint8_t* __restrict__ tmp, int which) {
    constexpr int kWords = (3 * K + 3) / 4;
    __shared__ uint32_t packed[4][kRows][48];
    if (which == 0 && desc[blockIdx.z].n < 2) return;  // block-uniform
    const GeoResize d = desc[blockIdx.z].r[which];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x_wave = blockIdx.x * 256 + wave * 64;
    const int y0 = blockIdx.y * kRows;
    const int ow = (int)d.dst_w, h = (int)d.src_h, kx = (int)d.kx;
    if (y0 >= h || x_wave >= ow) return;  // wave-uniform
    const int xx = min(x_wave + lane, ow - 1);
    const int first = tables[d.xb_off + 2 * xx];
    const int32_t* __restrict__ k = tables + d.xt_off + (int64_t)xx * kx;
    int tap[K];
#pragma unroll
    for (int t = 0; t < K; ++t) tap[t] = t < kx ? k[t] : 0;
    const int pitch = tmp_pitch(ow);
    const uint8_t* __restrict__ src = d.buf ? work : blob;
    uint8_t* __restrict__ staged = reinterpret_cast<uint8_t*>(&packed[wave][0][0]);
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
        const int y = min(y0 + r, h - 1);
        const int64_t a = d.off + (int64_t)y * d.pitch + 3 * first;
        const uint32_t* __restrict__ q = reinterpret_cast<const uint32_t*>(src + (a & ~(int64_t)3));
        const uint32_t shift = (uint32_t)(a & 3);
        uint32_t raw[kWords + 1], word[kWords];
#pragma unroll
        for (int i = 0; i <= kWords; ++i) raw[i] = q[i];
#pragma unroll
        for (int i = 0; i < kWords; ++i) word[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], shift);
        int s[3] = {1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1)};
#pragma unroll
        for (int t = 0; t < K; ++t)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int j = 3 * t + c;
                s[c] += __mul24((int)((word[j >> 2] >> (8 * (j & 3))) & 0xffu), tap[t]);
            }
        uint8_t* __restrict__ o = staged + r * 192 + 3 * lane;
        o[0] = clip8(s[0]); o[1] = clip8(s[1]); o[2] = clip8(s[2]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int byte0 = 3 * x_wave + 4 * lane;
    if (lane < 48 && byte0 < pitch) {
#pragma unroll
        for (int r = 0; r < kRows; ++r)
            if (y0 + r < h)
                *reinterpret_cast<uint32_t*>(tmp + d.tmp_off + (int64_t)(y0 + r) * pitch + byte0) = packed[wave][r][lane];
    }
}

// the vertical taps of one resize on the thread's 4 pixels of output row yy: 12 sums, rounding term included
__device__ __forceinline__ void geo_cols_quad(const uint8_t* __restrict__ tmp, const GeoResize& d, const int32_t* __restrict__ tables,
                                              int yy, int px0, int pitch, int* s) {
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = 1 << (kPrecisionBits - 1);
    const int first = tables[d.yb_off + 2 * yy], count = tables[d.yb_off + 2 * yy + 1];
    const int32_t* __restrict__ k = tables + d.yt_off + (int64_t)yy * d.ky;
    const uint8_t* __restrict__ p = tmp + d.tmp_off + (int64_t)first * pitch;
    for (int y = 0; y < count; ++y) {
        uint32_t v[3];
        load_quad(p, px0, pitch, v);
        const int t = k[y];
#pragma unroll
        for (int i = 0; i < 12; ++i) s[i] += __mul24((int)byte_of(v, i), t);
        p += pitch;
    }
}

// vertical pass of resize A -> uint8 rows of the work buffer (resample_cols_u8 without the statistics)
__global__ __launch_bounds__(256)
void geo_cols_u8(const uint8_t* __restrict__ tmp, const GeoDesc* __restrict__ desc, const int32_t* __restrict__ tables,
                 uint8_t* __restrict__ work) {
    if (desc[blockIdx.z].n < 2) return;  // block-uniform
    const GeoResize d = desc[blockIdx.z].r[0];
    // neighbouring rows share their source rows: one contiguous band of blocks per XCD (gridDim.x is a multiple of 8)
    const int block = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const int oh = (int)d.dst_h, ow = (int)d.dst_w, pitch = tmp_pitch(ow);
    const Quad q = quad_of(block, oh, ow);
    if (!q.active) return;
    int s[12];
    geo_cols_quad(tmp, d, tables, q.yy, q.px0, pitch, s);
    uint32_t o[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 12; ++i)
        if (q.px0 + i / 3 < ow) o[i >> 2] |= (uint32_t)clip8(s[i]) << (8 * (i & 3));
    store_quad(work + d.out_off + (int64_t)q.yy * pitch, q.px0, pitch, o);
}

// vertical pass of resize B + lookup + zero padding + mask: resample_cols_normalize on the geometry descriptor
__global__ __launch_bounds__(256)
void geo_cols_normalize(const uint8_t* __restrict__ tmp, const GeoDesc* __restrict__ desc, const int32_t* __restrict__ tables,
                        const float* __restrict__ lut, int out_h, int out_w, float* __restrict__ out, uint8_t* __restrict__ mask) {
    __shared__ float table[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += 256) table[i] = lut[i];
    __syncthreads();
    const GeoResize d = desc[blockIdx.z].r[1];
    int yy = blockIdx.y;  // one contiguous band of rows per XCD, see resample_cols_normalize
    if (gridDim.x == 1) yy = (yy & 7) * (gridDim.y >> 3) + (yy >> 3);
    const int px0 = 4 * (blockIdx.x * 256 + threadIdx.x);
    if (yy >= out_h || px0 >= out_w) return;
    const int ow = (int)d.dst_w, pitch = tmp_pitch(ow);
    int s[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const bool inside = yy < d.dst_h && px0 < ow;
    if (inside) geo_cols_quad(tmp, d, tables, yy, px0, pitch, s);
    const int64_t plane = (int64_t)out_h * out_w;
    float* __restrict__ o = out + (int64_t)blockIdx.z * 3 * plane + (int64_t)yy * out_w + px0;
    uint8_t* __restrict__ m = mask + (int64_t)blockIdx.z * plane + (int64_t)yy * out_w + px0;
    float f[3][4];
    uint32_t pad = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool real = inside && px0 + i < ow;
        pad |= real ? 0u : 1u << (8 * i);
#pragma unroll
        for (int c = 0; c < 3; ++c) f[c][i] = real ? table[c * 256 + clip8(s[3 * i + c])] : 0.f;
    }
    if ((out_w & 3) == 0) {  // rows of the planes are 16-byte aligned
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<float4*>(o + c * plane) = make_float4(f[c][0], f[c][1], f[c][2], f[c][3]);
        *reinterpret_cast<uint32_t*>(m) = pad;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (px0 + i < out_w) {
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c * plane + i] = f[c][i];
                m[i] = (uint8_t)(pad >> (8 * i));
            }
    }
}

void launch_geo_rows(hipStream_t s, const uint8_t* blob, const uint8_t* work, const GeoDesc* d, const int32_t* tables, uint8_t* tmp,
                     int which, int batch, int max_src_h, int max_dst_w, int max_kx) {
    const dim3 pixels((max_dst_w + 255) / 256, (max_src_h + kRows - 1) / kRows, batch);
    if (max_kx <= 7)
        hipLaunchKernelGGL(geo_rows_k<7>, pixels, dim3(256), 0, s, blob, work, d, tables, tmp, which);
    else if (max_kx <= 9)
        hipLaunchKernelGGL(geo_rows_k<9>, pixels, dim3(256), 0, s, blob, work, d, tables, tmp, which);
    else if (max_kx <= 13)
        hipLaunchKernelGGL(geo_rows_k<13>, pixels, dim3(256), 0, s, blob, work, d, tables, tmp, which);
    else
        hipLaunchKernelGGL(geo_rows_any, dim3((max_dst_w * 3 + 255) / 256, max_src_h, batch), dim3(256), 0, s,
                           blob, work, d, tables, tmp, which);
}

}  // namespace

extern "C" int grit_image_batch_geo_fwd(const uint8_t* src, const int64_t* geo, const int32_t* tables, uint8_t* tmp, uint8_t* work,
                                        const float* lut, int batch, int a_src_h, int a_dst_h, int a_dst_w, int a_kx, int b_src_h,
                                        int b_dst_w, int b_kx, int out_h, int out_w, float* out, uint8_t* mask, void* stream) {
    if (!src || !geo || !tables || !tmp || !lut || !out || !mask) return GRIT_ERR_BAD_ARG;
    if (batch <= 0 || b_src_h <= 0 || b_dst_w <= 0 || b_kx <= 0 || out_h <= 0 || out_w <= 0 || b_dst_w > out_w || a_src_h < 0)
        return GRIT_ERR_BAD_ARG;
    if (a_src_h > 0 && (!work || a_dst_h <= 0 || a_dst_w <= 0 || a_kx <= 0)) return GRIT_ERR_BAD_ARG;
    if (((uintptr_t)src | (uintptr_t)tmp | (uintptr_t)work) & 3 || (uintptr_t)geo & 7) return GRIT_ERR_BAD_ARG;
    if (a_src_h > 65535 || b_src_h > 65535 || out_h > 65535 || batch > 65535 || a_dst_h > 32767 || a_dst_w > 32767)
        return GRIT_ERR_UNSUPPORTED;
    const GeoDesc* d = reinterpret_cast<const GeoDesc*>(geo);
    const hipStream_t s = (hipStream_t)stream;
    if (a_src_h > 0) {  // some image takes two resizes
        launch_geo_rows(s, src, work, d, tables, tmp, 0, batch, a_src_h, a_dst_w, a_kx);
        hipLaunchKernelGGL(geo_cols_u8, dim3((int)GRIT_IMAGE_AUG_BLOCKS(a_dst_h, a_dst_w), 1, batch), dim3(256), 0, s, tmp, d, tables, work);
    }
    launch_geo_rows(s, src, work, d, tables, tmp, 1, batch, b_src_h, b_dst_w, b_kx);
    const int wide = (out_w + 1023) / 1024;
    hipLaunchKernelGGL(geo_cols_normalize, dim3(wide, wide == 1 ? (out_h + 7) / 8 * 8 : out_h, batch), dim3(256), 0, s,
                       tmp, d, tables, lut, out_h, out_w, out, mask);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}
