// JPEG decoding (DESIGN "JPEG decoding"): grit_jpeg_probe / grit_jpeg_entropy are the host stage of jpeg_host.h behind the
// C ABI; grit_jpeg_reconstruct turns the coefficient planes of a batch into RGB pixels in two launches:
//   1. dequantise + jpeg_idct_islow (jidctint.c: CONST_BITS 13, PASS1_BITS 2, columns first) + range limit -> uint8 planes
//   2. per pixel: Y, fancy chroma upsampling (jdsample.c), YCbCr -> RGB (jdcolor.c) -> [h, w, 3] uint8
// Integer arithmetic only; every output byte is written by exactly one thread.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/grit_hip.h"
#include "jpeg_host.h"

namespace {

constexpr int kBlocksPerGroup = 32;  // 8 threads per 8x8 block, 256 per workgroup
constexpr int kPitch = 9;            // ints per row of a block in LDS: column reads of the 8 blocks of a wave hit 32 banks twice

// One 1-D pass of jpeg_idct_islow over d[0..7]; returns the eight sums BEFORE the descale.  T = int32_t in pass 1, where
// |d| <= 8191 keeps every intermediate below 2^31 (DESIGN has the bound per term); T = uint32_t in pass 2, where the sums do
// leave 32 bits for wild blocks but only bits 18..27 of each are kept, and +, -, * by a constant commute with mod 2^32.
template <typename T>
__device__ __forceinline__ void idct_pass(const T* d, T* o) {
    T z2 = d[2], z3 = d[6];
    T z1 = (z2 + z3) * T(4433);
    T tmp2 = z1 + z3 * T(-15137);
    T tmp3 = z1 + z2 * T(6270);
    T tmp0 = (d[0] + d[4]) * T(8192);
    T tmp1 = (d[0] - d[4]) * T(8192);
    const T tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7];
    tmp1 = d[5];
    tmp2 = d[3];
    tmp3 = d[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    T z4 = tmp1 + tmp3;
    const T z5 = (z3 + z4) * T(9633);
    tmp0 *= T(2446);
    tmp1 *= T(16819);
    tmp2 *= T(25172);
    tmp3 *= T(12299);
    z1 *= T(-7373);
    z2 *= T(-20995);
    z3 = z3 * T(-16069) + z5;
    z4 = z4 * T(-3196) + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    o[0] = tmp10 + tmp3;
    o[7] = tmp10 - tmp3;
    o[1] = tmp11 + tmp2;
    o[6] = tmp11 - tmp2;
    o[2] = tmp12 + tmp1;
    o[5] = tmp12 - tmp1;
    o[3] = tmp13 + tmp0;
    o[4] = tmp13 - tmp0;
}

__device__ __forceinline__ uint32_t range_limit(uint32_t x) {  // libjpeg's table: a wrap, not a clamp
    const uint32_t i = x & 1023u;
    return i < 128u ? i + 128u : i < 512u ? 255u : i < 896u ? 0u : i - 896u;
}

__global__ __launch_bounds__(256)
void jpeg_idct(const grit_jpeg_job* __restrict__ jobs, const int16_t* __restrict__ coef, uint8_t* __restrict__ planes) {
    __shared__ int ws[kBlocksPerGroup * 8 * kPitch];
    __shared__ int quant[64];
    const grit_jpeg_job& job = jobs[blockIdx.y / 3];
    const int comp = blockIdx.y % 3;
    if (comp >= job.ncomp) return;
    const int bc = job.block_cols[comp];
    const int nblocks = bc * job.block_rows[comp];
    if ((int)blockIdx.x * kBlocksPerGroup >= nblocks) return;
    const int tid = threadIdx.x, local = tid >> 3, lane = tid & 7;
    const int blk = blockIdx.x * kBlocksPerGroup + local;
    const bool live = blk < nblocks;
    if (tid < 64) quant[tid] = job.quant[64 * comp + tid];
    __syncthreads();
    int* tile = ws + local * 8 * kPitch;
    if (live) {  // row `lane` of the block: one 16-byte load, dequantised into LDS
        const int4 raw = *reinterpret_cast<const int4*>(coef + job.coef_off[comp] + (long)blk * 64 + lane * 8);
        const int v[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            tile[lane * kPitch + 2 * k] = (int)(int16_t)(v[k] & 0xFFFF) * quant[lane * 8 + 2 * k];
            tile[lane * kPitch + 2 * k + 1] = (v[k] >> 16) * quant[lane * 8 + 2 * k + 1];
        }
    }
    __syncthreads();
    if (live) {  // pass 1 over column `lane`; a thread reads and writes only its own column
        int32_t d[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = tile[k * kPitch + lane];
        idct_pass<int32_t>(d, o);
#pragma unroll
        for (int k = 0; k < 8; ++k) tile[k * kPitch + lane] = (o[k] + 1024) >> 11;
    }
    __syncthreads();
    if (live) {  // pass 2 over row `lane`, eight samples = one 8-byte store
        uint32_t d[8], o[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = (uint32_t)tile[lane * kPitch + k];
        idct_pass<uint32_t>(d, o);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lo |= range_limit((o[k] + (1u << 17)) >> 18) << (8 * k);
            hi |= range_limit((o[k + 4] + (1u << 17)) >> 18) << (8 * k);
        }
        const int brow = blk / bc, bcol = blk - brow * bc;
        uint8_t* at = planes + job.plane_off[comp] + ((long)brow * 8 + lane) * (bc * 8) + bcol * 8;
        *reinterpret_cast<uint2*>(at) = make_uint2(lo, hi);
    }
}

// One chroma sample at output pixel (x, y).  plane: the component's samples, `pitch` bytes per row; dw x dh its real size.
__device__ __forceinline__ int chroma_at(const uint8_t* __restrict__ plane, int pitch, int dw, int dh, int hmax, int vmax, int x, int y) {
    if (hmax == 1) return plane[(long)y * pitch + x];
    const int i = x >> 1;
    if (dw <= 2) return plane[(long)(vmax == 2 ? y >> 1 : y) * pitch + i];  // the fancy filters are off
    if (vmax == 1) {
        const uint8_t* in = plane + (long)y * pitch;
        if (x & 1) return i == dw - 1 ? in[i] : (3 * in[i] + in[i + 1] + 2) >> 2;
        return i == 0 ? in[0] : (3 * in[i] + in[i - 1] + 1) >> 2;
    }
    const int n = y >> 1;
    const int f = (y & 1) ? min(n + 1, dh - 1) : max(n - 1, 0);
    const uint8_t* near = plane + (long)n * pitch;
    const uint8_t* far = plane + (long)f * pitch;
    const int s = 3 * near[i] + far[i];
    if (x & 1) return i == dw - 1 ? (4 * s + 7) >> 4 : (3 * s + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    return i == 0 ? (4 * s + 8) >> 4 : (3 * s + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

__device__ __forceinline__ uint32_t clamp255(int v) { return (uint32_t)min(max(v, 0), 255); }

__global__ __launch_bounds__(256)
void jpeg_colour(const grit_jpeg_job* __restrict__ jobs, const uint8_t* __restrict__ planes, uint8_t* __restrict__ out) {
    const grit_jpeg_job& job = jobs[blockIdx.y];
    const int w = job.width, h = job.height;
    const uint32_t npix = (uint32_t)w * (uint32_t)h;
    const uint32_t p0 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (p0 >= npix) return;
    const int count = (int)min(4u, npix - p0);
    const int hmax = job.hmax, vmax = job.vmax;
    const bool colour = job.ncomp == 3;
    const uint8_t* yp = planes + job.plane_off[0];
    const uint8_t* cbp = planes + job.plane_off[colour ? 1 : 0];
    const uint8_t* crp = planes + job.plane_off[colour ? 2 : 0];
    const int ypitch = job.block_cols[0] * 8, cpitch = job.block_cols[colour ? 1 : 0] * 8;
    const int dw = (w + hmax - 1) / hmax, dh = (h + vmax - 1) / vmax;
    int y = (int)(p0 / (uint32_t)w), x = (int)(p0 - (uint32_t)y * (uint32_t)w);
    uint32_t bytes[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t r = 0, g = 0, b = 0;
        if (k < count) {
            const int lum = yp[(long)y * ypitch + x];
            if (colour) {
                const int cb = chroma_at(cbp, cpitch, dw, dh, hmax, vmax, x, y) - 128;
                const int cr = chroma_at(crp, cpitch, dw, dh, hmax, vmax, x, y) - 128;
                r = clamp255(lum + ((91881 * cr + 32768) >> 16));
                g = clamp255(lum + ((-22554 * cb - 46802 * cr + 32768) >> 16));
                b = clamp255(lum + ((116130 * cb + 32768) >> 16));
            } else {
                r = g = b = (uint32_t)lum;
            }
            if (++x == w) {
                x = 0;
                ++y;
            }
        }
        bytes[3 * k] = r;
        bytes[3 * k + 1] = g;
        bytes[3 * k + 2] = b;
    }
    uint8_t* at = out + job.out_off + 3l * p0;
    if (count == 4 && (job.out_off & 3) == 0) {  // the usual case: 4 pixels = 3 whole dwords
        uint32_t* at4 = reinterpret_cast<uint32_t*>(at);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            at4[k] = bytes[4 * k] | (bytes[4 * k + 1] << 8) | (bytes[4 * k + 2] << 16) | (bytes[4 * k + 3] << 24);
    } else {  // an image at an odd offset of the packed buffer, or the last pixels of one
#pragma unroll
        for (int k = 0; k < 12; ++k)
            if (k < 3 * count) at[k] = (uint8_t)bytes[k];
    }
}

}  // namespace

extern "C" int grit_jpeg_probe(const uint8_t* data, long nbytes, grit_jpeg_info* info) {
    if (!data || !info || nbytes < 0) return GRIT_ERR_BAD_ARG;
    grit_jpeg::Header h;
    const int st = grit_jpeg::parse_header(data, nbytes, &h);
    if (st == GRIT_OK) memcpy(info, &h.info, sizeof(*info));
    return st;
}

extern "C" int grit_jpeg_entropy(const uint8_t* data, long nbytes, const grit_jpeg_info* info, void* coef, long coef_bytes) {
    if (!data || !coef || nbytes < 0 || ((uintptr_t)coef & 1)) return GRIT_ERR_BAD_ARG;
    return grit_jpeg::entropy(data, nbytes, info, static_cast<int16_t*>(coef), coef_bytes);
}

extern "C" long grit_jpeg_planes_bytes(const grit_jpeg_info* info) {
    return info ? (info->plane_bytes + 15) & ~15l : -1;
}

extern "C" int grit_jpeg_reconstruct(const grit_jpeg_job* jobs, int n_images, int max_blocks, long max_pixels, const void* coef,
                                     uint8_t* planes, uint8_t* out, void* stream) {
    if (!jobs || !coef || !planes || !out || n_images <= 0 || max_blocks <= 0 || max_pixels <= 0) return GRIT_ERR_BAD_ARG;
    if (((uintptr_t)coef | (uintptr_t)planes) & 15 || ((uintptr_t)out & 3)) return GRIT_ERR_BAD_ARG;
    if (n_images * 3l > 65535 || max_pixels >= (1l << 31)) return GRIT_ERR_UNSUPPORTED;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_idct, dim3((max_blocks + kBlocksPerGroup - 1) / kBlocksPerGroup, n_images * 3), dim3(256), 0, s, jobs,
                       static_cast<const int16_t*>(coef), planes);
    hipLaunchKernelGGL(jpeg_colour, dim3((unsigned)((max_pixels + 1023) / 1024), n_images), dim3(256), 0, s, jobs, planes, out);
    return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH;
}
