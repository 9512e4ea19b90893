// Multi-scale deformable attention for gfx950 (MI355X): forward gather + backward scatter.
//
// Semantics follow davidnvq/grit models/ops/src/cuda/ms_deform_im2col_cuda.cuh (forward :237-299 with the
// bilinear rule of :33-84, backward :406-510 with :87-159); the decomposition is CDNA4's own:
//
//   * one 64-lane wavefront owns one output row (b, q, m) -- all L*P sampling points of one head;
//   * forward fast path (D = 64 / 32): a row's D channels are D/4 lanes x float4, so a wave covers
//     64/(D/4) sampling points at once and every corner is one 16-byte load per lane (a whole
//     256-byte pixel-head slice per 16 lanes).  All 4 corners of all points are issued before any
//     is consumed: 16 independent dwordx4 loads in flight per lane hide the L2 / Infinity-Cache / HBM
//     latency of the gather.  Out-of-range corners load a clamped (valid) address and are
//     selected to zero, so there is no divergent branch around a load;
//   * loc / attn_w of the row are read ONCE by the wave (coalesced) and handed to the lanes by
//     ds_bpermute -- the reference re-reads them per channel thread;
//   * the blockIdx -> row map is XCD-aware: workgroups that share an XCD (same blockIdx % 8) walk
//     one contiguous chunk of rows, i.e. one batch element's value map, so its coarse levels stay
//     in that XCD's 4 MiB L2;
//   * backward: lane = channel, so every grad_value update of a corner is ONE wave-wide
//     global_atomic_add_f32 over 256 contiguous bytes (the full-rate shape of the memory-side
//     atomic units); grad_loc / grad_attn_w are wave-shuffle reductions -- no LDS tree, no barrier.
//
// No hipify, no CUDA dual path: this file only builds for gfx950.
#include <hip/hip_runtime.h>
#include "per_device.h"
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdlib.h>
#include <initializer_list>
#include <utility>
#include "../../include/grit_hip.h"

namespace {

constexpr int kWave = 64;
constexpr int kRowsPerBlock = 4;  // 4 waves / workgroup, one row each

// Bijective XCD remap (blocks b and b+8 share an XCD): logical id such that one XCD gets a
// contiguous range of logical blocks.  Speed only -- any placement gives the same result.
__device__ __forceinline__ int xcd_logical_block(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7;
    const int base = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (bid >> 3);
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// Corner geometry of one sampling point; weights of corners that fall outside are forced to 0 and
// their indices clamped inside the map, so a load through them is always legal.
template <typename T>
struct Corners {
    int o1, o2, o3, o4;  // pixel offsets (h*W + w) of the 4 corners, clamped
    T w1, w2, w3, w4;    // bilinear weights (hh*hw, hh*lw, lh*hw, lh*lw)
    bool k1, k2, k3, k4; // corner inside the map
    T lh, lw, hh, hw;
    bool live;           // point passes the (-1, H) x (-1, W) test
};

template <typename T>
__device__ __forceinline__ Corners<T> make_corners(T x, T y, int H, int W) {
    Corners<T> c;
    const T h_im = y * (T)H - (T)0.5;
    const T w_im = x * (T)W - (T)0.5;
    c.live = (h_im > (T)-1) && (w_im > (T)-1) && (h_im < (T)H) && (w_im < (T)W);
    const T hf = floor(h_im), wf = floor(w_im);
    // clamp before the int conversion so NaN / huge coordinates cannot produce wild indices
    const int h_low = (int)fmin(fmax(hf, (T)-2), (T)H);
    const int w_low = (int)fmin(fmax(wf, (T)-2), (T)W);
    const int h_high = h_low + 1, w_high = w_low + 1;
    c.lh = h_im - hf; c.lw = w_im - wf;
    c.hh = (T)1 - c.lh; c.hw = (T)1 - c.lw;
    const bool hl = h_low >= 0 && h_low <= H - 1, hhv = h_high >= 0 && h_high <= H - 1;
    const bool wl = w_low >= 0 && w_low <= W - 1, whv = w_high >= 0 && w_high <= W - 1;
    c.k1 = c.live && hl && wl;  c.k2 = c.live && hl && whv;
    c.k3 = c.live && hhv && wl; c.k4 = c.live && hhv && whv;
    const int hlc = min(max(h_low, 0), H - 1), hhc = min(max(h_high, 0), H - 1);
    const int wlc = min(max(w_low, 0), W - 1), whc = min(max(w_high, 0), W - 1);
    c.o1 = hlc * W + wlc; c.o2 = hlc * W + whc; c.o3 = hhc * W + wlc; c.o4 = hhc * W + whc;
    c.w1 = c.hh * c.hw; c.w2 = c.hh * c.lw; c.w3 = c.lh * c.hw; c.w4 = c.lh * c.lw;
    return c;
}

// One-row-per-wave kernels: the row (b, q, m) of the calling wave; a wave whose row is >= nrows leaves as a whole.
// images_interleaved > 1: consecutive workgroups take the same query block of DIFFERENT images (msda_bwd_d64_pk).
__device__ __forceinline__ int wave_row(int nblk, int images_interleaved = 1) {
    int blk = xcd_logical_block(blockIdx.x, nblk);
    if (images_interleaved > 1) {
        const int per_image = nblk / images_interleaved;
        blk = (blk % images_interleaved) * per_image + blk / images_interleaved;
    }
    return blk * kRowsPerBlock + (threadIdx.x >> 6);
}

// ... and what it needs to know about that row: the number of points, head m of image b.
struct RowId {
    int LP, m, b;
};

__device__ __forceinline__ RowId row_id(int row, int M, int L, int Lq, int P) {
    RowId r;
    r.LP = L * P;
    r.m = row % M;
    r.b = (row / M) / Lq;
    return r;
}

// the two bf16 of a 32-bit word as floats (exact)
__device__ __forceinline__ float bf16_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

// v_readlane: lane `src`'s x for the whole wave (an SGPR: scalar branches, scalar addresses).  The result leaves through a
// reference on purpose: a returned scalar is marked noundef, which lets the compiler drop the freeze it otherwise puts behind the
// read and changes the register allocation of the D = 64 backward kernels.
__device__ __forceinline__ void readlane(int& out, int x, int src) { out = __builtin_amdgcn_readlane(x, src); }
__device__ __forceinline__ void readlane(float& out, float x, int src) {
    out = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), src));
}

// What one lane holds of a (pixel, head) row in a 16-byte load: 4 floats or 8 bf16.  Raw: the slice as loaded; Acc: its
// elements as float accumulators; Packed: the slice as stored.
template <typename T>
struct Slice;

template <>
struct Slice<float> {
    static constexpr int kElems = 4;
    typedef float4 Raw;
    typedef float4 Acc;
    typedef float4 Packed;
    static __device__ __forceinline__ float& at(float4& a, int e) { return e == 0 ? a.x : e == 1 ? a.y : e == 2 ? a.z : a.w; }
    static __device__ __forceinline__ void unpack(const float4& u, float (&f)[4]) {
        f[0] = u.x; f[1] = u.y; f[2] = u.z; f[3] = u.w;
    }
    static __device__ __forceinline__ float4 pack(const float4& a) { return a; }
};

template <>
struct Slice<__hip_bfloat16> {
    static constexpr int kElems = 8;
    typedef uint4 Raw;
    struct Acc {
        float f[8];
    };
    typedef __bf16 Packed __attribute__((ext_vector_type(8)));
    static __device__ __forceinline__ float& at(Acc& a, int e) { return a.f[e]; }
    static __device__ __forceinline__ void unpack(const uint4& u, float (&f)[8]) {
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            f[2 * i] = bf16_lo(w[i]);
            f[2 * i + 1] = bf16_hi(w[i]);
        }
    }
    static __device__ __forceinline__ Packed pack(const float (&f)[8]) {
        Packed o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (__bf16)f[e];
        return o;
    }
    static __device__ __forceinline__ Packed pack(const Acc& a) { return pack(a.f); }
};

// ---------------------------------------------------------------------------------------------------
// Forward, fast path, one row per wave: a (pixel, head) row of D channels is LPP lanes x 16 bytes, so the wave covers
// G = 64 / LPP sampling points side by side; NIT = ceil(L*P / G) point rounds.  A pixel is pix_units * UNIT elements: M heads of
// UNIT = D for the dense f32 maps (64-bit products, as those kernels always formed them), pix_el elements of UNIT = 1 for bf16.
// ---------------------------------------------------------------------------------------------------
template <typename T, int LPP, int NIT, int UNIT>
__device__ __forceinline__ void msda_fwd_row(const T* value, const int64_t* shapes,
                                             const int64_t* lsi, const float* loc,
                                             const float* aw, int S, int M, int L, int Lq, int P,
                                             T* out, int nrows, int nblk, int pix_units) {
    typedef Slice<T> Sl;
    constexpr int E = Sl::kElems;
    constexpr int D = E * LPP;
    constexpr int G = kWave / LPP;  // sampling points handled side by side
    const int lane = threadIdx.x & (kWave - 1);
    const int row = wave_row(nblk);
    if (row >= nrows) return;
    const RowId r = row_id(row, M, L, Lq, P);
    const int LP = r.LP;

    // one coalesced read of the row's 2*LP coordinates and LP weights (LP <= 32 on this path)
    const float locv = lane < 2 * LP ? loc[(size_t)row * 2 * LP + lane] : 0.f;
    const float awv = lane < LP ? aw[(size_t)row * LP + lane] : 0.f;

    const int g = lane / LPP, ce = lane % LPP;
    const T* vrow = value + (size_t)r.b * S * pix_units * UNIT + (size_t)r.m * D + ce * E;
    const size_t pix_stride = (size_t)pix_units * UNIT;

    typename Sl::Raw v[NIT][4];
    float cw[NIT][4];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int idx = it * G + g;
        const bool have = idx < LP;
        const int idc = have ? idx : LP - 1;
        const float x = __shfl(locv, 2 * idc, kWave);
        const float y = __shfl(locv, 2 * idc + 1, kWave);
        // the shuffle stays outside the select: under `have ? ... : ...` only the lanes that have a point may run it, and a
        // lane reads 0 from a source lane that sits out -- lane L*P - 1 whenever L*P = G*it + 1 leaves it to one group
        const float wsrc = __shfl(awv, idc, kWave);
        const float wt = have ? wsrc : 0.f;
        const int l = idc / P;
        const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
        const T* vl = vrow + (size_t)lsi[l] * pix_stride;
        const Corners<float> c = make_corners<float>(x, y, H, W);
        v[it][0] = *reinterpret_cast<const typename Sl::Raw*>(vl + (size_t)c.o1 * pix_stride);
        v[it][1] = *reinterpret_cast<const typename Sl::Raw*>(vl + (size_t)c.o2 * pix_stride);
        v[it][2] = *reinterpret_cast<const typename Sl::Raw*>(vl + (size_t)c.o3 * pix_stride);
        v[it][3] = *reinterpret_cast<const typename Sl::Raw*>(vl + (size_t)c.o4 * pix_stride);
        cw[it][0] = c.k1 ? c.w1 * wt : 0.f;
        cw[it][1] = c.k2 ? c.w2 * wt : 0.f;
        cw[it][2] = c.k3 ? c.w3 * wt : 0.f;
        cw[it][3] = c.k4 ? c.w4 * wt : 0.f;
    }
    typename Sl::Acc acc;
#pragma unroll
    for (int e = 0; e < E; ++e) Sl::at(acc, e) = 0.f;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // select, not multiply: a non-finite value under a dropped corner must not leak
            const float w = cw[it][k];
            float f[E];
            Sl::unpack(v[it][k], f);
#pragma unroll
            for (int e = 0; e < E; ++e) Sl::at(acc, e) += w != 0.f ? w * f[e] : 0.f;
        }
    }
#pragma unroll
    for (int off = LPP; off < kWave; off <<= 1)
#pragma unroll
        for (int e = 0; e < E; ++e) Sl::at(acc, e) += __shfl_xor(Sl::at(acc, e), off, kWave);
    if (lane < LPP) {
        const typename Sl::Packed o = Sl::pack(acc);
        *reinterpret_cast<typename Sl::Packed*>(out + (size_t)row * D + lane * E) = o;
    }
}

// f32 maps, D = 4*LPP (64 or 32), dense
template <int LPP, int NIT>
__global__ __launch_bounds__(kWave * kRowsPerBlock)
void msda_fwd_vec4(const float* __restrict__ value, const int64_t* __restrict__ shapes,
                   const int64_t* __restrict__ lsi, const float* __restrict__ loc,
                   const float* __restrict__ aw, int S, int M, int L, int Lq, int P,
                   float* __restrict__ out, int nrows, int nblk) {
    msda_fwd_row<float, LPP, NIT, 4 * LPP>(value, shapes, lsi, loc, aw, S, M, L, Lq, P, out, nrows, nblk, M);
}

// bf16 maps (training path: value_proj output stays bf16, no fp32 staging copy), D = 64: a (pixel, head) slice is 128 bytes =
// 8 lanes x 16 bytes, so a wave covers 8 sampling points at once.  pix_el: elements per pixel, M*D when the map is dense.
template <int NIT>
__global__ __launch_bounds__(kWave * kRowsPerBlock)
void msda_fwd_bf16_d64(const __hip_bfloat16* __restrict__ value, const int64_t* __restrict__ shapes,
                       const int64_t* __restrict__ lsi, const float* __restrict__ loc, const float* __restrict__ aw,
                       int S, int M, int L, int Lq, int P, __hip_bfloat16* __restrict__ out, int nrows, int nblk,
                       int pix_el) {
    msda_fwd_row<__hip_bfloat16, 8, NIT, 1>(value, shapes, lsi, loc, aw, S, M, L, Lq, P, out, nrows, nblk, pix_el);
}

// ---------------------------------------------------------------------------------------------------
// Forward, any D / L / P, float or double: lanes stride the channels of the wave's row.
// ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kWave * kRowsPerBlock)
void msda_fwd_generic(const T* __restrict__ value, const int64_t* __restrict__ shapes,
                      const int64_t* __restrict__ lsi, const T* __restrict__ loc,
                      const T* __restrict__ aw, int S, int M, int D, int L, int Lq, int P,
                      T* __restrict__ out, int nrows, int nblk) {
    const int lane = threadIdx.x & (kWave - 1);
    const int row = wave_row(nblk);
    if (row >= nrows) return;
    const RowId r = row_id(row, M, L, Lq, P);
    const int LP = r.LP;
    const size_t pix_stride = (size_t)M * D;
    const T* vhead = value + (size_t)r.b * S * pix_stride + (size_t)r.m * D;
    const T* lrow = loc + (size_t)row * 2 * LP;
    const T* wrow = aw + (size_t)row * LP;
    for (int c = lane; c < D; c += kWave) {
        T acc = 0;
        for (int l = 0; l < L; ++l) {
            const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
            const T* vl = vhead + (size_t)lsi[l] * pix_stride + c;
            for (int p = 0; p < P; ++p) {
                const int idx = l * P + p;
                const Corners<T> k = make_corners<T>(lrow[2 * idx], lrow[2 * idx + 1], H, W);
                if (!k.live) continue;
                const T v1 = k.k1 ? vl[(size_t)k.o1 * pix_stride] : (T)0;
                const T v2 = k.k2 ? vl[(size_t)k.o2 * pix_stride] : (T)0;
                const T v3 = k.k3 ? vl[(size_t)k.o3 * pix_stride] : (T)0;
                const T v4 = k.k4 ? vl[(size_t)k.o4 * pix_stride] : (T)0;
                acc += (k.w1 * v1 + k.w2 * v2 + k.w3 * v3 + k.w4 * v4) * wrow[idx];
            }
        }
        out[(size_t)row * D + c] = acc;
    }
}

// ---------------------------------------------------------------------------------------------------
// Backward, any D / L / P: lane = channel (strided when D > 64).  PU points are loaded together
// (4*PU independent loads per lane) before the atomics of any of them are issued.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ void atomic_add_fast(float* p, float v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void atomic_add_fast(double* p, double v) { unsafeAtomicAdd(p, v); }

template <typename T, int PU>
__global__ __launch_bounds__(kWave * kRowsPerBlock)
void msda_bwd_generic(const T* __restrict__ value, const int64_t* __restrict__ shapes,
                      const int64_t* __restrict__ lsi, const T* __restrict__ loc,
                      const T* __restrict__ aw, const T* __restrict__ grad_out,
                      int S, int M, int D, int L, int Lq, int P,
                      T* __restrict__ grad_value, T* __restrict__ grad_loc, T* __restrict__ grad_aw,
                      int nrows, int nblk) {
    const int lane = threadIdx.x & (kWave - 1);
    const int row = wave_row(nblk);
    if (row >= nrows) return;
    const RowId r = row_id(row, M, L, Lq, P);
    const int LP = r.LP;
    const size_t pix_stride = (size_t)M * D;
    const size_t head_off = (size_t)r.b * S * pix_stride + (size_t)r.m * D;
    const T* lrow = loc + (size_t)row * 2 * LP;
    const T* wrow = aw + (size_t)row * LP;

    for (int i0 = 0; i0 < LP; i0 += PU) {
        T gx[PU], gy[PU], ga[PU];
#pragma unroll
        for (int u = 0; u < PU; ++u) gx[u] = gy[u] = ga[u] = 0;
        for (int c = lane; c < D; c += kWave) {
            const T go = grad_out[(size_t)row * D + c];
            Corners<T> k[PU];
            size_t base[PU];
            T wt[PU], v1[PU], v2[PU], v3[PU], v4[PU];
            int Hs[PU], Ws[PU];
#pragma unroll
            for (int u = 0; u < PU; ++u) {
                const int idx = min(i0 + u, LP - 1);
                const int l = idx / P;
                Hs[u] = (int)shapes[2 * l]; Ws[u] = (int)shapes[2 * l + 1];
                base[u] = head_off + (size_t)lsi[l] * pix_stride + c;
                k[u] = make_corners<T>(lrow[2 * idx], lrow[2 * idx + 1], Hs[u], Ws[u]);
                if (i0 + u >= LP) k[u].live = k[u].k1 = k[u].k2 = k[u].k3 = k[u].k4 = false;
                wt[u] = wrow[idx];
                v1[u] = value[base[u] + (size_t)k[u].o1 * pix_stride];
                v2[u] = value[base[u] + (size_t)k[u].o2 * pix_stride];
                v3[u] = value[base[u] + (size_t)k[u].o3 * pix_stride];
                v4[u] = value[base[u] + (size_t)k[u].o4 * pix_stride];
            }
#pragma unroll
            for (int u = 0; u < PU; ++u) {
                const Corners<T>& q = k[u];
                const T tgv = go * wt[u];
                const T a1 = q.k1 ? v1[u] : (T)0, a2 = q.k2 ? v2[u] : (T)0;
                const T a3 = q.k3 ? v3[u] : (T)0, a4 = q.k4 ? v4[u] : (T)0;
                if (q.k1) atomic_add_fast(grad_value + base[u] + (size_t)q.o1 * pix_stride, q.w1 * tgv);
                if (q.k2) atomic_add_fast(grad_value + base[u] + (size_t)q.o2 * pix_stride, q.w2 * tgv);
                if (q.k3) atomic_add_fast(grad_value + base[u] + (size_t)q.o3 * pix_stride, q.w3 * tgv);
                if (q.k4) atomic_add_fast(grad_value + base[u] + (size_t)q.o4 * pix_stride, q.w4 * tgv);
                // d/dh and d/dw of the bilinear form (dropped corners contribute nothing)
                const T gh = -q.hw * a1 - q.lw * a2 + q.hw * a3 + q.lw * a4;
                const T gw = -q.hh * a1 + q.hh * a2 - q.lh * a3 + q.lh * a4;
                const T val = q.w1 * a1 + q.w2 * a2 + q.w3 * a3 + q.w4 * a4;
                ga[u] += go * val;
                gx[u] += (T)Ws[u] * gw * tgv;
                gy[u] += (T)Hs[u] * gh * tgv;
            }
        }
#pragma unroll
        for (int u = 0; u < PU; ++u) {
            const T sx = wave_sum(gx[u]), sy = wave_sum(gy[u]), sa = wave_sum(ga[u]);
            if (lane == 0 && i0 + u < LP) {
                grad_aw[(size_t)row * LP + i0 + u] = sa;
                grad_loc[(size_t)row * 2 * LP + 2 * (i0 + u)] = sx;
                grad_loc[(size_t)row * 2 * LP + 2 * (i0 + u) + 1] = sy;
            }
        }
    }
}


// Forward for bf16 maps, D = 64, L*P <= 16 -- the training-step shape -- with the gather latency taken off the
// critical path.  The wave-per-row kernel above is latency x occupancy bound (two dependent HBM hops per wave:
// sampling geometry, then the corners; ~5 us of wave lifetime for < 1 us of work).  Here a wave owns FOUR rows:
//   * geometry: lane j computes point (j & 15) of row r0 + (j >> 4) ONCE (one coalesced float2 + float load for the
//     4 rows' 64 points) and parks {4 corner offsets, 4 corner weights x attention weight} in a wave-private 2 KB LDS
//     tile -- no ds_bpermute traffic, no 8x redundant corner arithmetic;
//   * gather: each 16-lane DPP row serves one output row; its two 8-lane halves walk 8 points each (a 128-byte
//     pixel-head slice = 8 lanes x 16 B), BATCH points (4*BATCH independent 16-byte loads per lane) in flight at a
//     time, addresses = uniform base + 32-bit offsets;
//   * fold: the two halves meet in ONE DPP row_ror:8 add per channel (no LDS shuffles), lanes 0-7 of each row store
//     the 128-byte output row.
//
// Rows4Point is the geometry stage, shared with msda_bwd_rows4: the point a lane computes for its wave's four rows.
struct Rows4Point {
    int row, p;               // row r0 + (lane >> 4), point lane & 15
    bool valid;               // the row exists and has a point p
    int rc;                   // row, clamped into the map (what the loads use)
    float wt;                 // attention weight, 0 when !valid
    int H, W;
    uint32_t base, pix;       // byte offset of the level's (image, head) map from `value`, bytes per pixel
    Corners<float> c;
};

__device__ __forceinline__ Rows4Point rows4_point(int r0, int lane, int nrows, const int64_t* shapes,
                                                  const int64_t* lsi, const float* loc,
                                                  const float* aw, int S, int M, int L, int Lq, int P,
                                                  int pix_el) {
    constexpr int D = 64;
    const int LP = L * P;
    Rows4Point g;
    g.row = r0 + (lane >> 4); g.p = lane & 15;
    g.valid = g.row < nrows && g.p < LP;
    g.rc = min(g.row, nrows - 1);
    const int pc = min(g.p, LP - 1);
    const float2 xy = *reinterpret_cast<const float2*>(loc + ((size_t)g.rc * LP + pc) * 2);
    g.wt = g.valid ? aw[(size_t)g.rc * LP + pc] : 0.f;
    const int l = pc / P;
    g.H = (int)shapes[2 * l]; g.W = (int)shapes[2 * l + 1];
    const uint32_t m = g.rc % M, b = (g.rc / M) / Lq;
    // byte offsets from `value` (pix_el elements per pixel, M*D when the map is dense); the launcher checks that
    // the whole map fits 32 bits
    g.pix = (uint32_t)pix_el * 2;
    g.base = (b * (uint32_t)S + (uint32_t)lsi[l]) * g.pix + m * (D * 2);
    g.c = make_corners<float>(xy.x, xy.y, g.H, g.W);
    return g;
}

// byte offset from `value` of the (pixel, head) slice at clamped pixel `o` of the point's level: always a legal address
__device__ __forceinline__ uint32_t rows4_offset(const Rows4Point& g, int o) { return g.base + o * g.pix; }

// where the 8 points that this lane's half (8 lanes) of its 16-lane row walks are parked in the wave's tile
__device__ __forceinline__ int rows4_half_points(int lane) { return (lane & 48) + (lane & 8); }

template <int BATCH>
__global__ __launch_bounds__(256)
void msda_fwd_bf16_rows4(const __hip_bfloat16* __restrict__ value, const int64_t* __restrict__ shapes,
                         const int64_t* __restrict__ lsi, const float* __restrict__ loc, const float* __restrict__ aw,
                         int S, int M, int L, int Lq, int P, __hip_bfloat16* __restrict__ out, int nrows, int nblk,
                         int pix_el) {
    constexpr int D = 64;
    __shared__ uint4 geo[4][64][2];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = (xcd_logical_block(blockIdx.x, nblk) * 4 + wave) * 4;
    if (r0 >= nrows) return;
    {
        const Rows4Point pt = rows4_point(r0, lane, nrows, shapes, lsi, loc, aw, S, M, L, Lq, P, pix_el);
        const Corners<float>& c = pt.c;
        const float wt = pt.wt;
        geo[wave][lane][0] = make_uint4(rows4_offset(pt, c.o1), rows4_offset(pt, c.o2), rows4_offset(pt, c.o3), rows4_offset(pt, c.o4));
        geo[wave][lane][1] = make_uint4(__float_as_uint(c.k1 ? c.w1 * wt : 0.f), __float_as_uint(c.k2 ? c.w2 * wt : 0.f),
                                        __float_as_uint(c.k3 ? c.w3 * wt : 0.f), __float_as_uint(c.k4 ? c.w4 * wt : 0.f));
    }
    __builtin_amdgcn_wave_barrier();
    const int c8 = lane & 7;
    const uint32_t cb = c8 * 16;
    const uint4(*g)[2] = &geo[wave][rows4_half_points(lane)];  // this half's 8 points of this row
    const char* vb = reinterpret_cast<const char*>(value);
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 acc[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};  // channels (2j, 2j+1): v_pk_fma_f32
#pragma unroll
    for (int it0 = 0; it0 < 8; it0 += BATCH) {
        uint4 v[BATCH][4];
        float w[BATCH][4];
#pragma unroll
        for (int i = 0; i < BATCH; ++i) {
            const uint4 o = g[it0 + i][0], ww = g[it0 + i][1];
            v[i][0] = *reinterpret_cast<const uint4*>(vb + (o.x + cb));
            v[i][1] = *reinterpret_cast<const uint4*>(vb + (o.y + cb));
            v[i][2] = *reinterpret_cast<const uint4*>(vb + (o.z + cb));
            v[i][3] = *reinterpret_cast<const uint4*>(vb + (o.w + cb));
            w[i][0] = __uint_as_float(ww.x); w[i][1] = __uint_as_float(ww.y);
            w[i][2] = __uint_as_float(ww.z); w[i][3] = __uint_as_float(ww.w);
        }
        __builtin_amdgcn_sched_barrier(0);  // every gather of the batch is in flight before the first one is consumed
#pragma unroll
        for (int i = 0; i < BATCH; ++i)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // a corner outside the map carries weight 0 and a clamped address: whatever was loaded there (even a
                // NaN) must contribute exactly nothing, as in the reference, which never reads it
                const bool dead = w[i][k] == 0.f;
                const uint32_t d[4] = {dead ? 0u : v[i][k].x, dead ? 0u : v[i][k].y, dead ? 0u : v[i][k].z, dead ? 0u : v[i][k].w};
                const f2 w2 = {w[i][k], w[i][k]};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f2 f = {bf16_lo(d[j]), bf16_hi(d[j])};
                    acc[j] = __builtin_elementwise_fma(w2, f, acc[j]);
                }
            }
    }
    float r[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // lanes l and l ^ 8 of a 16-lane row: row_ror:8
        r[2 * j] = acc[j].x + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(acc[j].x), 0x128, 0xf, 0xf, true));
        r[2 * j + 1] = acc[j].y + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(acc[j].y), 0x128, 0xf, 0xf, true));
    }
    const int row = r0 + (lane >> 4);
    if ((lane & 8) == 0 && row < nrows) {
        const Slice<__hip_bfloat16>::Packed o = Slice<__hip_bfloat16>::pack(r);
        *reinterpret_cast<Slice<__hip_bfloat16>::Packed*>(out + (size_t)row * D + c8 * 8) = o;
    }
}

// grad_loc / grad_attn_w for bf16 maps, D = 64, L*P <= 16, in the shape of msda_fwd_bf16_rows4: a wave owns four rows, lane j
// computes point (j & 15) of row r0 + (j >> 4) once and parks the corner offsets in LDS; each 16-lane row serves one (b, q, m)
// row, its two 8-lane halves walk 8 points each with 8 channels (16 B) per lane.  Everything the two gradients need from the
// value map are the four scalars  a_k = <grad_out row, corner k row>  per point (ms_deform_im2col_cuda.cuh:97-158 with the
// channel sum pulled inside): 8 multiply-adds per gathered 16 bytes, then ONE 32-value butterfly over the 8 lanes of a half
// (28 exchanges for four rows; the one-row-per-wave walk above spends 63 per row), after which lane j holds the four dots of
// exactly the point whose geometry it computed.
template <int BATCH>
__global__ __launch_bounds__(256)
void msda_bwd_rows4(const __hip_bfloat16* __restrict__ value, const int64_t* __restrict__ shapes,
                    const int64_t* __restrict__ lsi, const float* __restrict__ loc, const float* __restrict__ aw,
                    const __hip_bfloat16* __restrict__ grad_out, int S, int M, int L, int Lq, int P,
                    float* __restrict__ grad_loc, float* __restrict__ grad_aw, int nrows, int nblk, int pix_el) {
    constexpr int D = 64;
    __shared__ uint4 geo[4][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r0 = (xcd_logical_block(blockIdx.x, nblk) * 4 + wave) * 4;
    if (r0 >= nrows) return;
    const int LP = L * P;
    const Rows4Point pt = rows4_point(r0, lane, nrows, shapes, lsi, loc, aw, S, M, L, Lq, P, pix_el);
    const Corners<float>& c = pt.c;
    const int row = pt.row, p = pt.p, rc = pt.rc, H = pt.H, W = pt.W;
    const bool valid = pt.valid;
    const float wt = pt.wt;
    // a dead corner keeps its clamped (legal) address; bit 0 of the byte offset marks it (offsets are multiples of 16)
    geo[wave][lane] = make_uint4(rows4_offset(pt, c.o1) | (c.k1 ? 0u : 1u), rows4_offset(pt, c.o2) | (c.k2 ? 0u : 1u),
                                 rows4_offset(pt, c.o3) | (c.k3 ? 0u : 1u), rows4_offset(pt, c.o4) | (c.k4 ? 0u : 1u));
    __builtin_amdgcn_wave_barrier();
    const int c8 = lane & 7;
    const uint32_t cb = c8 * 16;
    const uint4* g = &geo[wave][rows4_half_points(lane)];  // this half's 8 points of this row
    const char* vb = reinterpret_cast<const char*>(value);
    typedef float f2 __attribute__((ext_vector_type(2)));
    f2 go2[4];
    {
        const uint4 gq = *reinterpret_cast<const uint4*>(grad_out + (size_t)rc * D + c8 * 8);
        const uint32_t gw[4] = {gq.x, gq.y, gq.z, gq.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) go2[j] = f2{bf16_lo(gw[j]), bf16_hi(gw[j])};
    }
    float d[32];  // d[4 i + k]: this lane's 8 channels of <grad_out, corner k of this half's point i>
#pragma unroll
    for (int it0 = 0; it0 < 8; it0 += BATCH) {
        uint4 v[BATCH][4];
        uint4 o[BATCH];
#pragma unroll
        for (int i = 0; i < BATCH; ++i) {
            o[i] = g[it0 + i];
            v[i][0] = *reinterpret_cast<const uint4*>(vb + ((o[i].x & ~1u) + cb));
            v[i][1] = *reinterpret_cast<const uint4*>(vb + ((o[i].y & ~1u) + cb));
            v[i][2] = *reinterpret_cast<const uint4*>(vb + ((o[i].z & ~1u) + cb));
            v[i][3] = *reinterpret_cast<const uint4*>(vb + ((o[i].w & ~1u) + cb));
        }
        __builtin_amdgcn_sched_barrier(0);  // every gather of the batch is in flight before the first one is consumed
#pragma unroll
        for (int i = 0; i < BATCH; ++i) {
            const uint32_t dead[4] = {o[i].x & 1u, o[i].y & 1u, o[i].z & 1u, o[i].w & 1u};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // a corner outside the map: whatever sits at its clamped address (even a NaN) contributes exactly nothing
                const uint32_t w4[4] = {dead[k] ? 0u : v[i][k].x, dead[k] ? 0u : v[i][k].y, dead[k] ? 0u : v[i][k].z,
                                        dead[k] ? 0u : v[i][k].w};
                f2 a = {0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    a = __builtin_elementwise_fma(go2[j], f2{bf16_lo(w4[j]), bf16_hi(w4[j])}, a);
                d[4 * (it0 + i) + k] = a.x + a.y;
            }
        }
    }
    // 32 values over the 8 lanes of the half: three halving exchanges (lane bit 2 <-> point bit 2, ...), after which lane j of the
    // half holds d[0..3] = the four dots of point j of the half, i.e. of point (lane & 15) of its row
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const bool hi = lane & 4;
        const float keep = hi ? d[16 + i] : d[i], send = hi ? d[i] : d[16 + i];
        d[i] = keep + __shfl_xor(send, 4, kWave);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const bool hi = lane & 2;
        const float keep = hi ? d[8 + i] : d[i], send = hi ? d[i] : d[8 + i];
        d[i] = keep + __shfl_xor(send, 2, kWave);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool hi = lane & 1;
        const float keep = hi ? d[4 + i] : d[i], send = hi ? d[i] : d[4 + i];
        d[i] = keep + __shfl_xor(send, 1, kWave);
    }
    if (valid) {
        const float a1 = d[0], a2 = d[1], a3 = d[2], a4 = d[3];  // already zero for dead corners
        const float gh = -c.hw * a1 - c.lw * a2 + c.hw * a3 + c.lw * a4;
        const float gw = -c.hh * a1 + c.hh * a2 - c.lh * a3 + c.lh * a4;
        const float val = c.w1 * a1 + c.w2 * a2 + c.w3 * a3 + c.w4 * a4;
        grad_aw[(size_t)row * LP + p] = val;
        *reinterpret_cast<float2*>(grad_loc + ((size_t)row * LP + p) * 2) = make_float2((float)W * wt * gw, (float)H * wt * gh);
    }
}

__device__ __forceinline__ float ldv(const float* p) { return *p; }
__device__ __forceinline__ float ldv(const __hip_bfloat16* p) { return __bfloat162float(*p); }


// 64-value butterfly: every lane holds v[0..63]; after 6 halving exchanges lane L holds the wave-wide sum of
// v[bitreverse6(L)].  63 shuffles instead of 64 x 6 for separate reductions.
template <int N>
__device__ __forceinline__ void halve_step(float (&v)[64], int lane, int off) {
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
        const bool hi = lane & off;
        const float keep = hi ? v[2 * i + 1] : v[2 * i];
        const float send = hi ? v[2 * i] : v[2 * i + 1];
        v[i] = keep + __shfl_xor(send, off, kWave);
    }
}

// The tail of the one-row-per-wave backward kernels: every lane holds its channels' share of part[0,16) = grad_attn_w per
// point and part[16,48) = grad_loc (x, y) per point; the butterfly sums them over the wave and each lane stores the one it owns.
__device__ __forceinline__ void store_row_grads(float (&part)[64], int lane, int row, int LP, float* grad_loc,
                                                float* grad_aw) {
    halve_step<64>(part, lane, 32);
    halve_step<32>(part, lane, 16);
    halve_step<16>(part, lane, 8);
    halve_step<8>(part, lane, 4);
    halve_step<4>(part, lane, 2);
    halve_step<2>(part, lane, 1);
    const int j = (int)(__brev((unsigned)lane) >> 26);  // index of the value this lane now owns
    if (j < LP) grad_aw[(size_t)row * LP + j] = part[0];
    else if (j >= 16 && j < 16 + 2 * LP) grad_loc[(size_t)row * 2 * LP + (j - 16)] = part[0];
}

// Geometry ONCE per row, point p on lane p (the reference and the generic kernel redo it on every channel lane); the per-point
// scalars then reach all lanes through readlane.  Lanes past the row's last point hold a copy of it with flags = 0, wt = 0.
struct LanePoint {
    int e1, e2, e3, e4;  // cells of the four corners inside one (image, head) map: level start + clamped corner offset
    int flags;           // bit k - 1: corner k lies inside the map
    float lh, lw, wt;    // bilinear fractions, attention weight
    float fW, fH;        // W * wt, H * wt
};

__device__ __forceinline__ LanePoint lane_point(const int64_t* shapes, const int64_t* lsi,
                                                const float* loc, const float* aw, int row, int lane,
                                                int LP, int P) {
    const int pi = min(lane, LP - 1), pl = pi / P;
    const int pH = (int)shapes[2 * pl], pW = (int)shapes[2 * pl + 1], pst = (int)lsi[pl];
    const float px = loc[(size_t)row * 2 * LP + 2 * pi], py = loc[(size_t)row * 2 * LP + 2 * pi + 1];
    const float pwt = lane < LP ? aw[(size_t)row * LP + pi] : 0.f;
    const Corners<float> c = make_corners<float>(px, py, pH, pW);
    LanePoint pt;
    pt.e1 = pst + c.o1; pt.e2 = pst + c.o2; pt.e3 = pst + c.o3; pt.e4 = pst + c.o4;
    pt.flags = lane < LP ? ((c.k1 ? 1 : 0) | (c.k2 ? 2 : 0) | (c.k3 ? 4 : 0) | (c.k4 ? 8 : 0)) : 0;
    pt.lh = c.lh; pt.lw = c.lw; pt.wt = pwt;
    pt.fW = (float)pW * pwt; pt.fH = (float)pH * pwt;
    return pt;
}

// point p of the row (the one lane p computed), the same on every lane
__device__ __forceinline__ LanePoint point_at(const LanePoint& pt, int p) {
    LanePoint u;
    readlane(u.flags, pt.flags, p);
    readlane(u.e1, pt.e1, p); readlane(u.e2, pt.e2, p); readlane(u.e3, pt.e3, p); readlane(u.e4, pt.e4, p);
    readlane(u.lh, pt.lh, p); readlane(u.lw, pt.lw, p); readlane(u.wt, pt.wt, p);
    readlane(u.fW, pt.fW, p); readlane(u.fH, pt.fH, p);
    return u;
}

// points p and q of the row have the same live corners in the same cells; read and compared field by field, as far as they agree
__device__ __forceinline__ bool same_at(int x, int p, int q) {
    int a, b;
    readlane(a, x, p);
    readlane(b, x, q);
    return a == b;
}

__device__ __forceinline__ bool same_cells(const LanePoint& pt, int p, int q) {
    return same_at(pt.e1, p, q) && same_at(pt.e2, p, q) && same_at(pt.e3, p, q) && same_at(pt.e4, p, q) &&
           same_at(pt.flags, p, q);
}

// Backward for D = 64, L*P <= 16, value / grad_out in f32 or bf16: one wave per (b, q, m) row, lane = channel.
// (Measured alternatives, see profiles/r01/msda_bwd_ablation.txt: keeping the coarse levels' gradient in LDS with
//  ds_add_f32 is SLOWER than global float atomics on gfx950 -- ~150 cycles per LDS float-atomic wave instruction --
//  and software-pipelining rows at 8 waves/CU loses more from the lower occupancy than it hides.)
template <typename VT>
__global__ __launch_bounds__(kWave * kRowsPerBlock)
void msda_bwd_d64(const VT* __restrict__ value, const int64_t* __restrict__ shapes, const int64_t* __restrict__ lsi,
                  const float* __restrict__ loc, const float* __restrict__ aw, const VT* __restrict__ grad_out,
                  int S, int M, int L, int Lq, int P, float* __restrict__ grad_value, float* __restrict__ grad_loc,
                  float* __restrict__ grad_aw, int nrows, int nblk) {
    constexpr int D = 64, kMaxLP = 16;
    const int lane = threadIdx.x & (kWave - 1);
    const int row = wave_row(nblk);
    if (row >= nrows) return;
    const RowId r = row_id(row, M, L, Lq, P);
    const int LP = r.LP;
    const int pix_stride = M * D;
    const size_t head_off = (size_t)r.b * S * pix_stride + (size_t)r.m * D;
    const VT* vhead = value + head_off + lane;
    float* ghead = grad_value + head_off + lane;
    const float go = ldv(grad_out + (size_t)row * D + lane);
    const LanePoint pt = lane_point(shapes, lsi, loc, aw, row, lane, LP, P);

    float part[64];  // [0,16): grad_attn_w per point, [16,48): grad_loc (x, y) per point, rest zero
#pragma unroll
    for (int i = 0; i < 64; ++i) part[i] = 0.f;
#pragma unroll
    for (int p = 0; p < kMaxLP; ++p) {
        if (p < LP) {
            const LanePoint u = point_at(pt, p);
            const int f = u.flags, s1 = u.e1, s2 = u.e2, s3 = u.e3, s4 = u.e4;
            const float lh = u.lh, lw = u.lw, wt = u.wt, sW = u.fW, sH = u.fH;
            const float hh = 1.f - lh, hw = 1.f - lw;
            // clamped indices are always legal: load all four, select by the validity bits
            const float r1 = ldv(vhead + (size_t)s1 * pix_stride), r2 = ldv(vhead + (size_t)s2 * pix_stride);
            const float r3 = ldv(vhead + (size_t)s3 * pix_stride), r4 = ldv(vhead + (size_t)s4 * pix_stride);
            const float a1 = (f & 1) ? r1 : 0.f, a2 = (f & 2) ? r2 : 0.f, a3 = (f & 4) ? r3 : 0.f, a4 = (f & 8) ? r4 : 0.f;
            const float tgv = go * wt;
            if (f & 1) atomic_add_fast(ghead + (size_t)s1 * pix_stride, hh * hw * tgv);
            if (f & 2) atomic_add_fast(ghead + (size_t)s2 * pix_stride, hh * lw * tgv);
            if (f & 4) atomic_add_fast(ghead + (size_t)s3 * pix_stride, lh * hw * tgv);
            if (f & 8) atomic_add_fast(ghead + (size_t)s4 * pix_stride, lh * lw * tgv);
            const float gh = -hw * a1 - lw * a2 + hw * a3 + lw * a4;
            const float gw = -hh * a1 + hh * a2 - lh * a3 + lh * a4;
            const float val = hh * hw * a1 + hh * lw * a2 + lh * hw * a3 + lh * lw * a4;
            part[p] = go * val;
            part[16 + 2 * p] = sW * gw * go;
            part[17 + 2 * p] = sH * gh * go;
        }
    }
    store_row_grads(part, lane, row, LP, grad_loc, grad_aw);
}

// Backward for bf16 maps with the value gradient accumulated IN bf16 by packed atomics (global_atomic_pk_add_bf16: two
// channels per 32-bit atomic -- measured 655 G channel-adds/s against 323 G for f32 atomics, tools/micro/atomic_rate.hip;
// the f32 kernel above is bound by exactly that rate).  This is what torch's own bf16 scatter / grid_sample backward do
// (atomic adds on the bf16 tensor); against f32 accumulation + one final rounding the relative L2 error of grad_value goes
// from 1.7e-3 to 4.0e-3 on the benchmark geometry (profiles/r01/msda_bwd_bf16_accumulate.txt).  The f32 kernel stays the
// parity path (f32 maps) and can be forced for bf16 maps (GRIT_MSDA_BWD_F32ACC=1).
// Lane = channel PAIR: the two 32-lane halves of the wave walk the even / odd points of the row, so one wave instruction
// gathers or scatters two 128-byte pixel-head rows; grad_loc / grad_w leave through the same 63-shuffle butterfly.
//
// STAGE = true: the same row walk (gathers, geometry, merges, grad_loc / grad_w) with the value gradient accumulated in
// FLOAT32 -- the reference's atomicAdd precision (ms_deform_im2col_cuda.cuh:125-152) -- into a dense staging map
// stage[B, S, M, 64] that arrives zeroed.  The scatter there is lane = channel with wave-uniform point and weight (one
// 256-byte contiguous wave atomic per corner, the full-rate shape of msda_bwd_d64), the weights taken by v_readlane from the
// lane that computed the point.  Every cell a row touches is marked in cell_flags[B, S, M] (plain byte stores of 1: all
// writers write the same value), so msda_stage_flush visits the touched cells only: it rounds them once into the bf16
// gradient map and leaves stage and flags zeroed for the next launch.
enum class Scatter {
    kPacked,  // packed-bf16 atomics into grad_value
    kStaged,  // (STAGE) f32 atomics into the staging map
    kNone,    // NO scatter at all: the row walk only produces grad_loc / grad_attn_w, the value gradient comes from the
              // gather-form kernel further down (msda_bwd_value)
};

// The four bilinear weights x attention weight of a point.
struct CornerWeights {
    float w1, w2, w3, w4;
};

__device__ __forceinline__ CornerWeights corner_weights(const LanePoint& u) {
    const float hh = (1.f - u.lh) * u.wt, lhw = u.lh * u.wt;
    return CornerWeights{hh * (1.f - u.lw), hh * u.lw, lhw * (1.f - u.lw), lhw * u.lw};
}

__device__ __forceinline__ void add(CornerWeights& a, const CornerWeights& b) {
    a.w1 += b.w1; a.w2 += b.w2; a.w3 += b.w3; a.w4 += b.w4;
}

// w += corner_weights(u), as the merged sums have always been written: each product and its add in one expression.  With this
// compiler add(w, corner_weights(u)) gives the same fma's and the same sums; the second spelling exists for register allocation
// alone (the packed kernel takes 94 instead of 92 VGPRs without it, at equal occupancy, profiles/msda_refactor/README.md).
__device__ __forceinline__ void add_corner_weights(CornerWeights& w, const LanePoint& u) {
    const float hh = (1.f - u.lh) * u.wt, lhw = u.lh * u.wt;
    w.w1 += hh * (1.f - u.lw); w.w2 += hh * u.lw; w.w3 += lhw * (1.f - u.lw); w.w4 += lhw * u.lw;
}

// the live corners of point u take w x (this lane's channel of grad_out) in f32: shead is the lane's channel of the staging map
__device__ __forceinline__ void staged_atomics(float* shead, int pix_stride, const LanePoint& u, const CornerWeights& w,
                                               float go_ch) {
    if (u.flags & 1) atomic_add_fast(shead + (size_t)u.e1 * pix_stride, w.w1 * go_ch);
    if (u.flags & 2) atomic_add_fast(shead + (size_t)u.e2 * pix_stride, w.w2 * go_ch);
    if (u.flags & 4) atomic_add_fast(shead + (size_t)u.e3 * pix_stride, w.w3 * go_ch);
    if (u.flags & 8) atomic_add_fast(shead + (size_t)u.e4 * pix_stride, w.w4 * go_ch);
}

// the live corners of point u take w x (this lane's channel pair go0, go1) as one packed bf16 atomic each
__device__ __forceinline__ void packed_atomics(__hip_bfloat16* ghead, int pix_stride, const LanePoint& u, const CornerWeights& w,
                                               float go0, float go1) {
    typedef __bf16 v2bf __attribute__((ext_vector_type(2)));
    typedef v2bf __attribute__((address_space(1))) * gv2bf_ptr;
    if (u.flags & 1) __builtin_amdgcn_global_atomic_fadd_v2bf16((gv2bf_ptr)(ghead + (size_t)u.e1 * pix_stride), v2bf{(__bf16)(w.w1 * go0), (__bf16)(w.w1 * go1)});
    if (u.flags & 2) __builtin_amdgcn_global_atomic_fadd_v2bf16((gv2bf_ptr)(ghead + (size_t)u.e2 * pix_stride), v2bf{(__bf16)(w.w2 * go0), (__bf16)(w.w2 * go1)});
    if (u.flags & 4) __builtin_amdgcn_global_atomic_fadd_v2bf16((gv2bf_ptr)(ghead + (size_t)u.e3 * pix_stride), v2bf{(__bf16)(w.w3 * go0), (__bf16)(w.w3 * go1)});
    if (u.flags & 8) __builtin_amdgcn_global_atomic_fadd_v2bf16((gv2bf_ptr)(ghead + (size_t)u.e4 * pix_stride), v2bf{(__bf16)(w.w4 * go0), (__bf16)(w.w4 * go1)});
}

// x of point 2i on the lower half of the wave, of point 2i + 1 on the upper
template <typename T>
__device__ __forceinline__ void pick(T& out, T x, int i, bool odd) {
    if (odd) readlane(out, x, 2 * i + 1);
    else readlane(out, x, 2 * i);
}

// Step i of a walk that gives the even points to the lower half of the wave and the odd ones to the upper: this half's point,
// with flags = 0 where the upper half has none (the last step of an odd L*P).
__device__ __forceinline__ LanePoint point_of_half(const LanePoint& pt, int i, bool odd, int LP) {
    LanePoint u;
    if (2 * i + 1 < LP || !odd) pick(u.flags, pt.flags, i, odd);
    else u.flags = 0;
    pick(u.e1, pt.e1, i, odd); pick(u.e2, pt.e2, i, odd); pick(u.e3, pt.e3, i, odd); pick(u.e4, pt.e4, i, odd);
    pick(u.lh, pt.lh, i, odd); pick(u.lw, pt.lw, i, odd); pick(u.wt, pt.wt, i, odd);
    pick(u.fW, pt.fW, i, odd); pick(u.fH, pt.fH, i, odd);
    return u;
}

template <Scatter MODE>
__global__ __launch_bounds__(kWave * kRowsPerBlock)
void msda_bwd_d64_pk(const __hip_bfloat16* __restrict__ value, const int64_t* __restrict__ shapes,
                     const int64_t* __restrict__ lsi, const float* __restrict__ loc, const float* __restrict__ aw,
                     const __hip_bfloat16* __restrict__ grad_out, int S, int M, int L, int Lq, int P,
                     __hip_bfloat16* __restrict__ grad_value, float* __restrict__ grad_loc, float* __restrict__ grad_aw,
                     int nrows, int nblk, int images_interleaved, int merge_disabled, int pix_el,
                     float* __restrict__ stage, unsigned char* __restrict__ cell_flags) {
    constexpr int D = 64, kMaxLP = 16;
    constexpr bool STAGE = MODE == Scatter::kStaged, PACKED = MODE == Scatter::kPacked;
    // image-interleaved order (wave_row): workgroups in flight together then scatter into different value maps.  A freshly
    // initialised GRIT puts every query's reference point near the image centre, so neighbouring queries of one image pile
    // their atomics onto the same few hundred pixels.
    const int lane = threadIdx.x & (kWave - 1);
    const int row = wave_row(nblk, images_interleaved);
    if (row >= nrows) return;
    const RowId r = row_id(row, M, L, Lq, P);
    const int LP = r.LP, m = r.m, b = r.b;
    const int pix_stride = pix_el;  // elements per pixel: M * D for a dense map
    const bool odd = lane >= 32;            // this half's points: 2i + odd
    const int cp = lane & 31;               // channels 2cp, 2cp + 1
    const size_t head_off = (size_t)b * S * pix_stride + (size_t)m * D + 2 * cp;
    const __hip_bfloat16* vhead = value + head_off;
    __hip_bfloat16* ghead = grad_value + head_off;

    const uint32_t gob = *reinterpret_cast<const uint32_t*>(grad_out + (size_t)row * D + 2 * cp);
    const float go0 = bf16_lo(gob), go1 = bf16_hi(gob);
    const LanePoint pt = lane_point(shapes, lsi, loc, aw, row, lane, LP, P);
    // STAGE: channel = lane view of this row's output gradient and of the staging map; touched cells flagged by the lane
    // that owns the point
    float go_ch = 0.f;
    float* shead = nullptr;
    if constexpr (STAGE) {
        go_ch = ldv(grad_out + (size_t)row * D + lane);
        shead = stage + (size_t)b * S * M * D + (size_t)m * D + lane;
        if (lane < LP) {
            unsigned char* fl = cell_flags + (size_t)b * S * M + m;
            if (pt.flags & 1) fl[(size_t)pt.e1 * M] = 1;
            if (pt.flags & 2) fl[(size_t)pt.e2 * M] = 1;
            if (pt.flags & 4) fl[(size_t)pt.e3 * M] = 1;
            if (pt.flags & 8) fl[(size_t)pt.e4 * M] = 1;
        }
    }

    float part[64];  // [0,16): grad_attn_w per point, [16,48): grad_loc (x, y) per point, rest zero
#pragma unroll
    for (int i = 0; i < 64; ++i) part[i] = 0.f;
    // all gathers of the row first (in the training step the value map is cold: one HBM round trip per row instead of
    // one per point pair), then the arithmetic and the scatters
    uint32_t rr[kMaxLP / 2][4];
#pragma unroll
    for (int i = 0; i < kMaxLP / 2; ++i) {
        if (2 * i < LP) {
            const LanePoint u = point_of_half(pt, i, odd, LP);
            const int s1 = u.e1, s2 = u.e2, s3 = u.e3, s4 = u.e4;
            rr[i][0] = *reinterpret_cast<const uint32_t*>(vhead + (size_t)s1 * pix_stride);
            rr[i][1] = *reinterpret_cast<const uint32_t*>(vhead + (size_t)s2 * pix_stride);
            rr[i][2] = *reinterpret_cast<const uint32_t*>(vhead + (size_t)s3 * pix_stride);
            rr[i][3] = *reinterpret_cast<const uint32_t*>(vhead + (size_t)s4 * pix_stride);
        }
    }
    // A freshly initialised model (and any query whose offsets are still small) puts the P points of a level into ONE
    // pixel cell: the four corner updates of the four points then hit the same four addresses.  That case is detected
    // per level with wave-uniform compares and the bilinear weights are summed first -- 4 half-wave atomics per level
    // instead of 8 full-wave ones, and a quarter of the same-address traffic.  Levels whose points differ take the
    // per-point path unchanged.
    const bool mergeable = MODE != Scatter::kNone && P == 4 && LP == kMaxLP && !merge_disabled;
    bool merged = false;
#pragma unroll
    for (int i = 0; i < kMaxLP / 2; ++i) {
        if (2 * i < LP) {
            if ((i & 1) == 0) {
                merged = mergeable;
                const int p0 = 2 * i;
#pragma unroll
                for (int k = 1; k < 4; ++k) merged = merged && same_cells(pt, p0, p0 + k);
                if (merged) {
                    CornerWeights sum = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < 4; ++k) add_corner_weights(sum, point_at(pt, p0 + k));
                    if constexpr (STAGE) {
                        staged_atomics(shead, M * D, point_at(pt, p0), sum, go_ch);
                    } else if (PACKED && !odd) {
                        packed_atomics(ghead, pix_stride, point_at(pt, p0), sum, go0, go1);
                    }
                }
            }
            const LanePoint u = point_of_half(pt, i, odd, LP);
            const int f = u.flags;
            const float lh = u.lh, lw = u.lw, wt = u.wt, sW = u.fW, sH = u.fH;
            const float hh = 1.f - lh, hw = 1.f - lw;
            const float w1 = hh * hw, w2 = hh * lw, w3 = lh * hw, w4 = lh * lw;
            if (!merged) {
                // the two points of this step (one per half-wave) in one cell: both halves would add to the same
                // addresses in the same instruction -- every lane can form the sum itself (the halves hold the same
                // channels), the lower half issues it
                const int pe = 2 * i, po = 2 * i + 1;  // the step's even and odd point
                const bool pair = mergeable && po < LP && same_cells(pt, pe, po);
                if constexpr (STAGE) {
                    // wave-uniform weights of the step's two points (pe on the lower half, po on the upper)
                    const LanePoint ue = point_at(pt, pe);
                    CornerWeights wa = corner_weights(ue);
                    if (po < LP) {
                        const LanePoint uo = point_at(pt, po);
                        const CornerWeights wb = corner_weights(uo);
                        if (pair) add(wa, wb);
                        else staged_atomics(shead, M * D, uo, wb, go_ch);
                    }
                    staged_atomics(shead, M * D, ue, wa, go_ch);
                }
                CornerWeights w = {w1 * wt, w2 * wt, w3 * wt, w4 * wt};
                bool issue = PACKED;
                if (pair) {
                    // the other half's point: 2i + 1 for the lower half (the only one that issues)
                    add_corner_weights(w, point_at(pt, po));
                    issue = PACKED && !odd;
                }
                if (PACKED && issue) packed_atomics(ghead, pix_stride, u, w, go0, go1);
            }
            // clamped indices are always legal: all four were loaded, select by the validity bits
            const uint32_t q1 = (f & 1) ? rr[i][0] : 0u, q2 = (f & 2) ? rr[i][1] : 0u, q3 = (f & 4) ? rr[i][2] : 0u, q4 = (f & 8) ? rr[i][3] : 0u;
            const float a1x = bf16_lo(q1), a1y = bf16_hi(q1);
            const float a2x = bf16_lo(q2), a2y = bf16_hi(q2);
            const float a3x = bf16_lo(q3), a3y = bf16_hi(q3);
            const float a4x = bf16_lo(q4), a4y = bf16_hi(q4);
            // the two channels of this lane folded right away: go . (d/dh, d/dw, value) of the bilinear form
            const float ghx = -hw * a1x - lw * a2x + hw * a3x + lw * a4x, ghy = -hw * a1y - lw * a2y + hw * a3y + lw * a4y;
            const float gwx = -hh * a1x + hh * a2x - lh * a3x + lh * a4x, gwy = -hh * a1y + hh * a2y - lh * a3y + lh * a4y;
            const float vx = w1 * a1x + w2 * a2x + w3 * a3x + w4 * a4x, vy = w1 * a1y + w2 * a2y + w3 * a3y + w4 * a4y;
            const float pa = go0 * vx + go1 * vy;
            const float plx = sW * (gwx * go0 + gwy * go1), ply = sH * (ghx * go0 + ghy * go1);
            part[2 * i] = odd ? 0.f : pa;          part[2 * i + 1] = odd ? pa : 0.f;
            part[16 + 4 * i] = odd ? 0.f : plx;    part[16 + 4 * i + 2] = odd ? plx : 0.f;
            part[17 + 4 * i] = odd ? 0.f : ply;    part[17 + 4 * i + 2] = odd ? ply : 0.f;
        }
    }
    store_row_grads(part, lane, row, LP, grad_loc, grad_aw);
}

// Second half of the f32-accumulating bf16 backward: every (image, pixel, head) cell whose flag is set gets its 64 staged
// f32 sums rounded ONCE to bf16 and written to its place in the (possibly strided) gradient map; the staged row and the
// flag are cleared, so stage / cell_flags leave the launch as they must enter the next one: all zero.  Untouched cells are
// not read (the gradient map was zero-filled): at GRIT's shapes the gather reaches 20-45 % of the cells.
// A wave owns 64 consecutive cells (lane = cell for the flag read, lane = channel for the rows), four rows in flight.
__global__ __launch_bounds__(256)
void msda_stage_flush(float* __restrict__ stage, unsigned char* __restrict__ cell_flags, __hip_bfloat16* __restrict__ grad_value,
                      long ncells, int S, int M, int pix_el) {
    const int lane = threadIdx.x & 63;
    const long base = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
    if (base >= ncells) return;
    const long cell = base + lane;
    const unsigned char fl = cell < ncells ? cell_flags[cell] : (unsigned char)0;
    unsigned long long mask = __ballot(fl != 0);
    if (fl) cell_flags[cell] = 0;
    while (mask) {
        long c[4];
        float v[4];
        int n = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (mask) {
                const int bit = __builtin_ctzll(mask);
                mask &= mask - 1;
                c[k] = base + bit;
                n = k + 1;
            } else {
                c[k] = -1;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) v[k] = stage[c[k] * 64 + lane];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) {
                stage[c[k] * 64 + lane] = 0.f;
                const long pix = c[k] / M;  // b * S + pixel
                const int m = (int)(c[k] - pix * M);
                grad_value[pix * pix_el + (long)m * 64 + lane] = __float2bfloat16(v[k]);
            }
    }
}

// ---------------------------------------------------------------------------------------------------
// Gather-form value gradient (bf16 maps, D = 64): no atomics on memory at all.
//
// The scatter of the reference (atomicAdd per corner and channel, ms_deform_im2col_cuda.cuh:125-152) is bound on gfx950 by
// the memory-side atomic units (~323 G f32 adds/s chip-wide, tools/micro/atomic_rate.hip): 157 M channel-adds per launch are
// ~460 us whatever the kernel does around them.  But WHERE every contribution goes is known from the sampling locations
// alone, and per (image, head) there are only Lq*L*P*4 of them (9 600 at GRIT's shapes) over S cells, reading Lq rows of
// grad_out (19 KB): the whole problem of one (image, head) fits the LDS of one CU.  msda_bwd_value, one 1024-thread workgroup
// per (image, head) -- 256 of them at B = 32, M = 8: one per CU --
//   1. loads its Lq rows of grad_out into LDS; bins the (query, point, corner) contributions by cell with LDS counters (the
//      value an LDS atomic returns is the contribution's position inside its cell's run);
//   2. scans the S counters in LDS (exclusive offsets);
//   3. writes the contributions, ordered by cell, into an LDS array {query, attention weight x bilinear weight};
//   4. walks the cells: eight lanes per cell (8 channels each), eight cells per wave instruction; a cell's lanes sum
//      w_i * grad_out[q_i][channels] in f32 registers, round ONCE to bf16 and store their 128-byte row -- every cell, zeros
//      included, so the gradient map needs no zero fill, no f32 staging copy and no flush, and nothing but the final rows
//      ever goes to memory.
// grad_loc / grad_attn_w come from the unchanged row walk with its scatter compiled out (msda_bwd_d64_pk<2>).
// f32 accumulation like the reference's atomicAdd; the order of the terms inside a cell follows the order in which the LDS
// counters were taken (like atomics, not fixed run to run, but the sum is rounded to bf16 once, after the last term).
constexpr int kValueThreads = 1024, kValuePts = 4;   // up to 4 096 (query, point) pairs per (image, head)
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __bf16 v8bf_m __attribute__((ext_vector_type(8)));
typedef short v4s_m __attribute__((ext_vector_type(4)));
typedef short v8s_m __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) v4s_m lds_v4s_m;

__device__ __forceinline__ float bf16_round(float x) {  // x rounded to the nearest bf16 (ties to even), as a float
    return __bfloat162float(__float2bfloat16(x));
}

__host__ __device__ inline size_t value_lds_bytes(int S, int L, int Lq, int P) {
    const size_t counters = ((size_t)S + 2) / 2 * 2 * 4;          // S + 1 offsets, padded to 8 bytes
    return counters + (size_t)Lq * L * P * 4 * 8 + ((size_t)Lq + 1) * 128 + 64;  // + one all-zero row of grad_out
}

__global__ __launch_bounds__(kValueThreads)
void msda_bwd_value(const int64_t* __restrict__ shapes, const int64_t* __restrict__ lsi, const float* __restrict__ loc,
                    const float* __restrict__ aw, const __hip_bfloat16* __restrict__ grad_out,
                    __hip_bfloat16* __restrict__ grad_value, int S, int M, int L, int Lq, int P, int pix_el, int parts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int LP = L * P, npts = Lq * LP, cap = npts * 4;
    int* cnt = reinterpret_cast<int*>(smem);                                     // [S + 1] counters, then exclusive offsets
    uint2* recs = reinterpret_cast<uint2*>(smem + ((size_t)S + 2) / 2 * 2 * 4);  // [cap] {query, weight}
    unsigned char* gol = reinterpret_cast<unsigned char*>(recs + cap);           // [Lq][128 B] rows of grad_out
    int* wsum = reinterpret_cast<int*>(gol + ((size_t)Lq + 1) * 128);            // [16] wave totals of the scan
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // parts > 1 (B * M below the CU count, e.g. 16 images x 8 heads on 256 CUs): `parts` workgroups per (image, head); each bins all
    // of the segment's contributions (steps 1 - 3, the cheap part) and takes an equal-cost share of the cell tiles in step 4
    const int seg = blockIdx.x / parts, part = blockIdx.x - seg * parts, b = seg / M, m = seg - b * M;

    // ---- 1. counters to zero, grad_out rows of this (image, head) into LDS, contributions binned
    for (int i = tid; i <= S; i += kValueThreads) cnt[i] = 0;
    if (tid < 32) reinterpret_cast<unsigned*>(gol + (size_t)Lq * 128)[tid] = 0u;  // row Lq: zeros (k slots past a run)
    for (int i = tid; i < Lq * 8; i += kValueThreads) {
        const int q = i >> 3, piece = i & 7;
        *reinterpret_cast<uint4*>(gol + (size_t)q * 128 + piece * 16) =
            *reinterpret_cast<const uint4*>(grad_out + ((size_t)(b * Lq + q) * M + m) * 64 + piece * 8);
    }
    __syncthreads();
    int cell[kValuePts][4], rank[kValuePts][4], qid[kValuePts];
    float wgt[kValuePts][4];
#pragma unroll
    for (int j = 0; j < kValuePts; ++j) {
        const int i = tid + j * kValueThreads;
#pragma unroll
        for (int k = 0; k < 4; ++k) cell[j][k] = -1;
        if (i < npts) {
            const int q = i / LP, p = i - q * LP, l = p / P;
            const size_t row = (size_t)(b * Lq + q) * M + m;
            qid[j] = q;
            const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1], st = (int)lsi[l];
            const float x = loc[row * 2 * LP + 2 * p], y = loc[row * 2 * LP + 2 * p + 1];
            const float a = aw[row * LP + p];
            const Corners<float> c = make_corners<float>(x, y, H, W);
            if (c.k1) { cell[j][0] = st + c.o1; wgt[j][0] = c.w1 * a; }
            if (c.k2) { cell[j][1] = st + c.o2; wgt[j][1] = c.w2 * a; }
            if (c.k3) { cell[j][2] = st + c.o3; wgt[j][2] = c.w3 * a; }
            if (c.k4) { cell[j][3] = st + c.o4; wgt[j][3] = c.w4 * a; }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (cell[j][k] >= 0) rank[j][k] = atomicAdd(&cnt[cell[j][k]], 1);  // position inside the cell's run
        }
    }
    __syncthreads();
    // ---- 2. exclusive scan of the S counters: a contiguous chunk per thread, wave scans of the chunk sums, 16 wave totals
    const int CH = (S + kValueThreads - 1) / kValueThreads, c0 = tid * CH;
    int local = 0;
    for (int k = 0; k < CH; ++k)
        if (c0 + k < S) local += cnt[c0 + k];
    int incl = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        const int v = lane < kValueThreads / 64 ? wsum[lane] : 0;
        int iv = v;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            const int t = __shfl_up(iv, o, 64);
            if (lane >= o) iv += t;
        }
        if (lane < kValueThreads / 64) wsum[lane] = iv - v;  // exclusive
    }
    __syncthreads();
    int run = incl - local + wsum[wave];
    for (int k = 0; k < CH; ++k)
        if (c0 + k < S) {
            const int c = cnt[c0 + k];
            cnt[c0 + k] = run;
            run += c;
        }
    if (tid == kValueThreads - 1) cnt[S] = run;  // the last thread's running total is the segment's record count
    __syncthreads();
    // ---- 3. contributions ordered by cell.  A record is 8 bytes: query (12 bits), cell within its 16-cell tile (4 bits) and the
    // weight as THREE bf16 terms hi + mid + lo (24 mantissa bits: the f32 weight exactly), the form step 4 feeds to the MFMA
#pragma unroll
    for (int j = 0; j < kValuePts; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (cell[j][k] >= 0) {
                const float w = wgt[j][k];
                const unsigned hi = __float_as_uint(bf16_round(w)) >> 16;
                const float r1 = w - __uint_as_float(hi << 16);
                const unsigned mid = __float_as_uint(bf16_round(r1)) >> 16;
                const float r2 = r1 - __uint_as_float(mid << 16);
                const unsigned lo = __float_as_uint(bf16_round(r2)) >> 16;
                recs[cnt[cell[j][k]] + rank[j][k]] =
                    make_uint2((unsigned)qid[j] | ((unsigned)(cell[j][k] & 15) << 12) | (hi << 16), mid | (lo << 16));
            }
    __syncthreads();
    // ---- 4. tiles of 16 consecutive cells:  Out^T[64 channels x 16 cells] = G^T[64 x n] . W[n x 16]  on the matrix cores, where
    // the n contributions of the tile are one contiguous run of records, G^T their grad_out rows (bf16, exact) read straight from
    // the LDS rows by transposing reads (every lane addresses the row of ITS record), and W[k][c] = weight of record k if it
    // belongs to cell c, else 0 -- three bf16 terms, three MFMAs into the same f32 accumulator.  No loop over cells, no
    // divergence between hot and empty cells; a wave takes a contiguous range of tiles of equal estimated cost.
    const int l15 = lane & 15, lg = lane >> 4, trq = l15 >> 2, trp = l15 & 3;
    const int T = (S + 15) >> 4, nwave = kValueThreads / 64;
    const int total = cnt[S] + 8 * T;  // cost model: a record ~ 1, a tile's fixed part ~ 8
    auto first_tile_at = [&](int target) {  // smallest t with cnt[16 t] + 8 t >= target (monotone in t)
        int lo = 0, hi = T;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cnt[min(16 * mid, S)] + 8 * mid >= target) hi = mid; else lo = mid + 1;
        }
        return lo;
    };
    const int gw = part * nwave + wave, ngw = parts * nwave;  // this wave among the segment's waves
    const int tlo = gw == 0 ? 0 : first_tile_at((int)((long)total * gw / ngw));
    const int thi = gw == ngw - 1 ? T : first_tile_at((int)((long)total * (gw + 1) / ngw));
    __hip_bfloat16* gbase = grad_value + (size_t)b * S * pix_el + (size_t)m * 64 + 4 * lg;
    const unsigned char* grow = gol + 8 * trp;  // + q * 128 + 32 * cb
    for (int t = tlo; t < thi; ++t) {
        const int beg = __builtin_amdgcn_readfirstlane(cnt[16 * t]);
        const int end = __builtin_amdgcn_readfirstlane(cnt[min(16 * t + 16, S)]);
        v4f acc[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[cb] = v4f{0.f, 0.f, 0.f, 0.f};
        for (int k0 = beg; k0 < end; k0 += 32) {
            // k slots of this lane (the order the transposing reads define): e < 4: k0 + 4 lg + e,  e >= 4: k0 + 16 + 4 lg + e - 4
            // masked record words first (2 selects per record), then three byte permutes per PAIR of records gather the hi /
            // mid / lo halves into the packed operand registers
            unsigned rx[8], ry[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = k0 + 4 * lg + (e & 3) + (e >> 2) * 16;
                const uint2 r = recs[min(k, cap - 1)];
                const bool mine = k < end && ((r.x >> 12) & 15u) == (unsigned)l15;
                rx[e] = mine ? r.x : 0u;
                ry[e] = mine ? r.y : 0u;
            }
            typedef unsigned u4v __attribute__((ext_vector_type(4)));
            u4v ph, pm, pl;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                // v_perm_b32(hi word, lo word, selector): selector bytes 0-3 index the low word, 4-7 the high word
                ph[e] = __builtin_amdgcn_perm(rx[2 * e + 1], rx[2 * e], 0x07060302u);  // hi halves: x >> 16
                pm[e] = __builtin_amdgcn_perm(ry[2 * e + 1], ry[2 * e], 0x05040100u);  // mid: y & 0xffff
                pl[e] = __builtin_amdgcn_perm(ry[2 * e + 1], ry[2 * e], 0x07060302u);  // lo: y >> 16
            }
            const v8bf_m bh = __builtin_bit_cast(v8bf_m, ph), bm = __builtin_bit_cast(v8bf_m, pm), bl = __builtin_bit_cast(v8bf_m, pl);
            // rows this lane addresses for the transposing reads: records k0 + 4 lg + trq and + 16 (past the run: the zero row)
            const int ka = k0 + 4 * lg + trq, kb = ka + 16;
            const unsigned qa = ka < end ? (recs[min(ka, cap - 1)].x & 0xfffu) : (unsigned)Lq;
            const unsigned qb = kb < end ? (recs[min(kb, cap - 1)].x & 0xfffu) : (unsigned)Lq;
            const unsigned char* ra = grow + (size_t)qa * 128;
            const unsigned char* rb = grow + (size_t)qb * 128;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const v4s_m x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_m*)(ra + 32 * cb));
                const v4s_m x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s_m*)(rb + 32 * cb));
                const v8s_m xs = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
                const v8bf_m a = __builtin_bit_cast(v8bf_m, xs);
                acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bh, acc[cb], 0, 0, 0);
                acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bm, acc[cb], 0, 0, 0);
                acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bl, acc[cb], 0, 0, 0);
            }
        }
        // acc[cb][r] = Out[cell 16 t + l15][channel 16 cb + 4 lg + r]
        const int cellw = 16 * t + l15;
        if (cellw < S) {
            __hip_bfloat16* dst = gbase + (size_t)cellw * pix_el;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                typedef __bf16 v4bf_m __attribute__((ext_vector_type(4)));
                const v4bf_m o = {(__bf16)acc[cb][0], (__bf16)acc[cb][1], (__bf16)acc[cb][2], (__bf16)acc[cb][3]};
                *reinterpret_cast<v4bf_m*>(dst + 16 * cb) = o;
            }
        }
    }
}

bool dims_ok(int B, int S, int M, int D, int L, int Lq, int P) {
    if (B <= 0 || S <= 0 || M <= 0 || D <= 0 || L <= 0 || Lq <= 0 || P <= 0) return false;
    const long long rows = (long long)B * Lq * M;
    return rows < (1LL << 31) - 8 && (long long)L * P < (1 << 20);
}

struct Dims {
    int B, S, M, D, L, Lq, P;
};

struct Aligned {
    const void* p;
    unsigned bytes;
};

// Argument check of every entry point.  Any GRIT_ERR_BAD_ARG condition (a null pointer, bad dimensions, a bad pixel stride)
// wins over any GRIT_ERR_UNSUPPORTED one (a shape or an alignment the entry point's kernels do not take).
//   stride_multiple: 0 for an entry point without a pixel stride, else what `pixel_stride` has to be a multiple of;
//   max_lp: 0 for any D and L*P, else the entry point needs D == 64 and L*P <= max_lp;
//   sorted: the shape also has to pass grit_msda_bwd_sorted_supported.
int check_args(std::initializer_list<const void*> ptrs, const Dims& d, long pixel_stride, int stride_multiple, int max_lp,
               std::initializer_list<Aligned> aligned, bool sorted = false) {
    if (stride_multiple &&
        (pixel_stride < (long)d.M * d.D || pixel_stride % stride_multiple || pixel_stride > 0x3fffffffL))
        return GRIT_ERR_BAD_ARG;
    for (const void* p : ptrs)
        if (!p) return GRIT_ERR_BAD_ARG;
    if (!dims_ok(d.B, d.S, d.M, d.D, d.L, d.Lq, d.P)) return GRIT_ERR_BAD_ARG;
    if (sorted) {
        const int ok = grit_msda_bwd_sorted_supported(d.B, d.S, d.M, d.L, d.Lq, d.P);
        if (ok != GRIT_OK) return ok;
    }
    if (max_lp && (d.D != 64 || d.L * d.P > max_lp)) return GRIT_ERR_UNSUPPORTED;
    for (const Aligned& a : aligned)
        if ((uintptr_t)a.p % a.bytes) return GRIT_ERR_UNSUPPORTED;
    return GRIT_OK;
}

// Workgroups of 256 threads that own rows_per_block rows each: 4 (a row per wave) or 16 (four rows per wave).
struct RowGrid {
    int nblk;
    dim3 grid, block;
};

RowGrid row_grid(int nrows, int rows_per_block) {
    const int nblk = (nrows + rows_per_block - 1) / rows_per_block;
    return RowGrid{nblk, dim3(nblk), dim3(kWave * kRowsPerBlock)};
}

int launched() { return hipGetLastError() == hipSuccess ? GRIT_OK : GRIT_ERR_LAUNCH; }

// The A/B knobs of this file, read from the environment once per process, on first use.  (GRIT_MSDA_BWD_F32ACC and
// GRIT_MSDA_BWD_METHOD choose between the bf16 backward entry points and are read by grit_amd/ops/msda.py.)
struct Knobs {
    int fwd_batch;     // GRIT_MSDA_FWD_BATCH: points in flight in msda_fwd_bf16_rows4 (1, 2, 4, 8; default and anything else: 2);
                       // 0: the row-per-wave kernel instead
    bool interleave;   // GRIT_MSDA_BWD_INTERLEAVE=0: no image-interleaved workgroup order in msda_bwd_d64_pk
    bool no_merge;     // GRIT_MSDA_BWD_MERGE=0: no merging of points that share a cell in msda_bwd_d64_pk
    int value_parts;   // GRIT_MSDA_VALUE_PARTS > 0: workgroups per (image, head) in msda_bwd_value
    bool rows1;        // GRIT_MSDA_BWD_ROWS1 != 0: grad_loc / grad_attn_w of the sorted backward by one row per wave
};

const Knobs& knobs() {
    static const Knobs k = [] {
        const auto env = [](const char* name, int otherwise) { return getenv(name) ? atoi(getenv(name)) : otherwise; };
        const int batch = env("GRIT_MSDA_FWD_BATCH", 2);
        return Knobs{(batch == 0 || batch == 1 || batch == 4 || batch == 8) ? batch : 2,
                     env("GRIT_MSDA_BWD_INTERLEAVE", 1) != 0, env("GRIT_MSDA_BWD_MERGE", 1) == 0,
                     env("GRIT_MSDA_VALUE_PARTS", 0), env("GRIT_MSDA_BWD_ROWS1", 0) != 0};
    }();
    return k;
}

// Runtime n -> template argument: calls f(std::integral_constant<int, N>) for the N of the list that equals n; false if none does.
template <int... Ns, typename F>
bool dispatch(int n, std::integer_sequence<int, Ns...>, F&& f) {
    return ((n == Ns && (f(std::integral_constant<int, Ns>{}), true)) || ...);
}

template <typename T>
int launch_fwd(const T* value, const int64_t* shapes, const int64_t* lsi, const T* loc, const T* aw,
               int B, int S, int M, int D, int L, int Lq, int P, T* out, hipStream_t st) {
    const int bad = check_args({value, shapes, lsi, loc, aw, out}, {B, S, M, D, L, Lq, P}, 0, 0, 0, {});
    if (bad) return bad;
    const int nrows = B * Lq * M;
    const RowGrid g = row_grid(nrows, kRowsPerBlock);
    bool done = false;
    if constexpr (sizeof(T) == 4) {
        const int LP = L * P;
        const bool aligned = ((uintptr_t)value % 16 == 0) && ((uintptr_t)out % 16 == 0);
        const auto vec4 = [&](auto lpp, auto nit) {
            hipLaunchKernelGGL((msda_fwd_vec4<decltype(lpp)::value, decltype(nit)::value>), g.grid, g.block, 0, st, value, shapes,
                               lsi, loc, aw, S, M, L, Lq, P, out, nrows, g.nblk);
        };
        if (aligned && D == 64 && LP <= 32)
            done = dispatch((LP + 3) / 4, std::integer_sequence<int, 1, 2, 3, 4, 6, 8>{},
                            [&](auto nit) { vec4(std::integral_constant<int, 16>{}, nit); });
        else if (aligned && D == 32 && LP <= 32)
            done = dispatch((LP + 7) / 8, std::integer_sequence<int, 1, 2, 3, 4>{},
                            [&](auto nit) { vec4(std::integral_constant<int, 8>{}, nit); });
    }
    if (!done)
        hipLaunchKernelGGL((msda_fwd_generic<T>), g.grid, g.block, 0, st, value, shapes, lsi, loc, aw,
                           S, M, D, L, Lq, P, out, nrows, g.nblk);
    return launched();
}

template <typename VT>
int launch_bwd_d64(const VT* value, const int64_t* shapes, const int64_t* lsi, const float* loc, const float* aw,
                   const VT* go, int B, int S, int M, int L, int Lq, int P, float* gv, float* gl, float* gw,
                   hipStream_t st) {
    const int nrows = B * Lq * M;
    const RowGrid g = row_grid(nrows, kRowsPerBlock);
    hipLaunchKernelGGL((msda_bwd_d64<VT>), g.grid, g.block, 0, st, value, shapes, lsi, loc, aw, go,
                       S, M, L, Lq, P, gv, gl, gw, nrows, g.nblk);
    return launched();
}

template <typename T>
int launch_bwd(const T* value, const int64_t* shapes, const int64_t* lsi, const T* loc, const T* aw,
               const T* go, int B, int S, int M, int D, int L, int Lq, int P,
               T* gv, T* gl, T* gw, hipStream_t st) {
    const int bad = check_args({value, shapes, lsi, loc, aw, go, gv, gl, gw}, {B, S, M, D, L, Lq, P}, 0, 0, 0, {});
    if (bad) return bad;
    if constexpr (sizeof(T) == 4) {
        if (D == 64 && L * P <= 16) return launch_bwd_d64<float>(value, shapes, lsi, loc, aw, go, B, S, M, L, Lq, P, gv, gl, gw, st);
    }
    const int nrows = B * Lq * M;
    const RowGrid g = row_grid(nrows, kRowsPerBlock);
    if ((L * P) % 4 == 0)
        hipLaunchKernelGGL((msda_bwd_generic<T, 4>), g.grid, g.block, 0, st, value, shapes, lsi, loc, aw, go,
                           S, M, D, L, Lq, P, gv, gl, gw, nrows, g.nblk);
    else
        hipLaunchKernelGGL((msda_bwd_generic<T, 1>), g.grid, g.block, 0, st, value, shapes, lsi, loc, aw, go,
                           S, M, D, L, Lq, P, gv, gl, gw, nrows, g.nblk);
    return launched();
}

// the row walk of the packed / staged / sorted bf16 backward
template <Scatter MODE>
void launch_bwd_pk(const void* value, long pixel_stride, const int64_t* shapes, const int64_t* lsi, const float* loc,
                   const float* aw, const void* go, int B, int S, int M, int L, int Lq, int P, void* gv, float* gl, float* gw,
                   float* stage, unsigned char* cell_flags, hipStream_t st) {
    const int nrows = B * Lq * M;
    const RowGrid g = row_grid(nrows, kRowsPerBlock);
    // image-interleaved workgroup order when the rows of an image fill whole workgroups; neither it nor the merge serves a walk
    // that scatters nothing
    const bool scatters = MODE != Scatter::kNone;
    const int images = (scatters && knobs().interleave && B > 1 && (Lq * M) % kRowsPerBlock == 0) ? B : 1;
    const int no_merge = (!scatters || knobs().no_merge) ? 1 : 0;
    hipLaunchKernelGGL(msda_bwd_d64_pk<MODE>, g.grid, g.block, 0, st, (const __hip_bfloat16*)value, shapes, lsi, loc, aw,
                       (const __hip_bfloat16*)go, S, M, L, Lq, P, (__hip_bfloat16*)gv, gl, gw, nrows, g.nblk, images, no_merge,
                       (int)pixel_stride, stage, cell_flags);
}

}  // namespace

extern "C" {

int grit_msda_fwd_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start,
                      const float* loc, const float* attn_w, int B, int S, int M, int D, int L, int Lq,
                      int P, float* out, void* stream) {
    return launch_fwd<float>(value, spatial_shapes, level_start, loc, attn_w, B, S, M, D, L, Lq, P, out,
                             (hipStream_t)stream);
}

int grit_msda_fwd_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start,
                      const double* loc, const double* attn_w, int B, int S, int M, int D, int L, int Lq,
                      int P, double* out, void* stream) {
    return launch_fwd<double>(value, spatial_shapes, level_start, loc, attn_w, B, S, M, D, L, Lq, P, out,
                              (hipStream_t)stream);
}

int grit_msda_bwd_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start,
                      const float* loc, const float* attn_w, const float* grad_out, int B, int S, int M,
                      int D, int L, int Lq, int P, float* grad_value, float* grad_loc, float* grad_attn_w,
                      void* stream) {
    return launch_bwd<float>(value, spatial_shapes, level_start, loc, attn_w, grad_out, B, S, M, D, L, Lq,
                             P, grad_value, grad_loc, grad_attn_w, (hipStream_t)stream);
}

int grit_msda_bwd_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start,
                      const double* loc, const double* attn_w, const double* grad_out, int B, int S, int M,
                      int D, int L, int Lq, int P, double* grad_value, double* grad_loc,
                      double* grad_attn_w, void* stream) {
    return launch_bwd<double>(value, spatial_shapes, level_start, loc, attn_w, grad_out, B, S, M, D, L, Lq,
                              P, grad_value, grad_loc, grad_attn_w, (hipStream_t)stream);
}

int grit_msda_fwd_bf16(const void* value, const int64_t* spatial_shapes, const int64_t* level_start, const float* loc,
                       const float* attn_w, int B, int S, int M, int D, int L, int Lq, int P, void* out, void* stream) {
    return grit_msda_fwd_bf16_strided(value, (long)M * D, spatial_shapes, level_start, loc, attn_w, B, S, M, D, L, Lq, P, out,
                                      stream);
}

int grit_msda_fwd_bf16_strided(const void* value, long pixel_stride, const int64_t* spatial_shapes,
                               const int64_t* level_start, const float* loc, const float* attn_w, int B, int S, int M,
                               int D, int L, int Lq, int P, void* out, void* stream) {
    const int bad = check_args({value, spatial_shapes, level_start, loc, attn_w, out}, {B, S, M, D, L, Lq, P}, pixel_stride, 8, 32,
                               {{value, 16}, {out, 16}});
    if (bad) return bad;
    const int pix_el = (int)pixel_stride;
    const int LP = L * P;
    const int nrows = B * Lq * M;
    const __hip_bfloat16* v = (const __hip_bfloat16*)value;
    __hip_bfloat16* o = (__hip_bfloat16*)out;
    hipStream_t st = (hipStream_t)stream;
    // four rows per wave when the byte offsets into the map fit 32 bits, else (and GRIT_MSDA_FWD_BATCH=0) one row per wave
    const bool rows4 = knobs().fwd_batch != 0 && LP <= 16 && (uint64_t)B * S * (uint64_t)pixel_stride * 2 < (1ull << 32);
    const RowGrid g = row_grid(nrows, rows4 ? 4 * kRowsPerBlock : kRowsPerBlock);
    if (rows4)
        dispatch(knobs().fwd_batch, std::integer_sequence<int, 1, 2, 4, 8>{}, [&](auto batch) {
            hipLaunchKernelGGL((msda_fwd_bf16_rows4<decltype(batch)::value>), g.grid, g.block, 0, st, v, spatial_shapes, level_start,
                               loc, attn_w, S, M, L, Lq, P, o, nrows, g.nblk, pix_el);
        });
    else
        dispatch((LP + 7) / 8, std::integer_sequence<int, 1, 2, 3, 4>{}, [&](auto nit) {  // LP <= 32: one of them
            hipLaunchKernelGGL((msda_fwd_bf16_d64<decltype(nit)::value>), g.grid, g.block, 0, st, v, spatial_shapes, level_start,
                               loc, attn_w, S, M, L, Lq, P, o, nrows, g.nblk, pix_el);
        });
    return launched();
}

int grit_msda_bwd_bf16(const void* value, const int64_t* spatial_shapes, const int64_t* level_start, const float* loc,
                       const float* attn_w, const void* grad_out, int B, int S, int M, int D, int L, int Lq, int P,
                       float* grad_value, float* grad_loc, float* grad_attn_w, void* stream) {
    const int bad = check_args({value, spatial_shapes, level_start, loc, attn_w, grad_out, grad_value, grad_loc, grad_attn_w},
                               {B, S, M, D, L, Lq, P}, 0, 0, 16, {});
    if (bad) return bad;
    return launch_bwd_d64<__hip_bfloat16>((const __hip_bfloat16*)value, spatial_shapes, level_start, loc, attn_w,
                                            (const __hip_bfloat16*)grad_out, B, S, M, L, Lq, P, grad_value, grad_loc,
                                            grad_attn_w, (hipStream_t)stream);
}

int grit_msda_bwd_bf16acc(const void* value, const int64_t* spatial_shapes, const int64_t* level_start, const float* loc,
                          const float* attn_w, const void* grad_out, int B, int S, int M, int D, int L, int Lq, int P,
                          void* grad_value, float* grad_loc, float* grad_attn_w, void* stream) {
    return grit_msda_bwd_bf16acc_strided(value, (long)M * D, spatial_shapes, level_start, loc, attn_w, grad_out, B, S, M, D, L,
                                         Lq, P, grad_value, grad_loc, grad_attn_w, stream);
}

int grit_msda_bwd_bf16acc_strided(const void* value, long pixel_stride, const int64_t* spatial_shapes,
                                  const int64_t* level_start, const float* loc, const float* attn_w, const void* grad_out,
                                  int B, int S, int M, int D, int L, int Lq, int P, void* grad_value, float* grad_loc,
                                  float* grad_attn_w, void* stream) {
    const int bad = check_args({value, spatial_shapes, level_start, loc, attn_w, grad_out, grad_value, grad_loc, grad_attn_w},
                               {B, S, M, D, L, Lq, P}, pixel_stride, 2, 16, {{value, 4}, {grad_out, 4}, {grad_value, 4}});
    if (bad) return bad;
    launch_bwd_pk<Scatter::kPacked>(value, pixel_stride, spatial_shapes, level_start, loc, attn_w, grad_out, B, S, M, L, Lq, P,
                                    grad_value, grad_loc, grad_attn_w, nullptr, nullptr, (hipStream_t)stream);
    return launched();
}

int grit_msda_bwd_bf16_staged(const void* value, long pixel_stride, const int64_t* spatial_shapes,
                              const int64_t* level_start, const float* loc, const float* attn_w, const void* grad_out,
                              int B, int S, int M, int D, int L, int Lq, int P, float* stage, unsigned char* cell_flags,
                              void* grad_value, float* grad_loc, float* grad_attn_w, void* stream) {
    const int bad = check_args({value, spatial_shapes, level_start, loc, attn_w, grad_out, grad_value, grad_loc, grad_attn_w,
                                stage, cell_flags},
                               {B, S, M, D, L, Lq, P}, pixel_stride, 2, 16,
                               {{value, 4}, {grad_out, 4}, {grad_value, 2}, {stage, 4}});
    if (bad) return bad;
    launch_bwd_pk<Scatter::kStaged>(value, pixel_stride, spatial_shapes, level_start, loc, attn_w, grad_out, B, S, M, L, Lq, P,
                                    nullptr, grad_loc, grad_attn_w, stage, cell_flags, (hipStream_t)stream);
    if (launched() != GRIT_OK) return GRIT_ERR_LAUNCH;
    const long ncells = (long)B * S * M;
    const long nwaves = (ncells + 63) / 64;
    hipLaunchKernelGGL(msda_stage_flush, dim3((unsigned)((nwaves + 3) / 4)), dim3(256), 0, (hipStream_t)stream, stage, cell_flags,
                       (__hip_bfloat16*)grad_value, ncells, S, M, (int)pixel_stride);
    return launched();
}

int grit_msda_bwd_sorted_supported(int B, int S, int M, int L, int Lq, int P) {
    if (B <= 0 || S <= 0 || M <= 0 || L <= 0 || Lq <= 0 || P <= 0) return GRIT_ERR_BAD_ARG;
    if ((long)Lq * L * P > (long)kValueThreads * kValuePts || Lq > 4095) return GRIT_ERR_UNSUPPORTED;
    if (value_lds_bytes(S, L, Lq, P) > 160 * 1024) return GRIT_ERR_UNSUPPORTED;
    return GRIT_OK;
}

int grit_msda_bwd_bf16_sorted(const void* value, long pixel_stride, const int64_t* spatial_shapes,
                              const int64_t* level_start, const float* loc, const float* attn_w, const void* grad_out,
                              int B, int S, int M, int D, int L, int Lq, int P, void* grad_value, float* grad_loc,
                              float* grad_attn_w, void* stream) {
    const int bad = check_args({value, spatial_shapes, level_start, loc, attn_w, grad_out, grad_value, grad_loc, grad_attn_w},
                               {B, S, M, D, L, Lq, P}, pixel_stride, 8, 16, {{value, 4}, {grad_out, 16}, {grad_value, 16}},
                               /*sorted=*/true);
    if (bad) return bad;
    hipStream_t st = (hipStream_t)stream;
    static grit_detail::PerDevice<bool> lds_attr_set_pd; bool& lds_attr_set = lds_attr_set_pd();  // idempotent attribute
    if (!lds_attr_set) {
        if (hipFuncSetAttribute((const void*)msda_bwd_value, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            return GRIT_ERR_LAUNCH;
        lds_attr_set = true;
    }
    // fewer (image, head) segments than CUs: several workgroups per segment (GRIT_MSDA_VALUE_PARTS overrides: A/B)
    int parts = knobs().value_parts > 0 ? knobs().value_parts : 256 / (B * M);
    parts = parts < 1 ? 1 : (parts > 8 ? 8 : parts);
    hipLaunchKernelGGL(msda_bwd_value, dim3(B * M * parts), dim3(kValueThreads), value_lds_bytes(S, L, Lq, P), st, spatial_shapes,
                       level_start, loc, attn_w, (const __hip_bfloat16*)grad_out, (__hip_bfloat16*)grad_value, S, M, L, Lq, P,
                       (int)pixel_stride, parts);
    if (launched() != GRIT_OK) return GRIT_ERR_LAUNCH;
    // grad_loc / grad_attn_w: four rows per wave when the byte offsets into the map fit 32 bits, else one row per wave
    if (!knobs().rows1 && (long)B * S * pixel_stride * 2 < (1LL << 32) && (uintptr_t)value % 16 == 0) {
        const int nrows = B * Lq * M;
        const RowGrid g = row_grid(nrows, 4 * kRowsPerBlock);
        hipLaunchKernelGGL(msda_bwd_rows4<2>, g.grid, g.block, 0, st, (const __hip_bfloat16*)value, spatial_shapes,
                           level_start, loc, attn_w, (const __hip_bfloat16*)grad_out, S, M, L, Lq, P, grad_loc, grad_attn_w,
                           nrows, g.nblk, (int)pixel_stride);
    } else {
        launch_bwd_pk<Scatter::kNone>(value, pixel_stride, spatial_shapes, level_start, loc, attn_w, grad_out, B, S, M, L, Lq, P,
                                      nullptr, grad_loc, grad_attn_w, nullptr, nullptr, st);
    }
    return launched();
}

}  // extern "C"
