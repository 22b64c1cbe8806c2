// macx_features.hip.h -- image features resident in device memory (macx_features_pack / macx_features_gather): a table of
// [rows][HW][C] images (NHWC rows, what the stem reads) in fp32 or fp16, filled once from the feature file's chunks, and the batch
// of a step gathered from it by row id.
//
//   pack     table[row0 + i] = convert(src[i]),  src [n][C][HW] (the file's layout: a transpose per image) or [n][HW][C]
//   gather   out[g] = (float) table[ids[g]]      fp16 tables here; an fp32 table is kb_gather_kernel's copy (macx_kb_gather.hip.h)
//
// fp32 -> fp16 is round-to-nearest-even with subnormals kept (v_cvt_f16_f32 under the default mode: no fast-math in this build);
// fp16 -> fp32 is exact.  Offsets are 64-bit: a table is tens of gigabytes.
#pragma once
#include "macx_common.hip.h"
#include "macx_kb_gather.hip.h"

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

namespace macx {

constexpr int FT_TILE = 64;                        // pack, file layout: a tile is 64 channels x 64 positions
constexpr int FT_PITCH = FT_TILE + 1;              // LDS row pitch in dwords: odd, see feat_pack_t_kernel
constexpr int FT_LOADS = 4;                        // gather / flat pack: 16-byte loads in flight per thread
constexpr int FT_CHUNK = 256 * FT_LOADS;           // gather / flat pack: units per workgroup and pass

// what a table element is made of, and whether a stored element trips the overflow word: an fp16 element that came out as an
// infinity or a NaN (the source was one, or rounded to one); an fp32 element that is one.
template <typename T> struct FeatElem;
template <> struct FeatElem<_Float16> {
  static __device__ __forceinline__ _Float16 from(float x) { return (_Float16)x; }
  static __device__ __forceinline__ bool bad(_Float16 h) { return (__builtin_bit_cast(uint16_t, h) & 0x7C00u) == 0x7C00u; }
};
template <> struct FeatElem<float> {
  static __device__ __forceinline__ float from(float x) { return x; }
  static __device__ __forceinline__ bool bad(float x) { return (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u; }
};

// ---- pack, file layout [n][C][HW] -> table rows [HW][C] --------------------------------------------------------------------------
// grid (HW tiles, C tiles, images; grid-stride over images), 256 threads.  The tile lives in LDS as tile[c][hw] fp32 at a pitch of
// 65 dwords.
//   load    coalesced along HW.  VL (HW % 4 == 0): 16 lanes x 16 bytes cover a channel's 64 positions, 16 channels per pass; each
//           lane writes its four dwords with ds_write_b32 at bank (c + 4*hq + j) % 32 -- 16 distinct banks per 32-lane group,
//           2-way, which a ds_write_b32 absorbs.  Otherwise 64 lanes x 4 bytes per channel: conflict-free.
//   store   coalesced along C.  VS (C % EPV == 0, EPV = elements per 16 bytes: 8 fp16, 4 fp32): a lane reads EPV channels of one
//           position (ds_read_b32 at bank (c + hw) % 32 with c = EPV*cg + k: 16 distinct banks per group, 2-way) and stores 16
//           bytes; 64/EPV lanes cover a position's 64 channels.  Otherwise 64 lanes x one element per position: conflict-free.
// A lane that stores an element with FeatElem::bad writes the constant 1 to overflow[0]: a plain store of the same value from every
// such lane, no atomics; the kernel never clears the word.
template <typename T, bool VL, bool VS>
__global__ __launch_bounds__(256) void feat_pack_t_kernel(const float* __restrict__ src, int n, int C, int HW, T* __restrict__ table,
                                                          size_t row0, int32_t* __restrict__ overflow) {
  constexpr int EPV = 16 / (int)sizeof(T);
  typedef T tvec __attribute__((ext_vector_type(EPV)));
  __shared__ float tile[FT_TILE * FT_PITCH];
  const int t = threadIdx.x;
  const int hw0 = blockIdx.x * FT_TILE, c0 = blockIdx.y * FT_TILE;
  const size_t image = (size_t)C * HW;
  bool bad = false;
  for (int i = blockIdx.z; i < n; i += gridDim.z) {
    const float* s = src + (size_t)i * image;
    T* o = table + (row0 + (size_t)i) * image;
    if (VL) {
      const int hq = t & 15, cl = t >> 4;
#pragma unroll
      for (int p = 0; p < FT_TILE / 16; ++p) {
        const int c = p * 16 + cl, hw = 4 * hq;
        f32x4 v{0.f, 0.f, 0.f, 0.f};
        if (c0 + c < C && hw0 + hw < HW) v = *reinterpret_cast<const f32x4*>(s + (size_t)(c0 + c) * HW + hw0 + hw);
#pragma unroll
        for (int j = 0; j < 4; ++j) tile[c * FT_PITCH + hw + j] = v[j];
      }
    } else {
      const int hw = t & 63, cl = t >> 6;
#pragma unroll
      for (int p = 0; p < FT_TILE / 4; ++p) {
        const int c = p * 4 + cl;
        tile[c * FT_PITCH + hw] = (c0 + c < C && hw0 + hw < HW) ? s[(size_t)(c0 + c) * HW + hw0 + hw] : 0.f;
      }
    }
    __syncthreads();
    if (VS) {
      constexpr int LPR = FT_TILE / EPV, RPP = 256 / LPR;        // lanes per position, positions per pass
      const int cg = t % LPR, hl = t / LPR;
#pragma unroll
      for (int p = 0; p < FT_TILE / RPP; ++p) {
        const int hw = p * RPP + hl, c = cg * EPV;
        if (hw0 + hw < HW && c0 + c < C) {
          tvec v;
#pragma unroll
          for (int k = 0; k < EPV; ++k) {
            v[k] = FeatElem<T>::from(tile[(c + k) * FT_PITCH + hw]);
            bad |= FeatElem<T>::bad(v[k]);
          }
          *reinterpret_cast<tvec*>(o + (size_t)(hw0 + hw) * C + c0 + c) = v;
        }
      }
    } else {
      const int c = t & 63, hl = t >> 6;
#pragma unroll
      for (int p = 0; p < FT_TILE / 4; ++p) {
        const int hw = p * 4 + hl;
        if (hw0 + hw < HW && c0 + c < C) {
          const T v = FeatElem<T>::from(tile[c * FT_PITCH + hw]);
          bad |= FeatElem<T>::bad(v);
          o[(size_t)(hw0 + hw) * C + c0 + c] = v;
        }
      }
    }
    __syncthreads();
  }
  if (bad && overflow) overflow[0] = 1;
}

// ---- pack, table layout [n][HW][C]: a conversion of n*C*HW contiguous elements -----------------------------------------------------
// A unit is Q quads of the source (Q * 16 bytes loaded, Q * 4 elements stored).  fp32 tables: Q = 1, a copy.  fp16 tables: Q = 2
// (16-byte stores) where an image is a multiple of 8 elements, which keeps every table row on a 16-byte boundary; else Q = 1
// (8-byte stores).  A capped grid-stride grid, FT_LOADS units in flight per thread.
template <typename T, int Q>
__global__ __launch_bounds__(256) void feat_pack_flat_kernel(const f32x4* __restrict__ src, size_t units, T* __restrict__ dst,
                                                             int32_t* __restrict__ overflow) {
  typedef T tvec __attribute__((ext_vector_type(4 * Q)));
  bool bad = false;
  for (size_t c = (size_t)blockIdx.x * FT_CHUNK; c < units; c += (size_t)gridDim.x * FT_CHUNK) {
    f32x4 v[FT_LOADS][Q];
#pragma unroll
    for (int k = 0; k < FT_LOADS; ++k) {
      const size_t u = c + (size_t)k * 256 + threadIdx.x;
#pragma unroll
      for (int q = 0; q < Q; ++q) v[k][q] = u < units ? src[u * Q + q] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int k = 0; k < FT_LOADS; ++k) {
      const size_t u = c + (size_t)k * 256 + threadIdx.x;
      tvec w;
#pragma unroll
      for (int e = 0; e < 4 * Q; ++e) {
        w[e] = FeatElem<T>::from(v[k][e / 4][e % 4]);
        bad |= FeatElem<T>::bad(w[e]);
      }
      if (u < units) reinterpret_cast<tvec*>(dst)[u] = w;
    }
  }
  if (bad && overflow) overflow[0] = 1;
}

// the pack launch of one table type (arguments already checked by macx_features_pack)
template <typename T>
inline hipError_t feat_pack_launch(const float* src, int layout, int n, int C, int HW, T* table, size_t row0, int32_t* overflow,
                                   hipStream_t st) {
  constexpr int EPV = 16 / (int)sizeof(T);
  const size_t image = (size_t)C * HW;
  if (layout == 1) {
    T* dst = table + row0 * image;
    constexpr int QW = sizeof(T) == 2 ? 2 : 1;                   // the wide unit of this type (fp32: a quad either way)
    const bool wide = QW == 2 && image % 8 == 0;
    const size_t units = (size_t)n * image / (wide ? 8 : 4);
    const dim3 grid = kbg_grid(units, FT_CHUNK, 1);
    if (wide)
      hipLaunchKernelGGL((feat_pack_flat_kernel<T, QW>), grid, dim3(256), 0, st, reinterpret_cast<const f32x4*>(src), units, dst, overflow);
    else
      hipLaunchKernelGGL((feat_pack_flat_kernel<T, 1>), grid, dim3(256), 0, st, reinterpret_cast<const f32x4*>(src), units, dst, overflow);
    return hipGetLastError();
  }
  const dim3 grid((unsigned)(((size_t)HW + FT_TILE - 1) / FT_TILE), (unsigned)(((size_t)C + FT_TILE - 1) / FT_TILE), n < 1024 ? n : 1024);
  const bool vl = HW % 4 == 0, vs = C % EPV == 0;
#define MACX_FT_LAUNCH(VL, VS) \
  hipLaunchKernelGGL((feat_pack_t_kernel<T, VL, VS>), grid, dim3(256), 0, st, src, n, C, HW, table, row0, overflow)
  if (vl && vs) MACX_FT_LAUNCH(true, true);
  else if (vl) MACX_FT_LAUNCH(true, false);
  else if (vs) MACX_FT_LAUNCH(false, true);
  else MACX_FT_LAUNCH(false, false);
#undef MACX_FT_LAUNCH
  return hipGetLastError();
}

// ---- gather from an fp16 table: kb_gather_kernel's contract and geometry ---------------------------------------------------------
// grid (chunks, output images) from kbg_grid.  A workgroup belongs to ONE output image, so the id it reads is uniform (a scalar
// load), and it is read when the kernel RUNS: a captured graph follows an id tensor rewritten between replays.  An id outside
// [0, rows) is never dereferenced: that image's block is quiet NaN.  A unit is Q quads of the output: Q = 2 (a 16-byte load of 8
// halves, two 16-byte stores) where an image is a multiple of 8 elements, else Q = 1 (8-byte loads); FT_LOADS loads in flight per
// thread, FT_CHUNK units per workgroup and pass.
template <int Q>
__global__ __launch_bounds__(256) void feat_gather_h_kernel(const _Float16* __restrict__ table, const int32_t* __restrict__ ids, int rows,
                                                            int G, size_t units, f32x4* __restrict__ out) {
  typedef _Float16 hvec __attribute__((ext_vector_type(4 * Q)));
  const float qnan = __int_as_float(0x7FC00000);
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    const int r = ids[g];
    const bool ok = r >= 0 && r < rows;
    const hvec* s = reinterpret_cast<const hvec*>(table) + (size_t)(ok ? r : 0) * units;
    f32x4* o = out + (size_t)g * units * Q;
    for (size_t c = (size_t)blockIdx.x * FT_CHUNK; c < units; c += (size_t)gridDim.x * FT_CHUNK) {
      hvec v[FT_LOADS];
#pragma unroll
      for (int k = 0; k < FT_LOADS; ++k) {
        const size_t u = c + (size_t)k * 256 + threadIdx.x;
        v[k] = (ok && u < units) ? s[u] : hvec{};
      }
#pragma unroll
      for (int k = 0; k < FT_LOADS; ++k) {
        const size_t u = c + (size_t)k * 256 + threadIdx.x;
        if (u < units) {
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            f32x4 w{qnan, qnan, qnan, qnan};
            if (ok) w = f32x4{(float)v[k][4 * q], (float)v[k][4 * q + 1], (float)v[k][4 * q + 2], (float)v[k][4 * q + 3]};
            o[u * Q + q] = w;
          }
        }
      }
    }
  }
}

}  // namespace macx
