// macx_kb_gather.hip.h -- the knowledge base of a batch whose questions share images (macx_kb_gather / macx_kb_gather_bwd):
// the stem runs once per IMAGE, and each question's [N, d] block is a copy of its image's block.
//
//   forward    kb[b] = kb_images[index[b]]                      one read and one write of B*N*d floats, dwordx4 both ways
//   backward   dkb_images[g] = sum over {b : index[b] == g} of dkb[b], b ascending, plain fp32 adds, no atomics
//
// One block is N*d floats = `quads` 16-byte quads.  A workgroup belongs to ONE question (forward) or ONE image (backward), so the
// index it reads is uniform over the workgroup (a scalar load); offsets are 64-bit.  The index is read when the kernel RUNS: a
// captured graph follows an index tensor rewritten between replays.
#pragma once
#include "macx_common.hip.h"

namespace macx {

constexpr int KBG_LOADS = 4;                       // forward: quads in flight per thread (64 bytes)
constexpr int KBG_CHUNK = 256 * KBG_LOADS;         // forward: quads per workgroup and pass = 16 KiB
constexpr int KBG_MAX_BLOCKS = 2048;               // a streaming grid's cap (256 CUs x 8 workgroups); the rest is grid-stride

// grid (chunks, questions).  An index outside [0, G) is never dereferenced: that question's block is filled with quiet NaN.
__global__ __launch_bounds__(256) void kb_gather_kernel(const f32x4* __restrict__ src, const int32_t* __restrict__ index, int G, int B,
                                                        size_t quads, f32x4* __restrict__ dst) {
  const float qnan = __int_as_float(0x7FC00000);
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int g = index[b];
    const bool ok = g >= 0 && g < G;
    const f32x4* s = src + (size_t)(ok ? g : 0) * quads;
    f32x4* o = dst + (size_t)b * quads;
    for (size_t c = (size_t)blockIdx.x * KBG_CHUNK; c < quads; c += (size_t)gridDim.x * KBG_CHUNK) {
      f32x4 v[KBG_LOADS];
#pragma unroll
      for (int k = 0; k < KBG_LOADS; ++k) {
        const size_t i = c + (size_t)k * 256 + threadIdx.x;
        v[k] = (ok && i < quads) ? s[i] : f32x4{qnan, qnan, qnan, qnan};
      }
#pragma unroll
      for (int k = 0; k < KBG_LOADS; ++k) {
        const size_t i = c + (size_t)k * 256 + threadIdx.x;
        if (i < quads) o[i] = v[k];
      }
    }
  }
}

// grid (chunks of 256 quads, images).  Every output quad is owned by one thread, which walks the questions in ascending order and
// adds the blocks of those that name its image: a fixed order, so identical calls give identical bits, and an image that no question
// names comes out as zeros (every element is written; nothing is cleared beforehand).  An index outside [0, G) matches no image.
__global__ __launch_bounds__(256) void kb_gather_bwd_kernel(const f32x4* __restrict__ dkb, const int32_t* __restrict__ index, int G, int B,
                                                            size_t quads, f32x4* __restrict__ out) {
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (size_t)gridDim.x * 256) {
      f32x4 acc{0.f, 0.f, 0.f, 0.f};
      for (int b = 0; b < B; ++b)
        if (index[b] == g) acc += dkb[(size_t)b * quads + i];
      out[(size_t)g * quads + i] = acc;
    }
  }
}

// ---- the same two with a knowledge-base SIZE per image (macx_kb_gather_l / macx_kb_gather_bwd_l) ----------------------------------
// image_lengths[g] (int32, device, read when the kernel runs) says how many of image g's N rows are live: L_g = clamp(., 1, N), the
// clamp of kb_attend_kernel.  A row is `row_quads` = d/4 quads, so the live part of a block is its first L_g * row_quads quads: a
// contiguous prefix, and the chunking of the plain kernels carries over with one more bound.
//
//   forward    rows n <  L_g of question b: the copy of its image's rows;  rows n >= L_g: +0.0f, the source is NOT read there (the
//              stem's output in padded rows is whatever it computed; the cell's backward pass wants finite padding);
//              len_out[b] = L_g.  An index outside [0, G): the all-NaN block of the plain kernel and len_out[b] = N, so that the
//              poison reaches the attention instead of hiding behind a length.
//   backward   rows n <  L_g of image g: the ascending-b fp32 sum of the plain kernel;  rows n >= L_g: zeros, dkb is NOT read there.
__global__ __launch_bounds__(256) void kb_gather_l_kernel(const f32x4* __restrict__ src, const int32_t* __restrict__ index,
                                                          const int32_t* __restrict__ lengths, int G, int B, int N, size_t row_quads,
                                                          f32x4* __restrict__ dst, int32_t* __restrict__ len_out) {
  const float qnan = __int_as_float(0x7FC00000);
  const size_t quads = (size_t)N * row_quads;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int g = index[b];
    const bool ok = g >= 0 && g < G;
    const int L = ok ? min(max(lengths[g], 1), N) : N;
    const size_t live = ok ? (size_t)L * row_quads : 0;          // quads read from the source
    const f32x4 fill = ok ? f32x4{0.f, 0.f, 0.f, 0.f} : f32x4{qnan, qnan, qnan, qnan};
    if (blockIdx.x == 0 && threadIdx.x == 0) len_out[b] = L;
    const f32x4* s = src + (size_t)(ok ? g : 0) * quads;
    f32x4* o = dst + (size_t)b * quads;
    for (size_t c = (size_t)blockIdx.x * KBG_CHUNK; c < quads; c += (size_t)gridDim.x * KBG_CHUNK) {
      f32x4 v[KBG_LOADS];
#pragma unroll
      for (int k = 0; k < KBG_LOADS; ++k) {
        const size_t i = c + (size_t)k * 256 + threadIdx.x;
        v[k] = i < live ? s[i] : fill;
      }
#pragma unroll
      for (int k = 0; k < KBG_LOADS; ++k) {
        const size_t i = c + (size_t)k * 256 + threadIdx.x;
        if (i < quads) o[i] = v[k];
      }
    }
  }
}

__global__ __launch_bounds__(256) void kb_gather_bwd_l_kernel(const f32x4* __restrict__ dkb, const int32_t* __restrict__ index,
                                                              const int32_t* __restrict__ lengths, int G, int B, int N,
                                                              size_t row_quads, f32x4* __restrict__ out) {
  const size_t quads = (size_t)N * row_quads;
  for (int g = blockIdx.y; g < G; g += gridDim.y) {
    const size_t live = (size_t)min(max(lengths[g], 1), N) * row_quads;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < quads; i += (size_t)gridDim.x * 256) {
      f32x4 acc{0.f, 0.f, 0.f, 0.f};
      if (i < live)
        for (int b = 0; b < B; ++b)
          if (index[b] == g) acc += dkb[(size_t)b * quads + i];
      out[(size_t)g * quads + i] = acc;
    }
  }
}

inline dim3 kbg_grid(size_t quads, int per_block, int outer) {
  const size_t chunks = (quads + per_block - 1) / per_block;
  const int oy = outer < 65535 ? outer : 65535;
  const size_t cap = (size_t)(KBG_MAX_BLOCKS / oy > 1 ? KBG_MAX_BLOCKS / oy : 1);
  return dim3((unsigned)(chunks < cap ? chunks : cap), (unsigned)oy);
}

}  // namespace macx
