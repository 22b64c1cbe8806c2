// macx_records.hip.h -- evaluation records resident in device memory (macx_records_scatter): a run's attention maps and logits filed
// by question id, table[ids[b]][i][:] = convert(src[i][b][:]) -- a transpose from step-major to question-major -- for up to
// MACX_RECORDS_MAX tables from ONE launch (the descriptors travel by value in the kernel argument, as PackList does).
//
// The ids are read when the kernel RUNS: a captured graph follows an id tensor rewritten between replays.  Slot rules as in
// macx_preds_scatter: only 0 <= id < Q stores, every other id is compared and never used as an offset; of a repeated id the HIGHEST
// slot's rows are the ones stored, decided by comparison: a slot stores only if no later slot names its id.
//
// A row unit is (table, step i, slot b): n contiguous source elements to n contiguous table elements.  One WAVE owns a unit, so the
// decision "a later slot names my id" is wave-uniform: the 64 lanes scan ids[b+1 .. B) 64 at a time and vote (__any); the scan ends at
// the first chunk that holds the id.  No atomics, no LDS, no allocation; offsets are 64-bit.
// fp32 -> fp16 is round-to-nearest-even with subnormals kept (v_cvt_f16_f32 under the default mode: no fast-math in this build), the
// sign of zero preserved, NaN -> NaN, beyond 65504 + half an ulp -> infinity; an fp32 table takes the source bits.
#pragma once
#include "macx_common.hip.h"

namespace macx {

constexpr int REC_MAX = 4;                         // MACX_RECORDS_MAX
constexpr int REC_MAX_BLOCKS = 512;                // grid cap in x (4 waves a workgroup, two workgroups per CU); the rest is grid-stride

// vec: elements per access (4, 2, 1) -- the widest that n, both base pointers and the table's element size allow
struct RecordDesc { const float* src; void* table; int steps, n, dtype, vec; };
struct RecordList { RecordDesc d[REC_MAX]; };
static_assert(sizeof(RecordList) <= 4096, "RecordList travels by value as a kernel argument");

template <typename T> struct RecElem;
template <> struct RecElem<float> { static __device__ __forceinline__ float from(float x) { return x; } };
template <> struct RecElem<_Float16> { static __device__ __forceinline__ _Float16 from(float x) { return (_Float16)x; } };

// one row of n elements by the wave's 64 lanes, V elements per access (n % V == 0; src and dst aligned to V elements)
template <typename T, int V>
__device__ __forceinline__ void rec_copy_row(const float* __restrict__ src, T* __restrict__ dst, int n, int lane) {
  typedef float fvec __attribute__((ext_vector_type(V)));
  typedef T tvec __attribute__((ext_vector_type(V)));
  for (int j = lane; j < n / V; j += 64) {
    if constexpr (V == 1) {
      dst[j] = RecElem<T>::from(src[j]);
    } else {
      const fvec x = reinterpret_cast<const fvec*>(src)[j];
      tvec y;
#pragma unroll
      for (int e = 0; e < V; ++e) y[e] = RecElem<T>::from(x[e]);
      reinterpret_cast<tvec*>(dst)[j] = y;
    }
  }
}

template <typename T>
__device__ __forceinline__ void rec_copy(const float* __restrict__ src, T* __restrict__ dst, int n, int vec, int lane) {
  if (vec == 4) rec_copy_row<T, 4>(src, dst, n, lane);
  else if (vec == 2) rec_copy_row<T, 2>(src, dst, n, lane);
  else rec_copy_row<T, 1>(src, dst, n, lane);
}

// blockIdx.y: the table; the waves of the x dimension stride over its steps * B row units
__global__ __launch_bounds__(256) void records_scatter_kernel(const RecordList L, const int32_t* __restrict__ ids, int B, int Q) {
  const RecordDesc q = L.d[blockIdx.y];
  const int lane = threadIdx.x & 63;
  const size_t wave = (size_t)blockIdx.x * 4 + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const size_t waves = (size_t)gridDim.x * 4, units = (size_t)q.steps * (size_t)B;
  for (size_t u = wave; u < units; u += waves) {
    const size_t i = u / (size_t)B, b = u - i * (size_t)B;
    const int id = ids[b];
    if (id < 0 || id >= Q) continue;                 // dead (-1) and every other id: nothing is stored, nothing is dereferenced
    bool later = false;                              // does a higher slot name this id?  (wave-uniform)
    for (size_t c0 = b + 1; c0 < (size_t)B && !later; c0 += 64) {
      const size_t c = c0 + lane;
      later = __any(c < (size_t)B && ids[c] == id) != 0;
    }
    if (later) continue;
    const float* src = q.src + (i * (size_t)B + b) * (size_t)q.n;
    const size_t at = ((size_t)id * (size_t)q.steps + i) * (size_t)q.n;
    if (q.dtype == MACX_FEATURES_F16) rec_copy(src, reinterpret_cast<_Float16*>(q.table) + at, q.n, q.vec, lane);
    else rec_copy(src, reinterpret_cast<float*>(q.table) + at, q.n, q.vec, lane);
  }
}

}  // namespace macx
