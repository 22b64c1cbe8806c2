// macx_questions.hip.h -- questions resident in device memory (macx_questions_gather / macx_preds_scatter): a question set as
// per-question tables (word ids [Q][S_tab], lengths, answers, image rows, knowledge-base sizes, weights), and the batch of a step
// gathered from them by question id -- every per-question static input of the tower's captured graphs from ONE launch.
//
//   gather    slot b <- question ids[b]: the word row (padded with 0 to S columns) and every scalar column; with grouping also the
//             batch's distinct image rows, numbered by first appearance, and each slot's group
//   scatter   table[ids[b]] = pred[b] for the live slots; of a repeated id the highest slot wins, decided by comparison
//
// The ids are read when the kernel RUNS: a captured graph follows an id tensor rewritten between replays.  What a slot holds:
//   live   0 <= id < Q     the question's row and columns; weight q_weights[id] (no table: 1.0f)
//   dead   id == -1        every integer column of slot 0's question when slot 0 is live, else of the pad question (words 0, length 0,
//                          answer 0, image row 0, kb length 1); weight +0.0f
//   other  anything else   never dereferenced.  words 0, length 0, answer -1, image row -1, kb length 1, weight 1.0f -- the loss
//                          kernel turns the label into a NaN loss, the feature gather the row into a NaN block -- and the constant
//                          1 goes to bad[0]: a plain store of the same value from every thread that sees one, never cleared here.
// No atomics, no allocation; offsets into the tables are 64-bit.
#pragma once
#include "macx_common.hip.h"

namespace macx {

constexpr int QG_MAX_BLOCKS = 256;                 // the gather's and the scatter's grid cap (one workgroup per CU); the rest is grid-stride
constexpr int QG_MAX_GROUP_B = 1024;               // grouping: the whole batch sits in one workgroup's LDS

struct QuestionsP {
  const int32_t *q_words, *q_lengths, *q_answers, *q_images, *q_kb_len;
  const float* q_weights;
  int Q, S_tab;
  const int32_t* ids;
  int B, S;
  int32_t *questions, *lengths, *answers, *image_ids, *kb_lengths;
  float* weights;
  int32_t* image_index;
  int G;
  int32_t* bad;
};

enum { QG_LIVE = 0, QG_PAD = 1, QG_POISON = 2 };

// where slot b's integer columns come from: the row of a live question (its own, or slot 0's for a dead slot), the pad question, or
// the poison.  `own`: the slot is live itself (its weight is the table's); an id is compared before it is ever used as an offset.
__device__ __forceinline__ int qg_resolve(const int32_t* __restrict__ ids, int Q, int b, int& row, bool& own) {
  const int id = ids[b];
  own = id >= 0 && id < Q;
  row = id;
  if (own) return QG_LIVE;
  if (id != -1) return QG_POISON;
  const int id0 = ids[0];
  row = id0;
  return (id0 >= 0 && id0 < Q) ? QG_LIVE : QG_PAD;
}

// grid-stride over units of V dwords (V = 4, 2, 1: 16-byte, 8-byte and scalar accesses; S_tab and S are multiples of V, so a unit
// lies wholly inside the table's columns or wholly in the padding).  The thread that owns a slot's first unit writes its scalar
// columns.  GROUP: workgroup 0 first numbers the batch's images (below) and writes image_ids / image_index; the row copy of every
// workgroup does not depend on it.
//
// Grouping (B <= QG_MAX_GROUP_B, one workgroup): the image rows of the LIVE slots in LDS; slot b's first occurrence is found by a
// linear search over the slots in front of it, a first occurrence's group number by counting the first occurrences in front of it --
// both quadratic in B (at most 4 slots x 1024 LDS reads per thread, every lane of a wave at the same address: broadcasts, no bank
// conflicts): fine for a batch of a few hundred questions, the intended range.
//   image_ids[g]     the g-th distinct row, g < min(D, G); slots D .. G-1 copies of image_ids[0] (no live slot at all: row 0)
//   image_index[b]   live: its row's group, or -1 when the group number is G or more (more distinct rows than G: bad[0] = 1);
//                    dead: slot 0's group, which is 0 (a live slot 0 is the first occurrence of its row; without one group 0 still
//                    names a valid image);  other: -1
template <int V, bool GROUP>
__global__ __launch_bounds__(256) void questions_gather_kernel(const QuestionsP a) {
  typedef int32_t ivec __attribute__((ext_vector_type(V)));
  const int t = threadIdx.x;
  bool bad = false;
  if (GROUP && blockIdx.x == 0) {
    __shared__ int32_t s_row[QG_MAX_GROUP_B];      // image row of a live slot
    __shared__ int16_t s_first[QG_MAX_GROUP_B];    // live: the first slot with the same row; dead: -1; other: -2
    __shared__ int16_t s_group[QG_MAX_GROUP_B];    // of a first occurrence: its number
    __shared__ int32_t s_row0, s_count;            // image_ids[0] and the number of distinct rows
    if (t == 0) { s_row0 = 0; s_count = 0; }
    for (int b = t; b < a.B; b += 256) {
      const int id = a.ids[b];
      const bool live = id >= 0 && id < a.Q;
      s_row[b] = live ? a.q_images[id] : 0;
      s_first[b] = live ? (int16_t)b : (int16_t)(id == -1 ? -1 : -2);
    }
    __syncthreads();
    int first[QG_MAX_GROUP_B / 256];
#pragma unroll
    for (int k = 0; k < QG_MAX_GROUP_B / 256; ++k) {
      const int b = k * 256 + t;
      first[k] = b < a.B ? s_first[b] : -2;
      if (first[k] >= 0) {
        const int row = s_row[b];
        for (int c = 0; c < b; ++c)
          if (s_first[c] >= 0 && s_row[c] == row) { first[k] = c; break; }
      }
    }
    __syncthreads();                               // (every search read s_first as the first pass left it)
#pragma unroll
    for (int k = 0; k < QG_MAX_GROUP_B / 256; ++k) {
      const int b = k * 256 + t;
      if (b < a.B) s_first[b] = (int16_t)first[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < QG_MAX_GROUP_B / 256; ++k) {
      const int b = k * 256 + t;
      if (b < a.B) {
        int n = 0;
        for (int c = 0; c < b; ++c) n += s_first[c] == c;
        const bool is_first = first[k] == b;
        s_group[b] = (int16_t)n;
        if (is_first && n == 0) s_row0 = s_row[b];
        if (b == a.B - 1) s_count = n + (is_first ? 1 : 0);
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < QG_MAX_GROUP_B / 256; ++k) {
      const int b = k * 256 + t;
      if (b < a.B) {
        int index = -1;
        if (first[k] >= 0) {
          const int g = s_group[first[k]];
          if (g < a.G) {
            index = g;
            if (first[k] == b) a.image_ids[g] = s_row[b];
          } else {
            bad = true;
          }
        } else if (first[k] == -1) {
          index = 0;
        }
        a.image_index[b] = index;
      }
    }
    for (int g = s_count + t; g < a.G; g += 256) a.image_ids[g] = s_row0;
  }
  const size_t tab_units = (size_t)(a.S_tab / V), row_units = (size_t)(a.S / V), units = (size_t)a.B * row_units;
  for (size_t u = (size_t)blockIdx.x * 256 + t; u < units; u += (size_t)gridDim.x * 256) {
    const int b = (int)(u / row_units);
    const size_t c = u - (size_t)b * row_units;
    int row;
    bool own;
    const int kind = qg_resolve(a.ids, a.Q, b, row, own);
    ivec w = {};
    if (kind == QG_LIVE && c < tab_units) w = reinterpret_cast<const ivec*>(a.q_words)[(size_t)row * tab_units + c];
    reinterpret_cast<ivec*>(a.questions)[u] = w;
    if (c == 0) {
      const bool live = kind == QG_LIVE, poison = kind == QG_POISON;
      bad |= poison;
      a.lengths[b] = live ? a.q_lengths[row] : 0;
      if (a.answers) a.answers[b] = live ? a.q_answers[row] : (poison ? -1 : 0);
      if (!GROUP && a.image_ids) a.image_ids[b] = live ? a.q_images[row] : (poison ? -1 : 0);
      if (a.kb_lengths) a.kb_lengths[b] = live ? a.q_kb_len[row] : 1;
      if (a.weights) a.weights[b] = own ? (a.q_weights ? a.q_weights[row] : 1.0f) : (poison ? 1.0f : 0.0f);
    }
  }
  if (bad && a.bad) a.bad[0] = 1;
}

inline unsigned qg_blocks(size_t units) {
  const size_t blocks = (units + 255) / 256;
  return (unsigned)(blocks < (size_t)QG_MAX_BLOCKS ? blocks : (size_t)QG_MAX_BLOCKS);
}

template <int V>
inline hipError_t questions_gather_launch(const QuestionsP& a, hipStream_t st) {
  const dim3 grid(qg_blocks((size_t)a.B * (a.S / V)));
  if (a.image_index)
    hipLaunchKernelGGL((questions_gather_kernel<V, true>), grid, dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL((questions_gather_kernel<V, false>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

// table[ids[b]] = pred[b] for 0 <= ids[b] < Q, unless a higher slot names the same id: then that slot's value is the one stored, and
// this thread stores nothing -- one store per table entry, whatever order the stores retire in.  The search for a later slot is
// linear, so the launch is quadratic in B: meant for a batch of a few hundred to a few thousand questions.
__global__ __launch_bounds__(256) void preds_scatter_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ ids, int B, int Q,
                                                            int32_t* __restrict__ table) {
  for (size_t b = (size_t)blockIdx.x * 256 + threadIdx.x; b < (size_t)B; b += (size_t)gridDim.x * 256) {
    const int id = ids[b];
    if (id < 0 || id >= Q) continue;
    bool last = true;
    for (size_t c = b + 1; c < (size_t)B && last; ++c) last = ids[c] != id;
    if (last) table[(size_t)id] = pred[b];
  }
}

}  // namespace macx
