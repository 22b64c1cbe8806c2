// macx_att_loss.hip.h -- a loss on the attention maps of a run (macx_att_loss): per (step, question) row of a stacked map [p,B,n]
// the loss value and the gradient d_att in the layout macx_state_grads takes, in ONE launch, so that a captured step can supervise
// its own maps between its forward and its backward launches.
//
//   w = scale * step_weights[i] * row_weights[b]          (NULL weights: 1),   L = clamp(lengths[b], 1, n)   (NULL: n)
//   MACX_ATT_LOSS_CE       row = -w sum_{j<L} t[j] log(a[j] + eps)       d_att[j] = -w t[j] / (a[j] + eps)
//   MACX_ATT_LOSS_ENTROPY  row =  w sum_{j<L} a[j] log(a[j] + eps)       d_att[j] =  w (log(a[j] + eps) + a[j] / (a[j] + eps))
//
// One wave per row, four rows per workgroup (answer_loss_kernel's shape), lanes strided over j, the per-lane partial sums combined
// by the xor shuffles of wave_sum: a fixed order, no atomics, identical calls give identical bits.  Cells j >= L are never read
// (they may hold NaN) and get d_att = +0.0f; a row with w == 0 reads nothing at all and is exact zeros.  (A LIVE cell whose target
// is exactly 0 gets CE's -w * 0 / (a + eps) = -0.0f under w > 0: +0.0f is promised for j >= L and for w == 0 only -- callers that
// compare bits.)  Weights and lengths are device data read when the kernel runs: one captured graph serves every batch.
//
// The per-element arithmetic is fp64 and rounds to fp32 once: the entropy's gradient log(a + eps) + a / (a + eps) passes through
// zero near a = 1/e, where an fp32 evaluation keeps no relative accuracy at all.  The map is p*B*n floats (150 K at the metric's
// shape); the kernel alone has not been timed -- the whole of supervision, this launch included, measures 0.028 ms per replayed step
// (DESIGN 4).  The sum over j runs in fp32 over the rounded terms.
#pragma once
#include "macx_common.hip.h"

namespace macx {

constexpr int ATT_LOSS_CE = 0, ATT_LOSS_ENTROPY = 1;        // MACX_ATT_LOSS_* of include/macx.h

struct AttLossP {
  const float* att;            // [p][B][n]
  const float* target;         // CE: [B][n] (target_steps 0) or [p][B][n]; entropy: unused
  const int32_t* lengths;      // [B] or null
  const float* step_weights;   // [p] or null
  const float* row_weights;    // [B] or null
  int p, B, n, target_steps;
  float eps, scale;
  float* loss_rows;            // [p][B]
  float* d_att;                // [p][B][n] or null
};

template <int KIND>
__global__ __launch_bounds__(256) void att_loss_kernel(AttLossP q) {
  const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= (size_t)q.p * q.B) return;                    // (wave-uniform: the shuffles below see whole waves)
  const int lane = threadIdx.x & 63;
  const int i = (int)(r / q.B), b = (int)(r % q.B);
  const double w = (double)q.scale * (q.step_weights ? q.step_weights[i] : 1.f) * (q.row_weights ? q.row_weights[b] : 1.f);
  float* d = q.d_att ? q.d_att + r * q.n : nullptr;
  if (w == 0.0) {                                          // an unsupervised row: exact zeros, whatever the map and the target hold
    if (lane == 0) q.loss_rows[r] = 0.f;
    if (d)
      for (int j = lane; j < q.n; j += 64) d[j] = 0.f;
    return;
  }
  const int L = q.lengths ? min(max(q.lengths[b], 1), q.n) : q.n;
  const float* a = q.att + r * q.n;
  const float* t = KIND == ATT_LOSS_CE ? q.target + (q.target_steps ? r : (size_t)b) * q.n : nullptr;
  float sum = 0.f;
  for (int j = lane; j < q.n; j += 64) {
    float g = 0.f;
    if (j < L) {
      const double ae = (double)a[j] + (double)q.eps, lg = log(ae);
      if (KIND == ATT_LOSS_CE) {
        const double tj = t[j];
        sum += (float)(tj * lg);
        g = (float)(-w * tj / ae);
      } else {
        const double aj = a[j];
        sum += (float)(aj * lg);
        g = (float)(w * (lg + aj / ae));
      }
    }
    if (d) d[j] = g;
  }
  sum = wave_sum(sum);
  if (lane == 0) q.loss_rows[r] = (float)((KIND == ATT_LOSS_CE ? -w : w) * (double)sum);
}

}  // namespace macx
