// macx_rnn.hip.h -- the recurrence of the question encoder's other cells (ops.createCell, ops.py:749-772), on the design of
// lstm_step_kernel / lstm_step_bwd_kernel (macx_small.hip.h):
//   BasicRNNCell   h' = tanh([x, h] K + b)
//   GRUCell (TF1)  r, u = split(sigmoid([x, h] Kg + bg)) ; c = tanh([x, r * h] Kc + bc) ; h' = u * h + (1 - u) * c
// under dynamic_rnn / bidirectional_dynamic_rnn semantics: past a question's end the state is copied through and the output is +0;
// direction 1 reads position L - 1 - tau and writes its output back there.
//
// A workgroup owns 16 questions x 16 units of one direction; the waves split the reduction over the product's k, the product is
// v_mfma_f32_16x16x4f32 (exact fp32) on pack-format-0 weights, the partial sums meet in LDS in fixed order.  The RNN takes one
// launch per time step and pass; the GRU two: its candidate needs r * h of ALL units of a question, and its backward needs
// d(r * h) = dc_pre Kc_h^T of all units before the second product [dr_pre, du_pre] Kg_h^T.  The units are split across
// workgroups, so that dependency is a launch boundary: no workgroup of these launches waits for another one.
//
// Per direction a position's columns are one row of width GT: the RNN's h pre-activations, or the GRU's [r | u | c] (GT = 3h).
// Zx (the input projections), kept (what the backward pass needs per step), dG (per step) and dZ (per position) share that row.
#pragma once
#include "macx_common.hip.h"

namespace macx {

enum { RNN_BASIC = 0, RNN_GRU_GATES = 1, RNN_GRU_CAND = 2 };
constexpr int rnn_mode_gates(int mode) { return mode == RNN_GRU_GATES ? 2 : 1; }

struct RnnStepP {
  int B, S, h, tau, dirs, GT;
  const int32_t* len;      // [B]
  const float* Wh;         // [dirs] packed [h/16][4][NG h][4] (pack format 0): the recurrent block of this launch's matrix
  const float* Zx;         // [dirs][B*S][GT]  x Wx + b  (all positions)
  float* hs;               // [dirs][S+1][B][h]
  float* kept;             // [dirs][S][B][GT]   GRU: r | u | c of the step
  float* rh;               // [dirs][S][B][h]    GRU: r * h_prev
  float* out;              // [B][S][dirs h]  (zero-initialised)
};

// Grid (h / 16, ceil(B / 16), dirs), 256 threads.
template <int MODE>
__global__ __launch_bounds__(256) void rnn_step_kernel(RnnStepP p) {
  constexpr int NG = rnn_mode_gates(MODE);
  __shared__ float red[4][NG][16][17];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int u0 = blockIdx.x * 16, r0 = blockIdx.y * 16, dir = blockIdx.z;
  const int h = p.h, G = NG * h, GT = p.GT;
  const size_t Bh = (size_t)p.B * h;
  // the product's left operand: h_prev, or for the candidate r * h_prev
  const float* hp = MODE == RNN_GRU_CAND ? p.rh + (size_t)(dir * p.S + p.tau) * Bh : p.hs + (size_t)(dir * (p.S + 1) + p.tau) * Bh;
  const float* Wd = p.Wh + (size_t)dir * h * G;
  const int rowc = min(r0 + li, p.B - 1);
  f32x4 acc[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nQ = h >> 4;
  constexpr int PF = 4;                     // k groups in flight per wave
  // what the cell needs behind the product is requested BEFORE it: this thread's (question, unit)
  const int crow = tid >> 4, cuu = tid & 15;
  const int cb = min(r0 + crow, p.B - 1), cu = u0 + cuu;
  const int cL = min(max(p.len[cb], 0), p.S);      // never index past the padded question (the host validates too)
  const int cpos = dir == 0 ? p.tau : max(cL - 1 - p.tau, 0);
  const size_t cs0 = (size_t)(dir * (p.S + 1) + p.tau) * Bh + (size_t)cb * h + cu;
  const float hpv = p.hs[cs0];
  const float* Zpre = p.Zx + ((size_t)dir * p.B * p.S + (size_t)cb * p.S + cpos) * GT;
  float* kp = p.kept + ((size_t)(dir * p.S + p.tau) * p.B + cb) * GT;
  float z[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) z[g] = Zpre[(MODE == RNN_GRU_CAND ? 2 * h : g * h) + cu];
  float upd = 0.f;
  if (MODE == RNN_GRU_CAND) upd = kp[h + cu];
  for (int Q0 = wave; Q0 < nQ; Q0 += 4 * PF) {
    f32x4 af[PF], bf[PF][NG];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int Q = min(Q0 + 4 * u, nQ - 1);
      af[u] = *reinterpret_cast<const f32x4*>(hp + (size_t)rowc * h + Q * 16 + lg * 4);
#pragma unroll
      for (int g = 0; g < NG; ++g)
        bf[u][g] = *reinterpret_cast<const f32x4*>(Wd + ((size_t)(Q * 4 + lg) * G + g * h + u0 + li) * 4);
    }
#pragma unroll
    for (int u = 0; u < PF; ++u)
      if (Q0 + 4 * u < nQ) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int g = 0; g < NG; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][e], bf[u][g][e], acc[g], 0, 0, 0);
      }
  }
  // accumulator map: unit = lane & 15, question = (lane >> 4) * 4 + e
#pragma unroll
  for (int g = 0; g < NG; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) red[wave][g][lg * 4 + e][li] = acc[g][e];
  __syncthreads();
  const int row = crow, uu = cuu;
  if (r0 + row >= p.B) return;
  float R[NG];
#pragma unroll
  for (int g = 0; g < NG; ++g) R[g] = ((red[0][g][row][uu] + red[1][g][row][uu]) + red[2][g][row][uu]) + red[3][g][row][uu];
  const bool active = p.tau < cL;
  if (MODE == RNN_GRU_GATES) {
    float r = 0.f, u = 0.f;
    if (active) {
      r = 1.0f / (1.0f + expf(-(R[0] + z[0])));
      u = 1.0f / (1.0f + expf(-(R[NG - 1] + z[NG - 1])));
    }
    kp[cu] = r; kp[h + cu] = u;
    p.rh[(size_t)(dir * p.S + p.tau) * Bh + (size_t)cb * h + cu] = r * hpv;
  } else {
    float hn = hpv, c = 0.f;
    if (active) {
      c = tanhf(R[0] + z[0]);
      hn = MODE == RNN_GRU_CAND ? upd * hpv + (1.0f - upd) * c : c;
      p.out[((size_t)cb * p.S + cpos) * p.dirs * h + dir * h + cu] = hn;
    }
    if (MODE == RNN_GRU_CAND) kp[2 * h + cu] = c;
    p.hs[cs0 + Bh] = hn;
  }
}

// The backward step: the cell's backward of the workgroup's 16 questions over all h units (recomputed by each of the h / 16
// workgroups that share the questions: the product needs every column), then [16 questions][16 units] = dG W^T from the LDS tile.
//   RNN_BASIC      dG = dh (1 - h'^2)                                   -> dh_prev = dG Kh^T            (+ dh where the question has ended)
//   RNN_GRU_CAND   dG_c = dh (1 - u)(1 - c^2)                           -> d(r h) = dG_c Kc_h^T         (first launch of the step)
//   RNN_GRU_GATES  dG_r = d(r h) h r (1 - r), dG_u = dh (h - c) u (1 - u) -> dh_prev = [dG_r, dG_u] Kg_h^T + d(r h) r + dh u
// with dh = the running gradient + the output's gradient at the step's position.  The running dh is double-buffered by the
// caller (a workgroup reads what its neighbours would otherwise be overwriting); each workgroup writes dG and dZ of its own units.
struct RnnStepBwdP {
  int B, S, h, tau, dirs, GT;
  const int32_t* len;
  const float* WT;         // [dirs] packed [NG h/16][4][h][4] (pack format 0 of the recurrent block's transpose)
  const float* hs;         // [dirs][S+1][B][h]
  const float* kept;       // [dirs][S][B][GT]
  const float* dout;       // [B][S][dirs h]
  const float* dh_in;      // [dirs][B][h] running state gradient after step tau + 1
  float* dh_out;           // ... after this step (RNN_GRU_CAND: unused)
  float* drh;              // [dirs][B][h]  d(r h): written by RNN_GRU_CAND, read by RNN_GRU_GATES
  float* dG;               // [dirs][S][B][GT]
  float* dZ;               // [dirs][B*S][GT] (zero-initialised)
};
constexpr int RSB_THREADS = 1024;
template <int MODE>
__global__ __launch_bounds__(RSB_THREADS) void rnn_step_bwd_kernel(RnnStepBwdP p) {
  constexpr int NG = rnn_mode_gates(MODE);
  extern __shared__ __attribute__((aligned(16))) float lsm[];
  const int h = p.h, G = NG * h, GT = p.GT;
  float* sG = lsm;                          // [16][G + 4] pre-activation gradients of the workgroup's questions
  float* sPass = sG + 16 * (G + 4);         // [16][16] what reaches dh_prev beside the product
  float* red = sPass + 256;                 // [16 waves][16][17]
  const int ldg = G + 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int u0 = blockIdx.x * 16, r0 = blockIdx.y * 16, dir = blockIdx.z;
  const size_t Bh = (size_t)p.B * h;
  // the weights of this wave's first k groups are requested ahead of the cell's backward
  const float* Wd = p.WT + (size_t)dir * G * h;
  const int nQ = G >> 4;
  constexpr int PF = 4, NW = RSB_THREADS / 64;
  f32x4 bf0[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) bf0[u] = *reinterpret_cast<const f32x4*>(Wd + ((size_t)(min(wave + NW * u, nQ - 1) * 4 + lg) * h + u0 + li) * 4);
#pragma unroll 4
  for (int it = tid; it < 16 * h; it += RSB_THREADS) {
    const int row = it / h, u = it - row * h;
    const int b = r0 + row;
    const bool own = u >= u0 && u < u0 + 16;
    float g0 = 0.f, g1 = 0.f, pass = 0.f;
    if (b < p.B) {
      const size_t i = (size_t)dir * Bh + (size_t)b * h + u;
      const int L = min(max(p.len[b], 0), p.S);
      const bool active = p.tau < L;
      const int pos = dir == 0 ? p.tau : L - 1 - p.tau;
      float dh = p.dh_in[i];
      pass = MODE == RNN_GRU_CAND ? 0.f : dh;
      if (active) {
        const size_t r = (size_t)b * h + u;
        const float* kp = p.kept + ((size_t)(dir * p.S + p.tau) * p.B + b) * GT;
        dh += p.dout[((size_t)b * p.S + pos) * p.dirs * h + dir * h + u];
        if (MODE == RNN_BASIC) {
          const float hn = p.hs[(size_t)(dir * (p.S + 1) + p.tau + 1) * Bh + r];
          g0 = dh * (1.0f - hn * hn);
          pass = 0.f;
        } else if (MODE == RNN_GRU_CAND) {
          const float uv = kp[h + u], c = kp[2 * h + u];
          g0 = dh * (1.0f - uv) * (1.0f - c * c);
        } else {
          const float rv = kp[u], uv = kp[h + u], c = kp[2 * h + u];
          const float hpv = p.hs[(size_t)(dir * (p.S + 1) + p.tau) * Bh + r];
          const float drh = p.drh[i];
          g0 = drh * hpv * rv * (1.0f - rv);
          g1 = dh * (hpv - c) * uv * (1.0f - uv);
          pass = drh * rv + dh * uv;
        }
        if (own) {
          float* zr = p.dZ + ((size_t)dir * p.B * p.S + (size_t)b * p.S + pos) * GT;
          if (MODE == RNN_GRU_CAND) zr[2 * h + u] = g0;
          else { zr[u] = g0; if (NG == 2) zr[h + u] = g1; }
        }
      }
      if (own) {
        float* gr = p.dG + ((size_t)(dir * p.S + p.tau) * p.B + b) * GT;
        if (MODE == RNN_GRU_CAND) gr[2 * h + u] = g0;
        else { gr[u] = g0; if (NG == 2) gr[h + u] = g1; }
      }
    }
    float* sg = sG + row * ldg;
    sg[u] = g0;
    if (NG == 2) sg[h + u] = g1;
    if (own) sPass[row * 16 + (u - u0)] = pass;
  }
  __syncthreads();
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int Q0 = wave; Q0 < nQ; Q0 += NW * PF) {
    f32x4 af[PF], bf[PF];
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int Q = min(Q0 + NW * u, nQ - 1);
      af[u] = *reinterpret_cast<const f32x4*>(sG + li * ldg + Q * 16 + lg * 4);
      bf[u] = Q0 == wave ? bf0[u] : *reinterpret_cast<const f32x4*>(Wd + ((size_t)(Q * 4 + lg) * h + u0 + li) * 4);
    }
#pragma unroll
    for (int u = 0; u < PF; ++u)
      if (Q0 + NW * u < nQ) {
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][e], bf[u][e], acc, 0, 0, 0);
      }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[(wave * 16 + lg * 4 + e) * 17 + li] = acc[e];
  __syncthreads();
  if (tid >= 256) return;
  const int row = tid >> 4, uu = tid & 15;
  const int b = r0 + row;
  if (b >= p.B) return;
  float v = red[row * 17 + uu];
#pragma unroll
  for (int w = 1; w < NW; ++w) v += red[(w * 16 + row) * 17 + uu];        // fixed order
  float* dst = MODE == RNN_GRU_CAND ? p.drh : p.dh_out;
  dst[(size_t)dir * Bh + (size_t)b * h + u0 + uu] = v + sPass[row * 16 + uu];
}
inline size_t rnn_step_bwd_lds(int h, int gates) { return ((size_t)16 * (gates * h + 4) + 256 + (RSB_THREADS / 64) * 16 * 17) * sizeof(float); }

}  // namespace macx
