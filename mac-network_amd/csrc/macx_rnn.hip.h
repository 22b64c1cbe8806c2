// macx_rnn.hip.h -- the question encoder (model.py:208-307, ops.py:749-911): the embedding lookup and the recurrence of every cell
// ops.createCell builds with an activation (ops.py:749-772):
//   BasicRNNCell         h' = tanh([x, h] K + b)
//   GRUCell (TF1)        r, u = split(sigmoid([x, h] Kg + bg)) ; c = tanh([x, r * h] Kc + bc) ; h' = u * h + (1 - u) * c
//   BasicLSTMCell (TF1)  gates i, j, f, o = split([x, h] K + b) ; c' = c * sigmoid(f + 1) + sigmoid(i) * tanh(j) ; h' = tanh(c') * sigmoid(o)
// under dynamic_rnn / bidirectional_dynamic_rnn semantics: past a question's end the state is copied through and the output is +0;
// direction 1 reads position L - 1 - tau and writes its output back there.
//
// One step of all directions is ONE launch, R = h_prev Wh and the cell behind it: a launch of its own for either was ~6 us of pure
// latency, 100 dependent pairs per forward pass.  A workgroup owns 16 questions x 16 units of one direction and so every gate of
// its units; the waves split the reduction over the product's k, the product is v_mfma_f32_16x16x4f32 (exact fp32) on
// pack-format-0 weights, the partial sums meet in LDS in fixed order.  The RNN and the LSTM take one launch per time step and
// pass; the GRU two: its candidate needs r * h of ALL units of a question, and its backward needs d(r * h) = dc_pre Kc_h^T of all
// units before the second product [dr_pre, du_pre] Kg_h^T.  The units are split across workgroups, so that dependency is a
// launch boundary: no workgroup of these launches waits for another one.
//
// Per direction a position's columns are one row of width GT: the RNN's h pre-activations, the GRU's [r | u | c] (GT = 3h), the
// LSTM's [i | j | f | o] (GT = 4h).  Zx (the input projections), kept (what the backward pass needs per step), dG (per step) and
// dZ (per position) share that row.
#pragma once
#include "macx_common.hip.h"

namespace macx {

// x[b][s][0:E] = dropout(embeddings[idx]) with embeddings = concat([zeros(1,E), emb]) (model.py:217); columns E..Ep-1 = 0
__global__ void embed_gather_kernel(const int32_t* __restrict__ idx, const float* __restrict__ emb, int rows, int E, int Ep, uint32_t row0,
                                    DropSpec ds, float* x) {
  ds = drop_resolve(ds);
  const size_t total = (size_t)rows * Ep;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / Ep;
    const int c = (int)(i - r * Ep);
    float v = 0.f;
    if (c < E) {
      const int t = idx[r];
      if (t > 0) v = emb[(size_t)(t - 1) * E + c];
      v = drop_apply(v, (uint32_t)((row0 + r) * E + c), ds);
    }
    x[i] = v;
  }
}

// d emb[v-1][c] = sum over tokens == v of dropmask * dx[r][c]   (one workgroup per vocabulary row: no atomics).
// The rows that hold token v are found 256 at a time by all threads (ballot + ordered compaction into LDS), then summed in
// ascending row order: the scan is rows / 256 short passes instead of `rows` sequential compares per thread.
__global__ __launch_bounds__(256) void embed_grad_kernel(const int32_t* __restrict__ idx, const float* __restrict__ dx, int rows, int E, int Ep,
                                                        uint32_t row0, DropSpec ds, float* demb) {
  ds = drop_resolve(ds);
  __shared__ int list[256];
  __shared__ int wcount[4];
  const int v = blockIdx.x + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int CMAX = 4;                           // columns per thread held in registers: blockIdx.y selects a chunk of 1024 columns
  const int c0 = blockIdx.y * 1024;
  float acc[CMAX];
#pragma unroll
  for (int k = 0; k < CMAX; ++k) acc[k] = 0.f;
  for (int r0 = 0; r0 < rows; r0 += 256) {
    const int r = r0 + tid;
    const bool m = r < rows && idx[r] == v;
    const unsigned long long mask = __ballot(m);
    const int before = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wcount[wave] = __popcll(mask);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { base += w < wave ? wcount[w] : 0; total += wcount[w]; }
    if (m) list[base + before] = r;
    __syncthreads();
    for (int k = 0; k < total; ++k) {                // ascending rows
      const int rr = list[k];
#pragma unroll
      for (int j = 0; j < CMAX; ++j) {
        const int c = c0 + tid + 256 * j;
        if (c < E) acc[j] += drop_apply(dx[(size_t)rr * Ep + c], (uint32_t)((row0 + rr) * E + c), ds);
      }
    }
    __syncthreads();                                 // list / wcount are rewritten by the next pass
  }
#pragma unroll
  for (int j = 0; j < CMAX; ++j) {
    const int c = c0 + tid + 256 * j;
    if (c < E) demb[(size_t)(v - 1) * E + c] = acc[j];
  }
}

enum { RNN_BASIC = 0, RNN_GRU_GATES = 1, RNN_GRU_CAND = 2, RNN_LSTM = 3 };
constexpr int rnn_mode_gates(int mode) { return mode == RNN_LSTM ? 4 : mode == RNN_GRU_GATES ? 2 : 1; }

struct RnnStepP {
  int B, S, h, tau, dirs, GT;
  const int32_t* len;      // [B]
  const float* Wh;         // [dirs] packed [h/16][4][NG h][4] (pack format 0): the recurrent block of this launch's matrix
  const float* Zx;         // [dirs][B*S][GT]  x Wx + b  (all positions)
  float* hs;               // [dirs][S+1][B][h]
  float* kept;             // [dirs][S][B][GT]   GRU: r | u | c of the step; LSTM: its gates i | j | f | o
  float* rh;               // [dirs][S][B][h]    GRU: r * h_prev
  float* out;              // [B][S][dirs h]  (zero-initialised)
  float* cs;               // [dirs][S+1][B][h]  LSTM: the cell state beside hs
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
  constexpr int PF = 4;                     // k groups in flight per wave (the LSTM at h = 256: the wave's whole share)
  // what the cell needs behind the product -- this thread's (question, unit): length, previous state, the input projection's
  // columns -- is requested BEFORE the product, so that its round trip does not start behind the barrier
  const int crow = tid >> 4, cuu = tid & 15;
  const int cb = min(r0 + crow, p.B - 1), cu = u0 + cuu;
  const int cL = min(max(p.len[cb], 0), p.S);      // never index past the padded question (the host validates too)
  const int cpos = dir == 0 ? p.tau : max(cL - 1 - p.tau, 0);
  const size_t cs0 = (size_t)(dir * (p.S + 1) + p.tau) * Bh + (size_t)cb * h + cu;
  const float hpv = p.hs[cs0];
  float cp = 0.f;
  if (MODE == RNN_LSTM) cp = p.cs[cs0];
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
  if constexpr (MODE == RNN_LSTM) {
    float hn = hpv, cn = cp;
    float gi = 0.f, gj = 0.f, gf = 0.f, go = 0.f;
    if (active) {
      gi = 1.0f / (1.0f + expf(-(R[0] + z[0])));
      gj = tanhf(R[1] + z[1]);
      gf = 1.0f / (1.0f + expf(-(R[2] + z[2] + 1.0f)));
      go = 1.0f / (1.0f + expf(-(R[3] + z[3])));
      cn = cp * gf + gi * gj;
      hn = tanhf(cn) * go;
      p.out[((size_t)cb * p.S + cpos) * p.dirs * h + dir * h + cu] = hn;
    }
    p.hs[cs0 + Bh] = hn;
    p.cs[cs0 + Bh] = cn;
    kp[cu] = gi; kp[h + cu] = gj; kp[2 * h + cu] = gf; kp[3 * h + cu] = go;
  } else if (MODE == RNN_GRU_GATES) {
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
// workgroups that share the questions: the product needs every column, and elementwise work is cheaper than a launch), then
// [16 questions][16 units] = dG W^T from the LDS tile.
//   RNN_BASIC      dG = dh (1 - h'^2)                                   -> dh_prev = dG Kh^T            (+ dh where the question has ended)
//   RNN_GRU_CAND   dG_c = dh (1 - u)(1 - c^2)                           -> d(r h) = dG_c Kc_h^T         (first launch of the step)
//   RNN_GRU_GATES  dG_r = d(r h) h r (1 - r), dG_u = dh (h - c) u (1 - u) -> dh_prev = [dG_r, dG_u] Kg_h^T + d(r h) r + dh u
//   RNN_LSTM       dc' = dc + dh o (1 - tanh(c')^2): dG_i = dc' j i (1 - i), dG_j = dc' i (1 - j^2), dG_f = dc' c f (1 - f),
//                  dG_o = dh tanh(c') o (1 - o), dc_prev = dc' f                -> dh_prev = dG Kh^T   (+ dh where the question has ended)
// with dh = the running gradient + the output's gradient at the step's position.  The running dh (the LSTM's dc beside it) is
// double-buffered by the caller (a workgroup reads what its neighbours would otherwise be overwriting); each workgroup writes
// dG, dZ and dc of its own units.
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
  const float* cs;         // [dirs][S+1][B][h]  LSTM
  const float* dc_in;      // [dirs][B][h]  LSTM: the running cell-state gradient, as dh_in
  float* dc_out;           // ... as dh_out
};
constexpr int RSB_THREADS = 1024;      // 16 waves: the elementwise part is h / 64 (question, unit) pairs per thread, the LSTM's product 4 k groups per wave at h = 256
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
  // the weights of this wave's first k groups are requested ahead of the cell's backward: their L2 round trip runs under it
  // instead of behind the barrier (the launch is latency, 100 of them in a row)
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
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f, pass = 0.f, dc = 0.f;
    if (b < p.B) {
      const size_t i = (size_t)dir * Bh + (size_t)b * h + u;
      const int L = min(max(p.len[b], 0), p.S);
      const bool active = p.tau < L;
      const int pos = dir == 0 ? p.tau : L - 1 - p.tau;
      float dh = p.dh_in[i];
      if (MODE == RNN_LSTM) dc = p.dc_in[i];
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
        } else if (MODE == RNN_GRU_GATES) {
          const float rv = kp[u], uv = kp[h + u], c = kp[2 * h + u];
          const float hpv = p.hs[(size_t)(dir * (p.S + 1) + p.tau) * Bh + r];
          const float drh = p.drh[i];
          g0 = drh * hpv * rv * (1.0f - rv);
          g1 = dh * (hpv - c) * uv * (1.0f - uv);
          pass = drh * rv + dh * uv;
        } else {
          const float gi = kp[u], gj = kp[h + u], gf = kp[2 * h + u], go = kp[3 * h + u];
          const float cp = p.cs[(size_t)(dir * (p.S + 1) + p.tau) * Bh + r];
          const float cn = p.cs[(size_t)(dir * (p.S + 1) + p.tau + 1) * Bh + r];
          const float tc = tanhf(cn);
          g3 = dh * tc * go * (1.0f - go);
          const float dct = dc + dh * go * (1.0f - tc * tc);
          g0 = dct * gj * gi * (1.0f - gi);
          g1 = dct * gi * (1.0f - gj * gj);
          g2 = dct * cp * gf * (1.0f - gf);
          dc = dct * gf;
          pass = 0.f;
        }
        if (own) {
          float* zr = p.dZ + ((size_t)dir * p.B * p.S + (size_t)b * p.S + pos) * GT;
          if (MODE == RNN_GRU_CAND) zr[2 * h + u] = g0;
          else { zr[u] = g0; if (NG >= 2) zr[h + u] = g1; if (NG == 4) { zr[2 * h + u] = g2; zr[3 * h + u] = g3; } }
        }
      }
      if (own) {
        float* gr = p.dG + ((size_t)(dir * p.S + p.tau) * p.B + b) * GT;
        if (MODE == RNN_GRU_CAND) gr[2 * h + u] = g0;
        else { gr[u] = g0; if (NG >= 2) gr[h + u] = g1; if (NG == 4) { gr[2 * h + u] = g2; gr[3 * h + u] = g3; } }
        if (MODE == RNN_LSTM) p.dc_out[i] = dc;
      }
    }
    float* sg = sG + row * ldg;
    sg[u] = g0;
    if (NG >= 2) sg[h + u] = g1;
    if (NG == 4) { sg[2 * h + u] = g2; sg[3 * h + u] = g3; }
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

// The launches of one time step, in the forward pass's order (the backward pass runs them last to first): the instantiation pair,
// the recurrent pack it multiplies by (the host's wh_p[mat] / whT_p[mat]) and the gate count that sizes the backward launch's LDS.
struct RnnLaunch { void (*fwd)(RnnStepP); void (*bwd)(RnnStepBwdP); int mat, gates; };
template <int MODE> constexpr RnnLaunch rnn_launch(int mat) { return {rnn_step_kernel<MODE>, rnn_step_bwd_kernel<MODE>, mat, rnn_mode_gates(MODE)}; }
struct RnnSteps { int n; RnnLaunch l[2]; };
inline RnnSteps rnn_steps(int cell) {
  switch (cell) {
    case MACX_RNN_GRU: return {2, {rnn_launch<RNN_GRU_GATES>(0), rnn_launch<RNN_GRU_CAND>(1)}};   // r * h of all units, then the candidate
    case MACX_RNN_LSTM: return {1, {rnn_launch<RNN_LSTM>(0), {}}};
    default: return {1, {rnn_launch<RNN_BASIC>(0), {}}};
  }
}

}  // namespace macx
