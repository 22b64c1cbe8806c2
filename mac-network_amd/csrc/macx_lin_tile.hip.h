// macx_lin_tile.hip.h -- one output tile of a [B,d]-sized linear (ops.linear, ops.py:298-333): the arithmetic of small_linear_kernel
// (macx_small.hip.h) as a device function, so that the forward chain kernel's filler workgroups (macx_chain_h2.hip.h) can compute
// the read unit's y = md Wy + by with exactly the launch's products, summation order and epilogue.
#pragma once
#include "macx_common.hip.h"

namespace macx {

struct LinSeg { const float* x; int ld; int K; size_t zstride; };
struct LinP {
  LinSeg seg[3];
  int Ktot, rows, n_out;
  const float* W; size_t zW;        // packed [Ktot/16][4][n_out][4]
  const float* bias; size_t zb; float bias_const;
  int act;
  float* out; int ldo; size_t zout;
  // optional epilogue pieces (applied in this order after bias/act)
  const float* actgrad_src; int actgrad_act; int ld_ag; size_t zag;  // val *= act'(src)
  int use_drop; DropSpec d1, d2; uint32_t drop_row0;                // val *= f1*f2, idx=(drop_row0+r)*drop_ld+j
  int drop_ld;                      // row stride of the dropout index: the logical width of a zero-padded cell; 0 = n_out
  float* out_drop; int ld_od;       // use_drop == 2: `out` keeps val, out_drop receives val*f1*f2 (the next consumer's dropped copy)
  const float* addend; int ld_add; size_t zadd;                      // val += addend
  // PART form (small_linear_part_launch): the input row of question b is the sum of the chain kernel's per-tile partials
  // part[tile][3][Ktot] over the 64-row tiles the question's `part_N` rows touch (macx_chain_h2.hip.h, dy_part) -- the reduction
  // that would otherwise be a launch of its own in front of this one.  Column block 0 also writes the summed rows to part_sum.
  const float* part; int part_N; float* part_sum; int part_shift;      // part_shift: log2 of the rows per tile
};
constexpr int LIN_PART_TILES = 6;     // tiles a question may touch in the PART form: N <= 320

// RTL row tiles of 16 per workgroup: 4 for tall inputs; 1 for the [B,d] chain (B <= 128 rows), where 64-row workgroups
// would leave a 32-workgroup grid on a 256-CU chip and the launch is pure latency.
// one (16 RTL rows) x (16 columns) output tile of a LinP: tile (bx, by) of matrix z.  `red`: [4][16 RTL][20] floats of LDS.
// Every thread of the workgroup must call it (barrier inside); callable more than once per kernel (a barrier guards `red`).
// tid: 0 .. 255 within the four waves that work on this tile (a 512-thread workgroup runs two tiles side by side: both halves call
// with their own tile, tid and `red`, and meet in the same barrier).  live = false: a half without a tile goes through the motions
// and stores nothing.  COH: the outputs leave as agent-scope stores (written through the XCD's L2: another workgroup of the SAME
// launch reads them with agent-scope loads, macx_chain_h2.hip.h).
// COHIN: the input rows are read with agent-scope loads too (another workgroup of the same launch wrote them); `poison` (uniform
// over the workgroup): the wait for them gave up -- a quiet NaN stands in for every input value.
// CTL: 16-column tiles side by side (1 for the launches; 2 -- `red` then holds [2 x 4] slabs -- where fewer, wider tiles save a
// round on a handful of workgroups): every output keeps its products and its summation order.
// NPT (PART): the tiles summed per question -- the most a question of the launch can touch (small_linear_part_launch), so that
// no load is requested for a tile that none of them reaches; a question that touches fewer re-reads its last tile (clamped, unused).
// The PART form takes LIN_PART_ROWS = 8 questions per workgroup: rows 8 .. 15 of its MFMA tile belong to nobody, so lanes 8 .. 15
// of a row group request the same 8 questions' partials of the NEXT k-group of the wave instead of rows of their own, and a
// rotation by 8 within the row group hands their sums to lanes 0 .. 7 for that k-group's product.  One request per pair of
// k-groups, on twice the workgroups: what the launch costs is the requests a compute unit issues (profiles/backward_tail_ab.txt).
// A row's products depend on nothing else in the tile, so every question keeps its sums, products and order.
constexpr int LIN_PART_ROWS = 8;
template <int RTL, bool PART = false, bool COH = false, bool COHIN = false, int CTL = 1, int NPT = LIN_PART_TILES>
__device__ __forceinline__ void small_linear_tile(const LinP& p, int bx, int by, int z, float (*red)[16 * RTL][20], int tid, bool live = true,
                                                  bool poison = false) {
  constexpr int L_ROWS = 16 * RTL;
  constexpr int NWV = 4;               // waves that share the tile's reduction dimension
  static_assert(CTL == 1 || (CTL == 2 && !PART), "one or two column tiles");
  static_assert(!PART || (RTL == 1 && NPT >= 1 && NPT <= LIN_PART_TILES), "PART: 8 questions per workgroup, 1 .. LIN_PART_TILES tiles each");
  constexpr int RL = PART ? LIN_PART_ROWS : L_ROWS;      // rows of the tile that are rows of the output
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c0 = bx * 16 * CTL;
  const int r0 = by * RL;
  const int li = lane & 15, lg = lane >> 4;
  const int lr = PART ? li & (RL - 1) : li, lh = PART ? li >> 3 : 0;      // PART: the lane's question, and which k-group of a pair it requests

  f32x4 acc[RTL][CTL];
#pragma unroll
  for (int t = 0; t < RTL; ++t)
#pragma unroll
    for (int c = 0; c < CTL; ++c) acc[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  int rowc[RTL];
#pragma unroll
  for (int t = 0; t < RTL; ++t) rowc[t] = min(r0 + 16 * t + lr, p.rows - 1);

  const float* Wz = p.W + (size_t)z * p.zW + ((size_t)lg * p.n_out + c0 + li) * 4;
  const int nQ = p.Ktot >> 4;
  // the epilogue's global operands (bias, addend, the activation output act' is taken from) do not depend on the product: they are
  // requested HERE, in front of the K loop, so that their L2 / HBM round trip runs under the loop's instead of behind the
  // cross-wave combine (round 6: one dependent round trip less in a launch that is a chain of three)
  const int er = tid / (4 * CTL), ecq = (tid % (4 * CTL)) * 4;
  const int erow = min(r0 + er, p.rows - 1), ecol = c0 + ecq;
  f32x4 e_bias = {0.f, 0.f, 0.f, 0.f}, e_add = {0.f, 0.f, 0.f, 0.f}, e_ag = {0.f, 0.f, 0.f, 0.f};
  auto ld4 = [](const float* q) __attribute__((always_inline)) {       // 16-byte load where the caller's pointer allows it
    if ((reinterpret_cast<uintptr_t>(q) & 15) == 0) return *reinterpret_cast<const f32x4*>(q);
    return f32x4{q[0], q[1], q[2], q[3]};
  };
  if (er < RL) {
    if (p.bias) e_bias = ld4(p.bias + (size_t)z * p.zb + ecol);
    if (p.addend) e_add = ld4(p.addend + (size_t)z * p.zadd + (size_t)erow * p.ld_add + ecol);
    if (p.actgrad_src) e_ag = ld4(p.actgrad_src + (size_t)z * p.zag + (size_t)erow * p.ld_ag + ecol);
  }
  // Operands are L2-resident and the chain is latency-bound: fetch the fragments of 8 k-groups
  // (40 x 16 B per lane in flight) before touching the matrix pipe.
  constexpr int PF = 8;
  // PART: the partial rows of this lane's question (fixed order: ascending tiles, as dc_reduce_kernel sums them)
  const float* pbase[NPT];
  bool pvalid[NPT];
  if (PART) {
    const uint32_t first = (uint32_t)rowc[0] * (uint32_t)p.part_N;
    const int t0 = (int)(first >> p.part_shift), t1 = (int)((first + p.part_N - 1) >> p.part_shift);
    // the question's slot in a tile is its distance from the tile's first question: every tile behind t0 starts inside the
    // question (slot 0), so only t0's slot takes a division
    const int seg0 = rowc[0] - (int)(((uint32_t)t0 << p.part_shift) / (uint32_t)p.part_N);
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
      const int tt = min(t0 + j, t1);
      const int seg = tt == t0 ? seg0 : 0;
      pbase[j] = p.part + ((size_t)tt * 3 + seg) * p.Ktot + lg * 4;
      pvalid[j] = t0 + j <= t1;
    }
  }
  for (int Q0 = wave; Q0 < nQ; Q0 += NWV * PF) {
    f32x4 bf[PF][CTL], af[PF][RTL];
    if (PART) {
      f32x4 pv[PF / 2][NPT];
#pragma unroll
      for (int v = 0; v < PF / 2; ++v) {       // k-groups 2v and 2v + 1 of this pass: one request, lanes 0 .. 7 | 8 .. 15 of a row group
#pragma unroll
        for (int h = 0; h < 2; ++h)
          bf[2 * v + h][0] = *reinterpret_cast<const f32x4*>(Wz + (size_t)min(Q0 + NWV * (2 * v + h), nQ - 1) * 4 * p.n_out * 4);
        const int Q = min(Q0 + NWV * (2 * v + lh), nQ - 1);
#pragma unroll
        for (int j = 0; j < NPT; ++j) pv[v][j] = *reinterpret_cast<const f32x4*>(pbase[j] + Q * 16);
      }
#pragma unroll
      for (int v = 0; v < PF / 2; ++v) {
        f32x4 sum = pv[v][0];
#pragma unroll
        for (int j = 1; j < NPT; ++j) sum += pvalid[j] ? pv[v][j] : f32x4{0.f, 0.f, 0.f, 0.f};
        // (a question that touches fewer than LIN_PART_TILES tiles has always had + 0 behind its last partial: -0 stays +0)
        if (NPT < LIN_PART_TILES) sum += f32x4{0.f, 0.f, 0.f, 0.f};
        const int Q = Q0 + NWV * (2 * v + lh);
        if (live && bx == 0 && Q < nQ && r0 + lr < p.rows)
          *reinterpret_cast<f32x4*>(p.part_sum + (size_t)(r0 + lr) * p.Ktot + Q * 16 + lg * 4) = sum;
        af[2 * v][0] = sum;                     // rows 0 .. 7: k-group 2v (rows 8 .. 15 hold the other one's: nobody's rows)
#pragma unroll
        for (int e = 0; e < 4; ++e) {           // row_ror:8 -- lanes 0 .. 7 of a row group receive lanes 8 .. 15: k-group 2v + 1
          const float se = sum[e];              // (by value: a bit cast of the vector element itself reads element 0)
          af[2 * v + 1][0][e] = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, se), 0x128, 0xF, 0xF, false));
        }
      }
    } else {
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int Q = min(Q0 + NWV * u, nQ - 1);
      int s = 0, koff = Q * 16;
      // (the walk over the three segments written out: as a loop over p.seg[s] it put the parameter block into scratch)
      if (koff >= p.seg[0].K) { koff -= p.seg[0].K; s = 1; if (koff >= p.seg[1].K) { koff -= p.seg[1].K; s = 2; } }
      const float* xs = p.seg[s].x + (size_t)z * p.seg[s].zstride + koff + lg * 4;
      const int ld = p.seg[s].ld;
#pragma unroll
      for (int c = 0; c < CTL; ++c) bf[u][c] = *reinterpret_cast<const f32x4*>(Wz + (size_t)Q * 4 * p.n_out * 4 + c * 64);
#pragma unroll
      for (int t = 0; t < RTL; ++t) {
        if constexpr (COHIN) {
          const uint64_t* q8 = reinterpret_cast<const uint64_t*>(xs + (size_t)rowc[t] * ld);
          const uint64_t lo = __hip_atomic_load(q8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const uint64_t hi = __hip_atomic_load(q8 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          af[u][t] = f32x4{__uint_as_float((uint32_t)lo), __uint_as_float((uint32_t)(lo >> 32)), __uint_as_float((uint32_t)hi),
                           __uint_as_float((uint32_t)(hi >> 32))};
          if (poison) { const float nan = __uint_as_float(0x7fc00000u); af[u][t] = f32x4{nan, nan, nan, nan}; }
        } else {
          af[u][t] = *reinterpret_cast<const f32x4*>(xs + (size_t)rowc[t] * ld);
        }
      }
    }
    }
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      if (Q0 + NWV * u < nQ) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int t = 0; t < RTL; ++t)
#pragma unroll
            for (int c = 0; c < CTL; ++c) acc[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][t][e], bf[u][c][e], acc[t][c], 0, 0, 0);
      }
    }
  }
  // accumulator map: col = lane & 15, row = 16 t + (lane >> 4) * 4 + e
#pragma unroll
  for (int t = 0; t < RTL; ++t)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int c = 0; c < CTL; ++c) red[c * NWV + wave][16 * t + lg * 4 + e][li] = acc[t][c][e];
  __syncthreads();
  const int r = tid / (4 * CTL), cqt = (tid % (4 * CTL)) * 4, cs = (cqt >> 4) * NWV, cq = cqt & 15;
  const int row = r0 + r;
  if (live && r < RL && row < p.rows) {
  f32x4 val, vald = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float t = ((red[cs][r][cq + e] + red[cs + 1][r][cq + e]) + red[cs + 2][r][cq + e]) + red[cs + 3][r][cq + e];      // fixed order
    val[e] = t;
  }
  const int col = c0 + cqt;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float v = val[e];
    v += e_bias[e];
    v += p.bias_const;
    v = act_apply(p.act, v);
    if (p.actgrad_src) v *= act_grad_from_out(p.actgrad_act, e_ag[e]);
    if (p.use_drop) {
      const uint32_t idx = (p.drop_row0 + row) * (uint32_t)(p.drop_ld > 0 ? p.drop_ld : p.n_out) + col + e;
      float f = 1.f;
      if (!keep_bit(idx, run_key(p.d1), p.d1.thr24)) f = 0.f; else f *= p.d1.inv_keep;
      if (!keep_bit(idx, run_key(p.d2), p.d2.thr24)) f = 0.f; else f *= p.d2.inv_keep;
      if (p.use_drop == 2) vald[e] = v * f;
      else v *= f;
    }
    v += e_add[e];
    val[e] = v;
  }
  if (COH) {
    float* o = p.out + (size_t)z * p.zout + (size_t)row * p.ldo + col;
#pragma unroll
    for (int e = 0; e < 4; ++e) __hip_atomic_store(o + e, val[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    *reinterpret_cast<f32x4*>(p.out + (size_t)z * p.zout + (size_t)row * p.ldo + col) = val;
  }
  if (p.use_drop == 2) {
    if (COH) {
      float* o = p.out_drop + (size_t)row * p.ld_od + col;
#pragma unroll
      for (int e = 0; e < 4; ++e) __hip_atomic_store(o + e, vald[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      *reinterpret_cast<f32x4*>(p.out_drop + (size_t)row * p.ld_od + col) = vald;
    }
  }
  }
}

}  // namespace macx
