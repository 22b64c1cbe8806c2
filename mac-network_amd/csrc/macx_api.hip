// macx_api.hip -- extern "C" entry points of libmacx.so (see include/macx.h) and the host-side
// sequencing of one MAC-cell run: what MACnet.MACnetwork's loop (model.py:453-458) makes TF execute,
// expressed as a fixed schedule of gfx950 kernels on one HIP stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "../../include/macx.h"
#include "macx_common.hip.h"
#include "macx_gemm.hip.h"
#include "macx_gemm6.hip.h"
#include "macx_gemm_tn.hip.h"
#include "macx_wgrad6.hip.h"
#include "macx_gemm3h.hip.h"
#include "macx_h2.hip.h"
#include "macx_gemm_h2.hip.h"
#include "macx_chain_api.hip.h"
#include "macx_wgrad_h2.hip.h"
#include "macx_small.hip.h"
#include "macx_rnn.hip.h"
#include "macx_ops.hip.h"
#include "macx_conv.hip.h"
#include "macx_kb_gather.hip.h"
#include "macx_features.hip.h"
#include "macx_questions.hip.h"
#include "macx_records.hip.h"
#include "macx_att_loss.hip.h"

using namespace macx;

#define CK(expr)                         \
  do {                                   \
    hipError_t _e = (expr);              \
    if (_e != hipSuccess) return (int)_e;\
  } while (0)
#define CKI(expr)             \
  do {                        \
    int _r = (expr);          \
    if (_r != 0) return _r;   \
  } while (0)

namespace {

inline size_t al4(size_t n) { return (n + 3) & ~(size_t)3; }

// The knowledge-base GEMM family runs on one of two kernels (macx_gemm_mode / macx_opts.gemm_family):
//   split (1): macx_gemm6.hip.h, fp32 operands as three exact bf16 pieces on the bf16 matrix pipe, fp32 accumulate;
//   native (0): macx_gemm.hip.h, v_mfma_f32_16x16x4_f32.
// They take different weight packings: plain weights -> format 1 (bf16 planes, 1.5x the floats) / 0, weights mixed
// with a per-question vector (B_YMIX_*) -> format 2 (fp32 k-major tiles) / 0.  Buffers are sized for the larger one.
//   h2 (2, the default): macx_gemm_h2.hip.h -- every [B,N,d] activation lives in HBM as two fp16 planes + per-row-block
//     exponents (macx_h2.hip.h), three fp16 MFMA terms per product; plain weights -> format 3 (H2 planes + exponent).
// the kernel family an ABI call runs on (macx_opts.gemm_family, when set) and the call's tuning table (macx_opts.tune): installed for
// the duration of the call, on this thread
struct ModeScope {
  int saved;
  TuneScope ts;
  explicit ModeScope(const macx_opts* o) : saved(gemm_call_override()), ts(o ? o->tune : nullptr) {
    if (o && o->gemm_family >= 1 && o->gemm_family <= 3) gemm_call_override() = o->gemm_family - 1;
  }
  ~ModeScope() { gemm_call_override() = saved; }
};
inline bool h2_mode() { return gemm_split_mode() == 2; }      // (the fused cell asks its CellRoute instead)
inline size_t wsize(size_t K, size_t n) { return K * n * 3 / 2; }     // covers format 1 (3/2) and format 3 (1 + the exponent)
inline hipError_t wgrad_any(const TnP& t, hipStream_t st) {
  return (gemm_split_mode() && !(kb_gemm_dbg() & 128)) ? wgrad_bf16x3_launch(t, st) : wgrad_tn_launch<A_PLAIN>(t, st);   // dbg 128: f32 TN kernel
}
// fp32-operand GEMM (stem convolutions, unit entry points, and the cell in modes 0 / 1); in h2 mode the fp32-operand
// callers that remain (the stem's implicit GEMM) run on the split-bf16 kernel, whose weight format they pack (1)
template <int AP, int BP, int EP, bool COLSUM>
inline hipError_t kb_gemm(const GemmP& g, hipStream_t st) {
  return gemm_split_mode() ? kb_gemm6_launch<AP, BP, EP, COLSUM>(g, st) : kb_gemm_launch<AP, BP, EP, COLSUM>(g, st);
}
inline int wfmt_plain_f32ops() { return gemm_split_mode() ? 1 : 0; }

inline DropSpec make_drop(float keep, uint32_t seed, uint32_t site, uint32_t step) {
  DropSpec s;
  s.word = nullptr;
  s.key = site_key(seed, site, step);
  if (keep >= 1.0f) {
    s.thr24 = 1u << 24;
    s.inv_keep = 1.0f;
  } else {
    s.thr24 = (uint32_t)floor((double)keep * 16777216.0);
    s.inv_keep = 1.0f / keep;
  }
  return s;
}
// a site of the cell: the run's mask word (macx_dropout.mask_word, device memory, may be null) rides along
inline DropSpec make_drop(float keep, const macx_dropout* dp, uint32_t site, uint32_t step) {
  DropSpec s = make_drop(keep, dp->seed, site, step);
  s.word = dp->mask_word;
  return s;
}
// a site outside the cell under a run's mask word (the _w entry points of the encoder, the stem and the output unit)
inline DropSpec make_drop(float keep, uint32_t seed, uint32_t site, uint32_t step, const uint32_t* word) {
  DropSpec s = make_drop(keep, seed, site, step);
  s.word = word;
  return s;
}
inline DropSpec no_drop() {
  DropSpec s;
  s.word = nullptr;
  s.key = 0;
  s.thr24 = 1u << 24;
  s.inv_keep = 1.0f;
  return s;
}

inline int write_in_dim(const macx_opts* o, int d) {
  int dim = d;
  if (o->write_inputs == MACX_WRITE_BOTH) dim = 2 * d;
  if (o->write_self_att) dim += d;
  return dim;
}

// ---- the route of a fused-cell call ------------------------------------------------------------
// Every choice among the cell's launch routes, taken ONCE per ABI call by plan_route() below (under the entry point's ModeScope) and
// read by the two layouts, by CellRun / CellBwd and by macx_cell_route: no other code of the cell asks the kernel family, the tuning
// table or the device.  (Launchers still pick their own kernel VARIANT from the tuning table in the kernel headers: chain_kv,
// wgrad_pipe_mode, MACX_TUNE_ROW_TILES / _NATIVE_WAVES / _SB_CONT / _DKB_UNI and the kb_gemm_dbg phase masks.)
struct CellRoute {
  // ---- decided by (opts, shapes) alone: all that make_saved and make_bwd read (the sizing calls know no dropout and no device)
  int family;                 // kernel family: 0 native f32 MFMA, 1 split-bf16, 2 H2 fp16 planes
  bool h2;                    // ... is the H2 family
  int wfmt_plain, wfmt_ymix;  // pack format of a plain weight / of one mixed with a per-question vector (B_YMIX_*) in that family
  bool chain;                 // the read unit's products in the chain kernels, one launch per direction (else one launch per product)
  int tile_rows, tile_shift;  // chain: rows of a tile (16 | 32 | 64) and their log2
  size_t ntile;               // chain: tiles of a launch
  bool chain_sums;            // the backward chain kernel leaves per-tile partials of dw_k / db2 / dc / db_k
  bool sb_deferred;           // dy comes from the chain kernel: dI1 is kept per step and S_b of all steps is ONE launch at the end
  bool dy_in_linear;          // ... and its per-tile partials are summed by the dy linear itself (small_linear PART form)
  bool dc_reduce_per_step;    // ... or by a dc_reduce launch behind every chain_bwd launch (which then reduces dc / db_k too)
  bool sb_wide;               // the deferred S_b contraction runs on sb_h2w_kernel (128 x 256 tiles, summation by parts)
  int sb_qpg;                 // questions per workgroup group of the S_b kernel in use
  size_t ngroup;              // ... and the groups of a launch
  size_t nslab_sb;            // slabs of dW1a / dW1b the closing reduction sums
  size_t ns_big;              // reduction splits the dW2 / dWx slabs are sized for
  size_t db_rows;             // rows per step of db1_part / dbx_part
  size_t dwk_rows;            // rows per step of dwk_part / db2_part
  // ---- decided with the run's dropout and the device's compute units: what macx_cell_forward's and the backward loop's chain launches
  // carry on the CUs their tile grids leave idle.  Never read by a layout.
  int nfill;                  // filler workgroups of a chain_fwd launch (0: none)
  bool fill_y;                // they compute the step's y = md Wy + by (PRE_YLIN)
  bool fill_stage0;           // ... and stage 0 of the next step (PRE_STAGE0_NEXT / _DONE)
  bool fill_write;            // ... and the previous step's write linear (PRE_WRITE_NEXT / _PREV)
  DkbFillPlan dkb;            // dKB jobs on chain_bwd's idle CUs (njobs = 0: the merged dKB launch)
};

// ---- layout of `saved` ------------------------------------------------------------------------
// The backward pass reads its weights in layouts of its own (transposes; H2 planes for the chain kernels): [wxT | w1aT | w1bT | w2T |
// wyT | wmT | wqT | wqUT | wccT | wcc2T | wscT | wgT], the first region of the backward workspace layout (make_bwd).  A run that keeps
// its activations packs them in the FORWARD pass's pack launch, into `saved` (round 5: one launch and its boundary less per step).
inline size_t bwd_packs_floats(const macx_opts* o, const macx_shapes* s) {
  const size_t d = s->d, p = s->p, win = write_in_dim(o, s->d);
  return 4 * al4(wsize(d, d)) + al4(d * d) + al4(win * d) + al4(d * d) + al4((o->control_input_unshared ? p : 1) * d * d) +
         al4(2 * d * d) + 3 * al4(d * d);
}

struct SavedLayout {
  size_t seg[MACX_SEG_COUNT];
  size_t seg_count[MACX_SEG_COUNT];
  size_t wx_p, w1a_p, w1b_p, w2_p;  // packed forward weights (read unit)
  size_t wy_p, wm_p, wq_p, wqU_p;   // packed forward weights of the [B,d] linears
  size_t wg_p, ws_p;                // packed gate / self-attention control projection
  size_t wc_p, wc2_p;               // packed contControl (+ _2) weights (recurrent control)
  size_t kb_bits, att_bits;         // [pk][B*N*d/32] keep bits of the two [B,N,d] dropout sites
  size_t bits_stride;               // words per step (0 when activations are not kept)
  size_t ctrl_t;                    // [B,d]   act(qInput(vecQ))
  size_t cI;                        // [p,B,d] controlInput per step (mac_cell.py:447)
  size_t cc;                        // [p,B,d] continuous control (alias of cI unless controlFeedPrev)
  size_t cc_h;                      // [p,B,d] hidden act(contControl) when controlContAct != NON
  size_t md;                        // [p,B,d] dropped memory fed to projY
  size_t y;                         // [p,B,d] projected memory
  size_t info_raw;                  // [p,B,d] information before write dropout
  size_t wlin;                      // [p,B,d] pre-activation output of linearLayernewMemory
  size_t mnew;                      // [p,B,d] post-activation, pre-gate new memory (gate only)
  size_t sc;                        // [p,B,d] projected control for self attention
  size_t self_smry;                 // [p,B,d]
  size_t logit_part;                // [d/128][B*N]
  size_t X, H1, I2;                 // [pk][B,N,d], pk = p (keep) or 1
  size_t KBd;                       // [pk][B,N,d] dropped knowledge base (ops.py:678)
  size_t act_stride;                // floats per kept step of X / H1 / I2 / KBd if keep else 0
  size_t act_floats;                // floats of one such tensor (B*N*d, or the H2 size in h2 mode)
  size_t wmax;                      // h2: max |W| of projX, memKbProj2, W1a, W1b (4 floats)
  size_t bwd_packs;                 // keep: the backward pass's weight packs (bwd_packs_floats), written by the forward pack launch; else 0
  size_t status;                    // STATUS_WORDS uint32 (macx_chain_api.hip.h; = seg[MACX_SEG_STATUS]): what the in-launch hand-offs report.
                                    // NOT zeroed by macx_cell_begin: macx_run_status reads it, only macx_run_status_reset clears it
  size_t sync;                      // SYNC_WORDS uint32: [i] the y counter of step i's chain launch (ChainPreP::yflag, p <= 32), [63] the fail
                                    // word, [64 + 16 i ..] step i's per-block counters (gflag); zeroed by macx_cell_begin's init_states launch
  size_t total;
};

SavedLayout make_saved(const macx_opts* o, const macx_shapes* s, int keep, const CellRoute& R) {
  SavedLayout L;
  memset(&L, 0, sizeof(L));
  const size_t B = s->B, S = s->S, N = s->N, d = s->d, p = s->p;
  size_t off = 0;
  auto take = [&](size_t n) { size_t r = off; off += al4(n); return r; };
  const size_t gate_w = o->write_gate ? (o->write_gate_shared ? 1 : d) : 0;
  const size_t counts[MACX_SEG_STATUS] = {(p + 1) * B * d, (p + 1) * B * d, p * B * d, p * B * S, p * B * N,
                                          o->write_self_att ? p * B * p : 0, p * B * gate_w};
  for (int i = 0; i < MACX_SEG_STATUS; ++i) {
    L.seg_count[i] = counts[i];
    L.seg[i] = take(counts[i]);
  }
  L.wx_p = take(wsize(d, d));
  L.w1a_p = take(wsize(d, d));
  L.w1b_p = take(wsize(d, d));
  L.w2_p = take(wsize(d, d));
  L.wy_p = take(d * d);
  L.wm_p = take((size_t)write_in_dim(o, s->d) * d);
  L.wq_p = take(d * d);
  L.wqU_p = take((o->control_input_unshared ? p : 1) * d * d);
  L.wg_p = o->write_gate ? take(d * d) : 0;
  L.ws_p = o->write_self_att ? take(d * d) : 0;
  L.wc_p = o->control_feed_prev ? take(2 * d * d) : 0;
  L.wc2_p = o->control_feed_prev ? take(d * d) : 0;
  L.ctrl_t = take(B * d);
  L.cI = take(p * B * d);
  if (o->control_feed_prev) {
    L.cc = take(p * B * d);
    L.cc_h = take(p * B * d);
  } else {
    L.cc = L.cI;
    L.cc_h = L.cI;
  }
  L.md = take(p * B * d);
  L.y = take(p * B * d);
  L.info_raw = take(p * B * d);
  L.wlin = take(p * B * d);
  L.mnew = o->write_gate ? take(p * B * d) : L.wlin;
  if (o->write_self_att) {
    L.sc = take(p * B * d);
    L.self_smry = take(p * B * d);
  }
  L.logit_part = take((d / 64) * B * N);   // one partial per 64- or 128-column tile
  const size_t pk = keep ? p : 1;
  // h2 mode: activations are H2 tensors (4 bytes per element + exponents + pad rows); the attention keep bits are kept as
  // one byte per 8-column slot in slot order [d/8][Rp]
  L.act_floats = R.h2 ? al4(h2_floats(B * N, d)) : B * N * d;
  L.act_stride = keep ? L.act_floats : 0;
  L.X = take(pk * L.act_floats);
  L.H1 = take(pk * L.act_floats);
  L.I2 = take(pk * L.act_floats);
  L.KBd = take(pk * L.act_floats);
  const size_t bits_floats = R.h2 ? al4(((B * N + H2_PAD_ROWS) * (d / 8) + 3) / 4) : B * N * d / 32;
  L.bits_stride = keep ? bits_floats : 0;
  L.kb_bits = take(pk * bits_floats);
  L.att_bits = take(pk * bits_floats);
  L.wmax = take(8 + 4 * 64);          // the four maxima (+ 4 spare), then absmax4's per-workgroup partials
  L.bwd_packs = keep ? take(bwd_packs_floats(o, s)) : 0;
  // the status words, then the counters: the last two segments, adjacent (the profiling stamps address one from the other)
  static_assert(STATUS_WORDS % 4 == 0 && SYNC_WORDS == SYNC_GFLAG0 + 32 * 16, "al4 adds nothing between status and sync");
  L.status = L.seg[MACX_SEG_STATUS] = take(STATUS_WORDS);
  L.seg_count[MACX_SEG_STATUS] = STATUS_WORDS;
  L.sync = take(SYNC_WORDS);
  L.total = off;
  return L;
}

inline int nrb_of(int N, int B, int d) {
  const int rows = kb_gemm_pick_rt(N, B, d / (16 * kb_gemm_nw())) * 16;
  return (N + rows - 1) / rows;
}

inline int wgrad_splits(int M, int Kd, int Jd) {
  // workgroups = splits x output tiles ~ one per CU; the split-bf16 kernel uses 128 x 256 tiles when Jd allows
  const int jw = (gemm_split_mode() && Jd % 256 == 0) ? 2 : 1;
  const int tiles = (Kd / T_TILE) * (Jd / (jw * T_TILE));
  int ns = 256 / tiles;
  if (ns < 1) ns = 1;
  const int max_by_rows = (M + 63) / 64;   // at least 64 rows per split
  if (ns > max_by_rows) ns = max_by_rows;
  if (ns < 1) ns = 1;
  return ns;
}
// ... of the deferred H2 contractions (macx_wgrad_h2.hip.h: up to 256 x 256 output tiles)
inline int wgrad_big_splits(bool h2, int M, int Kd, int Jd) {
  if (!h2) return wgrad_splits(M, Kd, Jd);
  int ns = 256 / wgrad_h2_tiles(Kd, Jd);
  const int max_by_rows = (M + 255) / 256;
  if (ns > max_by_rows) ns = max_by_rows;
  return ns < 1 ? 1 : ns;
}
inline int rows_per_split(int M, int ns) {
  int r = (M + ns - 1) / ns;
  return h2_mode() ? (r + 31) & ~31 : (r + 1) & ~1;       // H2: a 32-row stage never straddles two splits
}
inline int sb_qpg(bool h2, int B, int N) {   // questions per workgroup group in the S_b kernel: 16 tiles x groups ~ 256
  int qpg = (B + 15) / 16;
  if (qpg < 1) qpg = 1;
  if (h2) {                                 // the H2 kernel keeps one fp16 factor per (question, row) of a group in LDS
    const int rows_q = ((N + 31) / 32) * 32;
    const int cap = SBH_MAXROWS / rows_q;
    if (qpg > cap) qpg = cap < 1 ? 1 : cap;
    if (qpg > SBH_MAXQ) qpg = SBH_MAXQ;
  }
  return qpg;
}

// The one place the cell's route is decided.  dp: the run's dropout (null: none -- the sizing calls); keep: the run keeps its
// activations; ncu_: compute units to plan the fillers for, NCU_ASK: those of the current device (every launching call; 0 where
// there is none, hence no fillers), NCU_NONE: no device is asked (the sizing calls: no layout depends on it).  Call under the entry
// point's ModeScope: the family and the tuning table are the calling thread's.
constexpr int NCU_ASK = 0, NCU_NONE = -1;
CellRoute plan_route(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, int keep, int ncu_) {
  const int B = s->B, N = s->N, d = s->d, p = s->p;
  const int ncu = ncu_ == NCU_ASK ? device_cu_count() : ncu_;      // (cached per device)
  const size_t M = (size_t)B * N;
  CellRoute r;
  // macx_opts.gemm_family where set, else the process default (macx_gemm_mode)
  r.family = gemm_split_mode();
  r.h2 = r.family == 2;
  // plain weights: H2 planes + exponent (3) | bf16 planes (1) | f32 MFMA order (0); question-mixed ones: fp32 k-major tiles (2) | 0
  r.wfmt_plain = r.h2 ? 3 : (r.family ? 1 : 0);
  r.wfmt_ymix = r.family ? 2 : 0;
  // the chain kernels (macx_chain_h2.hip.h) exist in the H2 family for d <= 512 and N >= 16; MACX_TUNE_CHAIN = 0 falls back to the
  // per-product launches that also serve the other shapes
  r.chain = r.h2 && tune_get(MACX_TUNE_CHAIN, 1) && chain_supported(d, N);
  // the tallest tile that still leaves the chip one tile per CU (chain_tile_rows; short tiles exist for d = 512 only)
  r.tile_rows = r.chain ? chain_tile_rows(d, M) : 0;
  r.tile_shift = r.chain ? chain_tile_shift(d, M) : 0;
  r.ntile = r.chain ? chain_tiles(d, M) : 0;
  // a tile of N >= 32 touches at most three questions: chain_bwd then sums what is per question in three segments per tile
  r.chain_sums = r.chain && N >= 32;
  // dy from the chain kernel and S_b of all steps as one deferred launch; MACX_TUNE_SB_DEFER = 0: sb_h2 once per step (what N < 32 runs)
  r.sb_deferred = r.chain_sums && tune_get(MACX_TUNE_SB_DEFER, 1);
  // the PART form of small_linear sums at most LIN_PART_TILES tiles per question, for at most 128 questions
  r.dy_in_linear = r.sb_deferred && B <= 128 && ((N - 2) >> r.tile_shift) + 2 <= LIN_PART_TILES;
  // otherwise the next launch needs dy_i from a reduction of its own; the caller whose control unit is recurrent reduces per step too
  // (CellBwd::dc_in_loop, see CellBwd::dc_per_step)
  r.dc_reduce_per_step = r.sb_deferred && !r.dy_in_linear;
  // the deferred S_b contraction on 128 x 256 tiles with summation by parts (sb_h2w_kernel); MACX_TUNE_SB_WIDE = 0: the 128 x 128 kernel.
  // (Measured and removed: dW1a / dW1b as ONE dual-A contraction over X * y and X -- twice the matrix work, 392 against 345 us,
  // profiles/r05_dual_contraction_ab.txt; a side queue for the per-step dKB / dW2 contractions -- +8 % / +130 us per step,
  // profiles/r04_side_queue_ab.txt.)
  r.sb_wide = r.sb_deferred && tune_get(MACX_TUNE_SB_WIDE, 1) && sb_h2_wide_ok(B, N, d);
  // each S_b kernel's own rule: ~256 workgroups, what its LDS holds per group
  r.sb_qpg = r.sb_wide ? sb_h2_wide_qpg(B, N, d) : sb_qpg(r.h2, B, N);
  r.ngroup = (size_t)((B + r.sb_qpg - 1) / r.sb_qpg);
  // one slab per group: of the one deferred launch, or of every step's
  r.nslab_sb = (r.sb_deferred ? 1 : (size_t)p) * r.ngroup;
  // splits x output tiles ~ one workgroup per CU (wgrad_big_splits)
  r.ns_big = (size_t)wgrad_big_splits(r.h2, (int)((size_t)p * M), d, d);
  // column-sum partials of dI1 / dX: one row per tile of the chain kernel, or per GEMM workgroup row block (nrb_of)
  r.db_rows = r.chain ? r.ntile : (size_t)B * nrb_of(N, B, d);
  // dw_k / db2 partials: one row per tile when the chain kernel sums them, else per question
  r.dwk_rows = r.chain_sums ? r.ntile : (size_t)B;

  const bool rdrop = dp && dp->keep_read < 1.0f, wdrop = dp && dp->keep_write < 1.0f;
  const int pf = tune_get(MACX_TUNE_PRE_FILL, 1);
  // chain_fwd's idle CUs (pre_fill_count; d = 512 only), where the hand-off counters (p <= 32) and the linear tiles (B <= 128) reach
  r.nfill = (r.chain && p <= 32 && B <= 128) ? pre_fill_count(d, M, ncu) : 0;
  // any filler computes y
  r.fill_y = r.nfill > 0;
  // stage 0 depends on the step's site keys only; it exists as a stage of its own where the run keeps its dropped knowledge base
  r.fill_stage0 = r.nfill > 0 && keep && rdrop;
  // the write unit's linear where it is ONE launch: the plain write unit of the published flag files (MACX_TUNE_PRE_FILL = 2: not it)
  r.fill_write = r.nfill > 0 && !o->write_gate && !o->write_self_att && !o->control_feed_prev && !wdrop && pf >= 1 && pf != 2;
  // chain_bwd's idle CUs (dkb_fill_plan: d = 512, 64-row tiles, N >= 64, p >= 2)
  r.dkb = r.chain ? dkb_fill_plan(d, M, N, p, ncu) : DkbFillPlan{0, 0, 0};
  return r;
}

// ---- layout of the backward workspace ---------------------------------------------------------
struct BwdLayout {
  size_t wxT_p, w1aT_p, w1bT_p, w2T_p;
  size_t wyT, wmT, wqT, wqUT, wccT, wcc2T, wscT, wgT;
  size_t packs_end;
  size_t dI2, dI1, dX, da;
  size_t DM;        // [p+1,B,d]  dL/d memories
  size_t DC;        // [p+1,B,d]  dL/d controls
  size_t dcI;       // [p,B,d]    dL/d controlInput_i
  size_t dcc;       // [p,B,d]    dL/d continuous control (alias dcI unless controlFeedPrev)
  size_t dwlin;     // [p,B,d]    dL/d (newMemory linear output)
  size_t dwin;      // [p][B, win]   dL/d write inputs of every step
  size_t dinfo;     // [B,d]
  size_t dy_part;   // [2*d/128][B][d]
  size_t DY;        // [p,B,d]
  size_t dmd;       // [B,d]
  size_t dt, du;    // [B,d]
  size_t dt_part;   // [p,B,d] per-step products of the unshared control inputs' backward linear
  size_t slab_w2, slab_wx, slab_w1a, slab_w1b;     // [R.ns_big][d,d] twice, [R.nslab_sb][d,d] twice
  size_t dc_part, dls_part;   // chain kernel: per-row-group partials of dc / db_k, [p][R.dwk_rows][3][d] and [p][R.dwk_rows][3]
  size_t dyc_part;            // chain kernel: per-row-group partials of dy, [R.dwk_rows][3][d]
  size_t dI1_stride;          // floats between the steps' dI1 (0: one buffer)
  size_t db2_part, db1_part, dbx_part, dwk_part, dbk_part, dwc_part, dbc_part, ctrl_dl;
  size_t tmpBd[4];  // [B,d] scratch
  size_t dccx;      // [p+1,B,d] gradient reaching cc_i from the NEXT step's contControl input (feedPrevAtt off)
  size_t dlin1;     // [p,B,d] gradient wrt the first contControl layer's pre-activation
  size_t dxc;       // [B,2d]  gradient wrt the contControl input of the current step
  size_t dzpre;     // [p,B,d] gate pre-activation gradient
  size_t dsc;       // [p,B,d] gradient of the projected control of the self attention
  size_t dws_part, dbs_part;   // [p,B,d], [p,B]
  size_t small_slab, small_slab_stride;
  size_t tmp_dd;    // [d,d] scratch
  size_t act_floats;                 // floats of one [B,N,d] activation (H2 size in h2 mode)
  size_t ecom;                       // h2: [4][EMIN_NB][8] ints, partial minima of the row exponents of H1 / dI2 / KBd / dX over all steps
  size_t wg_ftab, wg_ftab2;          // h2: [d/128][d/128][Mpad] fp16 row factors of the two deferred weight-gradient contractions
  size_t total;
};

BwdLayout make_bwd(const macx_opts* o, const macx_shapes* s, const CellRoute& R) {
  BwdLayout L;
  memset(&L, 0, sizeof(L));
  const size_t B = s->B, N = s->N, d = s->d, p = s->p;
  const size_t win = write_in_dim(o, s->d);
  size_t off = 0;
  auto take = [&](size_t n) { size_t r = off; off += al4(n); return r; };
  L.wxT_p = take(wsize(d, d)); L.w1aT_p = take(wsize(d, d)); L.w1bT_p = take(wsize(d, d)); L.w2T_p = take(wsize(d, d));
  L.wyT = take(d * d);
  L.wmT = take(win * d);
  L.wqT = take(d * d);
  L.wqUT = take((o->control_input_unshared ? p : 1) * d * d);
  L.wccT = take(2 * d * d); L.wcc2T = take(d * d); L.wscT = take(d * d); L.wgT = take(d * d);
  L.packs_end = off;                  // == bwd_packs_floats(o, s).  These are offsets into SavedLayout::bwd_packs: the forward pass's pack
  off = 0;                            // launch writes the backward pass's packs into `saved`; the workspace proper starts here
  L.act_floats = R.h2 ? al4(h2_floats(B * N, d)) : B * N * d;
  L.dI1_stride = R.sb_deferred ? L.act_floats : 0;
  L.dI2 = take(p * L.act_floats); L.dI1 = take((R.sb_deferred ? p : 1) * L.act_floats); L.dX = take(p * L.act_floats); L.da = take(B * N);   // dI2, dX (dI1) kept per step
  L.DM = take((p + 1) * B * d);
  L.DC = take((p + 1) * B * d);
  L.dcI = take(p * B * d);
  L.dcc = o->control_feed_prev ? take(p * B * d) : L.dcI;
  L.dwlin = take(p * B * d);
  L.dwin = take(p * B * win);     // per step: the deferred dKB launch reads every step's dinfo (a column view of it)
  L.dinfo = take(p * B * d);
  L.dy_part = take((4 * d / 128) * B * d);      // 2 column partials per 128-column tile (4 on the H2 kernel)
  L.DY = take(p * B * d);
  L.dmd = take(B * d);
  L.dt = take(B * d); L.du = take(B * d);
  L.dt_part = o->control_input_unshared ? take(p * B * d) : 0;
  L.slab_w2 = take(R.ns_big * d * d);
  L.slab_wx = take(R.ns_big * d * d);
  L.slab_w1a = take(R.nslab_sb * d * d);
  L.slab_w1b = take(R.nslab_sb * d * d);
  L.db2_part = take(p * R.dwk_rows * d);
  L.db1_part = take(p * R.db_rows * d);       // column-sum partials of dI1 / dX
  L.dbx_part = take(p * R.db_rows * d);
  L.dwk_part = take(p * R.dwk_rows * d);
  if (R.chain_sums) { L.dc_part = take(p * R.dwk_rows * 3 * d); L.dls_part = take(p * R.dwk_rows * 3); L.dyc_part = take(R.dwk_rows * 3 * d); }
  L.dbk_part = take(p * B);
  L.dwc_part = take(B * d);
  L.dbc_part = take(p * B);
  L.ctrl_dl = take(p * B * (size_t)s->S);
  for (int i = 0; i < 4; ++i) L.tmpBd[i] = take(B * d);
  if (o->control_feed_prev) { L.dccx = take((p + 1) * B * d); L.dlin1 = take(p * B * d); L.dxc = take(B * 2 * d); }
  if (o->write_gate) L.dzpre = take(p * B * d);
  if (o->write_self_att) { L.dsc = take(p * B * d); L.dws_part = take(p * B * d); L.dbs_part = take(p * B); }
  // scratch slabs for the small weight gradients (largest: write unit, rows p*B, [win x d])
  size_t small = 0;
  {
    const int ns = wgrad_splits((int)(p * B), (int)d, (int)d);
    small = (size_t)ns * d * d;
  }
  L.small_slab_stride = al4(small);
  L.small_slab = take(8 * L.small_slab_stride);        // SmallWgradBatch: one slab set per batched contraction
  L.tmp_dd = take(d * d);
  L.ecom = take(4 * EMIN_NB * 8);
  L.wg_ftab = take(R.h2 ? (d / 128) * (d / 128) * wgrad_h2_mpad(p * B * N) / 2 + 4 : 4);
  L.wg_ftab2 = take(R.h2 ? (d / 128) * (d / 128) * wgrad_h2_mpad(p * B * N) / 2 + 4 : 4);
  L.total = off;
  return L;
}

// row stride of the dropout element index: the logical width of a zero-padded cell, else the width
inline int dlog_of(const macx_shapes* s) { return (s->d_logical > 0 && s->d_logical < s->d) ? s->d_logical : s->d; }

int check_impl(const macx_opts* o, const macx_shapes* s) {
  if (!o || !s) return MACX_EINVAL;
  if (o->abi_version != MACX_ABI_VERSION) return MACX_EINVAL;
  if (s->B < 1 || s->S < 1 || s->N < 1 || s->p < 1 || s->d < 128) return MACX_EINVAL;
  if (s->d % 128 != 0 || s->d > 1024) return MACX_EINVAL;
  if (s->d_logical != 0 && s->d_logical != s->d) {
    // a zero-padded cell: the dropout index is taken at the logical width (sites of the H2 kernel family only)
    if (s->d_logical % 8 != 0 || s->d_logical <= s->d - 128 || s->d_logical > s->d) return MACX_EINVAL;
    if (!h2_mode()) return MACX_EUNSUPPORTED;
  }
  if (s->S > C_MAXS || s->N > K_MAXN || s->p > CB_MAXZ) return MACX_EINVAL;
  if ((size_t)(s->b0 + s->B) * s->N * s->d >= (1ull << 32)) return MACX_EINVAL;  // 32-bit dropout index
  if (o->write_inputs != MACX_WRITE_BOTH) return MACX_EUNSUPPORTED;
  if (o->read_mem_act == MACX_ACT_NON) return MACX_EUNSUPPORTED;   // no memKbProj_2 layer then (ops.py:325)
  if (o->write_gate && o->write_gate_shared) return MACX_EREJECTED;   // [B,d] * [B] does not broadcast in the reference
  if (o->write_self_att && s->p + 1 > SA_MAXH) return MACX_EINVAL;
  return MACX_OK;
}

// a [K, Nout] weight in pack format 3 at `w` (macx_h2.hip.h: pack_h2_weight): the planes, and behind kn = K * Nout floats the exponent
inline ChainW h2_weight(const float* w, size_t kn) { return ChainW{reinterpret_cast<const char*>(w), reinterpret_cast<const int*>(w) + kn}; }
inline void set_h2_weight(GemmH2P& g, const float* w, size_t kn) { const ChainW c = h2_weight(w, kn); g.Wh = c.planes; g.w_exp = c.exp; }

// the parameter block of the read unit's forward chain kernel for step `i`; `ob`: the step whose X / H1 / I2 / KBd / keep-bit
// buffers receive the outputs (= i in a run; the timing hook rotates it)
LinP lin_basic(const float* x, int ldx, int K, int rows, const float* Wp, const float* bias, int n_out, int act, float* out, int ldo);

// the write unit's linear of step i without self attention and gate (mac_cell.py:305-375, writeInputs = BOTH): [m_i, info_i] Wm + bm
// -> m_{i+1}; with md_next its epilogue also leaves the next step's dropped memory (mac_cell.py:214-217, ops.py:679)
LinP make_write_lin(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P, float* saved,
                    const SavedLayout& L, int i, const float* info, float* wout, bool md_next) {
  const int B = s->B, d = s->d;
  const size_t Bd = (size_t)B * d;
  LinP l = lin_basic(saved + L.seg[MACX_SEG_MEMORIES] + (size_t)i * Bd, d, d, B, saved + L.wm_p, P->newMemory_b, d, o->write_mem_act, wout, d);
  l.seg[1] = LinSeg{info, d, d, 0};
  l.Ktot = 2 * d;
  if (md_next) {
    l.use_drop = 2; l.drop_ld = dlog_of(s);
    l.d1 = o->memory_variational_dropout ? make_drop(dp->keep_memory, dp, SITE_MEM_VAR, 0) : make_drop(dp->keep_memory, dp, SITE_MEM, i + 1);
    l.d2 = make_drop(dp->keep_read, dp, SITE_READ_MEM, i + 1);
    l.drop_row0 = (uint32_t)s->b0;
    l.out_drop = saved + L.md + (size_t)(i + 1) * Bd; l.ld_od = d;
  }
  return l;
}

// what a step's chain launch and its filler workgroups take over from the launches around it (ChainPreP); only where
// macx_cell_forward sequences the steps itself
enum {
  PRE_STAGE0_DONE = 1,    // stage 0 of this step was done by the previous step's launch (ChainFwdP::mode 2)
  PRE_STAGE0_NEXT = 2,    // this launch's fillers do stage 0 of step i + 1
  PRE_YLIN = 4,           // this launch's fillers compute the step's y (ChainPreP::ylin)
  PRE_WRITE_NEXT = 8,     // this step's write unit is left to the next launch
  PRE_WRITE_PREV = 16,    // this launch's fillers run the previous step's write unit (ChainPreP::wlin)
};
ChainFwdP make_chain_fwd(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                         const macx_inputs* in, float* saved, const SavedLayout& L, const CellRoute& route, int keep, int i, int ob,
                         int pre = 0) {
  const int B = s->B, N = s->N, d = s->d;
  const int R = B * N;
  const size_t Bd = (size_t)B * d, dd_ = (size_t)d * d;
  const bool rdrop = dp->keep_read < 1.0f;
  ChainFwdP c;
  memset(&c, 0, sizeof(c));
  c.M = R; c.N = N; c.d = d;
  // without read dropout the projected knowledge base is step-invariant: inference reads step 0's X back; a run that
  // keeps its activations recomputes it into the step's own buffers, as the reference's graph does (ops.py:688)
  c.mode = (rdrop || L.act_stride != 0 || i == 0) ? 0 : 1;
  c.dbg = (kb_gemm_dbg() >> 12) & 31;
  c.kb = in->knowledgeBase;
  c.dlog = dlog_of(s);
  c.first = (uint32_t)((size_t)s->b0 * N * c.dlog);
  c.thr1 = 1u << 24; c.inv1 = 1.0f; c.thr2 = 1u << 24; c.inv2 = 1.0f;
  if (rdrop) {
    const DropSpec dk = make_drop(dp->keep_read, dp, SITE_READ_KB, i);
    const DropSpec da = make_drop(dp->keep_read, dp, SITE_READ_ATT, i);
    c.key1 = dk.key; c.thr1 = dk.thr24; c.inv1 = dk.inv_keep;
    c.bits1 = reinterpret_cast<uint8_t*>(saved + L.kb_bits + (size_t)ob * L.bits_stride);
    c.key2 = da.key; c.thr2 = da.thr24; c.inv2 = da.inv_keep;
    c.word = dp->mask_word;
    c.bytes2 = reinterpret_cast<uint8_t*>(saved + L.att_bits + (size_t)ob * L.bits_stride);
  }
  if (rdrop || i == 0) {
    c.KBd = h2_view(rdrop ? saved + L.KBd + (size_t)ob * L.act_stride : saved + L.KBd, R, d);
  }
  c.Wx = h2_weight(saved + L.wx_p, dd_); c.W1a = h2_weight(saved + L.w1a_p, dd_); c.W1b = h2_weight(saved + L.w1b_p, dd_);
  c.W2 = h2_weight(saved + L.w2_p, dd_);
  c.bx = P->projX_b; c.b1 = P->memKbProj_b; c.b2 = P->memKbProj2_b;
  c.act1 = o->read_mem_act; c.act2 = o->read_ctrl_act;
  c.y = saved + L.y + (size_t)i * Bd;
  c.c = saved + L.seg[MACX_SEG_CONTROLS] + (size_t)(i + 1) * Bd;
  c.wk = P->kbLogits_w;
  c.X = h2_view(saved + L.X + (size_t)ob * L.act_stride, R, d);
  if (keep) {
    c.H1 = h2_view(saved + L.H1 + (size_t)ob * L.act_stride, R, d);
    c.I2 = h2_view(saved + L.I2 + (size_t)ob * L.act_stride, R, d);
  }
  c.logits = saved + L.logit_part;
  if (rdrop && c.mode == 0 && (pre & PRE_STAGE0_DONE)) c.mode = 2;
  if (pre & (PRE_STAGE0_NEXT | PRE_YLIN)) c.pre.nfill = route.nfill;
  if ((pre & PRE_YLIN) && c.pre.nfill) {
    // this step's y = md Wy + by on the filler workgroups (read_step then launches no linear for it)
    c.pre.ylin = lin_basic(saved + L.md + (size_t)i * Bd, d, d, B, saved + L.wy_p, P->projY_b, d, MACX_ACT_NON, saved + L.y + (size_t)i * Bd, d);
    c.pre.step = i;
    c.pre.yflag = reinterpret_cast<uint32_t*>(saved + L.sync) + i;
    c.pre.fail = reinterpret_cast<uint32_t*>(saved + L.sync) + SYNC_FAIL;
    c.pre.status = reinterpret_cast<uint32_t*>(saved + L.status);
    if ((pre & PRE_WRITE_PREV) && i > 0) {
      // ... after the previous step's write unit (cell_step did not launch it)
      c.pre.wlin = make_write_lin(o, s, dp, P, saved, L, i - 1, saved + L.seg[MACX_SEG_INFOS] + (size_t)(i - 1) * Bd,
                                  saved + L.seg[MACX_SEG_MEMORIES] + (size_t)i * Bd, true);
      c.pre.gflag = reinterpret_cast<uint32_t*>(saved + L.sync) + SYNC_GFLAG0 + 16 * i;
    }
  }
  if (rdrop && (pre & PRE_STAGE0_NEXT) && c.pre.nfill) {
    c.pre.key1 = make_drop(dp->keep_read, dp, SITE_READ_KB, i + 1).key;
    c.pre.key2 = make_drop(dp->keep_read, dp, SITE_READ_ATT, i + 1).key;
    c.pre.bits1 = reinterpret_cast<uint8_t*>(saved + L.kb_bits + (size_t)(ob + 1) * L.bits_stride);
    c.pre.bytes2 = reinterpret_cast<uint8_t*>(saved + L.att_bits + (size_t)(ob + 1) * L.bits_stride);
    c.pre.KBd = h2_view(saved + L.KBd + (size_t)(ob + 1) * L.act_stride, R, d);
  }
  return c;
}

inline bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

hipError_t pack(const float* src, int ld_k, int ld_j, int K, int Nout, float* dst, hipStream_t st) {
  hipLaunchKernelGGL(pack_weight_kernel, dim3(256), dim3(256), 0, st, src, ld_k, ld_j, K, Nout, dst);
  return hipGetLastError();
}
// ---- device-side fills and copies as KERNELS.  No hipMemsetAsync / hipMemcpyAsync on any capturable path of this library (the one
// copy call is macx_run_status's read-back to the host, which refuses a capturing stream): under HIP-graph
// replay (ROCm 7.2) a memset node was seen to run out of order with the kernel nodes around it -- in round 3 behind the packed
// weights' maxima, in round 4 behind dL/dc of a captured training step (the control unit's gradients differed from the eager
// step's in three of four fresh processes, every replay alike; tools/graph_train_probe_verify.py) -- while kernel nodes keep
// their order.  Sizes in bytes, multiples of 4.
__global__ void fill_u32_kernel(uint32_t* dst, size_t n, uint32_t v) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = v;
}
__global__ void copy2d_u32_kernel(uint32_t* dst, size_t dpitch, const uint32_t* __restrict__ src, size_t spitch, size_t width, size_t rows) {
  const size_t n = width * rows;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t r = i / width, c = i - r * width;
    dst[r * dpitch + c] = src[r * spitch + c];
  }
}
inline unsigned fill_grid(size_t n) { return (unsigned)std::min<size_t>(1024, std::max<size_t>(1, (n + 1023) / 1024)); }
inline hipError_t dev_zero(void* dst, size_t bytes, hipStream_t st) {
  if (!bytes) return hipSuccess;
  hipLaunchKernelGGL(fill_u32_kernel, dim3(fill_grid(bytes / 4)), dim3(256), 0, st, reinterpret_cast<uint32_t*>(dst), bytes / 4, 0u);
  return hipGetLastError();
}
inline hipError_t dev_copy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t rows, hipStream_t st) {
  if (!width || !rows) return hipSuccess;
  hipLaunchKernelGGL(copy2d_u32_kernel, dim3(fill_grid(width / 4 * rows)), dim3(256), 0, st, reinterpret_cast<uint32_t*>(dst), dpitch / 4,
                     reinterpret_cast<const uint32_t*>(src), spitch / 4, width / 4, rows);
  return hipGetLastError();
}
inline hipError_t dev_copy(void* dst, const void* src, size_t bytes, hipStream_t st) { return dev_copy2d(dst, bytes, src, bytes, bytes, 1, st); }

// the maximum |W| behind a format-3 pack's exponent: matrix k of absmax4's four (projX, memKbProj_2, W1a, W1b).  Where the chain
// kernels run every consumer of the maxima is a pack of this run's ONE pack launch, which combines absmax_kernel's per-workgroup
// partials itself (fold: no absmax_finish launch); elsewhere the y-mixing GEMM kernels read the finished values.
struct WMaxRef { const float* src; int n; float* out; };
inline WMaxRef wmax_ref(const float* saved, size_t wmax, int k, bool fold) {
  float* base = const_cast<float*>(saved) + wmax;
  return fold ? WMaxRef{base + 8 + (size_t)k * 64, 64, base + k} : WMaxRef{base + k, 0, nullptr};
}

struct Packer {
  PackList L;
  int n = 0;
  void add(const float* src, int ld_k, int ld_j, int K, int Nout, float* dst, int k_src = -1, int n_src = -1, int fmt = 0,
           const float* maxabs = nullptr, float* exp_dst = nullptr, int maxabs_n = 0, float* maxabs_out = nullptr) {
    L.d[n++] = PackDesc{src, dst, ld_k, ld_j, K, Nout, k_src < 0 ? K : k_src, n_src < 0 ? Nout : n_src, fmt, maxabs_n, maxabs, exp_dst, maxabs_out};
  }
  hipError_t run(hipStream_t st) {
    if (n == 0) return hipSuccess;
    size_t big = 0;
    for (int i = 0; i < n; ++i) big = std::max(big, (size_t)L.d[i].K * L.d[i].Nout);
    // (grid-stride kernels: 64 workgroups per matrix cover the cell's d x d weights in two passes; the stem's 9 Cin x Cout
    // kernels are 18 - 36 times larger and took 60 - 90 us on that grid)
    hipLaunchKernelGGL(pack_weights_kernel, dim3(big > ((size_t)1 << 20) ? 512 : 64, n), dim3(256), 0, st, L);
    n = 0;
    return hipGetLastError();
  }
};


// ---- H2 helpers (macx_h2.hip.h) -------------------------------------------------------------------------------
// min over n entries of [n][cb] minimum-exponent arrays -> out[cb]
// minimum row exponents of up to four families of H2 tensors -> per-workgroup partials (macx_h2.hip.h: h2_emin_list_kernel)
hipError_t emin_list(const EminList& L, int count, hipStream_t st) {
  hipLaunchKernelGGL(h2_emin_list_kernel, dim3(EMIN_NB, count), dim3(256), 0, st, L);
  return hipGetLastError();
}
hipError_t h2_from_f32(const H2FromP& f, hipStream_t st) {
  hipError_t e = lds_attr_once(reinterpret_cast<const void*>(h2_from_f32_kernel), H2C_LDS);
  if (e != hipSuccess) return e;
  const int nrb = (f.N + H2C_ROWS - 1) / H2C_ROWS;
  hipLaunchKernelGGL(h2_from_f32_kernel, dim3(f.B * nrb, f.C / 128), dim3(H2C_THREADS), H2C_LDS, st, f);
  return hipGetLastError();
}
// out[0..3] = max |.| of four tensors; part: 4 * ABSMAX_BLOCKS floats of scratch, or null (one workgroup per tensor: slower)
constexpr int ABSMAX_BLOCKS = 64;
hipError_t absmax4(const float* a, size_t na, const float* b, size_t nb, const float* c, size_t nc, const float* d_, size_t nd,
                   float* out, float* part, hipStream_t st, bool finish = true) {
  AbsMaxList L;
  memset(&L, 0, sizeof(L));
  L.src[0] = a; L.n[0] = na; L.src[1] = b; L.n[1] = nb; L.src[2] = c; L.n[2] = nc; L.src[3] = d_; L.n[3] = nd;
  L.out = out; L.part = part;
  hipLaunchKernelGGL(absmax_kernel, dim3(part ? ABSMAX_BLOCKS : 1, 4), dim3(256), 0, st, L);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !part || !finish) return e;        // !finish: the consumer (pack_h2_weight) combines the partials itself
  hipLaunchKernelGGL(absmax_finish_kernel, dim3(1), dim3(256), 0, st, (const float*)part, ABSMAX_BLOCKS, out);
  return hipGetLastError();
}

// out[0] = max |.| of one large tensor (n % 4 == 0); part: AMAX_BIG_BLOCKS floats of scratch
constexpr int AMAX_BIG_BLOCKS = 512;
hipError_t absmax_big(const float* a, size_t n, float* out, float* part, hipStream_t st) {
  hipLaunchKernelGGL(absmax_vec_kernel, dim3(AMAX_BIG_BLOCKS), dim3(256), 0, st, a, n / 4, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(absmax_finish_kernel, dim3(1), dim3(64), 0, st, (const float*)part, AMAX_BIG_BLOCKS, out);
  return hipGetLastError();
}

hipError_t transpose(const float* src, int R, int C, float* dst, hipStream_t st) {
  hipLaunchKernelGGL(transpose_kernel, dim3((C + 31) / 32, (R + 31) / 32), dim3(256), 0, st, src, R, C, dst);
  return hipGetLastError();
}

LinP lin_basic(const float* x, int ldx, int K, int rows, const float* Wp, const float* bias, int n_out,
               int act, float* out, int ldo) {
  LinP p;
  memset(&p, 0, sizeof(p));
  p.seg[0] = LinSeg{x, ldx, K, 0};
  p.seg[1] = LinSeg{nullptr, 0, 1 << 30, 0};
  p.seg[2] = LinSeg{nullptr, 0, 1 << 30, 0};
  p.Ktot = K;
  p.rows = rows;
  p.n_out = n_out;
  p.W = Wp;
  p.bias = bias;
  p.act = act;
  p.out = out; p.ldo = ldo;
  p.d1 = no_drop(); p.d2 = no_drop();
  return p;
}

hipError_t mask_bits(float keep, uint32_t seed, uint32_t site, uint32_t step, uint32_t first, size_t nwords, uint32_t* out,
                     hipStream_t st) {
  const DropSpec ds = make_drop(keep, seed, site, step);
  int grid = (int)((nwords + 255) / 256);
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(mask_bits_kernel, dim3(grid), dim3(256), 0, st, ds.key, ds.thr24, first, nwords, out);
  return hipGetLastError();
}

hipError_t rowsum(const float* src, int rows, int n, size_t ld, float* dst, hipStream_t st, int nz = 1, size_t zsrc = 0, size_t zdst = 0) {
  if (!dst) return hipSuccess;
  hipLaunchKernelGGL(rowsum_kernel, dim3((n + ROWSUM_COLS - 1) / ROWSUM_COLS, nz), dim3(1024), 0, st, src, rows, n, ld, dst, zsrc, zdst);
  return hipGetLastError();
}
// row sums collected while a pass is enqueued and launched together at its end (sources must stay untouched until then)
struct RowsumBatch {
  RowsumList L;
  int n = 0, max_n = 0;
  hipError_t add(const float* src, int rows, int cols, size_t ld, float* dst, hipStream_t st, int nz = 1, size_t zsrc = 0, size_t zdst = 0) {
    if (!dst) return hipSuccess;
    for (int z = 0; z < nz; ++z) {
      if (n == ROWSUM_MAX) { hipError_t e = run(st); if (e != hipSuccess) return e; }
      L.d[n++] = RowsumDesc{src + (size_t)z * zsrc, dst + (size_t)z * zdst, rows, cols, ld};
      max_n = cols > max_n ? cols : max_n;
    }
    return hipSuccess;
  }
  hipError_t run(hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(rowsum_list_kernel, dim3((max_n + ROWSUM_COLS - 1) / ROWSUM_COLS, n), dim3(1024), 0, st, L);
    n = 0; max_n = 0;
    return hipGetLastError();
  }
};
hipError_t axpy(const float* x, size_t n, float* y, hipStream_t st) {
  hipLaunchKernelGGL(axpy_kernel, dim3(64), dim3(256), 0, st, x, n, y);
  return hipGetLastError();
}

int wgrad_impl(const float* A, int lda, const float* G, int ldg, int M, int Kd, int Jd, float* out, float* ws,
               hipStream_t st) {
  TnP t;
  memset(&t, 0, sizeof(t));
  t.M = M; t.Kd = Kd; t.Jd = Jd;
  t.nsplit = wgrad_splits(M, Kd, Jd);
  t.rows_per_split = rows_per_split(M, t.nsplit);
  t.A = A; t.lda = lda; t.a_mod = M; t.G = G; t.ldg = ldg;
  t.part = (t.nsplit == 1) ? out : ws;
  CK(wgrad_any(t, st));
  if (t.nsplit > 1) CK(slab_reduce_launch(ws, t.nsplit, (size_t)Kd * Jd, out, 0, st));
  return 0;
}

// The weight gradients of the [B,d]-sized linears (768 reduction rows each at p = 12: 17 us of latency per launch + a slab
// reduction) collected and run as ONE contraction launch + ONE slab reduction (wgrad6_list_kernel).  An entry that does not fit
// the batch (other tile geometry, the f32 kernel family, more than 8) runs on its own at once.
struct SmallWgradBatch {
  TnList L; SlabList S;
  int n = 0, nred = 0, jw = 0;
  size_t max_n = 0;
  float* slab; size_t slab_stride;
  SmallWgradBatch(float* slab_, size_t stride) : slab(slab_), slab_stride(stride) { memset(&L, 0, sizeof(L)); memset(&S, 0, sizeof(S)); }
  int add(const float* A, int lda, const float* G, int ldg, int M, int Kd, int Jd, float* out, hipStream_t st) {
    const bool ok = gemm_split_mode() && !(kb_gemm_dbg() & 128) && n < 8 && (jw == 0 || jw == wgrad_split_jw(Jd));
    if (!ok) return wgrad_impl(A, lda, G, ldg, M, Kd, Jd, out, slab + (size_t)7 * slab_stride, st);
    jw = wgrad_split_jw(Jd);
    TnP& t = L.d[n];
    t.M = M; t.Kd = Kd; t.Jd = Jd;
    t.nsplit = wgrad_splits(M, Kd, Jd);
    t.rows_per_split = rows_per_split(M, t.nsplit);
    t.A = A; t.lda = lda; t.a_mod = M; t.G = G; t.ldg = ldg;
    t.part = (t.nsplit == 1) ? out : slab + (size_t)n * slab_stride;
    L.nblk[n] = (Kd / T_TILE) * (Jd / (jw * T_TILE)) * t.nsplit;
    if (t.nsplit > 1) {
      S.d[nred++] = SlabDesc{t.part, t.nsplit, (size_t)Kd * Jd / 4, out, 0};
      max_n = std::max(max_n, (size_t)Kd * Jd);
    }
    ++n;
    return 0;
  }
  int run(hipStream_t st) {
    if (n == 0) return 0;
    CK(jw == 2 ? wgrad6_list_launch_t<2>(L, n, st) : wgrad6_list_launch_t<1>(L, n, st));
    if (nred) CK(slab_reduce_list_launch(S, nred, max_n, st));
    n = nred = 0;
    return 0;
  }
};

// ---- the H2 row contractions as entry points of their own (macx_h2_wgrad / macx_h2_sb): what the exports refuse and how their
// workspaces are laid out.  Every limit here is one a kernel or a launcher of macx_wgrad_h2.hip.h rests on.
constexpr int H2X_MAX_DIM = 1024;        // 8 column blocks: what h2_emin_list_kernel's partials and the factor kernel's sE[2][8] hold
constexpr size_t H2X_MAX_ROWS = (size_t)1 << 24;   // rows of one call: row, slot and table indices stay inside 32 bits
constexpr int H2X_MAX_SPLITS = 4096, H2X_MAX_STEPS = 1024;
constexpr int H2X_ES = EMIN_NB * 8;      // ints of one family's partial minima
// the H2 family and the caller's tuning table for the duration of one of these calls
struct H2Scope {
  ModeScope ms;
  explicit H2Scope(const macx_opts* o) : ms(o) { gemm_call_override() = 2; }     // (~ModeScope restores what it found)
};
inline bool h2x_dim_ok(int d) { return d >= 128 && d % 128 == 0 && d <= H2X_MAX_DIM; }
// tensors `stride` floats apart: 16-byte steps, and no tensor inside the next one
inline bool h2x_stride_ok(size_t stride, int nt, size_t rows, int cols) {
  return nt <= 1 || (stride % 4 == 0 && stride >= al4(h2_floats(rows, (size_t)cols)));
}
struct H2WgradWs { size_t ecom, ftab[2], slab[2], total; int rows_per_split; };
// call under an H2Scope (rows_per_split asks the family).  false: a shape the contraction is not written for
inline bool h2_wgrad_plan(int nt, int R, int Kd, int Jd, int nsplit, int pair, H2WgradWs* w) {
  if (nt < 1 || R < 1 || nsplit < 1 || nsplit > H2X_MAX_SPLITS || !h2x_dim_ok(Kd) || !h2x_dim_ok(Jd)) return false;
  if ((size_t)nt * R > H2X_MAX_ROWS) return false;
  const size_t M = (size_t)nt * R;
  w->rows_per_split = rows_per_split((int)M, nsplit);
  if (w->rows_per_split % 32 || (size_t)nsplit * w->rows_per_split > (size_t)INT32_MAX) return false;
  const size_t ft = al4(((size_t)(Kd >> 7) * (Jd >> 7) * wgrad_h2_mpad(M) * sizeof(uint16_t) + 3) / 4);
  const size_t sl = (size_t)nsplit * Kd * Jd;
  size_t off = 0;
  w->ecom = off; off += 4 * (size_t)H2X_ES;                       // h2_wgrad's [A families | G families][EMIN_NB][8]
  for (int i = 0; i < 2; ++i) { w->ftab[i] = off; off += (i == 0 || pair) ? ft : 0; }
  for (int i = 0; i < 2; ++i) { w->slab[i] = off; off += (i == 0 || pair) ? sl : 0; }
  w->total = off;
  return true;
}
struct H2SbWs { size_t slab_a, slab_b, total; int qpg, ngroup; };
inline bool h2_sb_plan(int B, int N, int d, int nsteps, int qpg, int wide, int with_dy, H2SbWs* w) {
  if (B < 1 || N < 1 || !h2x_dim_ok(d) || nsteps < 1 || nsteps > H2X_MAX_STEPS || qpg < 0 || (wide != 0 && wide != 1)) return false;
  if ((size_t)B * N > H2X_MAX_ROWS || (size_t)B * N * nsteps > H2X_MAX_ROWS) return false;
  if (with_dy && (wide || nsteps > 1)) return false;              // dy is per question and per step: the narrow kernel, one step
  const int rows_q = ((N + 31) / 32) * 32;
  if (wide) {
    if (!sb_h2_wide_ok(B, N, d)) return false;
    if (qpg == 0) qpg = sb_h2_wide_qpg(B, N, d);
    if (qpg > SBW_MAXQ || (size_t)qpg * rows_q > SBW_MAXROWS / 2) return false;
  } else {
    if (rows_q > SBH_MAXROWS) return false;
    if (qpg == 0) qpg = sb_qpg(true, B, N);
    if (qpg > SBH_MAXQ || (size_t)qpg * rows_q > SBH_MAXROWS) return false;
  }
  if (qpg < 1) return false;
  w->qpg = qpg;
  w->ngroup = (B + qpg - 1) / qpg;
  const size_t dd = (size_t)d * d;
  w->slab_a = 0; w->slab_b = (size_t)w->ngroup * dd; w->total = 2 * (size_t)w->ngroup * dd;
  return true;
}

// ---- launch sequences on plain operands.  The fused cell's member functions and the unit-level exports both call these: each
// parameter block is filled, and each of these kernels launched, in one place.

// the control unit's question projections (mac_cell.py:442-448): t = act(vecQ Wq + bq), then the p control inputs cI_i = t WqU_i +
// bqU_i in one launch (qInput is step-invariant; one WqU and bias per step where `unshared`).  wq_p, wqU_p: packed weights
int ctrl_inputs_fwd(const float* vecQ, const float* wq_p, const float* bq, const float* wqU_p, const float* bqU, bool unshared, int act,
                    int B, int d, int p, float* ctrl_t, float* cI, hipStream_t st) {
  LinP l = lin_basic(vecQ, d, d, B, wq_p, bq, d, act, ctrl_t, d);
  CK(small_linear_launch(l, 1, st));
  LinP u = lin_basic(ctrl_t, d, d, B, wqU_p, bqU, d, MACX_ACT_NON, cI, d);
  if (unshared) { u.zW = (size_t)d * d; u.zb = d; }
  u.zout = (size_t)B * d;
  CK(small_linear_launch(u, p, st));
  return MACX_OK;
}

// ... backward: dt = sum_i dcI_i WqU_i^T ; du = dt * act'(t) ; dvecQ = du Wq^T (+ q_add, or NULL), and the gradients of qInput /
// qInputU -- those whose field of GP is not NULL.  wqT, wqUT: packed transposes.  The row sums and qInput_W's contraction join the
// caller's batches, which the caller runs; x.dt_part is read only where `unshared`
struct CtrlInputsScratch { float* dt_part; float* dt; float* du; float* dcI_sum; float* slab; };    // [p,B,d], 3 x [B,d], wgrad_impl's
int ctrl_inputs_bwd(bool unshared, int act, int B, int d, int p, const float* vecQ, const float* ctrl_t, const float* dcI,
                    const float* wqT, const float* wqUT, const float* q_add, const CtrlInputsScratch& x, float* dvecQ,
                    const macx_param_grads* GP, RowsumBatch& rs, SmallWgradBatch& wb, hipStream_t st) {
  const size_t Bd = (size_t)B * d, dd = (size_t)d * d;
  if (unshared) {
    // dt: one batched launch of the p products (1536 workgroups at p = 12, one batch of operand loads each) and a fixed-order sum
    // over the steps.  (Rounds 2-5 ran it as ONE linear over K = p d: 128 workgroups whose waves walked 96 k-groups in twelve
    // dependent load batches -- 27.6 us of latency for 0.4 GFLOP.)
    LinP li = lin_basic(dcI, d, d, B, wqUT, nullptr, d, MACX_ACT_NON, x.dt_part, d);
    li.seg[0].zstride = Bd; li.zW = dd; li.zout = Bd;
    CK(small_linear_launch(li, p, st));
    // ... which also leaves du = dt * act'(t)
    hipLaunchKernelGGL(sum_parts_kernel, dim3(256), dim3(256), 0, st, (const float*)x.dt_part, p, Bd, x.dt, ctrl_t, act, x.du);
    CK(hipGetLastError());
    // the p weight gradients ctrl_t^T dcI_i share A: one batched launch (B rows -> a single split, no slabs)
    if (GP->qInputU_W && gemm_split_mode() && !(kb_gemm_dbg() & 128) && wgrad_splits(B, d, d) == 1) {
      TnP t;
      memset(&t, 0, sizeof(t));
      t.M = B; t.Kd = d; t.Jd = d; t.nsplit = 1; t.rows_per_split = rows_per_split(B, 1);
      t.A = ctrl_t; t.lda = d; t.a_mod = B; t.G = dcI; t.ldg = d;
      t.part = GP->qInputU_W; t.nz = p; t.zG = Bd; t.zpart = dd;
      CK(wgrad_bf16x3_launch(t, st));
    } else if (GP->qInputU_W) {
      for (int i = 0; i < p; ++i) CKI(wgrad_impl(ctrl_t, d, dcI + (size_t)i * Bd, d, B, d, d, GP->qInputU_W + (size_t)i * dd, x.slab, st));
    }
    CK(rs.add(dcI, B, d, d, GP->qInputU_b, st, p, Bd, d));
  } else {
    hipLaunchKernelGGL(sum_parts_kernel, dim3(256), dim3(256), 0, st, dcI, p, Bd, x.dcI_sum);
    CK(hipGetLastError());
    LinP ls = lin_basic(x.dcI_sum, d, d, B, wqUT, nullptr, d, MACX_ACT_NON, x.dt, d);
    CK(small_linear_launch(ls, 1, st));
    if (GP->qInputU_W) CKI(wgrad_impl(ctrl_t, d, x.dcI_sum, d, B, d, d, GP->qInputU_W, x.slab, st));
    CK(rs.add(x.dcI_sum, B, d, d, GP->qInputU_b, st));
    hipLaunchKernelGGL(mul_actgrad_kernel, dim3(64), dim3(256), 0, st, (const float*)x.dt, ctrl_t, act, Bd, x.du);
    CK(hipGetLastError());
  }
  LinP l = lin_basic(x.du, d, d, B, wqT, nullptr, d, MACX_ACT_NON, dvecQ, d);
  if (q_add) { l.addend = q_add; l.ld_add = d; }
  CK(small_linear_launch(l, 1, st));
  if (GP->qInput_W) CKI(wb.add(vecQ, d, x.du, d, B, d, d, GP->qInput_W, st));
  CK(rs.add(x.du, B, d, d, GP->qInput_b, st));
  return MACX_OK;
}

// the word attention (mac_cell.py:141-151) of nz steps in one launch: cc, att and control are [nz][B][.]
int control_attend(int B, int S, int d, int nz, const float* cc, const float* words, const int32_t* lengths, const float* w,
                   const float* bias, float* att, float* control, hipStream_t st) {
  CtrlP c;
  c.B = B; c.S = S; c.d = d;
  c.cc = cc; c.z_cc = (size_t)B * d;
  c.words = words; c.lengths = lengths;
  c.w = w; c.bias = bias;
  c.att = att; c.z_att = (size_t)B * S;
  c.control = control; c.z_ctl = (size_t)B * d;
  hipLaunchKernelGGL(control_attend_kernel, dim3(B, nz), dim3(256), 0, st, c);
  CK(hipGetLastError());
  return MACX_OK;
}

// ... backward, its two kernels: dcontrol, cc, att, g_att (dL/d(att) of a loss on the map itself, or NULL), dl (scratch) and dcc
// are [nz][B][.]; dwords and dw_part are written, or with acc_words added to (a recurrent control differentiates a step per call)
int control_attend_bwd(int B, int S, int d, int nz, const float* dcontrol, const float* cc, const float* att, const float* words,
                       const float* w, const float* g_att, float* dl, float* dcc, float* dwords, int acc_words, float* dw_part,
                       float* db_part, hipStream_t st) {
  CtrlBwdP c;
  c.B = B; c.S = S; c.d = d; c.nz = nz;
  c.dcontrol = dcontrol; c.z_dc = (size_t)B * d;
  c.cc = cc; c.z_cc = (size_t)B * d;
  c.att = att; c.z_att = (size_t)B * S;
  c.words = words; c.w = w;
  c.dl = dl;
  c.dcc = dcc; c.z_dcc = (size_t)B * d;
  c.dwords = dwords; c.acc_words = acc_words;
  c.dw_part = dw_part; c.db_part = db_part;
  c.g_att = g_att; c.z_g = (size_t)B * S;
  hipLaunchKernelGGL(control_bwd_dl_kernel, dim3(B, nz), dim3(256), 0, st, c);
  CK(hipGetLastError());
  hipLaunchKernelGGL(control_bwd_apply_kernel, dim3(B, d / 64), dim3(256), 0, st, c);
  CK(hipGetLastError());
  return MACX_OK;
}

// attention over the knowledge base + summary (mac_cell.py:266-275) from nparts partial logits; kb_len: NULL, or the live cells
int kb_attend(int B, int N, int d, int nparts, const float* logit_part, const float* bias, const float* kb, const int32_t* kb_len,
              float* att, float* info, hipStream_t st) {
  KbAttP a;
  a.B = B; a.N = N; a.d = d; a.nparts = nparts;
  a.logit_part = logit_part; a.bias = bias;
  a.kb = kb; a.kb_len = kb_len;
  a.att = att; a.info = info;
  hipLaunchKernelGGL(kb_attend_kernel, dim3(B, d / 128), dim3(KA_THREADS), 0, st, a);
  CK(hipGetLastError());
  return MACX_OK;
}

// da = dinfo . KB (+ g_att, dL/d(att) of a loss on the map itself, or NULL)
int kb_att_da(int B, int N, int d, const float* dinfo, int ld_dinfo, const float* kb, const float* g_att, float* da, hipStream_t st) {
  hipLaunchKernelGGL(kb_att_da_kernel, dim3((B * N + 3) / 4), dim3(256), 0, st, dinfo, ld_dinfo, kb, B, N, d, da, g_att);
  CK(hipGetLastError());
  return MACX_OK;
}

// S_b = X_b^T dI1_b -> dW1a / dW1b slabs (and with dy_part the dy partials: the narrow kernel, one step) over nsteps steps in one
// launch: the operands of step i lie x_stride / g_stride / y_stride floats behind step 0's (macx_wgrad_h2.hip.h)
int sb_h2(int B, int N, int d, int nsteps, int qpg, bool wide, const float* hX, size_t x_stride, const float* hdI1, size_t g_stride,
          const float* y, size_t y_stride, const float* W1a, float* slab_a, float* slab_b, float* dy_part, hipStream_t st) {
  SbH2P q;
  memset(&q, 0, sizeof(q));
  q.B = B; q.N = N; q.d = d; q.qpg = qpg;
  q.X = h2_view(hX, B * N, d); q.dI1 = h2_view(hdI1, B * N, d);
  q.y = y; q.W1a = W1a;
  q.dW1a_part = slab_a; q.dW1b_part = slab_b; q.dy_part = dy_part;
  q.nsteps = nsteps;
  q.x_step = x_stride * sizeof(float); q.g_step = g_stride * sizeof(float); q.y_step = y_stride;
  q.dbg = kb_gemm_dbg();
  CK(wide ? sb_h2w_launch(q, st) : sb_h2_launch(q, st));
  return MACX_OK;
}

// One or two contractions sum_t A_t^T G_t over nt H2 tensors of R rows each (a_shared: tensor 0 of A at every t) into slabs
// [nsplit][Kd][Jd]: the row-exponent minima, then the (pair) launch; the caller reduces the slabs.
// ecom: [the np A families | the np G families][EMIN_NB][8]
struct H2WgradOp { const float* A; size_t a_stride; bool a_shared; const float* G; size_t g_stride; float* ftab; float* slab; };
int h2_wgrad(const H2WgradOp* op, int np, int nt, int R, int Kd, int Jd, int nsplit, int rows_per_split, int* ecom, hipStream_t st) {
  {
    EminList el;
    memset(&el, 0, sizeof(el));
    for (int i = 0; i < np; ++i) {
      el.base[i] = reinterpret_cast<const char*>(op[i].A); el.stride[i] = op[i].a_stride * sizeof(float); el.nt[i] = op[i].a_shared ? 1 : nt;
      el.base[np + i] = reinterpret_cast<const char*>(op[i].G); el.stride[np + i] = op[i].g_stride * sizeof(float); el.nt[np + i] = nt;
    }
    el.R = R; el.C = Kd; el.part = ecom;
    if (Kd == Jd) {
      CK(emin_list(el, 2 * np, st));
    } else {        // a list has one column count: the G families as a list of their own
      CK(emin_list(el, np, st));
      for (int i = 0; i < np; ++i) { el.base[i] = el.base[np + i]; el.stride[i] = el.stride[np + i]; el.nt[i] = nt; }
      el.C = Jd; el.part = ecom + np * H2X_ES;
      CK(emin_list(el, np, st));
    }
  }
  TnH2P t;
  memset(&t, 0, sizeof(t));
  t.M = nt * R; t.Kd = Kd; t.Jd = Jd; t.nsplit = nsplit; t.rows_per_split = rows_per_split;
  t.R = R;
  t.A = reinterpret_cast<const char*>(op[0].A); t.a_stride = op[0].a_stride * sizeof(float); t.a_mod = op[0].a_shared ? R : 0;
  t.G = reinterpret_cast<const char*>(op[0].G); t.g_stride = op[0].g_stride * sizeof(float);
  t.ecomA = ecom; t.ecomG = ecom + np * H2X_ES; t.ecom_nb = EMIN_NB;
  t.ftab = reinterpret_cast<uint16_t*>(op[0].ftab);
  t.dbg = kb_gemm_dbg();
  t.part = op[0].slab;
  if (np == 1) {
    CK(wgrad_h2_launch(t, st));
    return MACX_OK;
  }
  TnH2P u = t;
  u.A = reinterpret_cast<const char*>(op[1].A); u.a_stride = op[1].a_stride * sizeof(float); u.a_mod = op[1].a_shared ? R : 0;
  u.G = reinterpret_cast<const char*>(op[1].G); u.g_stride = op[1].g_stride * sizeof(float);
  u.ecomA = ecom + H2X_ES; u.ecomG = ecom + 3 * H2X_ES;
  u.ftab = reinterpret_cast<uint16_t*>(op[1].ftab);     // (a table of its own: the pair form builds both before either is read)
  u.part = op[1].slab;
  CK(wgrad_h2_launch_pair(t, u, st));
  return MACX_OK;
}

}  // namespace

// =================================================================================================
extern "C" {

int macx_abi_version(void) { return MACX_ABI_VERSION; }

const char* macx_strerror(int code) {
  switch (code) {
    case MACX_OK: return "ok";
    case MACX_EINVAL: return "invalid shapes, null or misaligned pointer";
    case MACX_EUNSUPPORTED: return "option combination has no HIP path yet";
    case MACX_EREJECTED: return "option value that raises in the reference";
    case MACX_ESMALL: return "saved/ws buffer too small";
    case MACX_EWAIT: return "an in-launch hand-off wait gave up: the run's results are poisoned (NaN)";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown macx error";
  }
}

int macx_check(const macx_opts* o, const macx_shapes* s) { ModeScope ms(o); return check_impl(o, s); }

int macx_cell_route(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, int keep, int ncu, macx_route* out) {
  ModeScope ms(o);
  CKI(check_impl(o, s));
  if (!out) return MACX_EINVAL;
  const CellRoute r = plan_route(o, s, dp, keep, ncu > 0 ? ncu : NCU_ASK);      // the plan the launches follow, copied field by field
  const int kw = r.h2 ? wgrad_h2_kw(s->d) : 0;                                  // (the launcher's own rule, by width alone)
  *out = macx_route{r.family, r.chain, r.tile_rows, (int32_t)r.ntile, r.chain_sums, r.sb_deferred, r.dy_in_linear, r.dc_reduce_per_step,
                    r.sb_wide, r.sb_qpg, (int32_t)r.ngroup, (int32_t)r.nslab_sb, (int32_t)r.ns_big, kw, (int32_t)r.db_rows,
                    (int32_t)r.dwk_rows, r.wfmt_plain, r.wfmt_ymix, r.nfill, r.fill_y, r.fill_stage0, r.fill_write, r.dkb.njobs,
                    r.dkb.nfill, r.dkb.nskip};
  return MACX_OK;
}

size_t macx_saved_floats(const macx_opts* o, const macx_shapes* s, int keep) {
  ModeScope ms(o);
  if (check_impl(o, s) != MACX_OK) return 0;
  return make_saved(o, s, keep, plan_route(o, s, nullptr, keep, NCU_NONE)).total;
}

size_t macx_ws_floats(const macx_opts* o, const macx_shapes* s, int for_backward) {
  ModeScope ms(o);
  if (check_impl(o, s) != MACX_OK) return 0;
  if (!for_backward) return 4;   // forward keeps everything in `saved`
  return make_bwd(o, s, plan_route(o, s, nullptr, 1, NCU_NONE)).total;
}

int macx_saved_segment(const macx_opts* o, const macx_shapes* s, int keep, int segment, size_t* offset, size_t* count) {
  ModeScope ms(o);
  CKI(check_impl(o, s));
  if (segment < 0 || segment >= MACX_SEG_COUNT || !offset || !count) return MACX_EINVAL;
  const SavedLayout L = make_saved(o, s, keep, plan_route(o, s, nullptr, keep, NCU_NONE));
  *offset = L.seg[segment];
  *count = L.seg_count[segment];
  return MACX_OK;
}

// ---- the run's hand-off status (SavedLayout::status) ----------------------------------------------
namespace {
__global__ void run_status_reset_kernel(uint32_t* st) {
  if (threadIdx.x < STATUS_WORDS) st[threadIdx.x] = 0u;
}
// wait_counter's two exits on words of its own: w[0] a counter that holds the wanted value, w[1] one that holds less and is waited
// for with budget 0; w[2] the fail word, w[4 + 2 c], w[5 + 2 c] the status pair of call c.  out[4 c ..]: arrived, status bits, step
// word, whether EVERY thread of the workgroup learnt of a give-up (the LDS flag + barrier protocol of the chain kernel)
__global__ __launch_bounds__(256) void handoff_selftest_kernel(uint32_t* w, uint32_t* out) {
  __shared__ uint32_t sGave;
  if (threadIdx.x == 0) __hip_atomic_store(w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int c = 0; c < 2; ++c) {
    bool ok = true;
    if (threadIdx.x == 0) {
      ok = wait_counter<1>(w + c, 1u, c == 0 ? HANDOFF_BUDGET : 0u, w + 2, w + 4 + 2 * c, 6, c == 0 ? HANDOFF_Y : HANDOFF_WRITE);
      sGave = ok ? 0u : 1u;
    }
    __syncthreads();
    const int told = __syncthreads_count(sGave != 0u);
    if (threadIdx.x == 0) {
      out[4 * c + 0] = ok ? 1u : 0u;
      out[4 * c + 1] = __hip_atomic_load(w + 4 + 2 * c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      out[4 * c + 2] = __hip_atomic_load(w + 5 + 2 * c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      out[4 * c + 3] = told == (int)blockDim.x ? 1u : 0u;
    }
    __syncthreads();
  }
}
int status_layout(const macx_opts* o, const macx_shapes* s, int keep, const float* saved, size_t saved_floats, size_t* off) {
  ModeScope ms(o);
  CKI(check_impl(o, s));
  if (!saved || misaligned(saved)) return MACX_EINVAL;
  const SavedLayout L = make_saved(o, s, keep, plan_route(o, s, nullptr, keep, NCU_NONE));
  if (saved_floats < L.total) return MACX_ESMALL;
  *off = L.status;
  return MACX_OK;
}
}  // namespace

int macx_run_status(const macx_opts* o, const macx_shapes* s, int keep, const float* saved, size_t saved_floats, void* stream,
                    uint32_t* host_status, int32_t* host_first_step) {
  size_t off = 0;
  CKI(status_layout(o, s, keep, saved, saved_floats, &off));
  hipStream_t st = (hipStream_t)stream;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  CK(hipStreamIsCapturing(st, &cap));
  if (cap != hipStreamCaptureStatusNone) return (int)hipErrorStreamCaptureUnsupported;    // a synchronising call cannot be a graph node
  uint32_t w[2] = {0u, 0u};
  CK(hipMemcpyAsync(w, saved + off, sizeof(w), hipMemcpyDeviceToHost, st));     // (never captured: the library's only copy call)
  CK(hipStreamSynchronize(st));
  if (host_status) *host_status = w[0];
  if (host_first_step) *host_first_step = (int32_t)w[1] - 1;
  return w[0] ? MACX_EWAIT : MACX_OK;
}

int macx_run_status_reset(const macx_opts* o, const macx_shapes* s, int keep, float* saved, size_t saved_floats, void* stream) {
  size_t off = 0;
  CKI(status_layout(o, s, keep, saved, saved_floats, &off));
  hipLaunchKernelGGL(run_status_reset_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, reinterpret_cast<uint32_t*>(saved + off));
  CK(hipGetLastError());
  return MACX_OK;
}

int macx_handoff_selftest(void* stream, uint32_t* host_out) {
  if (!host_out) return MACX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  CK(hipStreamIsCapturing(st, &cap));
  if (cap != hipStreamCaptureStatusNone) return (int)hipErrorStreamCaptureUnsupported;
  uint32_t* dev = nullptr;          // 16 words for the waits + 8 for the report: this self-test's own, freed before it returns
  CK(hipMalloc(&dev, 24 * sizeof(uint32_t)));
  hipError_t e = dev_zero(dev, 24 * sizeof(uint32_t), st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(handoff_selftest_kernel, dim3(1), dim3(256), 0, st, dev, dev + 16);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(host_out, dev + 16, 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  const hipError_t ef = hipFree(dev);
  if (e != hipSuccess) return (int)e;
  return ef == hipSuccess ? MACX_OK : (int)ef;
}

// -------------------------------------------------------------------------------------------------
namespace {
// One call of the fused cell, forward or backward: its arguments, its route (planned once per call under the entry point's
// ModeScope, for the current device), the layout of `saved` and the derived sizes
struct CellRun {
  const macx_opts* o; const macx_shapes* s; const macx_dropout* dp; const macx_params* P; const macx_inputs* in;
  float* saved;
  CellRoute R;
  SavedLayout L;
  hipStream_t st;
  int B, N, d, p, keep;
  size_t Bd, dd;
  bool rdrop;     // read dropout
  CellRun(const macx_opts* o_, const macx_shapes* s_, const macx_dropout* dp_, const macx_params* P_, const macx_inputs* in_,
          float* saved_, int keep_, void* stream)
      : o(o_), s(s_), dp(dp_), P(P_), in(in_), saved(saved_), R(plan_route(o_, s_, dp_, keep_, NCU_ASK)),
        L(make_saved(o_, s_, keep_, R)), st((hipStream_t)stream), B(s_->B), N(s_->N), d(s_->d), p(s_->p), keep(keep_),
        Bd((size_t)s_->B * s_->d), dd((size_t)s_->d * s_->d), rdrop(dp_->keep_read < 1.0f) {}
  WMaxRef mx(int k) const { return wmax_ref(saved, L.wmax, k, R.chain); }
  float* controls() const { return saved + L.seg[MACX_SEG_CONTROLS]; }
  float* memories() const { return saved + L.seg[MACX_SEG_MEMORIES]; }
  // step i's information before the write dropout (mac_cell.py:461-463); self.infos keeps the dropped value (mac_cell.py:474)
  float* info_raw(int i) const { return saved + (dp->keep_write < 1.0f ? L.info_raw : L.seg[MACX_SEG_INFOS]) + (size_t)i * Bd; }
  GemmH2P h2_gemm_params() const;
  // weight packs: the forward pass's, or with W the backward pass's transposes
  hipError_t read_weight_maxima() const;
  void add_read_packs(Packer& pk, const BwdLayout* W = nullptr) const;
  void add_write_packs(Packer& pk, const BwdLayout* W = nullptr) const;
  int add_control_packs(Packer& pk, const BwdLayout* W = nullptr) const;
  // forward: the units of step i
  int control_step(int i) const;
  int read_products_chain(int i, int pre) const;
  int read_products_h2(int i) const;
  int read_products_f32(int i) const;
  int read_step(int i, int pre, bool md_fused) const;
  int write_step(int i, bool md_fused) const;
  int cell_step(int i, int pre) const;
};

// the parameter block of a knowledge-base GEMM on H2 operands: sizes, timing knobs, the read-dropout scale
GemmH2P CellRun::h2_gemm_params() const {
  GemmH2P g;
  memset(&g, 0, sizeof(g));
  g.B = B; g.N = N; g.K = d; g.Nout = d;
  g.dbg = kb_gemm_dbg() & (1 | 2 | 4 | 8 | 16 | 32 | 64 | 128);      // phase-timing knobs (results are wrong under a non-zero mask)
  g.e_inv_keep = rdrop ? 1.0f / dp->keep_read : 1.0f;
  return g;
}

// ---- weights -> MFMA operand layouts (memKbProj rows [0,d) multiply x*y, rows [d,2d) multiply x: ops.py:718).  One helper per
// unit appends that unit's packs to the caller's Packer: the forward pass's into `saved`, or with W the backward pass's transposes
// into saved + L.bwd_packs (BwdLayout's first region): a run that keeps its activations packs those in the same launch.
// W: [K, Nout] row-major; T: pack W^T
void add_pack(Packer& pk, bool T, const float* W, int K, int Nout, float* dst, int fmt = 0, WMaxRef m = WMaxRef{nullptr, 0, nullptr}) {
  if (T) pk.add(W, 1, Nout, Nout, K, dst, -1, -1, fmt, m.src, nullptr, m.n, m.out);
  else pk.add(W, Nout, 1, K, Nout, dst, -1, -1, fmt, m.src, nullptr, m.n, m.out);
}

// h2: per-matrix maxima -> weight exponents (plain weights) and the bound of the question-mixed tile (W1a, W1b)
hipError_t CellRun::read_weight_maxima() const {
  static_assert(ABSMAX_BLOCKS == 64, "wmax_ref's partial layout");
  return absmax4(P->projX_W, dd, P->memKbProj2_W, dd, P->memKbProj_W, dd, P->memKbProj_W + dd, dd, saved + L.wmax,
                 saved + L.wmax + 8, st, !R.chain);
}

void CellRun::add_read_packs(Packer& pk, const BwdLayout* W) const {
  const bool T = W != nullptr;
  float* wT = saved + L.bwd_packs;
  const float* W1 = P->memKbProj_W;
  float* w1a = T ? wT + W->w1aT_p : saved + L.w1a_p;
  float* w1b = T ? wT + W->w1bT_p : saved + L.w1b_p;
  add_pack(pk, T, P->projX_W, d, d, T ? wT + W->wxT_p : saved + L.wx_p, R.wfmt_plain, mx(0));
  if (R.chain) {      // the chain kernels apply y to the accumulators: W1a and W1b are plain H2 weights there
    add_pack(pk, T, W1, d, d, w1a, 3, mx(2));
    add_pack(pk, T, W1 + dd, d, d, w1b, 3, mx(3));
  } else {
    add_pack(pk, T, W1, d, d, w1a, R.wfmt_ymix);
    add_pack(pk, T, W1 + dd, d, d, w1b, R.wfmt_ymix);
  }
  add_pack(pk, T, P->memKbProj2_W, d, d, T ? wT + W->w2T_p : saved + L.w2_p, R.wfmt_plain, mx(1));
  add_pack(pk, T, P->projY_W, d, d, T ? wT + W->wyT : saved + L.wy_p);
}

void CellRun::add_write_packs(Packer& pk, const BwdLayout* W) const {
  const bool T = W != nullptr;
  float* wT = saved + L.bwd_packs;
  add_pack(pk, T, P->newMemory_W, write_in_dim(o, d), d, T ? wT + W->wmT : saved + L.wm_p);
  if (o->write_gate) add_pack(pk, T, P->gate_W, d, d, T ? wT + W->wgT : saved + L.wg_p);
  if (o->write_self_att) add_pack(pk, T, P->selfCtrl_W, d, d, T ? wT + W->wscT : saved + L.ws_p);
}

int CellRun::add_control_packs(Packer& pk, const BwdLayout* W) const {
  const bool T = W != nullptr;
  float* wT = saved + L.bwd_packs;
  add_pack(pk, T, P->qInput_W, d, d, T ? wT + W->wqT : saved + L.wq_p);
  if (o->control_feed_prev) {
    add_pack(pk, T, P->contControl_W, o->control_feed_inputs ? 2 * d : d, d, T ? wT + W->wccT : saved + L.wc_p);
    if (o->control_cont_act != MACX_ACT_NON) add_pack(pk, T, P->contControl2_W, d, d, T ? wT + W->wcc2T : saved + L.wc2_p);
  }
  float* wqU = T ? wT + W->wqUT : saved + L.wqU_p;
  for (int i = 0; i < (o->control_input_unshared ? p : 1); ++i) {
    if (pk.n == PACK_MAX) CK(pk.run(st));
    add_pack(pk, T, P->qInputU_W + i * dd, d, d, wqU + i * dd);
  }
  return MACX_OK;
}
}  // namespace

int macx_cell_begin(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                    const macx_inputs* in, float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                    int keep, void* stream) {
  ModeScope ms(o);
  CKI(check_impl(o, s));
  if (!dp || !P || !in || !saved) return MACX_EINVAL;
  if (misaligned(saved) || misaligned(in->knowledgeBase) || misaligned(in->words) || misaligned(in->vecQuestions))
    return MACX_EINVAL;
  const CellRun r(o, s, dp, P, in, saved, keep, stream);
  if (saved_floats < r.L.total) return MACX_ESMALL;
  (void)ws; (void)ws_floats;
  const SavedLayout& L = r.L;
  const int B = r.B, d = r.d, p = r.p;
  hipStream_t st = r.st;

  {
    Packer pk;
    if (r.R.h2) CK(r.read_weight_maxima());
    r.add_read_packs(pk);
    r.add_write_packs(pk);
    if (keep && L.bwd_packs) {        // a run that keeps its activations will be differentiated
      const BwdLayout W = make_bwd(o, s, r.R);
      r.add_read_packs(pk, &W);
      r.add_write_packs(pk, &W);
      CKI(r.add_control_packs(pk, &W));
    }
    CKI(r.add_control_packs(pk));
    CK(pk.run(st));
  }

  // initial state (mac_cell.py:546-553), both tensors in one launch
  float* controls = r.controls();
  float* memories = r.memories();
  // ... and step 0's dropped memory (mac_cell.py:214-217, ops.py:679) where macx_cell_step would otherwise launch drop2 for it
  // (md_fused there: the whole cell without a gate; later steps get theirs from the write unit's linear)
  {
    const bool md0 = !o->write_gate;
    const DropSpec dm = o->memory_variational_dropout ? make_drop(dp->keep_memory, dp, SITE_MEM_VAR, 0) : make_drop(dp->keep_memory, dp, SITE_MEM, 0);
    const DropSpec dry = make_drop(dp->keep_read, dp, SITE_READ_MEM, 0);
    hipLaunchKernelGGL(init_states_kernel, dim3(64), dim3(256), 0, st, o->init_ctrl, P->initCtrl, controls, o->init_mem, P->initMem, memories,
                       in->vecQuestions, B, d, md0 ? saved + L.md : nullptr, (uint32_t)s->b0, dm, dry, dlog_of(s),
                       reinterpret_cast<uint32_t*>(saved + L.sync));
    CK(hipGetLastError());
  }

  // control inputs (mac_cell.py:442-448).  qInput is step-invariant; qInput{i} is batched over steps.
  CKI(ctrl_inputs_fwd(in->vecQuestions, saved + L.wq_p, P->qInput_b, saved + L.wqU_p, P->qInputU_b, o->control_input_unshared,
                      o->control_input_act, B, d, p, saved + L.ctrl_t, saved + L.cI, st));
  // control is not recurrent (mac_cell.py:141-151): all p word attentions in one launch
  if (!o->control_feed_prev)
    CKI(control_attend(B, s->S, d, p, saved + L.cc, in->words, in->questionLengths, P->ctrlLogits_w, P->ctrlLogits_b,
                       saved + L.seg[MACX_SEG_ATT_QUESTION], controls + (size_t)B * d, st));
  return MACX_OK;
}

namespace {
// macx_cell_forward_chain_time: an event pair that receives the start / stop timestamps of every forward chain launch of the passes
// this thread runs while `on`
struct ChainProbe { hipEvent_t ev[2 * 64]; int n; bool on; };
inline ChainProbe* chain_probe() { static thread_local ChainProbe p = {}; return &p; }

// ---- forward: the units of step i
// the control unit when it is recurrent (mac_cell.py:141-151, configs/args1.txt)
int CellRun::control_step(int i) const {
  const int S = s->S;
  const float* prev = o->control_feed_prev_att ? controls() + (size_t)i * Bd
                                               : (i == 0 ? controls() : saved + L.cc + (size_t)(i - 1) * Bd);
  float* cc_i = saved + L.cc + (size_t)i * Bd;
  const bool two = o->control_cont_act != MACX_ACT_NON;       // ops.linear stacks a second layer (ops.py:325-328)
  float* lin1 = two ? saved + L.cc_h + (size_t)i * Bd : cc_i;
  LinP l = lin_basic(prev, d, d, B, saved + L.wc_p, P->contControl_b, d, o->control_cont_act, lin1, d);
  if (o->control_feed_inputs) { l.seg[1] = LinSeg{saved + L.cI + (size_t)i * Bd, d, d, 0}; l.Ktot = 2 * d; }
  CK(small_linear_launch(l, 1, st));
  if (two) {
    LinP l2 = lin_basic(lin1, d, d, B, saved + L.wc2_p, P->contControl2_b, d, MACX_ACT_NON, cc_i, d);
    CK(small_linear_launch(l2, 1, st));
  }
  return control_attend(B, S, d, 1, cc_i, in->words, in->questionLengths, P->ctrlLogits_w, P->ctrlLogits_b,
                        saved + L.seg[MACX_SEG_ATT_QUESTION] + (size_t)i * B * S, controls() + (size_t)(i + 1) * Bd, st);
}

// the read unit's three knowledge-base products, X = dropout(KB) Wx + bx, H1 = act(X (diag(y) W1a + W1b) + b1), I2 = H1 W2 + b2,
// and the attention logits: KB -> X -> H1 -> I2 -> logits in one launch (macx_chain_h2.hip.h)
int CellRun::read_products_chain(int i, int pre) const {
  const ChainFwdP c = make_chain_fwd(o, s, dp, P, in, saved, L, R, keep, i, i, pre);
  ChainProbe& cp = *chain_probe();
  if (cp.on && cp.n < 64) {      // the kernel's own start / stop timestamps into the probe's event pair
    CK(chain_fwd_launch(c, st, cp.ev[2 * cp.n], cp.ev[2 * cp.n + 1]));
    ++cp.n;
  } else {
    CK(chain_fwd_launch(c, st));
  }
  return MACX_OK;
}

// ... on H2 operands, one launch per product (macx_gemm_h2.hip.h): the knowledge base enters the format (through its dropout site)
// once per step -- once per run without read dropout -- and X, H1, I2 never exist as fp32 tensors
int CellRun::read_products_h2(int i) const {
  const int M = B * N;
  const H2View hX = h2_view(saved + L.X + (size_t)i * L.act_stride, M, d), hH1 = h2_view(saved + L.H1 + (size_t)i * L.act_stride, M, d),
               hI2 = h2_view(saved + L.I2 + (size_t)i * L.act_stride, M, d);
  const H2View hKB = h2_view(saved + L.KBd + (rdrop ? (size_t)i * L.act_stride : 0), M, d);
  uint8_t* att_bytes = rdrop ? reinterpret_cast<uint8_t*>(saved + L.att_bits + (size_t)i * L.bits_stride) : nullptr;
  if (rdrop || i == 0) {
    H2FromP f;
    memset(&f, 0, sizeof(f));
    f.src = in->knowledgeBase; f.B = B; f.N = N; f.C = d; f.out = hKB;
    f.ldrop = dlog_of(s);
    f.first = (uint32_t)((size_t)s->b0 * N * f.ldrop);
    f.thr24 = 1u << 24; f.inv_keep = 1.0f; f.thr24_2 = 1u << 24;
    if (rdrop) {
      const DropSpec dk = make_drop(dp->keep_read, dp, SITE_READ_KB, i);
      const DropSpec da = make_drop(dp->keep_read, dp, SITE_READ_ATT, i);
      f.key = dk.key; f.thr24 = dk.thr24; f.inv_keep = dk.inv_keep;
      f.bits = reinterpret_cast<uint32_t*>(saved + L.kb_bits + (size_t)i * L.bits_stride);
      f.key2 = da.key; f.thr24_2 = da.thr24; f.bytes2 = att_bytes;
      f.word = dp->mask_word;
    }
    CK(h2_from_f32(f, st));
  }
  GemmH2P g = h2_gemm_params();
  // X = dropout(KB) Wx + bx  (ops.py:678,688)
  g.A = hKB;
  set_h2_weight(g, saved + L.wx_p, dd);
  g.out = hX; g.bias = P->projX_b; g.act = MACX_ACT_NON;
  if (rdrop || L.act_stride != 0 || i == 0) CK((kb_gemm_h2_launch<B_PLAIN, E_BIAS_ACT, false>(g, st)));
  // H1 = act( X (diag(y) W1a + W1b) + b1 )   (ops.py:703,718; mac_cell.py:237)
  g.A = hX; g.Wh = nullptr; g.w_exp = nullptr;
  g.Wt = saved + L.w1a_p; g.Wt2 = saved + L.w1b_p; g.w_max = saved + L.wmax + 2; g.y = saved + L.y + (size_t)i * Bd; g.ldy = d;
  g.out = hH1; g.bias = P->memKbProj_b; g.act = o->read_mem_act;
  CK((kb_gemm_h2_launch<B_YMIX_ROW, E_BIAS_ACT, false>(g, st)));
  // I2 = H1 W2 + b2 ; logits = dropout(act(I2 * c)) . w_k   (ops.py:326; mac_cell.py:248,262,266)
  g.A = hH1; g.Wt = nullptr; g.Wt2 = nullptr; g.y = nullptr;
  set_h2_weight(g, saved + L.w2_p, dd);
  g.out = hI2; g.bias = P->memKbProj2_b; g.act = o->read_ctrl_act;
  g.cvec = controls() + (size_t)(i + 1) * Bd; g.wvec = P->kbLogits_w; g.logit_part = saved + L.logit_part;
  g.e_bytes = att_bytes;
  CK((kb_gemm_h2_launch<B_PLAIN, E_I2_LOGIT, false>(g, st)));
  return MACX_OK;
}

// ... on fp32 operands (the split and native kernel families)
int CellRun::read_products_f32(int i) const {
  uint32_t* att_bits = reinterpret_cast<uint32_t*>(saved + L.att_bits + (size_t)i * L.bits_stride);
  float* KBd = saved + L.KBd + (size_t)i * L.act_stride;
  float* X = saved + L.X + (size_t)i * L.act_stride;
  float* H1 = saved + L.H1 + (size_t)i * L.act_stride;
  if (rdrop) {
    const uint32_t first = (uint32_t)((size_t)s->b0 * N * d);
    const DropSpec dk = make_drop(dp->keep_read, dp, SITE_READ_KB, i);
    const DropSpec da = make_drop(dp->keep_read, dp, SITE_READ_ATT, i);     // same keep probability, own stream
    hipLaunchKernelGGL(kb_dropout_kernel, dim3(2048), dim3(256), 0, st, in->knowledgeBase, (size_t)B * N * d / 4, dk.key, dk.thr24,
                       dk.inv_keep, first, KBd, reinterpret_cast<uint32_t*>(saved + L.kb_bits + (size_t)i * L.bits_stride), da.key,
                       att_bits, dp->mask_word);
    CK(hipGetLastError());
  }
  GemmP g;
  memset(&g, 0, sizeof(g));
  g.B = B; g.N = N; g.K = d; g.Nout = d;
  g.e_inv_keep = rdrop ? 1.0f / dp->keep_read : 1.0f;
  // X = dropout(KB) Wx + bx  (ops.py:678,688)
  g.A = rdrop ? KBd : in->knowledgeBase; g.lda = d;
  g.Wp = saved + L.wx_p;
  g.out = X; g.ldo = d; g.bias = P->projX_b; g.act = MACX_ACT_NON;
  // Without read dropout the projected knowledge base is the same at every step (the reference recomputes it,
  // ops.py:688); when the activations are not kept (inference) all steps share one X buffer, so step 0's is reused.
  if (rdrop || L.act_stride != 0 || i == 0) CK((kb_gemm<A_PLAIN, B_PLAIN, E_BIAS_ACT, false>(g, st)));
  // H1 = act( concat([X*y, X]) W1 + b1 ) = act( X (diag(y) W1a + W1b) + b1 )   (ops.py:703,718; mac_cell.py:237)
  g.A = X;
  g.Wp = saved + L.w1a_p; g.Wp2 = saved + L.w1b_p; g.y = saved + L.y + (size_t)i * Bd; g.ldy = d;
  g.out = H1; g.bias = P->memKbProj_b; g.act = o->read_mem_act;
  CK((kb_gemm<A_PLAIN, B_YMIX_ROW, E_BIAS_ACT, false>(g, st)));
  // I2 = H1 W2 + b2 ; logits = dropout(act(I2 * c)) . w_k   (ops.py:326; mac_cell.py:248,262,266)
  g.A = H1; g.Wp = saved + L.w2_p; g.Wp2 = nullptr; g.y = nullptr;
  g.out = saved + L.I2 + (size_t)i * L.act_stride; g.bias = P->memKbProj2_b; g.act = o->read_ctrl_act;
  g.cvec = controls() + (size_t)(i + 1) * Bd; g.wvec = P->kbLogits_w;
  g.logit_part = saved + L.logit_part;
  g.e_bits = rdrop ? att_bits : nullptr;
  CK((kb_gemm<A_PLAIN, B_PLAIN, E_I2_LOGIT, false>(g, st)));
  return MACX_OK;
}

// the read unit (mac_cell.py:209-277).  md_fused: the step's dropped memory is there already (macx_cell_begin left step 0's, the
// previous step's write unit every later one's)
int CellRun::read_step(int i, int pre, bool md_fused) const {
  float* md = saved + L.md + (size_t)i * Bd;
  if (!md_fused) {
    // memory dropout (mac_cell.py:214-217) then the read-dropout of ops.mul's y input (ops.py:679)
    const DropSpec dm = o->memory_variational_dropout ? make_drop(dp->keep_memory, dp, SITE_MEM_VAR, 0)
                                                        : make_drop(dp->keep_memory, dp, SITE_MEM, i);
    const DropSpec dry = make_drop(dp->keep_read, dp, SITE_READ_MEM, i);
    hipLaunchKernelGGL(drop2_kernel, dim3(64), dim3(256), 0, st, (const float*)(memories() + (size_t)i * Bd), B, d,
                       (uint32_t)s->b0, dm, dry, md, dlog_of(s));
    CK(hipGetLastError());
  }
  if (!((pre & PRE_YLIN) && R.chain)) {
    LinP l = lin_basic(md, d, d, B, saved + L.wy_p, P->projY_b, d, MACX_ACT_NON, saved + L.y + (size_t)i * Bd, d);
    CK(small_linear_launch(l, 1, st));
  }
  CKI(R.chain ? read_products_chain(i, pre) : R.h2 ? read_products_h2(i) : read_products_f32(i));
  // attention over the knowledge base + summary (mac_cell.py:266-275)
  return kb_attend(B, N, d, R.chain ? 1 : d / (16 * kb_gemm_nw()), saved + L.logit_part, P->kbLogits_b, in->knowledgeBase,
                   in->kbLengths, saved + L.seg[MACX_SEG_ATT_KB] + (size_t)i * B * N, info_raw(i), st);
}

// the write unit (mac_cell.py:305-375), writeInputs = BOTH: act(concat([memory, info (, selfSmry)]) W + b).  md_fused: its linear
// also leaves the next step's dropped memory (mac_cell.py:214-217 and ops.py:679 ride the epilogue)
int CellRun::write_step(int i, bool md_fused) const {
  const float* c_i = controls() + (size_t)(i + 1) * Bd;
  const float* m_prev = memories() + (size_t)i * Bd;
  float* m_new = memories() + (size_t)(i + 1) * Bd;
  float* info = saved + L.seg[MACX_SEG_INFOS] + (size_t)i * Bd;
  // write dropout (mac_cell.py:461-463)
  if (dp->keep_write < 1.0f) {
    const DropSpec dw = make_drop(dp->keep_write, dp, SITE_WRITE_INFO, i);
    hipLaunchKernelGGL(drop2_kernel, dim3(64), dim3(256), 0, st, (const float*)info_raw(i), B, d, (uint32_t)s->b0, dw, no_drop(), info,
                       dlog_of(s));
    CK(hipGetLastError());
  }
  float* self_smry = nullptr;
  if (o->write_self_att) {
    // mac_cell.py:316-330.  selfControl = contControl (CONT) or the new control; histories hold the
    // initial state and steps 0..i-1 because the appends happen after write (mac_cell.py:472-474)
    const float* sctl = o->write_self_att_cont ? saved + L.cc + (size_t)i * Bd : c_i;
    float* sc = saved + L.sc + (size_t)i * Bd;
    LinP l = lin_basic(sctl, d, d, B, saved + L.ws_p, P->selfCtrl_b, d, MACX_ACT_NON, sc, d);
    CK(small_linear_launch(l, 1, st));
    self_smry = saved + L.self_smry + (size_t)i * Bd;
    SelfAttP q;
    q.B = B; q.d = d; q.nh = i + 1;
    q.sc = sc; q.C = controls(); q.M = memories(); q.w = P->selfLogits_w; q.bias = P->selfLogits_b;
    q.att = saved + L.seg[MACX_SEG_ATT_SELF] + (size_t)i * B * p; q.ld_att = p;
    q.smry = self_smry;
    hipLaunchKernelGGL(self_attend_kernel, dim3(B), dim3(256), 0, st, q);
    CK(hipGetLastError());
  }
  float* wout = o->write_gate ? saved + L.mnew + (size_t)i * Bd : m_new;
  LinP l = make_write_lin(o, s, dp, P, saved, L, i, info, wout, md_fused && i + 1 < p);
  if (self_smry) { l.seg[2] = LinSeg{self_smry, d, d, 0}; l.Ktot = 3 * d; }
  CK(small_linear_launch(l, 1, st));
  if (o->write_gate) {
    // z = sigmoid(control Wg + bg + gateBias); m = newMemory * z + memory * (1 - z)   (mac_cell.py:358-367)
    float* z = saved + L.seg[MACX_SEG_ATT_GATE] + (size_t)i * Bd;
    LinP gl = lin_basic(c_i, d, d, B, saved + L.wg_p, P->gate_b, d, MACX_ACT_SIGMOID, z, d);
    gl.bias_const = o->write_gate_bias;
    CK(small_linear_launch(gl, 1, st));
    hipLaunchKernelGGL(gate_mix_kernel, dim3(64), dim3(256), 0, st, (const float*)wout, (const float*)z, m_prev, Bd, m_new);
    CK(hipGetLastError());
  }
  return MACX_OK;
}

// step i of the cell; pre: what the chain launches' filler workgroups take over (PRE_*)
int CellRun::cell_step(int i, int pre) const {
  // without a gate the write unit's linear also writes the next step's dropped memory
  const bool md_fused = !o->write_gate;
  if (o->control_feed_prev) CKI(control_step(i));
  CKI(read_step(i, pre, md_fused));
  if (pre & PRE_WRITE_NEXT) return MACX_OK;
  return write_step(i, md_fused);
}
}  // namespace

int macx_cell_step(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                   const macx_inputs* in, float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                   int keep, int step, void* stream) {
  ModeScope ms(o);
  (void)ws; (void)ws_floats;
  CKI(check_impl(o, s));
  if (!dp || !P || !in || !saved) return MACX_EINVAL;
  if (step < 0 || step >= s->p) return MACX_EINVAL;
  const CellRun r(o, s, dp, P, in, saved, keep, stream);
  if (saved_floats < r.L.total) return MACX_ESMALL;
  return r.cell_step(step, 0);
}

int macx_cell_forward(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                      const macx_inputs* in, float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                      int keep, void* stream) {
  CKI(macx_cell_begin(o, s, dp, P, in, saved, saved_floats, ws, ws_floats, keep, stream));
  ModeScope ms(o);
  const CellRun r(o, s, dp, P, in, saved, keep, stream);
  // a training run's steps are sequenced here: stage 0 of the read unit's chain for step i + 1 (state-independent) rides the
  // launch of step i on its idle CUs (ChainPreP), and what else the route lets the fillers take over.  The step-wise entry point
  // makes no assumption about what ran before it.
  const CellRoute& R = r.R;
  for (int i = 0; i < s->p; ++i) {
    const int flags = (R.fill_stage0 && i > 0 ? PRE_STAGE0_DONE : 0) | (R.fill_stage0 && i + 1 < s->p ? PRE_STAGE0_NEXT : 0) |
                      (R.fill_y ? PRE_YLIN : 0) | (R.fill_write && i + 1 < s->p ? PRE_WRITE_NEXT : 0) |
                      (R.fill_write && i > 0 ? PRE_WRITE_PREV : 0);
    CKI(r.cell_step(i, flags));
  }
  return MACX_OK;
}

// -------------------------------------------------------------------------------------------------
// phase 0: everything; 1: all of it except the deferred read-unit weight contractions; 2: only those (after a phase-1 call
// on the same buffers).  A data-parallel host launches the all-reduce of every gradient phase 1 completes on a side stream
// while phase 2 -- the last ~10 % of the backward pass -- still runs (macx.dp.OverlappedBuckets).
namespace {
// a [B, ld] slab per step: step i's at base + i * step
struct StepSlab {
  const float* base; int ld; size_t step;
  const float* at(int i) const { return base + (size_t)i * step; }
};

// step i's H2 operands of the read unit's backward products
struct ReadH2 { H2View X, H1, I2, dI2, dI1, dX; };

// a backward call: the forward run's `saved` (only read here), the workspace, the gradients and the batches that collect the
// call's small contractions
struct CellBwd : CellRun {
  float* ws;
  BwdLayout W;
  const float* wT;              // the backward pass's weight packs, left in `saved` by the forward pass's pack launch
  float* DM;                    // [p + 1][B,d] dL/dm_i
  float* DC;                    // [p + 1][B,d] dL/dc_i
  float* dwlin_all;             // [p][B,d] dL/d(newMemory linear output); with writeMemAct = NON and no gate it IS dL/dm_{1..p}
  const macx_param_grads* GP; const macx_input_grads* GI;
  int win;
  StepSlab dinfo;               // dL/d(info_i), the read unit's output (ahead of the write dropout)
  // the recurrent control unit differentiates through dL/dc_i inside iteration i; otherwise every step's dc / db_k partials are
  // reduced in one launch after the loop
  bool dc_in_loop = false;
  // a dc_reduce launch follows every chain_bwd launch (read_bwd_chain); else ONE follows the loop (read_dc_reduce_all)
  bool dc_per_step() const { return R.chain_sums && (dc_in_loop || R.dc_reduce_per_step); }
  ChainDkbP dkb_q;
  RowsumBatch rs;               // bias-gradient row sums of this call: one launch at the end of each phase
  SmallWgradBatch wb;           // weight gradients of the [B,d] linears: one launch at the end of phase 1
  // gradients that arrive at the run's attention maps and step states themselves (macx_cell_backward_x): all null = none, and
  // then every launch below is the one a plain backward call issues
  macx_state_grads sg{};
  CellBwd(const macx_opts* o_, const macx_shapes* s_, const macx_dropout* dp_, const macx_params* P_, const macx_inputs* in_,
          const float* saved_, float* ws_, const macx_param_grads* GP_, const macx_input_grads* GI_, void* stream)
      : CellRun(o_, s_, dp_, P_, in_, const_cast<float*>(saved_), 1, stream), ws(ws_), W(make_bwd(o_, s_, R)), wT(saved_ + L.bwd_packs),
        DM(ws_ + W.DM), DC(ws_ + W.DC), dwlin_all((o_->write_mem_act == MACX_ACT_NON && !o_->write_gate) ? DM + Bd : ws_ + W.dwlin),
        GP(GP_), GI(GI_), win(write_in_dim(o_, d)), wb(ws_ + W.small_slab, W.small_slab_stride) {
    dinfo = dp->keep_write < 1.0f ? StepSlab{ws + W.dinfo, d, Bd} : StepSlab{ws + W.dwin + d, win, (size_t)B * win};
    memset(&dkb_q, 0, sizeof(dkb_q));
  }
  int check_bwd_buffers(size_t saved_floats, size_t ws_floats, int phase) const;
  int init_state_grads(const float* d_memory, const float* d_control);
  void plan_dkb_fill();
  // the units of step i
  int write_unit_bwd(int i);
  int read_bwd_chain(int i, const ReadH2& v);
  int read_bwd_h2(int i, const ReadH2& v);
  int dkb_merged_h2();
  int read_bwd_f32(int i);
  int read_unit_bwd(int i);
  int dy_linear_bwd(int i, bool with_write);
  int control_step_bwd(int i);
  // after the step loop
  int read_dc_reduce_all();
  int control_bwd_tail();
  int gate_wgrads();
  int control_inputs_bwd();
  int initial_state_bwd();
  int read_linear_wgrads();
  int write_linear_wgrads();
  int read_weight_contractions();
};

// the buffers of a backward call (checked before anything is launched)
int CellBwd::check_bwd_buffers(size_t saved_floats, size_t ws_floats, int phase) const {
  if (saved_floats < L.total || ws_floats < W.total) return MACX_ESMALL;
  // a run is differentiated only if it kept its activations, and then it packed the backward pass's weights too
  if (phase != 2 && !L.bwd_packs) return MACX_EINVAL;
  return MACX_OK;
}

// DM / DC: zeros (or the gradients a loss sends to the histories themselves, sg.d_memories / sg.d_controls), the incoming
// gradients of the final state added to the last slabs
int CellBwd::init_state_grads(const float* d_memory, const float* d_control) {
  const size_t hist = (size_t)(p + 1) * Bd;
  if (DC == DM + hist && !misaligned(d_memory) && !misaligned(d_control)) {
    // (adjacent in the workspace: one launch)
    hipLaunchKernelGGL(bwd_init_kernel, dim3(fill_grid(2 * hist)), dim3(256), 0, st, DM, Bd, p, d_memory, d_control, 0,
                       sg.d_memories, sg.d_controls);
    CK(hipGetLastError());
  } else {
    const float* fin[2] = {d_memory, d_control};
    const float* his[2] = {sg.d_memories, sg.d_controls};
    float* dst[2] = {DM, DC};
    for (int k = 0; k < 2; ++k) {
      if (his[k]) CK(dev_copy(dst[k], his[k], hist * sizeof(float), st));
      else CK(dev_zero(dst[k], hist * sizeof(float), st));
      if (fin[k] && his[k]) CK(axpy(fin[k], Bd, dst[k] + (size_t)p * Bd, st));
      else if (fin[k]) CK(dev_copy(dst[k] + (size_t)p * Bd, fin[k], Bd * sizeof(float), st));
    }
  }
  return MACX_OK;
}

// dKB of step i + 1 rides chain_bwd's launch of step i on the CUs that launch leaves idle (ChainDkbP, macx_chain_api.hip.h); what
// the fillers leave out and step 0 run in chain_dkb_rest_launch after the last step.  Off (njobs = 0): the merged dKB launch.
void CellBwd::plan_dkb_fill() {
  if (!R.dkb.njobs) return;
  ChainDkbP& q = dkb_q;
  q.njobs = R.dkb.njobs; q.nfill = R.dkb.nfill; q.nskip = R.dkb.nskip; q.p = p;
  q.dX = reinterpret_cast<const char*>(ws + W.dX); q.dx_step = W.act_floats * sizeof(float);
  q.WxT = h2_weight(wT + W.wxT_p, dd);
  q.bits = rdrop ? reinterpret_cast<const uint8_t*>(saved + L.kb_bits) : nullptr;
  q.bits_step = L.bits_stride * sizeof(uint32_t);
  q.inv_keep = rdrop ? 1.0f / dp->keep_read : 1.0f;
  q.att = saved + L.seg[MACX_SEG_ATT_KB]; q.att_step = (size_t)B * N;
  q.dinfo = dinfo.base; q.ld_dinfo = dinfo.ld; q.dinfo_step = dinfo.step;
  q.out = GI->knowledgeBase;
  q.dbg = (kb_gemm_dbg() >> 22) & 31;
#ifdef MACX_FILL_PROF
  q.prof = reinterpret_cast<uint32_t*>(saved + L.sync) + SYNC_PROF_DKB;
#endif
}

// ---- backward: the units of step i
// the write unit: dL/dm_i -> dwin = [dL/dm_{i-1} part | dL/d(info) (| dL/d(selfSmry))] and the gate's part of dL/dc_i; leaves
// dL/d(info_i) at r.dinfo.at(i)
int CellBwd::write_unit_bwd(int i) {
  const float* dm_i = DM + (size_t)(i + 1) * Bd;   // dL/d m_i, complete at this point
  float* dwlin = dwlin_all + (size_t)i * Bd;
  float* dwin = ws + W.dwin + (size_t)i * B * win;
  const float* dmnew = dm_i;              // gradient wrt the (post-activation) new memory
  const float* mnew_out = memories() + (size_t)(i + 1) * Bd;
  if (o->write_gate) {
    // m_i = mnew * z + m_{i-1} * (1 - z)
    const float* z = saved + L.seg[MACX_SEG_ATT_GATE] + (size_t)i * Bd;
    mnew_out = saved + L.mnew + (size_t)i * Bd;
    float* dzpre = ws + W.dzpre + (size_t)i * Bd;
    hipLaunchKernelGGL(gate_bwd_kernel, dim3(64), dim3(256), 0, st, dm_i, z, mnew_out, memories() + (size_t)i * Bd, Bd,
                       ws + W.tmpBd[2], ws + W.tmpBd[3], dzpre, sg.d_att_gate ? sg.d_att_gate + (size_t)i * Bd : nullptr);
    CK(hipGetLastError());
    dmnew = ws + W.tmpBd[2];
    // dL/dc_i += dzpre Wg^T
    LinP gl = lin_basic(dzpre, d, d, B, wT + W.wgT, nullptr, d, MACX_ACT_NON, DC + (size_t)(i + 1) * Bd, d);
    gl.addend = DC + (size_t)(i + 1) * Bd; gl.ld_add = d;
    CK(small_linear_launch(gl, 1, st));
  }
  // dwlin = dmnew * act'(mnew) ; [dm_prev part | dinfo (| dselfSmry)] = dwlin Wm^T
  if (o->write_mem_act != MACX_ACT_NON || o->write_gate) {
    hipLaunchKernelGGL(mul_actgrad_kernel, dim3(64), dim3(256), 0, st, dmnew, mnew_out, o->write_mem_act, Bd, dwlin);
    CK(hipGetLastError());
  }
  LinP l = lin_basic(dwlin, d, d, B, wT + W.wmT, nullptr, win, MACX_ACT_NON, dwin, win);
  CK(small_linear_launch(l, 1, st));
  // d(info) through the write dropout (mac_cell.py:463); without write dropout r.dinfo is a column view of dwin
  if (dp->keep_write < 1.0f) {
    hipLaunchKernelGGL(copy_cols_drop_kernel, dim3(64), dim3(256), 0, st, (const float*)dwin, win, d, B, d, (uint32_t)s->b0,
                       make_drop(dp->keep_write, dp, SITE_WRITE_INFO, i), ws + W.dinfo + (size_t)i * Bd, dlog_of(s));
    CK(hipGetLastError());
  }
  if (o->write_self_att) {
    SelfAttBwdP q;
    q.B = B; q.d = d; q.nh = i + 1;
    q.dsmry = dwin + 2 * d; q.ld_ds = win;
    q.sc = saved + L.sc + (size_t)i * Bd; q.C = controls(); q.M = memories(); q.w = P->selfLogits_w;
    q.att = saved + L.seg[MACX_SEG_ATT_SELF] + (size_t)i * B * p; q.ld_att = p;
    q.DMh = DM; q.DCh = DC;
    q.dsc = ws + W.dsc + (size_t)i * Bd;
    q.dw_part = ws + W.dws_part + (size_t)i * Bd;
    q.db_part = ws + W.dbs_part + (size_t)i * B;
    if (sg.d_att_self) q.g_att = sg.d_att_self + (size_t)i * B * p;
    hipLaunchKernelGGL(self_attend_bwd_kernel, dim3(B), dim3(256), 0, st, q);
    CK(hipGetLastError());
  }
  return MACX_OK;
}

// the read unit's products backward, dl -> dI2 -> dI1 -> dX, in one launch (macx_chain_h2.hip.h)
int CellBwd::read_bwd_chain(int i, const ReadH2& v) {
  ChainBwdP c;
  memset(&c, 0, sizeof(c));
  c.M = B * N; c.N = N; c.d = d;
  c.dbg = (kb_gemm_dbg() >> 17) & 31;
  c.att = saved + L.seg[MACX_SEG_ATT_KB] + (size_t)i * B * N; c.da = ws + W.da;
  c.I2 = v.I2; c.c = controls() + (size_t)(i + 1) * Bd; c.wk = P->kbLogits_w; c.act2 = o->read_ctrl_act;
  if (R.chain_sums) {
    c.dwk_part = ws + W.dwk_part + (size_t)i * R.dwk_rows * d;
    c.db2_part = ws + W.db2_part + (size_t)i * R.dwk_rows * d;
    c.dc_part = ws + W.dc_part + (size_t)i * R.dwk_rows * 3 * d; c.dls_part = ws + W.dls_part + (size_t)i * R.dwk_rows * 3;
  }
  c.bytes2 = rdrop ? reinterpret_cast<const uint8_t*>(saved + L.att_bits + (size_t)i * L.bits_stride) : nullptr;
  c.inv2 = rdrop ? 1.0f / dp->keep_read : 1.0f;
  c.dI2 = v.dI2;
  c.W2T = h2_weight(wT + W.w2T_p, dd); c.H1 = v.H1; c.act1 = o->read_mem_act;
  c.dI1 = v.dI1; c.db1_part = ws + W.db1_part + (size_t)i * R.db_rows * d;
  c.W1aT = h2_weight(wT + W.w1aT_p, dd); c.W1bT = h2_weight(wT + W.w1bT_p, dd); c.y = saved + L.y + (size_t)i * Bd;
  c.dX = v.dX; c.dbx_part = ws + W.dbx_part + (size_t)i * R.db_rows * d;
  if (R.sb_deferred) { c.X = v.X; c.dy_part = ws + W.dyc_part; }
  if (R.dkb.njobs && i + 1 < p) { c.dkb = dkb_q; c.dkb.step = i + 1; }
  CK(chain_bwd_launch(c, st));
  if (dc_per_step()) {
    // the per-tile partials of this step: dL/dc_i += read-unit part, db_k partials, dy_i (the next launch needs dy_i)
    DcReduceP q;
    memset(&q, 0, sizeof(q));
    q.B = B; q.N = N; q.d = d;
    q.dc_part = ws + W.dc_part + (size_t)i * R.dwk_rows * 3 * d; q.dls_part = ws + W.dls_part + (size_t)i * R.dwk_rows * 3;
    q.dc = DC + (size_t)(i + 1) * Bd; q.dbk_part = ws + W.dbk_part + (size_t)i * B;
    q.tile_shift = R.tile_shift;
    if (R.dc_reduce_per_step) { q.dy_part = ws + W.dyc_part; q.dy = ws + W.DY + (size_t)i * Bd; }
    hipLaunchKernelGGL(dc_reduce_kernel, dim3(B, 1), dim3(128), 0, st, q);
    CK(hipGetLastError());
  }
  return MACX_OK;
}

// ... on H2 operands, one launch per product
int CellBwd::read_bwd_h2(int i, const ReadH2& v) {
  const size_t parts = (size_t)i * R.db_rows * d;
  GemmH2P g = h2_gemm_params();
  // dI1 = (dI2 W2^T) * act'(H1) ; db1 partials
  g.A = v.dI2;
  set_h2_weight(g, wT + W.w2T_p, dd);
  g.out = v.dI1; g.aux = v.H1; g.act = o->read_mem_act;
  g.colsum_part = ws + W.db1_part + parts;
  CK((kb_gemm_h2_launch<B_PLAIN, E_MUL_DACT, true>(g, st)));
  // dX = dI1 (diag(y) W1a + W1b)^T ; dbx partials
  g.A = v.dI1; g.Wh = nullptr; g.w_exp = nullptr;
  g.Wt = wT + W.w1aT_p; g.Wt2 = wT + W.w1bT_p; g.w_max = saved + L.wmax + 2; g.y = saved + L.y + (size_t)i * Bd; g.ldy = d;
  g.out = v.dX;
  g.colsum_part = ws + W.dbx_part + parts;
  CK((kb_gemm_h2_launch<B_YMIX_COL, E_PLAIN, true>(g, st)));
  return MACX_OK;
}

// dKB = sum_i (dX_i Wx^T) * kbmask_i + att_i (x) dinfo_i: ONE launch over all steps
int CellBwd::dkb_merged_h2() {
  GemmH2P g = h2_gemm_params();
  g.A = h2_view(ws + W.dX, B * N, d);
  set_h2_weight(g, wT + W.wxT_p, dd);
  g.nsteps = p; g.a_step_bytes = W.act_floats * sizeof(float);
  g.a_row_exp = R.chain ? 1 : 0;          // chain_bwd_kernel gives a row of dX ONE exponent: the merged launch may fold once per step
  g.out_f32 = GI->knowledgeBase; g.ldo = d;
  g.dr = dinfo.base; g.ld_dr = dinfo.ld; g.dr_step = dinfo.step;
  g.att = saved + L.seg[MACX_SEG_ATT_KB]; g.att_step = (size_t)B * N;
  g.e_bits = rdrop ? reinterpret_cast<const uint32_t*>(saved + L.kb_bits) : nullptr;
  g.bits_step_words = L.bits_stride;
  CK((kb_gemm_h2_launch<B_PLAIN, E_DKB, false>(g, st)));
  return MACX_OK;
}

// ... on fp32 operands: the attention, dI1, dX, S_b and this step's dKB term, one launch each
int CellBwd::read_bwd_f32(int i) {
  const float* att_i = saved + L.seg[MACX_SEG_ATT_KB] + (size_t)i * B * N;
  const float* y = saved + L.y + (size_t)i * Bd;
  float* dI2_i = ws + W.dI2 + (size_t)i * W.act_floats;
  float* dX_i = ws + W.dX + (size_t)i * W.act_floats;
  {
    ReadAttBwdP q;
    q.B = B; q.N = N; q.d = d; q.b0 = s->b0;
    q.att = att_i; q.da = ws + W.da; q.I2 = saved + L.I2 + (size_t)i * L.act_stride; q.c = controls() + (size_t)(i + 1) * Bd;
    q.wk = P->kbLogits_w;
    q.act = o->read_ctrl_act;
    q.bits = rdrop ? reinterpret_cast<const uint32_t*>(saved + L.att_bits + (size_t)i * L.bits_stride) : nullptr;
    q.inv_keep = rdrop ? 1.0f / dp->keep_read : 1.0f;
    q.dI2 = dI2_i;
    q.dc = DC + (size_t)(i + 1) * Bd;   // dL/dc_i += read-unit part
    q.dwk_part = ws + W.dwk_part + (size_t)i * Bd;
    q.db2_part = ws + W.db2_part + (size_t)i * Bd;
    q.dbk_part = ws + W.dbk_part + (size_t)i * B;
    hipLaunchKernelGGL(read_att_bwd_kernel, dim3(B, d / 128), dim3(RAB_THREADS), 0, st, q);
    CK(hipGetLastError());
  }
  GemmP g;
  memset(&g, 0, sizeof(g));
  g.B = B; g.N = N; g.K = d; g.Nout = d;
  g.e_inv_keep = rdrop ? 1.0f / dp->keep_read : 1.0f;
  // dI1 = (dI2 W2^T) * act'(H1) ; db1 partials
  g.A = dI2_i; g.lda = d; g.Wp = wT + W.w2T_p;
  g.out = ws + W.dI1; g.ldo = d; g.aux = saved + L.H1 + (size_t)i * L.act_stride; g.act = o->read_mem_act;
  g.colsum_part = ws + W.db1_part + (size_t)i * R.db_rows * d;
  CK((kb_gemm<A_PLAIN, B_PLAIN, E_MUL_DACT, true>(g, st)));
  // dX = dI1 (diag(y) W1a + W1b)^T ; dbx partials
  g.A = ws + W.dI1; g.Wp = wT + W.w1aT_p; g.Wp2 = wT + W.w1bT_p; g.y = y; g.ldy = d;
  g.out = dX_i; g.aux = nullptr;
  g.colsum_part = ws + W.dbx_part + (size_t)i * R.db_rows * d;
  CK((kb_gemm<A_PLAIN, B_YMIX_COL, E_PLAIN, true>(g, st)));
  // S_b = X_b^T dI1_b -> dW1a / dW1b slabs and dy partials
  {
    SbP q;
    q.B = B; q.N = N; q.d = d; q.qpg = R.sb_qpg;
    q.X = saved + L.X + (size_t)i * L.act_stride; q.dI1 = ws + W.dI1; q.y = y; q.W1a = P->memKbProj_W;
    q.dW1a_part = ws + W.slab_w1a + (size_t)i * R.ngroup * dd;
    q.dW1b_part = ws + W.slab_w1b + (size_t)i * R.ngroup * dd;
    q.dy_part = ws + W.dy_part;
    CK((gemm_split_mode() && !(kb_gemm_dbg() & 256)) ? sb6_wgrad_launch(q, st) : sb_wgrad_launch(q, st));   // dbg 256: f32 kernel
  }
  // dKB (+)= (dX Wx^T) * kbmask + att * dinfo
  g.A = dX_i; g.Wp = wT + W.wxT_p; g.Wp2 = nullptr; g.y = nullptr;
  g.out = GI->knowledgeBase; g.aux = dinfo.at(i); g.ld_aux = dinfo.ld; g.att = att_i;
  g.e_bits = rdrop ? reinterpret_cast<const uint32_t*>(saved + L.kb_bits + (size_t)i * L.bits_stride) : nullptr;
  g.accumulate = (i != p - 1);
  g.colsum_part = nullptr;
  CK((kb_gemm<A_PLAIN, B_PLAIN, E_DKB, false>(g, st)));
  return MACX_OK;
}

// the read unit, from dL/d(info_i): dL/dc_i += its part, the dy partials, the products' gradients and dKB
int CellBwd::read_unit_bwd(int i) {
  const int M = B * N;
  CKI(kb_att_da(B, N, d, dinfo.at(i), dinfo.ld, in->knowledgeBase, sg.d_att_kb ? sg.d_att_kb + (size_t)i * B * N : nullptr, ws + W.da, st));
  if (!R.h2) return read_bwd_f32(i);
  const size_t a = (size_t)i * L.act_stride;
  float* dI1_i = ws + W.dI1 + (size_t)i * W.dI1_stride;
  const ReadH2 v{h2_view(saved + L.X + a, M, d), h2_view(saved + L.H1 + a, M, d), h2_view(saved + L.I2 + a, M, d),
                 h2_view(ws + W.dI2 + (size_t)i * W.act_floats, M, d), h2_view(dI1_i, M, d),
                 h2_view(ws + W.dX + (size_t)i * W.act_floats, M, d)};
  if (!R.chain_sums) {
    ReadAttBwdH2P q;
    q.dl = nullptr; q.no_out = R.chain ? 1 : 0;    // chain with tiny N: only dc / dw_k / db2 / db_k (dI2 comes from the chain kernel)
    q.B = B; q.N = N; q.d = d;
    q.att = saved + L.seg[MACX_SEG_ATT_KB] + (size_t)i * B * N; q.da = ws + W.da; q.I2 = v.I2;
    q.c = controls() + (size_t)(i + 1) * Bd; q.wk = P->kbLogits_w;
    q.act = o->read_ctrl_act;
    q.bytes = rdrop ? reinterpret_cast<const uint8_t*>(saved + L.att_bits + (size_t)i * L.bits_stride) : nullptr;
    q.inv_keep = rdrop ? 1.0f / dp->keep_read : 1.0f;
    q.dI2 = v.dI2;
    q.dc = DC + (size_t)(i + 1) * Bd;
    q.dwk_part = ws + W.dwk_part + (size_t)i * R.dwk_rows * d;
    q.db2_part = ws + W.db2_part + (size_t)i * R.dwk_rows * d;
    q.dbk_part = ws + W.dbk_part + (size_t)i * B;
    hipLaunchKernelGGL(read_att_bwd_h2_kernel, dim3(B, d / 128), dim3(RABH_THREADS), 0, st, q);
    CK(hipGetLastError());
  }
  CKI(R.chain ? read_bwd_chain(i, v) : read_bwd_h2(i, v));
  // S_b = X_b^T dI1_b -> dW1a / dW1b slabs and dy partials (deferred: one launch over all steps in phase 2, dy from the chain kernel)
  if (!R.sb_deferred)
    CKI(sb_h2(B, N, d, 1, R.sb_qpg, false, saved + L.X + a, 0, dI1_i, 0, saved + L.y + (size_t)i * Bd, 0, P->memKbProj_W,
              ws + W.slab_w1a + (size_t)i * R.ngroup * dd, ws + W.slab_w1b + (size_t)i * R.ngroup * dd, ws + W.dy_part, st));
  // dKB of every step after step 0: the merged launch, or where chain_bwd's launches carried steps p - 1 .. 1 on their idle CUs,
  // the closing launch of that route
  if (i == 0 && R.dkb.njobs) CK(chain_dkb_rest_launch(dkb_q, B * N, N, d, st));
  else if (i == 0) CKI(dkb_merged_h2());
  return MACX_OK;
}

// dy -> d(md) -> dL/d m_{i-1} = dwin[:, :d] + (dy Wy^T) * memmask * readmask  (dwin: with_write, the write unit is in the call)
int CellBwd::dy_linear_bwd(int i, bool with_write) {
  float* DYi = ws + W.DY + (size_t)i * Bd;
  float* dm_prev = DM + (size_t)i * Bd;
  if (!R.sb_deferred) {
    hipLaunchKernelGGL(sum_parts_kernel, dim3(256), dim3(256), 0, st, (const float*)(ws + W.dy_part), (R.h2 ? SBH_CW / 2 : 2) * d / 128, Bd, DYi);
    CK(hipGetLastError());
  }
  // with self attention DM[i] already holds the parts later steps sent to this memory, with a loss on the memories history the
  // part that loss sent: accumulate
  const bool acc_prev = with_write && (o->write_self_att || o->write_gate || sg.d_memories);
  LinP l = lin_basic(DYi, d, d, B, wT + W.wyT, nullptr, d, MACX_ACT_NON, acc_prev ? ws + W.tmpBd[0] : dm_prev, d);
  l.use_drop = 1; l.drop_ld = dlog_of(s);
  l.d1 = o->memory_variational_dropout ? make_drop(dp->keep_memory, dp, SITE_MEM_VAR, 0)
                                       : make_drop(dp->keep_memory, dp, SITE_MEM, i);
  l.d2 = make_drop(dp->keep_read, dp, SITE_READ_MEM, i);
  l.drop_row0 = (uint32_t)s->b0;
  if (with_write) { l.addend = ws + W.dwin + (size_t)i * B * win; l.ld_add = win; }
  if (R.dy_in_linear) {
    l.part = ws + W.dyc_part; l.part_N = N; l.part_sum = DYi; l.part_shift = R.tile_shift;
    CK(small_linear_part_launch(l, st));
  } else {
    CK(small_linear_launch(l, 1, st));
  }
  if (acc_prev) {
    CK(axpy(ws + W.tmpBd[0], Bd, dm_prev, st));
    if (o->write_gate) CK(axpy(ws + W.tmpBd[3], Bd, dm_prev, st));   // dm * (1 - z)
  }
  return MACX_OK;
}

// the recurrent control unit of step i (dL/dc_i is complete now)
int CellBwd::control_step_bwd(int i) {
  const int S = s->S;
  const int cin = o->control_feed_inputs ? 2 * d : d;
  if (o->write_self_att && !o->write_self_att_cont) {
    LinP l = lin_basic(ws + W.dsc + (size_t)i * Bd, d, d, B, wT + W.wscT, nullptr, d, MACX_ACT_NON, DC + (size_t)(i + 1) * Bd, d);
    l.addend = DC + (size_t)(i + 1) * Bd; l.ld_add = d;
    CK(small_linear_launch(l, 1, st));
  }
  float* dcc_i = ws + W.dcc + (size_t)i * Bd;
  CKI(control_attend_bwd(B, S, d, 1, DC + (size_t)(i + 1) * Bd, saved + L.cc + (size_t)i * Bd,
                         saved + L.seg[MACX_SEG_ATT_QUESTION] + (size_t)i * B * S, in->words, P->ctrlLogits_w,
                         sg.d_att_question ? sg.d_att_question + (size_t)i * B * S : nullptr, ws + W.ctrl_dl, dcc_i, GI->words, 1,
                         ws + W.dwc_part, ws + W.dbc_part + (size_t)i * B, st));
  // parts of dL/dcc_i that did not come through the word attention
  if (!o->control_feed_prev_att) CK(axpy(ws + W.dccx + (size_t)(i + 1) * Bd, Bd, dcc_i, st));
  if (o->write_self_att && o->write_self_att_cont) {
    LinP l = lin_basic(ws + W.dsc + (size_t)i * Bd, d, d, B, wT + W.wscT, nullptr, d, MACX_ACT_NON, dcc_i, d);
    l.addend = dcc_i; l.ld_add = d;
    CK(small_linear_launch(l, 1, st));
  }
  // through contControl(_2): dlin1 = (dcc Wc2^T) * act'(h)  or  dcc
  float* dlin1 = ws + W.dlin1 + (size_t)i * Bd;
  if (o->control_cont_act != MACX_ACT_NON) {
    LinP l2 = lin_basic(dcc_i, d, d, B, wT + W.wcc2T, nullptr, d, MACX_ACT_NON, dlin1, d);
    l2.actgrad_src = saved + L.cc_h + (size_t)i * Bd; l2.actgrad_act = o->control_cont_act; l2.ld_ag = d;
    CK(small_linear_launch(l2, 1, st));
  } else {
    CK(dev_copy(dlin1, dcc_i, Bd * sizeof(float), st));
  }
  // dx = dlin1 Wc^T = [d prev | d cI_i]
  LinP lx = lin_basic(dlin1, d, d, B, wT + W.wccT, nullptr, cin, MACX_ACT_NON, ws + W.dxc, cin);
  CK(small_linear_launch(lx, 1, st));
  float* dprev_dst = o->control_feed_prev_att ? DC + (size_t)i * Bd : (i == 0 ? DC : ws + W.dccx + (size_t)i * Bd);
  hipLaunchKernelGGL(copy_cols_drop_kernel, dim3(64), dim3(256), 0, st, (const float*)(ws + W.dxc), cin, 0, B, d, 0u, no_drop(),
                     ws + W.tmpBd[0]);
  CK(hipGetLastError());
  CK(axpy(ws + W.tmpBd[0], Bd, dprev_dst, st));
  if (o->control_feed_inputs) {
    hipLaunchKernelGGL(copy_cols_drop_kernel, dim3(64), dim3(256), 0, st, (const float*)(ws + W.dxc), cin, d, B, d, 0u, no_drop(),
                       ws + W.dcI + (size_t)i * Bd);
    CK(hipGetLastError());
  } else {
    CK(dev_zero(ws + W.dcI + (size_t)i * Bd, Bd * sizeof(float), st));
  }
  return MACX_OK;
}

// ---- backward: after the step loop
// the chain launches' per-tile partials of every step that did not reduce its own: dL/dc_i += read-unit part, db_k partials
int CellBwd::read_dc_reduce_all() {
  if (!R.chain_sums || dc_per_step()) return MACX_OK;
  DcReduceP q;
  memset(&q, 0, sizeof(q));
  q.B = B; q.N = N; q.d = d;
  q.dc_part = ws + W.dc_part; q.dls_part = ws + W.dls_part; q.dc = DC + Bd; q.dbk_part = ws + W.dbk_part;
  q.part_step = R.dwk_rows * 3 * d; q.dls_step = R.dwk_rows * 3; q.dc_step = Bd; q.dbk_step = B;
  q.tile_shift = R.tile_shift;
  hipLaunchKernelGGL(dc_reduce_kernel, dim3(B, p), dim3(128), 0, st, q);
  CK(hipGetLastError());
  return MACX_OK;
}

// the control unit (not recurrent: every control depends on the question only, so all p steps at once; recurrent: the parameters
// of its linears) and the self attention's control projection
int CellBwd::control_bwd_tail() {
  const int S = s->S;
  if (o->write_self_att && !o->write_self_att_cont && !o->control_feed_prev) {
    // selfControl = the NEW control: dL/dc_i += dsc_i Ws^T before the word attention is differentiated
    LinP l = lin_basic(ws + W.dsc, d, d, B, wT + W.wscT, nullptr, d, MACX_ACT_NON, DC + Bd, d);
    l.seg[0].zstride = Bd; l.zout = Bd; l.addend = DC + Bd; l.ld_add = d; l.zadd = Bd;
    CK(small_linear_launch(l, p, st));
  }
  if (o->control_feed_prev) {
    // word-attention parameter partials were accumulated step by step
    CK(rs.add(ws + W.dwc_part, B, d, d, GP->ctrlLogits_w, st));
    CK(rs.add(ws + W.dbc_part, p * B, 1, 1, GP->ctrlLogits_b, st));
    // contControl weights: one contraction over all p*B rows per input segment
    if (o->control_feed_prev_att) {   // rows of step i = c_{i-1} = controls[i]
      CKI(wgrad_impl(controls(), d, ws + W.dlin1, d, p * B, d, d, GP->contControl_W, ws + W.small_slab, st));
    } else {
      // prev of step 0 is the initial control, prev of step i > 0 is cc_{i-1}
      CKI(wgrad_impl(controls(), d, ws + W.dlin1, d, B, d, d, GP->contControl_W, ws + W.small_slab, st));
      if (p > 1) {
        CKI(wgrad_impl(saved + L.cc, d, ws + W.dlin1 + Bd, d, (p - 1) * B, d, d, ws + W.tmp_dd, ws + W.small_slab, st));
        CK(axpy(ws + W.tmp_dd, dd, GP->contControl_W, st));
      }
    }
    if (o->control_feed_inputs)
      CKI(wgrad_impl(saved + L.cI, d, ws + W.dlin1, d, p * B, d, d, GP->contControl_W + dd, ws + W.small_slab, st));
    CK(rs.add(ws + W.dlin1, p * B, d, d, GP->contControl_b, st));
    if (o->control_cont_act != MACX_ACT_NON) {
      CKI(wgrad_impl(saved + L.cc_h, d, ws + W.dcc, d, p * B, d, d, GP->contControl2_W, ws + W.small_slab, st));
      CK(rs.add(ws + W.dcc, p * B, d, d, GP->contControl2_b, st));
    }
  } else {
    CKI(control_attend_bwd(B, S, d, p, DC + Bd, saved + L.cc, saved + L.seg[MACX_SEG_ATT_QUESTION], in->words, P->ctrlLogits_w,
                           sg.d_att_question, ws + W.ctrl_dl, ws + W.dcc, GI->words, 0, ws + W.dwc_part, ws + W.dbc_part, st));
    CK(rs.add(ws + W.dwc_part, B, d, d, GP->ctrlLogits_w, st));
    CK(rs.add(ws + W.dbc_part, p * B, 1, 1, GP->ctrlLogits_b, st));
  }
  if (o->write_self_att) {
    // the self-attention control projection reads contControl (== controlInput here) or the control:
    // d(source)_i += dsc_i Ws^T, in place, all steps in one launch
    float* dst = o->write_self_att_cont ? ws + W.dcc : DC + Bd;
    LinP l = lin_basic(ws + W.dsc, d, d, B, wT + W.wscT, nullptr, d, MACX_ACT_NON, dst, d);
    l.seg[0].zstride = Bd; l.zout = Bd; l.addend = dst; l.ld_add = d; l.zadd = Bd;
    if (o->write_self_att_cont && !o->control_feed_prev) CK(small_linear_launch(l, p, st));
    const float* src = o->write_self_att_cont ? saved + L.cc : controls() + Bd;
    CKI(wb.add(src, d, ws + W.dsc, d, p * B, d, d, GP->selfCtrl_W, st));
    CK(rs.add(ws + W.dsc, p * B, d, d, GP->selfCtrl_b, st));
    CK(rs.add(ws + W.dws_part, p * B, d, d, GP->selfLogits_w, st));
    CK(rs.add(ws + W.dbs_part, p * B, 1, 1, GP->selfLogits_b, st));
  }
  return MACX_OK;
}

int CellBwd::gate_wgrads() {
  if (!o->write_gate) return MACX_OK;
  CKI(wb.add(controls() + Bd, d, ws + W.dzpre, d, p * B, d, d, GP->gate_W, st));
  CK(rs.add(ws + W.dzpre, p * B, d, d, GP->gate_b, st));
  return MACX_OK;
}

// the control inputs (mac_cell.py:442-448): dt = sum_i dcI_i WqU_i^T ; du = dt * act'(t) ; dvecQ = du Wq^T
int CellBwd::control_inputs_bwd() {
  // (dL/d(initial state) where a state is initialised from the question vector, mac_cell.py:496-505: the first of them rides the
  // dvecQ launch's epilogue instead of an axpy of its own)
  const float* q_add = o->init_ctrl == MACX_INIT_Q ? DC : (o->init_mem == MACX_INIT_Q ? DM : nullptr);
  const CtrlInputsScratch x{ws + W.dt_part, ws + W.dt, ws + W.du, ws + W.tmpBd[1], ws + W.small_slab};
  return ctrl_inputs_bwd(o->control_input_unshared, o->control_input_act, B, d, p, in->vecQuestions, saved + L.ctrl_t, ws + W.dcI,
                         wT + W.wqT, wT + W.wqUT, q_add, x, GI->vecQuestions, GP, rs, wb, st);
}

// the initial state (mac_cell.py:496-505)
int CellBwd::initial_state_bwd() {
  if (o->init_mem == MACX_INIT_PRM) CK(rs.add(DM, B, d, d, GP->initMem, st));
  else if (o->init_mem == MACX_INIT_Q && o->init_ctrl == MACX_INIT_Q) CK(axpy(DM, Bd, GI->vecQuestions, st));   // (else: dvecQ's addend)
  if (o->init_ctrl == MACX_INIT_PRM) CK(rs.add(DC, B, d, d, GP->initCtrl, st));
  return MACX_OK;
}

// weight gradients of the [B,d] linears, one contraction over all p*B rows each: the read unit's projY ...
int CellBwd::read_linear_wgrads() {
  CKI(wb.add(saved + L.md, d, ws + W.DY, d, p * B, d, d, GP->projY_W, st));
  CK(rs.add(ws + W.DY, p * B, d, d, GP->projY_b, st));
  return MACX_OK;
}

// ... and the write unit's newMemory
int CellBwd::write_linear_wgrads() {
  const int rows = p * B;
  CKI(wb.add(memories(), d, dwlin_all, d, rows, d, d, GP->newMemory_W, st));
  CKI(wb.add(saved + L.seg[MACX_SEG_INFOS], d, dwlin_all, d, rows, d, d, GP->newMemory_W + dd, st));
  if (o->write_self_att)
    CKI(wb.add(saved + L.self_smry, d, dwlin_all, d, rows, d, d, GP->newMemory_W + 2 * dd, st));
  CK(rs.add(dwlin_all, rows, d, d, GP->newMemory_b, st));
  return MACX_OK;
}

// phase 2: the read unit's weights -- a fixed-order reduction of the per-step slabs.  dW2 = sum_i H1_i^T dI2_i and
// dWx = sum_i dropout_i(KB)^T dX_i: ONE contraction each over all p*B*N rows (the per-step operands are kept; 288 GB of HBM makes
// that the cheap choice)
int CellBwd::read_weight_contractions() {
  int ns_w = (int)R.ns_big;          // reduction splits of the dW2 / dWx contractions (H2 family: decided below)
  if (R.h2) {
    // mode 3: the two contractions share ONE launch AND the chip -- half the reduction splits each, so that the 2 x 128 workgroups
    // are all resident at once (one per CU) instead of 2 x 256 in two rounds: a workgroup's prologue, its 256 KB slab and the slab
    // reduction's input are paid for once per CU instead of twice
    ns_w = (wgrad_pipe_mode() >= 3 && wgrad_h2_kw(d) == 2 && wgrad_h2_jw(d) == 2 && R.ns_big >= 2) ? (int)R.ns_big / 2 : (int)R.ns_big;
    const H2WgradOp op[2] = {
        {saved + L.H1, L.act_stride, false, ws + W.dI2, W.act_floats, ws + W.wg_ftab, ws + W.slab_w2},
        // (no dropout: the same (converted) KB every step)
        {saved + L.KBd, L.act_stride, !rdrop, ws + W.dX, W.act_floats, ws + W.wg_ftab2, ws + W.slab_wx}};
    CKI(h2_wgrad(op, 2, p, B * N, d, d, ns_w, rows_per_split(p * B * N, ns_w), reinterpret_cast<int*>(ws + W.ecom), st));
  } else {
    TnP t;
    memset(&t, 0, sizeof(t));
    t.M = p * B * N; t.Kd = d; t.Jd = d; t.nsplit = (int)R.ns_big; t.rows_per_split = rows_per_split(t.M, t.nsplit);
    t.A = saved + L.H1; t.lda = d; t.a_mod = t.M; t.G = ws + W.dI2; t.ldg = d;
    t.part = ws + W.slab_w2;
    CK(wgrad_any(t, st));
    if (rdrop) { t.A = saved + L.KBd; t.a_mod = t.M; }        // the dropped KB of every step was kept
    else { t.A = in->knowledgeBase; t.a_mod = B * N; }        // no dropout: the same KB each step
    t.G = ws + W.dX;
    t.part = ws + W.slab_wx;
    CK(wgrad_any(t, st));
  }
  if (R.sb_deferred) {
    // dW1a = sum_i sum_b diag(y_ib) S_ib, dW1b = sum_i sum_b S_ib, S_ib = X_ib^T dI1_ib: every step in one launch, the two
    // accumulators of a workgroup run through all of them (macx_wgrad_h2.hip.h)
    CKI(sb_h2(B, N, d, p, R.sb_qpg, R.sb_wide, saved + L.X, L.act_stride, ws + W.dI1, W.dI1_stride, saved + L.y, Bd, P->memKbProj_W,
              ws + W.slab_w1a, ws + W.slab_w1b, nullptr, st));
  }
  SlabList sl;
  sl.d[0] = SlabDesc{ws + W.slab_w2, ns_w, dd / 4, GP->memKbProj2_W, 0};
  sl.d[1] = SlabDesc{ws + W.slab_wx, ns_w, dd / 4, GP->projX_W, 0};
  sl.d[2] = SlabDesc{ws + W.slab_w1a, (int)R.nslab_sb, dd / 4, GP->memKbProj_W, 0};
  sl.d[3] = SlabDesc{ws + W.slab_w1b, (int)R.nslab_sb, dd / 4, GP->memKbProj_W + dd, 0};
  CK(slab_reduce_list_launch(sl, 4, dd, st));
  CK(rs.add(ws + W.db2_part, p * (int)R.dwk_rows, d, d, GP->memKbProj2_b, st));
  CK(rs.add(ws + W.db1_part, p * (int)R.db_rows, d, d, GP->memKbProj_b, st));
  CK(rs.add(ws + W.dbx_part, p * (int)R.db_rows, d, d, GP->projX_b, st));
  CK(rs.add(ws + W.dwk_part, p * (int)R.dwk_rows, d, d, GP->kbLogits_w, st));
  CK(rs.add(ws + W.dbk_part, p * B, 1, 1, GP->kbLogits_b, st));
  CK(rs.run(st));
  return MACX_OK;
}
}  // namespace

int macx_cell_backward_phase_x(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                               const macx_inputs* in, const float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                               const float* d_memory, const float* d_control, const macx_param_grads* GP,
                               const macx_input_grads* GI, const macx_state_grads* SG, int phase, void* stream) {
  ModeScope ms(o);
  if (phase < 0 || phase > 2) return MACX_EINVAL;
  CKI(check_impl(o, s));
  if (!dp || !P || !in || !saved || !ws || !GP || !GI) return MACX_EINVAL;
  if (!GI->knowledgeBase || !GI->words || !GI->vecQuestions) return MACX_EINVAL;
  // a gradient for an attention map this option set does not have: refused before anything is launched
  if (SG && ((SG->d_att_self && !o->write_self_att) || (SG->d_att_gate && !o->write_gate))) return MACX_EINVAL;
  CellBwd r(o, s, dp, P, in, saved, ws, GP, GI, stream);
  if (SG) r.sg = *SG;
  CKI(r.check_bwd_buffers(saved_floats, ws_floats, phase));
  if (phase != 2) {
    CKI(r.init_state_grads(d_memory, d_control));
    if (o->control_feed_prev) {
      CK(dev_zero(GI->words, (size_t)r.B * s->S * r.d * sizeof(float), r.st));
      CK(dev_zero(ws + r.W.dwc_part, r.Bd * sizeof(float), r.st));
      CK(dev_zero(ws + r.W.dccx, (size_t)(r.p + 1) * r.Bd * sizeof(float), r.st));
      r.dc_in_loop = true;
    }
    r.plan_dkb_fill();
    for (int i = r.p - 1; i >= 0; --i) {
      CKI(r.write_unit_bwd(i));
      CKI(r.read_unit_bwd(i));
      CKI(r.dy_linear_bwd(i, true));
      if (o->control_feed_prev) CKI(r.control_step_bwd(i));
    }
    CKI(r.read_dc_reduce_all());
    CKI(r.control_bwd_tail());
    CKI(r.gate_wgrads());
    CKI(r.control_inputs_bwd());
    CKI(r.initial_state_bwd());
    CKI(r.read_linear_wgrads());
    CKI(r.write_linear_wgrads());
    CKI(r.wb.run(r.st));
  }
  CK(r.rs.run(r.st));
  return phase == 1 ? MACX_OK : r.read_weight_contractions();
}

int macx_cell_backward_phase(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                             const macx_inputs* in, const float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                             const float* d_memory, const float* d_control, const macx_param_grads* GP,
                             const macx_input_grads* GI, int phase, void* stream) {
  return macx_cell_backward_phase_x(o, s, dp, P, in, saved, saved_floats, ws, ws_floats, d_memory, d_control, GP, GI, nullptr, phase, stream);
}

int macx_cell_backward_x(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                         const macx_inputs* in, const float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                         const float* d_memory, const float* d_control, const macx_param_grads* GP,
                         const macx_input_grads* GI, const macx_state_grads* SG, void* stream) {
  return macx_cell_backward_phase_x(o, s, dp, P, in, saved, saved_floats, ws, ws_floats, d_memory, d_control, GP, GI, SG, 0, stream);
}

int macx_cell_backward(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                       const macx_inputs* in, const float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                       const float* d_memory, const float* d_control, const macx_param_grads* GP,
                       const macx_input_grads* GI, void* stream) {
  return macx_cell_backward_x(o, s, dp, P, in, saved, saved_floats, ws, ws_floats, d_memory, d_control, GP, GI, nullptr, stream);
}

// =================================================================================================
// unit-level entry points
// =================================================================================================
// ---- one read / write unit on caller-owned buffers: the cell's own unit functions.
// shapes->p == 1: the unit of step 0 (the dropout streams are keyed by (seed, site, step 0)).
namespace {
int unit_check(const macx_opts* o, const macx_shapes* s, bool write) {
  CKI(check_impl(o, s));
  if (s->p != 1) return MACX_EINVAL;
  if (write && o->write_self_att) return MACX_EUNSUPPORTED;   // needs the histories of a running cell
  return MACX_OK;
}
}  // namespace

size_t macx_workspace_bytes(const macx_opts* o, const macx_shapes* s, int for_backward) {
  return macx_ws_floats(o, s, for_backward) * sizeof(float);
}

int macx_read_fwd(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                  const float* knowledgeBase, const float* memory, const float* control, float* saved, size_t saved_floats,
                  float* info, float* att, void* stream) {
  return macx_read_fwd_l(o, s, dp, P, knowledgeBase, nullptr, memory, control, saved, saved_floats, info, att, stream);
}

// kb_lengths: macx_inputs.kbLengths of this one unit (NULL: every question attends over all N cells)
int macx_read_fwd_l(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                    const float* knowledgeBase, const int32_t* kb_lengths, const float* memory, const float* control, float* saved,
                    size_t saved_floats, float* info, float* att, void* stream) {
  ModeScope ms(o);
  CKI(unit_check(o, s, false));
  if (!dp || !P || !knowledgeBase || !memory || !control || !saved || !info || !att) return MACX_EINVAL;
  if (misaligned(saved) || misaligned(knowledgeBase)) return MACX_EINVAL;
  macx_inputs in{};
  in.knowledgeBase = knowledgeBase;
  in.kbLengths = kb_lengths;
  const CellRun r(o, s, dp, P, &in, saved, 1, stream);
  if (saved_floats < r.L.total) return MACX_ESMALL;
  {
    Packer pk;
    if (r.R.h2) CK(r.read_weight_maxima());
    r.add_read_packs(pk);
    if (r.L.bwd_packs) {
      const BwdLayout W = make_bwd(o, s, r.R);
      r.add_read_packs(pk, &W);
    }
    CK(pk.run(r.st));
  }
  CK(dev_copy(r.memories(), memory, r.Bd * sizeof(float), r.st));
  CK(dev_copy(r.controls() + r.Bd, control, r.Bd * sizeof(float), r.st));
  CKI(r.read_step(0, 0, false));
  CK(dev_copy(info, r.info_raw(0), r.Bd * sizeof(float), r.st));
  CK(dev_copy(att, saved + r.L.seg[MACX_SEG_ATT_KB], (size_t)r.B * r.N * sizeof(float), r.st));
  return MACX_OK;
}

int macx_read_bwd(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                  const float* knowledgeBase, const float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                  const float* d_info, const macx_param_grads* GP, float* d_knowledgeBase, float* d_memory, float* d_control,
                  void* stream) {
  ModeScope ms(o);
  CKI(unit_check(o, s, false));
  if (!knowledgeBase || !d_info || !d_knowledgeBase || !d_memory || !d_control) return MACX_EINVAL;
  if (!dp || !P || !saved || !ws || !GP) return MACX_EINVAL;
  macx_inputs in{};
  in.knowledgeBase = knowledgeBase;
  macx_input_grads GI{};
  GI.knowledgeBase = d_knowledgeBase;
  CellBwd r(o, s, dp, P, &in, saved, ws, GP, &GI, stream);
  CKI(r.check_bwd_buffers(saved_floats, ws_floats, 0));
  CKI(r.init_state_grads(nullptr, nullptr));
  r.dinfo = StepSlab{d_info, r.d, r.Bd};
  CKI(r.read_unit_bwd(0));
  CKI(r.dy_linear_bwd(0, false));
  CKI(r.read_dc_reduce_all());
  CKI(r.read_linear_wgrads());
  // dL/d(memory) = (dy Wy^T) through the two masks, dL/d(control) from the attention logits
  CK(dev_copy(d_memory, r.DM, r.Bd * sizeof(float), r.st));
  CK(dev_copy(d_control, r.DC + r.Bd, r.Bd * sizeof(float), r.st));
  CKI(r.wb.run(r.st));
  CK(r.rs.run(r.st));
  return r.read_weight_contractions();
}

int macx_write_fwd(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                   const float* memory, const float* info, const float* control, float* saved, size_t saved_floats,
                   float* new_memory, void* stream) {
  ModeScope ms(o);
  CKI(unit_check(o, s, true));
  if (!dp || !P || !memory || !info || !control || !saved || !new_memory) return MACX_EINVAL;
  if (misaligned(saved)) return MACX_EINVAL;
  const CellRun r(o, s, dp, P, nullptr, saved, 1, stream);
  if (saved_floats < r.L.total) return MACX_ESMALL;
  {
    Packer pk;
    r.add_write_packs(pk);
    if (r.L.bwd_packs) {
      const BwdLayout W = make_bwd(o, s, r.R);
      r.add_write_packs(pk, &W);
    }
    CK(pk.run(r.st));
  }
  CK(dev_copy(r.memories(), memory, r.Bd * sizeof(float), r.st));
  CK(dev_copy(r.info_raw(0), info, r.Bd * sizeof(float), r.st));
  CK(dev_copy(r.controls() + r.Bd, control, r.Bd * sizeof(float), r.st));
  CKI(r.write_step(0, false));
  CK(dev_copy(new_memory, r.memories() + r.Bd, r.Bd * sizeof(float), r.st));
  return MACX_OK;
}

int macx_write_bwd(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                   const float* saved, size_t saved_floats, float* ws, size_t ws_floats, const float* d_new_memory,
                   const macx_param_grads* GP, float* d_memory, float* d_info, float* d_control, void* stream) {
  ModeScope ms(o);
  CKI(unit_check(o, s, true));
  if (!d_new_memory || !d_memory || !d_info || !d_control) return MACX_EINVAL;
  if (!dp || !P || !saved || !ws || !GP) return MACX_EINVAL;
  CellBwd r(o, s, dp, P, nullptr, saved, ws, GP, nullptr, stream);
  CKI(r.check_bwd_buffers(saved_floats, ws_floats, 0));
  CKI(r.init_state_grads(d_new_memory, nullptr));
  CKI(r.write_unit_bwd(0));
  // dL/d(memory) = dwin[:, :d] (+ dm (1 - z) under the gate), dL/d(info), dL/d(control) (the gate's)
  const size_t wbytes = (size_t)r.d * sizeof(float);
  CK(dev_copy2d(d_memory, wbytes, ws + r.W.dwin, (size_t)r.win * sizeof(float), wbytes, r.B, r.st));
  if (o->write_gate) CK(axpy(ws + r.W.tmpBd[3], r.Bd, d_memory, r.st));
  CK(dev_copy2d(d_info, wbytes, r.dinfo.base, (size_t)r.dinfo.ld * sizeof(float), wbytes, r.B, r.st));
  CK(dev_copy(d_control, r.DC + r.Bd, r.Bd * sizeof(float), r.st));
  CKI(r.gate_wgrads());
  CKI(r.write_linear_wgrads());
  CKI(r.wb.run(r.st));
  CK(r.rs.run(r.st));
  return MACX_OK;
}

int macx_linear(const float* x1, int k1, const float* x2, int k2, int rows, const float* Wp, const float* b, float bias_const,
                int n_out, int act, float* out, void* stream) {
  if (!x1 || !Wp || !out || rows < 1 || n_out < 16 || n_out % 16) return MACX_EINVAL;
  if (k1 % 16 != 0 || k2 % 16 != 0 || k1 < 16 || (x2 == nullptr) != (k2 == 0)) return MACX_EINVAL;
  if (misaligned(x1) || misaligned(x2) || misaligned(Wp) || misaligned(out)) return MACX_EINVAL;
  LinP l = lin_basic(x1, k1, k1, rows, Wp, b, n_out, act, out, n_out);
  if (x2) { l.seg[1] = LinSeg{x2, k2, k2, 0}; l.Ktot = k1 + k2; }
  l.bias_const = bias_const;
  CK(small_linear_launch(l, 1, (hipStream_t)stream));
  return MACX_OK;
}

int macx_linear_part(const float* part, int part_N, int part_shift, int k, int rows, const float* Wp, const float* b, float bias_const,
                     int n_out, int act, float* part_sum, float* out, void* stream) {
  if (!part || !Wp || !part_sum || !out || rows < 1 || rows > 128 || n_out < 16 || n_out % 16 || k < 16 || k % 16) return MACX_EINVAL;
  if (part_N < 1 || part_shift < 4 || part_shift > 6 || ((part_N - 2) >> part_shift) + 2 > LIN_PART_TILES) return MACX_EINVAL;
  if ((1 << part_shift) > 2 * part_N) return MACX_EINVAL;      // a tile has three slots: it may reach into at most three questions
  if (misaligned(part) || misaligned(Wp) || misaligned(part_sum) || misaligned(out)) return MACX_EINVAL;
  LinP l = lin_basic(part_sum, k, k, rows, Wp, b, n_out, act, out, n_out);
  l.bias_const = bias_const;
  l.part = part; l.part_N = part_N; l.part_sum = part_sum; l.part_shift = part_shift;
  CK(small_linear_part_launch(l, (hipStream_t)stream));
  return MACX_OK;
}

int macx_pack_weight(const float* Wt, int K, int n_out, int flags, float* out, void* stream) {
  const int transpose = flags;
  if (!Wt || !out || K < 16 || K % 16 || n_out < 16 || n_out % 16) return MACX_EINVAL;
  const int fmt = transpose >> 1;      // bits 1..: pack format (0 fp32 MFMA layout, 1 split-bf16 planes, 2 fp32 k-major tiles)
  if (fmt < 0 || fmt > 2 || (fmt && K % 32)) return MACX_EINVAL;
  Packer pk;
  if (transpose & 1) pk.add(Wt, 1, K, K, n_out, out, -1, -1, fmt);
  else pk.add(Wt, n_out, 1, K, n_out, out, -1, -1, fmt);
  CK(pk.run((hipStream_t)stream));
  return MACX_OK;
}

int macx_kb_project(const macx_shapes* s, const macx_dropout* dp, int step, const float* kb, const float* Wp, const float* b,
                    float* out, float* bits_ws, void* stream) {
  if (!s || !dp || !kb || !Wp || !b || !out) return MACX_EINVAL;
  if (s->d % 128 != 0 || s->N > K_MAXN || ((size_t)s->B * s->N * s->d) % 32) return MACX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  const int d = s->d;
  GemmP g;
  memset(&g, 0, sizeof(g));
  g.B = s->B; g.N = s->N; g.K = d; g.Nout = d;
  g.A = kb; g.lda = d;
  g.Wp = Wp; g.out = out; g.ldo = d; g.bias = b; g.act = MACX_ACT_NON;
  if (dp->keep_read < 1.0f) {
    if (!bits_ws) return MACX_EINVAL;
    // scratch: [B*N*d] dropped KB, then [B*N*d/32] keep bits
    const size_t n = (size_t)s->B * s->N * d;
    const DropSpec dk = make_drop(dp->keep_read, dp, SITE_READ_KB, step);
    hipLaunchKernelGGL(kb_dropout_kernel, dim3(2048), dim3(256), 0, st, kb, n / 4, dk.key, dk.thr24, dk.inv_keep,
                       (uint32_t)((size_t)s->b0 * s->N * d), bits_ws, reinterpret_cast<uint32_t*>(bits_ws + n), 0u, (uint32_t*)nullptr,
                       dk.word);
    CK(hipGetLastError());
    g.A = bits_ws;
  }
  CK((kb_gemm<A_PLAIN, B_PLAIN, E_BIAS_ACT, false>(g, st)));     // Wp: pack format 1 (split mode) or 0
  return MACX_OK;
}

int macx_control_attend(const macx_shapes* s, const float* cc, const float* words, const int32_t* lengths, const float* w,
                        const float* b, float* att, float* control, void* stream) {
  if (!s || !cc || !words || !lengths || !w || !b || !att || !control) return MACX_EINVAL;
  if (s->B < 1 || s->S < 1 || s->S > C_MAXS || s->d < 4 || s->d % 4 != 0) return MACX_EINVAL;
  return control_attend(s->B, s->S, s->d, 1, cc, words, lengths, w, b, att, control, (hipStream_t)stream);
}

size_t macx_control_attend_bwd_ws_floats(const macx_shapes* s) {
  if (!s) return 0;
  return al4((size_t)s->B * s->S) + al4((size_t)s->B * s->d) + al4((size_t)s->B);
}

int macx_control_attend_bwd(const macx_shapes* s, const float* d_control, const float* cc, const float* att, const float* words,
                            const float* w, float* ws, size_t ws_floats, float* d_cc, float* d_words, float* d_w, float* d_b,
                            void* stream) {
  if (!s || !d_control || !cc || !att || !words || !w || !ws || !d_cc || !d_words || !d_w || !d_b) return MACX_EINVAL;
  if (s->B < 1 || s->S < 1 || s->S > C_MAXS || s->d < 64 || s->d % 64 != 0) return MACX_EINVAL;
  if (ws_floats < macx_control_attend_bwd_ws_floats(s)) return MACX_ESMALL;
  hipStream_t st = (hipStream_t)stream;
  const int B = s->B, S = s->S, d = s->d;
  float* dw_part = ws + al4((size_t)B * S);
  float* db_part = dw_part + al4((size_t)B * d);
  CKI(control_attend_bwd(B, S, d, 1, d_control, cc, att, words, w, nullptr, ws, d_cc, d_words, 0, dw_part, db_part, st));
  CK(rowsum(dw_part, B, d, d, d_w, st));
  CK(rowsum(db_part, B, 1, 1, d_b, st));
  return MACX_OK;
}

int macx_embed_lookup(const int32_t* ids, const float* emb, int rows, int E, int ld, float keep, uint32_t seed, uint32_t first_row,
                      float* x, void* stream) {
  if (!ids || !emb || !x || rows < 1 || E < 1 || ld < E) return MACX_EINVAL;
  hipLaunchKernelGGL(embed_gather_kernel, dim3(512), dim3(256), 0, (hipStream_t)stream, ids, emb, rows, E, ld, first_row,
                     make_drop(keep, seed, SITE_ENC_INPUT, 0), x);
  CK(hipGetLastError());
  return MACX_OK;
}

int macx_embed_lookup_bwd(const int32_t* ids, const float* dx, int rows, int E, int ld, int V, float keep, uint32_t seed,
                          uint32_t first_row, float* d_emb, void* stream) {
  if (!ids || !dx || !d_emb || rows < 1 || E < 1 || ld < E || V < 1) return MACX_EINVAL;
  hipLaunchKernelGGL(embed_grad_kernel, dim3(V, (E + 1023) / 1024), dim3(256), 0, (hipStream_t)stream, ids, dx, rows, E, ld, first_row,
                     make_drop(keep, seed, SITE_ENC_INPUT, 0), d_emb);
  CK(hipGetLastError());
  return MACX_OK;
}

int macx_dropout_mask_w(uint32_t seed, uint32_t site, uint32_t step, float keep, uint32_t first, size_t n, const uint32_t* mask_word,
                        float* out, void* stream) {
  if (!out) return MACX_EINVAL;
  const DropSpec ds = make_drop(keep, seed, site, step);
  hipLaunchKernelGGL(dropout_mask_kernel, dim3(256), dim3(256), 0, (hipStream_t)stream, ds.key, ds.thr24, first, n, out, mask_word);
  CK(hipGetLastError());
  return MACX_OK;
}
int macx_dropout_mask(uint32_t seed, uint32_t site, uint32_t step, float keep, uint32_t first, size_t n, float* out, void* stream) {
  return macx_dropout_mask_w(seed, site, step, keep, first, n, nullptr, out, stream);
}

// ---- answer loss + prediction (model.py:593-612): SURVEY 8f row 2 -------------------------------------------------
// loss_rows[b] = sparse softmax cross-entropy of question b (the caller's loss is their mean: tf.reduce_mean, model.py:596);
// pred[b] = argmax; dlogits (may be NULL) = (softmax - onehot) * grad_scale, i.e. pass 1/B for the gradient of the mean loss
int macx_answer_loss(const float* logits, const int32_t* answers, int B, int A, float* loss_rows, int32_t* pred, float* dlogits,
                     float grad_scale, void* stream) {
  if (!logits || !answers || !loss_rows || !pred || B < 1 || A < 1) return MACX_EINVAL;
  hipLaunchKernelGGL(answer_loss_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, answers, B, A, loss_rows, pred,
                     dlogits, grad_scale);
  CK(hipGetLastError());
  return MACX_OK;
}

// ---- a loss on a run's attention maps: rows [p,B] and d_att [p,B,n] in one launch (macx_att_loss.hip.h) ------------------------
int macx_att_loss(const float* att, const float* target, const int32_t* lengths, const float* step_weights, const float* row_weights,
                  int p, int B, int n, int kind, int target_steps, float eps, float scale, float* loss_rows, float* d_att, void* stream) {
  if (!att || !loss_rows || p < 1 || B < 1 || n < 1) return MACX_EINVAL;
  if (!(eps > 0.f && eps < INFINITY)) return MACX_EINVAL;          // (NaN fails both comparisons)
  if (kind != ATT_LOSS_CE && kind != ATT_LOSS_ENTROPY) return MACX_EINVAL;
  if (kind == ATT_LOSS_CE && !target) return MACX_EINVAL;
  AttLossP q;
  q.att = att; q.target = target; q.lengths = lengths; q.step_weights = step_weights; q.row_weights = row_weights;
  q.p = p; q.B = B; q.n = n; q.target_steps = target_steps != 0; q.eps = eps; q.scale = scale; q.loss_rows = loss_rows; q.d_att = d_att;
  const dim3 grid((unsigned)(((size_t)p * B + 3) / 4));
  if (kind == ATT_LOSS_CE) hipLaunchKernelGGL(att_loss_kernel<ATT_LOSS_CE>, grid, dim3(256), 0, (hipStream_t)stream, q);
  else hipLaunchKernelGGL(att_loss_kernel<ATT_LOSS_ENTROPY>, grid, dim3(256), 0, (hipStream_t)stream, q);
  CK(hipGetLastError());
  return MACX_OK;
}

// ---- the answer loss under per-question device weights, its weighted mean and an evaluation loop's running totals ---------------
// (contract: include/macx.h; one workgroup of AW_WAVES waves, answer_loss_weighted_kernel in macx_ops.hip.h)
int macx_answer_loss_weighted(const float* logits, const int32_t* answers, const float* weights, int B, int A, float* loss_rows,
                              int32_t* pred, float* dlogits, float* loss_out, double* totals, float grad_scale, void* stream) {
  if (!logits || !answers || !loss_rows || !pred || B < 1 || A < 1) return MACX_EINVAL;
  hipLaunchKernelGGL(answer_loss_weighted_kernel, dim3(1), dim3(AW_WAVES * 64), 0, (hipStream_t)stream, logits, answers, weights, B, A,
                     loss_rows, pred, dlogits, loss_out, totals, grad_scale);
  CK(hipGetLastError());
  return MACX_OK;
}

// ---- the knowledge-base attention unit on its own (the fused cell's kernels behind a per-unit contract) -----------------
// forward: att = softmax_n(logits + bias), info = sum_n att KB       (ops.inter2att :140-146 + ops.att2Smry :149-150)
int macx_kb_attend_fwd(int B, int N, int d, const float* logits, const float* bias, const float* kb, float* att, float* info,
                       void* stream) {
  return macx_kb_attend_fwd_l(B, N, d, logits, bias, kb, nullptr, att, info, stream);
}
// ... over the first kb_lengths[b] cells of question b (clamped to [1, N]; NULL: all N): att[b][n >= length] = 0 exactly, and neither the
// logits nor the knowledge-base rows of those cells are used
int macx_kb_attend_fwd_l(int B, int N, int d, const float* logits, const float* bias, const float* kb, const int32_t* kb_lengths,
                         float* att, float* info, void* stream) {
  if (!logits || !bias || !kb || !att || !info || B < 1 || N < 1 || N > K_MAXN || d < 128 || d % 128) return MACX_EINVAL;
  return kb_attend(B, N, d, 1, logits, bias, kb, kb_lengths, att, info, (hipStream_t)stream);
}
size_t macx_kb_attend_bwd_ws_floats(int B, int N, int d) { return (size_t)B * N + 8; (void)d; }
// backward: da = dinfo . KB ; dlogits = att (da - sum_n att da) ; dKB (=, or += with accumulate) att (x) dinfo
int macx_kb_attend_bwd(int B, int N, int d, const float* att, const float* kb, const float* dinfo, float* dlogits, float* dkb,
                       int accumulate, float* ws, size_t ws_floats, void* stream) {
  if (!att || !kb || !dinfo || !dlogits || !ws || B < 1 || N < 1 || d < 128 || d % 128) return MACX_EINVAL;
  if (ws_floats < macx_kb_attend_bwd_ws_floats(B, N, d)) return MACX_ESMALL;
  hipStream_t st = (hipStream_t)stream;
  float* da = ws;
  CKI(kb_att_da(B, N, d, dinfo, d, kb, nullptr, da, st));
  hipLaunchKernelGGL(op_softmax_bwd_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, att, (const float*)da, (size_t)B, N, dlogits);
  CK(hipGetLastError());
  if (dkb) {
    const size_t n = (size_t)B * N * d;
    hipLaunchKernelGGL(kb_attend_dkb_kernel, dim3(op_grid(n)), dim3(256), 0, st, att, dinfo, n, N, d, accumulate, dkb);
    CK(hipGetLastError());
  }
  return MACX_OK;
}

// ---- the ops.py primitives as single kernels (macx_ops.hip.h): the generic option path ---------------------------
int macx_op_act(int act, const float* x, const float* alpha, size_t n, int inner, float* out, void* stream) {
  const bool ext = act == OP_ACT_PRELU || act == OP_ACT_RSQRT_EPS;
  if (!x || !out || inner < 1 || (ext && !alpha) || (!ext && (act < 0 || act > ACT_RELU))) return MACX_EINVAL;
  if (n == 0) return MACX_OK;
  hipLaunchKernelGGL(op_act_kernel, dim3(op_grid(n)), dim3(256), 0, (hipStream_t)stream, act, x, alpha, n, inner, out);
  CK(hipGetLastError());
  return MACX_OK;
}
int macx_op_act_bwd(int act, const float* x, const float* alpha, const float* dy, size_t n, int inner, float* dx, float* dalpha_elem,
                    void* stream) {
  const bool ext = act == OP_ACT_PRELU || act == OP_ACT_RSQRT_EPS;
  if (!x || !dy || !dx || inner < 1 || (ext && !alpha) || (act == OP_ACT_PRELU && !dalpha_elem) || (!ext && (act < 0 || act > ACT_RELU)))
    return MACX_EINVAL;
  if (n == 0) return MACX_OK;
  hipLaunchKernelGGL(op_act_bwd_kernel, dim3(op_grid(n)), dim3(256), 0, (hipStream_t)stream, act, x, alpha, dy, n, inner, dx, dalpha_elem);
  CK(hipGetLastError());
  return MACX_OK;
}
int macx_op_binary(int op, int bmode, const float* a, const float* b, size_t n, int mid, int inner, float scale, float* out, void* stream) {
  if (!a || !b || !out || op < OP_ADD || op > OP_MUL || bmode < OP_B_SAME || bmode > OP_B_ROW || mid < 1 || inner < 1) return MACX_EINVAL;
  if (n % ((size_t)inner * (bmode == OP_B_MID ? mid : 1))) return MACX_EINVAL;
  if (n == 0) return MACX_OK;
  hipLaunchKernelGGL(op_binary_kernel, dim3(op_grid(n)), dim3(256), 0, (hipStream_t)stream, op, bmode, a, b, n, mid, inner, scale, out);
  CK(hipGetLastError());
  return MACX_OK;
}
int macx_op_reduce(int mode, const float* x, size_t outer, int mid, int inner, float* out, float* ws, void* stream) {
  if (!x || !out || outer < 1 || mid < 1 || inner < 1) return MACX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (mode == OP_R_MID) {
    if (outer > 0x7FFFFFFF) return MACX_EINVAL;
    hipLaunchKernelGGL(op_reduce_mid_kernel, dim3((unsigned)((outer * inner + 255) / 256)), dim3(256), 0, st, x, (int)outer, mid, inner, out);
  } else if (mode == OP_R_LAST) {
    hipLaunchKernelGGL(op_reduce_last_kernel, dim3((unsigned)((outer + 3) / 4)), dim3(256), 0, st, x, outer, inner, out);
  } else if (mode == OP_R_ROWS) {
    if (!ws) return MACX_EINVAL;
    hipLaunchKernelGGL(op_reduce_rows_kernel, dim3((inner + 255) / 256, OP_ROWS_SPLIT), dim3(256), 0, st, x, outer, inner, ws);
    hipLaunchKernelGGL(op_reduce_rows_final_kernel, dim3((inner + 255) / 256), dim3(256), 0, st, ws, inner, out);
  } else {
    return MACX_EINVAL;
  }
  CK(hipGetLastError());
  return MACX_OK;
}
int macx_op_softmax(const float* x, const int32_t* lengths, int rows_per_len, size_t rows, int n, float* out, void* stream) {
  if (!x || !out || rows < 1 || n < 1 || (lengths && rows_per_len < 1)) return MACX_EINVAL;
  hipLaunchKernelGGL(op_softmax_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, lengths, rows_per_len, rows, n,
                     out);
  CK(hipGetLastError());
  return MACX_OK;
}
int macx_op_softmax_bwd(const float* a, const float* da, size_t rows, int n, float* dx, void* stream) {
  if (!a || !da || !dx || rows < 1 || n < 1) return MACX_EINVAL;
  hipLaunchKernelGGL(op_softmax_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, da, rows, n, dx);
  CK(hipGetLastError());
  return MACX_OK;
}
int macx_op_dropout_w(const float* x, size_t n, uint32_t seed, uint32_t site, uint32_t step, float keep, uint32_t first,
                      const uint32_t* mask_word, float* out, void* stream) {
  if (!x || !out || !(keep > 0.f) || keep > 1.f) return MACX_EINVAL;
  if (n == 0) return MACX_OK;
  const DropSpec ds = make_drop(keep, seed, site, step);
  hipLaunchKernelGGL(op_dropout_kernel, dim3(op_grid(n)), dim3(256), 0, (hipStream_t)stream, x, n, first, ds.key, ds.thr24, ds.inv_keep, out,
                     mask_word);
  CK(hipGetLastError());
  return MACX_OK;
}
int macx_op_dropout(const float* x, size_t n, uint32_t seed, uint32_t site, uint32_t step, float keep, uint32_t first, float* out,
                    void* stream) {
  return macx_op_dropout_w(x, n, seed, site, step, keep, first, nullptr, out, stream);
}

// =================================================================================================
// output unit + classifier (model.py:512-576, ops.py:349-359): SURVEY 8f row 2
// =================================================================================================
namespace {
struct OutLayout {
  size_t woq_p, w0_p, w1_p;   // packed forward weights
  size_t eq;                  // [B,d]   outQuestion(vecQ)
  size_t x0;                  // [B,in]  dropped concat([memory, eq])
  size_t h;                   // [B,H]   act(fc_0)
  size_t x1;                  // [B,H]   dropped h
  size_t logits_pad;          // [B,Ap]
  size_t total;
};
inline int pad16(int n) { return (n + 15) & ~15; }
OutLayout make_out(const macx_out_shapes* s) {
  OutLayout L;
  memset(&L, 0, sizeof(L));
  size_t off = 0;
  auto take = [&](size_t n) { size_t r = off; off += al4(n); return r; };
  const size_t B = s->B, d = s->d, in = 2 * (size_t)s->d, H = s->hidden, Ap = pad16(s->answers);
  L.woq_p = take(d * d); L.w0_p = take(in * H); L.w1_p = take(H * Ap);
  L.eq = take(B * d); L.x0 = take(B * in); L.h = take(B * H); L.x1 = take(B * H); L.logits_pad = take(B * Ap);
  L.total = off;
  return L;
}
struct OutBwdLayout {
  size_t woqT, w0T, w1T;
  size_t dlog_pad, dx1, dh, dx0, deq, total;
};
OutBwdLayout make_out_bwd(const macx_out_shapes* s) {
  OutBwdLayout L;
  memset(&L, 0, sizeof(L));
  size_t off = 0;
  auto take = [&](size_t n) { size_t r = off; off += al4(n); return r; };
  const size_t B = s->B, d = s->d, in = 2 * (size_t)s->d, H = s->hidden, Ap = pad16(s->answers);
  L.woqT = take(d * d); L.w0T = take(H * in); L.w1T = take(Ap * H);
  L.dlog_pad = take(B * Ap); L.dx1 = take(B * H); L.dh = take(B * H); L.dx0 = take(B * in); L.deq = take(B * d);
  L.total = off;
  return L;
}
int out_check(const macx_out_shapes* s) {
  if (!s || s->B < 1 || s->d < 16 || s->d % 16 || s->hidden < 16 || s->hidden % 16 || s->answers < 1) return MACX_EINVAL;
  return MACX_OK;
}
}  // namespace

size_t macx_output_saved_floats(const macx_out_shapes* s) { return out_check(s) ? 0 : make_out(s).total; }
size_t macx_output_ws_floats(const macx_out_shapes* s) { return out_check(s) ? 0 : make_out_bwd(s).total; }

int macx_output_forward(const macx_out_shapes* s, int act, float keep, uint32_t seed, const macx_out_params* P, const float* memory,
                        const float* vecQ, float* logits, float* saved, size_t saved_floats, void* stream) {
  return macx_output_forward_w(s, act, keep, seed, P, memory, vecQ, logits, saved, saved_floats, nullptr, stream);
}

int macx_output_forward_w(const macx_out_shapes* s, int act, float keep, uint32_t seed, const macx_out_params* P, const float* memory,
                          const float* vecQ, float* logits, float* saved, size_t saved_floats, const uint32_t* mask_word,
                          void* stream) {
  CKI(out_check(s));
  if (!P || !memory || !vecQ || !logits || !saved) return MACX_EINVAL;
  const OutLayout L = make_out(s);
  if (saved_floats < L.total) return MACX_ESMALL;
  hipStream_t st = (hipStream_t)stream;
  const int B = s->B, d = s->d, in = 2 * d, H = s->hidden, A = s->answers, Ap = pad16(A);
  Packer pk;
  pk.add(P->outQuestion_W, d, 1, d, d, saved + L.woq_p);
  pk.add(P->fc0_W, H, 1, in, H, saved + L.w0_p);
  pk.add(P->fc1_W, A, 1, H, Ap, saved + L.w1_p, H, A);
  CK(pk.run(st));
  // outputOp (model.py:512-528): features = concat([memory, outQuestion(vecQ)])
  LinP q = lin_basic(vecQ, d, d, B, saved + L.woq_p, P->outQuestion_b, d, MACX_ACT_NON, saved + L.eq, d);
  CK(small_linear_launch(q, 1, st));
  // classifier (model.py:547-576 -> ops.FCLayer ops.py:349-359): dropout on every layer input, act between layers
  const DropSpec d0 = make_drop(keep, seed, SITE_OUT_FC0, 0, mask_word), d1 = make_drop(keep, seed, SITE_OUT_FC1, 0, mask_word);
  // the concat is built in place: columns [0,d) memory, [d,2d) eq, with the layer-input mask indexed over [B, 2d]
  CK(dev_copy2d(saved + L.x0, (size_t)in * sizeof(float), memory, (size_t)d * sizeof(float), (size_t)d * sizeof(float), B, st));
  CK(dev_copy2d(saved + L.x0 + d, (size_t)in * sizeof(float), saved + L.eq, (size_t)d * sizeof(float), (size_t)d * sizeof(float), B, st));
  hipLaunchKernelGGL(drop2_kernel, dim3(64), dim3(256), 0, st, (const float*)(saved + L.x0), B, in, (uint32_t)s->b0, d0, no_drop(),
                     saved + L.x0);
  LinP f0 = lin_basic(saved + L.x0, in, in, B, saved + L.w0_p, P->fc0_b, H, act, saved + L.h, H);
  CK(small_linear_launch(f0, 1, st));
  hipLaunchKernelGGL(drop2_kernel, dim3(64), dim3(256), 0, st, (const float*)(saved + L.h), B, H, (uint32_t)s->b0, d1, no_drop(),
                     saved + L.x1);
  CK(hipGetLastError());
  // fc_1: bias padded with zeros by reading through a guarded copy
  CK(dev_zero(saved + L.logits_pad, (size_t)B * Ap * sizeof(float), st));
  LinP f1 = lin_basic(saved + L.x1, H, H, B, saved + L.w1_p, nullptr, Ap, MACX_ACT_NON, saved + L.logits_pad, Ap);
  CK(small_linear_launch(f1, 1, st));
  hipLaunchKernelGGL(crop_cols_kernel, dim3(16), dim3(256), 0, st, (const float*)(saved + L.logits_pad), Ap, B, A, logits);
  // + bias (the packed layer ran without it because the bias vector is not padded)
  hipLaunchKernelGGL(add_bias_kernel, dim3(16), dim3(256), 0, st, P->fc1_b, B, A, logits);
  CK(hipGetLastError());
  return MACX_OK;
}

int macx_output_backward(const macx_out_shapes* s, int act, float keep, uint32_t seed, const macx_out_params* P, const float* memory,
                         const float* vecQ, const float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                         const float* d_logits, const macx_out_grads* G, float* d_memory, float* d_vecQ, void* stream) {
  return macx_output_backward_w(s, act, keep, seed, P, memory, vecQ, saved, saved_floats, ws, ws_floats, d_logits, G, d_memory, d_vecQ,
                                nullptr, stream);
}

int macx_output_backward_w(const macx_out_shapes* s, int act, float keep, uint32_t seed, const macx_out_params* P, const float* memory,
                           const float* vecQ, const float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                           const float* d_logits, const macx_out_grads* G, float* d_memory, float* d_vecQ, const uint32_t* mask_word,
                           void* stream) {
  CKI(out_check(s));
  if (!P || !memory || !vecQ || !saved || !ws || !d_logits || !G || !d_memory || !d_vecQ) return MACX_EINVAL;
  const OutLayout L = make_out(s);
  const OutBwdLayout W = make_out_bwd(s);
  if (saved_floats < L.total || ws_floats < W.total) return MACX_ESMALL;
  hipStream_t st = (hipStream_t)stream;
  const int B = s->B, d = s->d, in = 2 * d, H = s->hidden, A = s->answers, Ap = pad16(A);
  Packer pk;
  pk.add(P->outQuestion_W, 1, d, d, d, ws + W.woqT);
  pk.add(P->fc0_W, 1, H, H, in, ws + W.w0T);          // W0^T: [H] -> [2d]
  pk.add(P->fc1_W, 1, A, Ap, H, ws + W.w1T, A, H);    // W1^T: [Ap] -> [H], rows past A are zero
  CK(pk.run(st));
  const DropSpec d0 = make_drop(keep, seed, SITE_OUT_FC0, 0, mask_word), d1 = make_drop(keep, seed, SITE_OUT_FC1, 0, mask_word);
  hipLaunchKernelGGL(pad_cols_kernel, dim3(16), dim3(256), 0, st, d_logits, A, B, Ap, ws + W.dlog_pad);
  // fc_1
  hipLaunchKernelGGL(outer_sum_kernel, dim3(64), dim3(256), 0, st, saved + L.x1, H, d_logits, A, B, H, A, G->fc1_W);
  CK(rowsum(d_logits, B, A, A, G->fc1_b, st));
  LinP b1 = lin_basic(ws + W.dlog_pad, Ap, Ap, B, ws + W.w1T, nullptr, H, MACX_ACT_NON, ws + W.dx1, H);
  CK(small_linear_launch(b1, 1, st));
  // through dropout(h) and the activation: dh = dx1 * mask1 * act'(h)
  hipLaunchKernelGGL(drop2_kernel, dim3(64), dim3(256), 0, st, (const float*)(ws + W.dx1), B, H, (uint32_t)s->b0, d1, no_drop(), ws + W.dx1);
  hipLaunchKernelGGL(mul_actgrad_kernel, dim3(64), dim3(256), 0, st, (const float*)(ws + W.dx1), saved + L.h, act, (size_t)B * H, ws + W.dh);
  // fc_0
  hipLaunchKernelGGL(outer_sum_kernel, dim3(512), dim3(256), 0, st, saved + L.x0, in, (const float*)(ws + W.dh), H, B, in, H, G->fc0_W);
  CK(rowsum(ws + W.dh, B, H, H, G->fc0_b, st));
  LinP b0 = lin_basic(ws + W.dh, H, H, B, ws + W.w0T, nullptr, in, MACX_ACT_NON, ws + W.dx0, in);
  CK(small_linear_launch(b0, 1, st));
  hipLaunchKernelGGL(drop2_kernel, dim3(64), dim3(256), 0, st, (const float*)(ws + W.dx0), B, in, (uint32_t)s->b0, d0, no_drop(), ws + W.dx0);
  // split the concat gradient
  hipLaunchKernelGGL(copy_cols_drop_kernel, dim3(64), dim3(256), 0, st, (const float*)(ws + W.dx0), in, 0, B, d, 0u, no_drop(), d_memory);
  hipLaunchKernelGGL(copy_cols_drop_kernel, dim3(64), dim3(256), 0, st, (const float*)(ws + W.dx0), in, d, B, d, 0u, no_drop(), ws + W.deq);
  // outQuestion
  hipLaunchKernelGGL(outer_sum_kernel, dim3(256), dim3(256), 0, st, vecQ, d, (const float*)(ws + W.deq), d, B, d, d, G->outQuestion_W);
  CK(rowsum(ws + W.deq, B, d, d, G->outQuestion_b, st));
  LinP bq = lin_basic(ws + W.deq, d, d, B, ws + W.woqT, nullptr, d, MACX_ACT_NON, d_vecQ, d);
  CK(small_linear_launch(bq, 1, st));
  CK(hipGetLastError());
  return MACX_OK;
}

// =================================================================================================
// stem CNN (model.py:165-204, ops.CNNLayer ops.py:380-438): SURVEY 8f row 1.  Two 3x3 SAME
// convolutions as implicit GEMMs on the knowledge-base GEMM kernel (K = 9 * C_in, per-image tiles).
// =================================================================================================
namespace {
struct StemLayout {
  size_t k0_p, k1_p;     // packed HWIO kernels [9*Cin][Cmid], [9*Cmid][Cout]
  size_t in0p;           // [B][Np][Cin]   dropped, halo-padded image features
  size_t X1;             // [B][N][Cmid]   act(conv0)
  size_t in1p;           // [B][Np][Cmid]  dropped, halo-padded X1
  size_t bits1;          // [B*N*Cmid/32]  keep bits of the layer-1 input dropout
  size_t amax;           // 3h family: largest magnitudes [kernel0, kernel1, in0p, in1p] (+ 4 spare), then scratch for the absmax passes
  size_t total;
};
struct StemGeo { int N, wp, np; };
inline StemGeo stem_geo(const macx_stem_shapes* s) { return StemGeo{s->H * s->W, s->W + 2, (s->H + 2) * (s->W + 2)}; }
StemLayout make_stem(const macx_stem_shapes* s) {
  StemLayout L;
  memset(&L, 0, sizeof(L));
  const StemGeo g = stem_geo(s);
  size_t off = 0;
  auto take = [&](size_t n) { size_t r = off; off += al4(n); return r; };
  const size_t B = s->B, Ci = s->Cin, Cm = s->Cmid, Co = s->Cout;
  L.k0_p = take(wsize(9 * Ci, Cm)); L.k1_p = take(wsize(9 * Cm, Co));
  L.in0p = take(B * g.np * Ci); L.X1 = take(B * g.N * Cm); L.in1p = take(B * g.np * Cm);
  L.bits1 = take(B * g.N * Cm / 32 + 8);
  L.amax = take(8 + 4 * AMAX_BIG_BLOCKS);
  L.total = off;
  return L;
}
inline int conv_splits(int tiles, int M) {
  // fill whole rounds of 256 workgroups; fewest splits among the best fillings
  int best = 1; double beff = 0.0;
  for (int ns = 1; ns <= 16; ++ns) {
    if ((M + ns - 1) / ns < 256) break;
    const int blocks = tiles * ns;
    const double eff = (double)blocks / (double)(((blocks + 255) / 256) * 256);
    if (eff > beff + 0.02) { beff = eff; best = ns; }
  }
  return best;
}
struct StemBwdLayout {
  size_t k1T_p;          // packed backward-data weights [9*Cout][Cmid]
  size_t dY2, dY2p, dY1; // [B][N][Cout], [B][Np][Cout], [B][N][Cmid]
  size_t slab0, slab1;   // weight-gradient partial slabs
  int ns0, ns1;
  size_t amax;           // 3h family: largest magnitudes [dY2, dY1] (+ 6 spare), then scratch
  size_t total;
};
StemBwdLayout make_stem_bwd(const macx_stem_shapes* s) {
  StemBwdLayout L;
  memset(&L, 0, sizeof(L));
  const StemGeo g = stem_geo(s);
  size_t off = 0;
  auto take = [&](size_t n) { size_t r = off; off += al4(n); return r; };
  const size_t B = s->B, Ci = s->Cin, Cm = s->Cmid, Co = s->Cout;
  L.k1T_p = take(wsize(9 * Co, Cm));
  L.dY2 = take(B * g.N * Co); L.dY2p = take(B * g.np * Co); L.dY1 = take(B * g.N * Cm);
  L.ns0 = conv_splits((int)(9 * Ci / T_TILE * (Cm / T_TILE)), (int)(B * g.N));
  L.ns1 = conv_splits((int)(9 * Cm / T_TILE * (Co / T_TILE)), (int)(B * g.N));
  L.slab0 = take((size_t)L.ns0 * 9 * Ci * Cm);
  L.slab1 = take((size_t)L.ns1 * 9 * Cm * Co);
  L.amax = take(8 + 2 * AMAX_BIG_BLOCKS);
  L.total = off;
  return L;
}
int stem_check(const macx_stem_shapes* s) {
  if (!s || s->B < 1 || s->H < 1 || s->W < 2) return MACX_EINVAL;
  if (s->Cin % 128 || s->Cmid % 128 || s->Cout % 128 || s->Cin < 128 || s->Cmid < 128 || s->Cout < 128) return MACX_EINVAL;
  if (s->H * s->W > K_MAXN) return MACX_EINVAL;
  if ((size_t)(s->b0 + s->B) * s->H * s->W * (size_t)(s->Cin > s->Cmid ? s->Cin : s->Cmid) >= (1ull << 32)) return MACX_EINVAL;
  // the CONV weight-gradient kernels take the image of flattened row m as __umulhi(m, magic), magic = ceil(2^32 / N) (conv_wgrad):
  // m magic / 2^32 = m / N + m e / (N 2^32) with e = magic N - 2^32 < N, whose floor is m / N for every remainder while m e < 2^32.
  // Refuse what the largest row, B N - 1, does not satisfy (N a power of two: e = 0, never refused; the pixel's row, n < 1024
  // by W <= 1024, always satisfies it).  Conservative, and exact below the bound: tests/test_stem_geometry_host.py.
  {
    const uint64_t N = (uint64_t)s->H * s->W;
    const uint64_t e = (((1ull << 32) + N - 1) / N) * N - (1ull << 32);
    if (e && ((uint64_t)s->B * N - 1) * e >= (1ull << 32)) return MACX_EINVAL;
  }
  return MACX_OK;
}
hipError_t launch_pad_drop(const float* src, const PadP& q, float keep, uint32_t seed, uint32_t site, uint32_t first, float* dst,
                           uint32_t* bits, const uint32_t* word, hipStream_t st) {
  const DropSpec ds = make_drop(keep, seed, site, 0);
  hipLaunchKernelGGL(pad_drop_kernel, dim3(2048), dim3(256), 0, st, src, q, ds.key, ds.thr24, ds.inv_keep, first, dst, bits, word);
  return hipGetLastError();
}
void conv_gemm_params(GemmP& g, const macx_stem_shapes* s, const StemGeo& geo, const float* Apad, int cin, int nout, int sign) {
  memset(&g, 0, sizeof(g));
  g.B = s->B; g.N = geo.N; g.K = 9 * cin; g.Nout = nout;
  g.A = Apad; g.lda = cin; g.a_qstride = (size_t)geo.np * cin;
  g.conv_taps = 9; g.conv_w = s->W; g.conv_wp = geo.wp; g.conv_cin = cin; g.conv_sign = sign;
  g.ldo = nout; g.e_inv_keep = 1.0f;
}
int conv_wgrad(const macx_stem_shapes* s, const StemGeo& geo, const float* Apad, int cin, const float* G, int cout, int ns, float* slab,
               float* out, hipStream_t st, const float* a_max = nullptr, const float* g_max = nullptr) {
  TnP t;
  memset(&t, 0, sizeof(t));
  t.M = s->B * geo.N; t.Kd = 9 * cin; t.Jd = cout; t.nsplit = ns; t.rows_per_split = rows_per_split(t.M, ns);
  t.A = Apad; t.lda = cin; t.a_mod = t.M; t.G = G; t.ldg = cout;
  t.conv_taps = 9; t.conv_w = s->W; t.conv_wp = geo.wp; t.conv_cin = cin; t.conv_n = geo.N; t.conv_np = geo.np;
  t.magic_n = (uint32_t)(((1ull << 32) + geo.N - 1) / geo.N);
  t.magic_w = (uint32_t)(((1ull << 32) + s->W - 1) / s->W);
  t.part = (ns == 1) ? out : slab;
  t.a_maxabs = a_max; t.g_maxabs = g_max;
  if (a_max && g_max) CK(wgrad_fp16x2_launch(t, st));      // three fp16 terms (macx_wgrad6.hip.h)
  else CK(wgrad_any(t, st));
  if (ns > 1) CK(slab_reduce_launch(slab, ns, (size_t)t.Kd * t.Jd, out, 0, st));
  return 0;
}
}  // namespace

size_t macx_stem_saved_floats(const macx_stem_shapes* s) { return stem_check(s) ? 0 : make_stem(s).total; }
size_t macx_stem_ws_floats(const macx_stem_shapes* s) { return stem_check(s) ? 0 : make_stem_bwd(s).total; }

int macx_stem_forward(const macx_stem_shapes* s, int act, float keep, uint32_t seed, const macx_stem_params* P, const float* images,
                      float* kb, float* saved, size_t saved_floats, void* stream) {
  return macx_stem_forward_w(s, act, keep, seed, P, images, kb, saved, saved_floats, nullptr, stream);
}

int macx_stem_forward_w(const macx_stem_shapes* s, int act, float keep, uint32_t seed, const macx_stem_params* P, const float* images,
                        float* kb, float* saved, size_t saved_floats, const uint32_t* mask_word, void* stream) {
  CKI(stem_check(s));
  if (!P || !images || !kb || !saved || misaligned(images) || misaligned(kb) || misaligned(saved)) return MACX_EINVAL;
  const StemLayout L = make_stem(s);
  if (saved_floats < L.total) return MACX_ESMALL;
  hipStream_t st = (hipStream_t)stream;
  const StemGeo geo = stem_geo(s);
  const int Ci = s->Cin, Cm = s->Cmid, Co = s->Cout;
  // the default (H2) family runs the stem on three fp16 MFMA terms with one exponent per operand tensor (macx_gemm3h.hip.h);
  // the other two families keep the six-term bf16 split / the f32 MFMA
  const bool h3 = h2_mode();
  float* amax = saved + L.amax;
  Packer pk;
  if (h3) {
    CK(absmax_big(P->kernel0, (size_t)9 * Ci * Cm, amax + 0, amax + 8, st));
    CK(absmax_big(P->kernel1, (size_t)9 * Cm * Co, amax + 1, amax + 8 + AMAX_BIG_BLOCKS, st));
    pk.add(P->kernel0, Cm, 1, 9 * Ci, Cm, saved + L.k0_p, -1, -1, 3, amax + 0);
    pk.add(P->kernel1, Co, 1, 9 * Cm, Co, saved + L.k1_p, -1, -1, 3, amax + 1);
  } else {
  pk.add(P->kernel0, Cm, 1, 9 * Ci, Cm, saved + L.k0_p, -1, -1, wfmt_plain_f32ops());     // HWIO flattened = [9*Cin][Cmid] row-major
  pk.add(P->kernel1, Co, 1, 9 * Cm, Co, saved + L.k1_p, -1, -1, wfmt_plain_f32ops());
  }
  CK(pk.run(st));
  float* ascr = amax + 8 + 2 * AMAX_BIG_BLOCKS;
  PadP q0{s->B, geo.N, s->W, geo.wp, geo.np, Ci};
  PadP q1{s->B, geo.N, s->W, geo.wp, geo.np, Cm};
  // cnn_0: dropout -> conv3x3 SAME -> + b -> act   (ops.py:400-411)
  CK(launch_pad_drop(images, q0, keep, seed, SITE_STEM0, (uint32_t)((size_t)s->b0 * geo.N * Ci), saved + L.in0p, nullptr,
                     mask_word, st));
  GemmP g;
  conv_gemm_params(g, s, geo, saved + L.in0p, Ci, Cm, +1);
  g.Wp = saved + L.k0_p; g.out = saved + L.X1; g.bias = P->bias0; g.act = act;
  if (h3) {
    CK(absmax_big(saved + L.in0p, (size_t)s->B * geo.np * Ci, amax + 2, ascr, st));
    g.a_maxabs = amax + 2;
    CK((kb_gemm3h_launch<A_PLAIN, B_PLAIN, E_BIAS_ACT, false>(g, st)));
  } else
  CK((kb_gemm<A_PLAIN, B_PLAIN, E_BIAS_ACT, false>(g, st)));
  // cnn_1
  CK(launch_pad_drop(saved + L.X1, q1, keep, seed, SITE_STEM1, (uint32_t)((size_t)s->b0 * geo.N * Cm), saved + L.in1p,
                     reinterpret_cast<uint32_t*>(saved + L.bits1), mask_word, st));
  conv_gemm_params(g, s, geo, saved + L.in1p, Cm, Co, +1);
  g.Wp = saved + L.k1_p; g.out = kb; g.bias = P->bias1; g.act = act;
  if (h3) {
    CK(absmax_big(saved + L.in1p, (size_t)s->B * geo.np * Cm, amax + 3, ascr + AMAX_BIG_BLOCKS, st));
    g.a_maxabs = amax + 3;
    CK((kb_gemm3h_launch<A_PLAIN, B_PLAIN, E_BIAS_ACT, false>(g, st)));
  } else
  CK((kb_gemm<A_PLAIN, B_PLAIN, E_BIAS_ACT, false>(g, st)));
  return MACX_OK;
}

int macx_stem_backward(const macx_stem_shapes* s, int act, float keep, uint32_t seed, const macx_stem_params* P, const float* kb,
                       const float* saved, size_t saved_floats, float* ws, size_t ws_floats, const float* d_kb,
                       const macx_stem_grads* G, void* stream) {
  return macx_stem_backward_w(s, act, keep, seed, P, kb, saved, saved_floats, ws, ws_floats, d_kb, G, nullptr, stream);
}

// (the backward pass hashes nothing: layer 0's dropped input and layer 1's keep bits are in `saved`, written by the forward pass
// under its word -- mask_word is taken so that the pair of calls has one shape, and ignored)
int macx_stem_backward_w(const macx_stem_shapes* s, int act, float keep, uint32_t seed, const macx_stem_params* P, const float* kb,
                         const float* saved, size_t saved_floats, float* ws, size_t ws_floats, const float* d_kb,
                         const macx_stem_grads* G, const uint32_t* mask_word, void* stream) {
  (void)mask_word;
  CKI(stem_check(s));
  if (!P || !kb || !saved || !ws || !d_kb || !G) return MACX_EINVAL;
  const StemLayout L = make_stem(s);
  const StemBwdLayout W = make_stem_bwd(s);
  if (saved_floats < L.total || ws_floats < W.total) return MACX_ESMALL;
  hipStream_t st = (hipStream_t)stream;
  const StemGeo geo = stem_geo(s);
  const int Ci = s->Cin, Cm = s->Cmid, Co = s->Cout, M = s->B * geo.N;
  (void)seed;
  const bool h3 = h2_mode();
  const float* fmax = saved + L.amax;                    // [kernel0, kernel1, in0p, in1p] from the forward pass
  float* bmax = ws + W.amax;
  // backward-data weights of cnn_1: B[(tap, co)][ci] = K1[tap][ci][co]
  {
    Packer pk;
    for (int tap = 0; tap < 9; ++tap) {
      if (h3)      // nine per-tap transposes back to back = ONE [9 Cout][Cmid] matrix of format 3, one exponent behind the last
        pk.add(P->kernel1 + (size_t)tap * Cm * Co, 1, Co, Co, Cm, ws + W.k1T_p + (size_t)tap * Co * Cm, -1, -1, 3, fmax + 1,
               ws + W.k1T_p + (size_t)9 * Co * Cm);
      else
      pk.add(P->kernel1 + (size_t)tap * Cm * Co, 1, Co, Co, Cm, ws + W.k1T_p + (size_t)tap * (gemm_split_mode() ? wsize(Co, Cm) : (size_t)Co * Cm), -1, -1,
             wfmt_plain_f32ops());
    }
    CK(pk.run(st));
  }
  // dY2 = d_kb * act'(kb)
  PadP q2{s->B, geo.N, s->W, geo.wp, geo.np, Co};
  hipLaunchKernelGGL(pad_mul_actgrad_kernel, dim3(2048), dim3(256), 0, st, d_kb, kb, act, q2, ws + W.dY2, ws + W.dY2p);
  CK(hipGetLastError());
  CK(rowsum(ws + W.dY2, M, Co, Co, G->bias1, st));
  if (h3) CK(absmax_big(ws + W.dY2, (size_t)M * Co, bmax + 0, bmax + 8, st));
  CKI(conv_wgrad(s, geo, saved + L.in1p, Cm, ws + W.dY2, Co, W.ns1, ws + W.slab1, G->kernel1, st, h3 ? fmax + 3 : nullptr, h3 ? bmax + 0 : nullptr));
  // dY1 = convT(dY2) * dropmask1 * act'(X1): gather with the opposite tap offsets
  GemmP g;
  conv_gemm_params(g, s, geo, ws + W.dY2p, Co, Cm, -1);
  g.Wp = ws + W.k1T_p; g.out = ws + W.dY1; g.aux = saved + L.X1; g.act = act;
  if (keep < 1.0f) { g.e_bits = reinterpret_cast<const uint32_t*>(saved + L.bits1); g.e_inv_keep = 1.0f / keep; }
  if (h3) {
    g.a_maxabs = bmax + 0;                              // the padded copy holds the same values
    CK((kb_gemm3h_launch<A_PLAIN, B_PLAIN, E_MUL_DACT, false>(g, st)));
  } else
  CK((kb_gemm<A_PLAIN, B_PLAIN, E_MUL_DACT, false>(g, st)));
  CK(rowsum(ws + W.dY1, M, Cm, Cm, G->bias0, st));
  if (h3) CK(absmax_big(ws + W.dY1, (size_t)M * Cm, bmax + 1, bmax + 8 + AMAX_BIG_BLOCKS, st));
  CKI(conv_wgrad(s, geo, saved + L.in0p, Ci, ws + W.dY1, Cm, W.ns0, ws + W.slab0, G->kernel0, st, h3 ? fmax + 2 : nullptr, h3 ? bmax + 1 : nullptr));
  return MACX_OK;
}

int macx_images_to_nhwc(const float* nchw, int B, int C, int HW, float* nhwc, void* stream) {
  if (!nchw || !nhwc || B < 1 || C < 1 || HW < 1 || B > 65535) return MACX_EINVAL;
  hipLaunchKernelGGL(transpose_kernel, dim3((HW + 31) / 32, (C + 31) / 32, B), dim3(256), 0, (hipStream_t)stream, nchw, C, HW, nhwc);
  return (int)hipGetLastError();
}

// =================================================================================================
// general convolution (the generic stem's layers, ops.cnn ops.py:380-411): macx_conv.hip.h
// =================================================================================================
namespace {
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// the shapes the conv kernels take (sizes, 16-byte channel rows, 32-bit GEMM indices) -> geometry; false: MACX_EINVAL
inline bool conv_ok(const macx_conv_shapes* s, macx::ConvGeom* g) {
  if (!s || s->B < 1 || s->H < 1 || s->W < 1 || s->Cin < 4 || s->Cout < 4 || s->k < 1 || s->stride < 1) return false;
  if (s->Cin % 4 || s->Cout % 4) return false;
  if ((long long)s->B * s->H * s->W >= (1ll << 31)) return false;
  if ((long long)s->k * s->k * (s->Cin > s->Cout ? s->Cin : s->Cout) >= (1ll << 31)) return false;
  *g = macx::conv_geom(s->B, s->H, s->W, s->Cin, s->Cout, s->k, s->stride);
  return true;
}
}  // namespace

size_t macx_conv2d_ws_floats(const macx_conv_shapes* s) {
  macx::ConvGeom g;
  if (!conv_ok(s, &g)) return 0;
  int slabs = 1, span = 0;
  macx::conv_wgrad_split(g, &slabs, &span);
  return slabs > 1 ? (size_t)slabs * g.k * g.k * g.Cin * g.Cout : 0;
}

int macx_conv2d_fwd(const macx_conv_shapes* s, const float* x, const float* w, const float* bias, float* y, void* stream) {
  macx::ConvGeom g;
  if (!conv_ok(s, &g) || !x || !w || !y || !al16(x) || !al16(w) || !al16(y)) return MACX_EINVAL;
  macx::ConvArgs a{};
  a.g = g; a.a = x; a.b = w; a.bias = bias; a.out = y;
  a.M = g.B * g.Ho * g.Wo; a.N = g.Cout; a.K = g.k * g.k * g.Cin;
  a.kspan = (a.K + macx::CV_BK - 1) / macx::CV_BK * macx::CV_BK;
  CK(macx::conv_launch<macx::CV_FWD>(a, 1, (hipStream_t)stream));
  return MACX_OK;
}

int macx_conv2d_bwd_data(const macx_conv_shapes* s, const float* dy, const float* w, float* dx, void* stream) {
  macx::ConvGeom g;
  if (!conv_ok(s, &g) || !dy || !w || !dx || !al16(dy) || !al16(w) || !al16(dx)) return MACX_EINVAL;
  macx::ConvArgs a{};
  a.g = g; a.a = dy; a.b = w; a.out = dx;
  a.M = g.B * g.H * g.W; a.N = g.Cin; a.K = g.k * g.k * g.Cout;
  a.kspan = (a.K + macx::CV_BK - 1) / macx::CV_BK * macx::CV_BK;
  CK(macx::conv_launch<macx::CV_BWD>(a, 1, (hipStream_t)stream));
  return MACX_OK;
}

int macx_conv2d_wgrad(const macx_conv_shapes* s, const float* x, const float* dy, float* dw, float* ws, size_t ws_floats,
                      void* stream) {
  macx::ConvGeom g;
  if (!conv_ok(s, &g) || !x || !dy || !dw || !al16(x) || !al16(dy) || !al16(dw)) return MACX_EINVAL;
  const size_t need = macx_conv2d_ws_floats(s);
  if (need && (!ws || !al16(ws) || ws_floats < need)) return MACX_EINVAL;
  int slabs = 1, span = 0;
  macx::conv_wgrad_split(g, &slabs, &span);
  macx::ConvArgs a{};
  a.g = g; a.a = x; a.b = dy;
  a.M = g.k * g.k * g.Cin; a.N = g.Cout; a.K = g.B * g.Ho * g.Wo;
  a.kspan = span;
  const size_t n = (size_t)a.M * a.N;
  a.out = slabs > 1 ? ws : dw;
  a.slab = slabs > 1 ? n : 0;
  hipStream_t st = (hipStream_t)stream;
  CK(macx::conv_launch<macx::CV_WGRAD>(a, slabs, st));
  if (slabs > 1) {
    hipLaunchKernelGGL(macx::conv_slab_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ws, n, slabs, dw);
    CK(hipGetLastError());
  }
  return MACX_OK;
}

// =================================================================================================
// question encoder (model.py:208-307; ops.biRNNLayer ops.py:859-911): SURVEY 8f row 4
// =================================================================================================
// One implementation for every cell and direction count (macx_rnn_encoder_*); macx_encoder_* is its (LSTM, 2) case.  Per direction
// a position's columns are one row of width GT that holds the cell's matrices side by side: the LSTM's [i | j | f | o] (4h), the
// RNN's h, the GRU's gates [r | u] and candidate [c] (3h).  Zx, the kept per-step values, dG and dZ all have that row.
namespace {
inline int pad128(int n) { return (n + 127) & ~127; }
struct RnnGeom {
  int cell, dirs, nmat, GT;
  int col[2], w[2];        // matrix m: columns [col, col + w) of the row; its kernel is [E + h, w]
};
RnnGeom rnn_geom(const macx_rnn_shapes* s) {
  RnnGeom g;
  memset(&g, 0, sizeof(g));
  g.cell = s->cell; g.dirs = s->dirs; g.nmat = 1;
  if (s->cell == MACX_RNN_LSTM) g.w[0] = 4 * s->h;
  else if (s->cell == MACX_RNN_GRU) { g.nmat = 2; g.w[0] = 2 * s->h; g.col[1] = 2 * s->h; g.w[1] = s->h; }
  else g.w[0] = s->h;
  g.GT = g.col[g.nmat - 1] + g.w[g.nmat - 1];
  return g;
}
inline const float* rnn_kernel(const macx_rnn_params* P, int dir, int m) {
  return m ? (dir ? P->bw_candidate_kernel : P->fw_candidate_kernel) : (dir ? P->bw_kernel : P->fw_kernel);
}
inline const float* rnn_bias(const macx_rnn_params* P, int dir, int m) {
  return m ? (dir ? P->bw_candidate_bias : P->fw_candidate_bias) : (dir ? P->bw_bias : P->fw_bias);
}
inline float* rnn_dkernel(const macx_rnn_grads* P, int dir, int m) {
  return m ? (dir ? P->bw_candidate_kernel : P->fw_candidate_kernel) : (dir ? P->bw_kernel : P->fw_kernel);
}
inline float* rnn_dbias(const macx_rnn_grads* P, int dir, int m) {
  return m ? (dir ? P->bw_candidate_bias : P->fw_candidate_bias) : (dir ? P->bw_bias : P->fw_bias);
}
struct EncLayout {
  size_t wx_p;           // packed [dirs][Ep x GT]: matrix m's [Ep x w] pack at Ep * col
  size_t wh_p[2];        // packed [dirs][h x w] per matrix
  size_t Xp;             // [B*S][Ep]  dropped embedded words (columns E..Ep-1 zero)
  size_t Zx;             // [dirs][B*S][GT]
  size_t hs, cs;         // [dirs][S+1][B][h]  (cs: LSTM)
  size_t gates;          // [dirs][S][B][GT]   (LSTM: the gates; GRU: r | u | c)
  size_t rh;             // [dirs][S][B][h]    (GRU: r * h_prev)
  size_t total;
};
EncLayout make_enc(const macx_rnn_shapes* s) {
  EncLayout L;
  memset(&L, 0, sizeof(L));
  size_t off = 0;
  auto take = [&](size_t n) { size_t r = off; off += al4(n); return r; };
  const RnnGeom g = rnn_geom(s);
  const size_t B = s->B, S = s->S, h = s->h, Ep = pad128(s->E), G = g.GT, D = s->dirs;
  L.wx_p = take(D * Ep * G);
  for (int m = 0; m < g.nmat; ++m) L.wh_p[m] = take(D * h * g.w[m]);
  L.Xp = take(B * S * Ep); L.Zx = take(D * B * S * G);
  L.hs = take(D * (S + 1) * B * h);
  if (s->cell == MACX_RNN_LSTM) L.cs = take(D * (S + 1) * B * h);
  if (s->cell != MACX_RNN_BASIC) L.gates = take(D * S * B * G);
  if (s->cell == MACX_RNN_GRU) L.rh = take(D * S * B * h);
  L.total = off;
  return L;
}
struct EncBwdLayout {
  size_t wxT_p, whT_p[2], dG, dZ, dh, dc, dh_pass, dc2, drh, dXp, tmpW, slab, dq, total;
};
EncBwdLayout make_enc_bwd(const macx_rnn_shapes* s) {
  EncBwdLayout L;
  memset(&L, 0, sizeof(L));
  size_t off = 0;
  auto take = [&](size_t n) { size_t r = off; off += al4(n); return r; };
  const RnnGeom g = rnn_geom(s);
  const size_t B = s->B, S = s->S, h = s->h, Ep = pad128(s->E), G = g.GT, D = s->dirs;
  L.wxT_p = take(D * G * Ep);
  for (int m = 0; m < g.nmat; ++m) L.whT_p[m] = take(D * g.w[m] * h);
  L.dG = take(D * S * B * G); L.dZ = take(D * B * S * G);
  L.dh = take(D * B * h); L.dh_pass = take(D * B * h);                           // dh_pass: the second dh buffer
  if (s->cell == MACX_RNN_LSTM) { L.dc = take(D * B * h); L.dc2 = take(D * B * h); }
  if (s->cell == MACX_RNN_GRU) L.drh = take(D * B * h);
  L.dXp = take(B * S * Ep); L.tmpW = take(Ep * (size_t)g.w[0]);
  // split-reduction slabs of the kernel-gradient contractions (input block [Ep, w], recurrent block [h, w]): the largest
  {
    size_t slab = 0;
    for (int m = 0; m < g.nmat; ++m) {
      const size_t in_blk = (size_t)wgrad_splits((int)(B * S), (int)Ep, g.w[m]) * Ep * g.w[m];
      const size_t rec_blk = (size_t)wgrad_splits((int)(B * S), (int)h, g.w[m]) * h * g.w[m];
      slab = std::max(slab, std::max(in_blk, rec_blk));
    }
    L.slab = take(slab);
  }
  L.dq = take(B * D * h);
  L.total = off;
  return L;
}
constexpr size_t ENC_LDS_MAX = 160 * 1024;      // LDS of one CU (gfx950)
int rnn_check(const macx_rnn_shapes* s) {
  if (!s || s->B < 1 || s->S < 1 || s->V < 1 || s->E < 1 || s->h < 128 || s->h % 128) return MACX_EINVAL;
  if (s->cell < MACX_RNN_BASIC || s->cell > MACX_RNN_LSTM || s->dirs < 1 || s->dirs > 2) return MACX_EINVAL;
  // the LSTM's backward step keeps the gate gradients of 16 questions x 4h columns in LDS: past one CU's 160 KB (h > 512) the
  // forward pass would run and only the backward launch fail, so the shape is refused before anything is sized or launched
  // (one bound for every cell: the GRU's and the RNN's tiles are smaller)
  if (rnn_step_bwd_lds(s->h, 4) > ENC_LDS_MAX) return MACX_EUNSUPPORTED;
  return MACX_OK;
}
// a NULL pointer among those the cell and the direction count need (parameters; with Gr, their gradients as well)
bool rnn_lacks(const macx_rnn_params* P, const macx_rnn_grads* Gr, bool grads, const macx_rnn_shapes* s) {
  if (!P || !P->emb || (grads && (!Gr || !Gr->emb))) return true;
  for (int dir = 0; dir < s->dirs; ++dir)
    for (int m = 0; m < (s->cell == MACX_RNN_GRU ? 2 : 1); ++m) {
      if (!rnn_kernel(P, dir, m) || !rnn_bias(P, dir, m)) return true;
      if (grads && (!rnn_dkernel(Gr, dir, m) || !rnn_dbias(Gr, dir, m))) return true;
    }
  return false;
}

int rnn_forward(const macx_rnn_shapes* s, float keep_input, float keep_question, uint32_t seed, const macx_rnn_params* P,
                const int32_t* questions, const int32_t* lengths, float* words, float* vecQ, float* saved, size_t saved_floats,
                const uint32_t* mask_word, void* stream) {
  CKI(rnn_check(s));
  if (!P || !questions || !lengths || !words || !vecQ || !saved) return MACX_EINVAL;
  const EncLayout L = make_enc(s);
  if (saved_floats < L.total) return MACX_ESMALL;
  hipStream_t st = (hipStream_t)stream;
  const RnnGeom g = rnn_geom(s);
  const int B = s->B, S = s->S, E = s->E, h = s->h, Ep = pad128(E), G = g.GT, D = s->dirs;
  const size_t Bh = (size_t)B * h;
  Packer pk;
  for (int dir = 0; dir < D; ++dir)
    for (int m = 0; m < g.nmat; ++m) {
      const float* K = rnn_kernel(P, dir, m);      // [E + h, w]: rows [0,E) input, [E,E+h) recurrent
      const int w = g.w[m];
      pk.add(K, w, 1, Ep, w, saved + L.wx_p + (size_t)dir * Ep * G + (size_t)Ep * g.col[m], E, w);
      pk.add(K + (size_t)E * w, w, 1, h, w, saved + L.wh_p[m] + (size_t)dir * h * w);
    }
  CK(pk.run(st));
  hipLaunchKernelGGL(embed_gather_kernel, dim3(512), dim3(256), 0, st, questions, P->emb, B * S, E, Ep, (uint32_t)s->b0 * (uint32_t)S,
                     make_drop(keep_input, seed, SITE_ENC_INPUT, 0, mask_word), saved + L.Xp);
  CK(hipGetLastError());
  // input projections of every position, Zx = X Wx + b: the cell bias is added here once per position, so the per-step
  // recurrent product needs none and all directions go in one launch (the bias vectors are separate tensors)
  for (int dir = 0; dir < D; ++dir)
    for (int m = 0; m < g.nmat; ++m) {
      LinP l = lin_basic(saved + L.Xp, Ep, Ep, B * S, saved + L.wx_p + (size_t)dir * Ep * G + (size_t)Ep * g.col[m], rnn_bias(P, dir, m), g.w[m],
                         MACX_ACT_NON, saved + L.Zx + (size_t)dir * B * S * G + g.col[m], G);
      CK(small_linear_launch(l, 1, st));
    }
  CK(dev_zero(saved + L.hs, D * (size_t)(S + 1) * Bh * sizeof(float), st));
  if (s->cell == MACX_RNN_LSTM) CK(dev_zero(saved + L.cs, D * (size_t)(S + 1) * Bh * sizeof(float), st));
  CK(dev_zero(words, (size_t)B * S * D * h * sizeof(float), st));
  const dim3 grid(h / 16, (B + 15) / 16, D);
  const RnnSteps steps = rnn_steps(s->cell);
  RnnStepP c;
  c.B = B; c.S = S; c.h = h; c.dirs = D; c.GT = G; c.len = lengths;
  c.Zx = saved + L.Zx; c.hs = saved + L.hs; c.out = words;
  c.kept = s->cell != MACX_RNN_BASIC ? saved + L.gates : nullptr;
  c.rh = s->cell == MACX_RNN_GRU ? saved + L.rh : nullptr;
  c.cs = s->cell == MACX_RNN_LSTM ? saved + L.cs : nullptr;
  for (int tau = 0; tau < S; ++tau) {
    // R = h_prev Wh and the cell, all directions, one launch per time step (the GRU: gates, then candidate)
    c.tau = tau;
    for (int k = 0; k < steps.n; ++k) {
      c.Wh = saved + L.wh_p[steps.l[k].mat];
      hipLaunchKernelGGL(steps.l[k].fwd, grid, dim3(256), 0, st, c);
      CK(hipGetLastError());
    }
  }
  // vecQuestions = dropout(concat of the directions' final h)   (ops.py:905-906, model.py:292)
  for (int dir = 0; dir < D; ++dir)
    CK(dev_copy2d(vecQ + dir * h, (size_t)D * h * sizeof(float), saved + L.hs + ((size_t)dir * (S + 1) + S) * Bh,
                        (size_t)h * sizeof(float), (size_t)h * sizeof(float), B, st));
  hipLaunchKernelGGL(drop2_kernel, dim3(64), dim3(256), 0, st, (const float*)vecQ, B, D * h, (uint32_t)s->b0,
                     make_drop(keep_question, seed, SITE_QUESTION, 0, mask_word), no_drop(), vecQ);
  CK(hipGetLastError());
  return MACX_OK;
}

int rnn_backward(const macx_rnn_shapes* s, float keep_input, float keep_question, uint32_t seed, const macx_rnn_params* P,
                 const int32_t* questions, const int32_t* lengths, const float* saved, size_t saved_floats, float* ws,
                 size_t ws_floats, const float* d_words, const float* d_vecQ, const macx_rnn_grads* Gr,
                 const uint32_t* mask_word, void* stream) {
  CKI(rnn_check(s));
  if (!P || !questions || !lengths || !saved || !ws || !d_words || !d_vecQ || !Gr) return MACX_EINVAL;
  const EncLayout L = make_enc(s);
  const EncBwdLayout W = make_enc_bwd(s);
  if (saved_floats < L.total || ws_floats < W.total) return MACX_ESMALL;
  hipStream_t st = (hipStream_t)stream;
  const RnnGeom g = rnn_geom(s);
  const int B = s->B, S = s->S, E = s->E, h = s->h, Ep = pad128(E), G = g.GT, D = s->dirs;
  const size_t Bh = (size_t)B * h;
  Packer pk;
  for (int dir = 0; dir < D; ++dir)
    for (int m = 0; m < g.nmat; ++m) {
      const float* K = rnn_kernel(P, dir, m);
      const int w = g.w[m];
      // Wx^T: [w] -> [Ep], columns >= E zero; the matrices' packs stack along k into one [GT] -> [Ep] weight per direction
      pk.add(K, 1, w, w, Ep, ws + W.wxT_p + (size_t)dir * G * Ep + (size_t)g.col[m] * Ep, w, E);
      pk.add(K + (size_t)E * w, 1, w, w, h, ws + W.whT_p[m] + (size_t)dir * w * h);   // Wh^T: [w] -> [h]
    }
  CK(pk.run(st));
  CK(dev_zero(ws + W.dZ, D * (size_t)B * S * G * sizeof(float), st));
  if (s->cell == MACX_RNN_LSTM) CK(dev_zero(ws + W.dc, D * Bh * sizeof(float), st));
  // d(final states) = d_vecQ through the question dropout, split per direction
  hipLaunchKernelGGL(drop2_kernel, dim3(64), dim3(256), 0, st, d_vecQ, B, D * h, (uint32_t)s->b0,
                     make_drop(keep_question, seed, SITE_QUESTION, 0, mask_word), no_drop(), ws + W.dq);
  for (int dir = 0; dir < D; ++dir)
    CK(dev_copy2d(ws + W.dh + (size_t)dir * Bh, (size_t)h * sizeof(float), ws + W.dq + dir * h, (size_t)D * h * sizeof(float),
                        (size_t)h * sizeof(float), B, st));
  {
    const dim3 grid(h / 16, (B + 15) / 16, D);
    const RnnSteps steps = rnn_steps(s->cell);
    for (int k = 0; k < steps.n; ++k)
      CK(lds_attr_once(reinterpret_cast<const void*>(steps.l[k].bwd), rnn_step_bwd_lds(h, steps.l[k].gates)));
    // the running dh / dc alternate between two buffers (a workgroup reads what its neighbours would otherwise overwrite)
    float* dhb[2] = {ws + W.dh, ws + W.dh_pass};
    float* dcb[2] = {ws + W.dc, ws + W.dc2};
    const bool lstm = s->cell == MACX_RNN_LSTM;
    RnnStepBwdP c;
    c.B = B; c.S = S; c.h = h; c.dirs = D; c.GT = G; c.len = lengths;
    c.hs = saved + L.hs; c.dout = d_words; c.dG = ws + W.dG; c.dZ = ws + W.dZ;
    c.kept = s->cell != MACX_RNN_BASIC ? saved + L.gates : nullptr;
    c.drh = s->cell == MACX_RNN_GRU ? ws + W.drh : nullptr;
    c.cs = lstm ? saved + L.cs : nullptr;
    int cur = 0;
    for (int tau = S - 1; tau >= 0; --tau, cur ^= 1) {
      c.tau = tau;
      c.dh_in = dhb[cur]; c.dh_out = dhb[cur ^ 1];
      c.dc_in = lstm ? dcb[cur] : nullptr; c.dc_out = lstm ? dcb[cur ^ 1] : nullptr;
      // last to first: the GRU's d(r h) of all units before its gates' backward, which needs it across the workgroups' unit split
      for (int k = steps.n - 1; k >= 0; --k) {
        c.WT = ws + W.whT_p[steps.l[k].mat];
        hipLaunchKernelGGL(steps.l[k].bwd, grid, dim3(RSB_THREADS), rnn_step_bwd_lds(h, steps.l[k].gates), st, c);
        CK(hipGetLastError());
      }
    }
  }
  for (int dir = 0; dir < D; ++dir)
    for (int m = 0; m < g.nmat; ++m) {
      float* dK = rnn_dkernel(Gr, dir, m);
      const int w = g.w[m];
      const float* dZm = ws + W.dZ + (size_t)dir * B * S * G + g.col[m];
      const float* dGm = ws + W.dG + (size_t)dir * S * B * G + g.col[m];
      // input block of the kernel: X^T dZ (rows [0,E) of the padded product)
      CKI(wgrad_impl(saved + L.Xp, Ep, dZm, G, B * S, Ep, w, ws + W.tmpW, ws + W.slab, st));
      CK(dev_copy(dK, ws + W.tmpW, (size_t)E * w * sizeof(float), st));
      // recurrent block: sum_tau h_prev(tau)^T dG_tau (the GRU's candidate: (r h_prev)^T)  -- one contraction over S*B rows
      const float* A = m ? saved + L.rh + (size_t)dir * S * Bh : saved + L.hs + (size_t)dir * (S + 1) * Bh;
      CKI(wgrad_impl(A, h, dGm, G, S * B, h, w, dK + (size_t)E * w, ws + W.slab, st));
      CK(rowsum(dGm, S * B, w, G, rnn_dbias(Gr, dir, m), st));
    }
  // d(embedded words) = [dZ_fw | dZ_bw] [Wx_fw^T ; Wx_bw^T], then through the input dropout into the embedding rows
  {
    LinP l = lin_basic(ws + W.dZ, G, G, B * S, ws + W.wxT_p, nullptr, Ep, MACX_ACT_NON, ws + W.dXp, Ep);
    if (D == 2) {
      l.seg[1] = LinSeg{ws + W.dZ + (size_t)B * S * G, G, G, 0};
      l.Ktot = 2 * G;
    }
    CK(small_linear_launch(l, 1, st));
  }
  hipLaunchKernelGGL(embed_grad_kernel, dim3(s->V, (E + 1023) / 1024), dim3(256), 0, st, questions, (const float*)(ws + W.dXp), B * S, E, Ep,
                     (uint32_t)s->b0 * (uint32_t)S, make_drop(keep_input, seed, SITE_ENC_INPUT, 0, mask_word), Gr->emb);
  CK(hipGetLastError());
  return MACX_OK;
}

// macx_encoder_* is the bidirectional LSTM of the general implementation: the launches, their order and arguments of before
inline macx_rnn_shapes enc_as_rnn(const macx_enc_shapes* s) {
  return macx_rnn_shapes{s->B, s->S, s->V, s->E, s->h, s->b0, MACX_RNN_LSTM, 2};
}
}  // namespace

size_t macx_rnn_encoder_saved_floats(const macx_rnn_shapes* s) { return rnn_check(s) ? 0 : make_enc(s).total; }
size_t macx_rnn_encoder_ws_floats(const macx_rnn_shapes* s) { return rnn_check(s) ? 0 : make_enc_bwd(s).total; }

int macx_rnn_encoder_forward_w(const macx_rnn_shapes* s, float keep_input, float keep_question, uint32_t seed, const macx_rnn_params* P,
                               const int32_t* questions, const int32_t* lengths, float* words, float* vecQ, float* saved,
                               size_t saved_floats, const uint32_t* mask_word, void* stream) {
  CKI(rnn_check(s));
  if (rnn_lacks(P, nullptr, false, s)) return MACX_EINVAL;
  return rnn_forward(s, keep_input, keep_question, seed, P, questions, lengths, words, vecQ, saved, saved_floats, mask_word, stream);
}

int macx_rnn_encoder_backward_w(const macx_rnn_shapes* s, float keep_input, float keep_question, uint32_t seed, const macx_rnn_params* P,
                                const int32_t* questions, const int32_t* lengths, const float* saved, size_t saved_floats, float* ws,
                                size_t ws_floats, const float* d_words, const float* d_vecQ, const macx_rnn_grads* Gr,
                                const uint32_t* mask_word, void* stream) {
  CKI(rnn_check(s));
  if (rnn_lacks(P, Gr, true, s)) return MACX_EINVAL;
  return rnn_backward(s, keep_input, keep_question, seed, P, questions, lengths, saved, saved_floats, ws, ws_floats, d_words, d_vecQ, Gr,
                      mask_word, stream);
}

size_t macx_encoder_saved_floats(const macx_enc_shapes* s) {
  if (!s) return 0;
  const macx_rnn_shapes r = enc_as_rnn(s);
  return macx_rnn_encoder_saved_floats(&r);
}
size_t macx_encoder_ws_floats(const macx_enc_shapes* s) {
  if (!s) return 0;
  const macx_rnn_shapes r = enc_as_rnn(s);
  return macx_rnn_encoder_ws_floats(&r);
}

int macx_encoder_forward(const macx_enc_shapes* s, float keep_input, float keep_question, uint32_t seed, const macx_enc_params* P,
                         const int32_t* questions, const int32_t* lengths, float* words, float* vecQ, float* saved,
                         size_t saved_floats, void* stream) {
  return macx_encoder_forward_w(s, keep_input, keep_question, seed, P, questions, lengths, words, vecQ, saved, saved_floats, nullptr, stream);
}

int macx_encoder_forward_w(const macx_enc_shapes* s, float keep_input, float keep_question, uint32_t seed, const macx_enc_params* P,
                           const int32_t* questions, const int32_t* lengths, float* words, float* vecQ, float* saved,
                           size_t saved_floats, const uint32_t* mask_word, void* stream) {
  if (!s) return MACX_EINVAL;
  const macx_rnn_shapes r = enc_as_rnn(s);
  CKI(rnn_check(&r));
  if (!P) return MACX_EINVAL;
  const macx_rnn_params RP = {P->emb, P->fw_kernel, P->fw_bias, P->bw_kernel, P->bw_bias, nullptr, nullptr, nullptr, nullptr};
  return rnn_forward(&r, keep_input, keep_question, seed, &RP, questions, lengths, words, vecQ, saved, saved_floats, mask_word, stream);
}

int macx_encoder_backward(const macx_enc_shapes* s, float keep_input, float keep_question, uint32_t seed, const macx_enc_params* P,
                          const int32_t* questions, const int32_t* lengths, const float* saved, size_t saved_floats, float* ws,
                          size_t ws_floats, const float* d_words, const float* d_vecQ, const macx_enc_grads* Gr, void* stream) {
  return macx_encoder_backward_w(s, keep_input, keep_question, seed, P, questions, lengths, saved, saved_floats, ws, ws_floats, d_words,
                                 d_vecQ, Gr, nullptr, stream);
}

int macx_encoder_backward_w(const macx_enc_shapes* s, float keep_input, float keep_question, uint32_t seed, const macx_enc_params* P,
                            const int32_t* questions, const int32_t* lengths, const float* saved, size_t saved_floats, float* ws,
                            size_t ws_floats, const float* d_words, const float* d_vecQ, const macx_enc_grads* Gr,
                            const uint32_t* mask_word, void* stream) {
  if (!s) return MACX_EINVAL;
  const macx_rnn_shapes r = enc_as_rnn(s);
  CKI(rnn_check(&r));
  if (!P || !Gr) return MACX_EINVAL;
  const macx_rnn_params RP = {P->emb, P->fw_kernel, P->fw_bias, P->bw_kernel, P->bw_bias, nullptr, nullptr, nullptr, nullptr};
  const macx_rnn_grads RG = {Gr->emb, Gr->fw_kernel, Gr->fw_bias, Gr->bw_kernel, Gr->bw_bias, nullptr, nullptr, nullptr, nullptr};
  return rnn_backward(&r, keep_input, keep_question, seed, &RP, questions, lengths, saved, saved_floats, ws, ws_floats, d_words, d_vecQ, &RG,
                      mask_word, stream);
}

// =================================================================================================
// optimizer step (model.py:615-669): SURVEY 8f row 3
// =================================================================================================
namespace {
// lr_t_dev null: the by-value rate `lr_t`; else the kernel reads the rate from device memory when it runs
// guard null: the plain update kernel; else the guarded one (skip_above, guard: see opt_apply_guarded_kernel)
int adam_ema_launch(size_t n, float* params, const float* grads, float* m, float* v, float* ema, float lr_t, const float* lr_t_dev,
                    float beta1, float beta2, float eps, float clip_norm, float ema_decay, float* ws, float* norm_out, void* stream,
                    float skip_above = 0.f, uint32_t* guard = nullptr) {
  hipStream_t st = (hipStream_t)stream;
  int blocks = (int)((n + 255) / 256);
  if (blocks > OPT_BLOCKS) blocks = OPT_BLOCKS;
  hipLaunchKernelGGL(opt_sumsq_kernel, dim3(blocks), dim3(256), 0, st, grads, n, ws);
  OptP q;
  q.n = n; q.p = params; q.g = grads; q.m = m; q.v = v; q.ema = ema;
  q.lr_t = lr_t; q.lr_t_dev = lr_t_dev;
  q.beta1 = beta1; q.beta2 = beta2; q.eps = eps; q.clip = clip_norm; q.ema_decay = ema_decay;
  q.part = ws; q.nparts = blocks; q.norm_out = norm_out;
  if (guard) hipLaunchKernelGGL(opt_apply_guarded_kernel, dim3(blocks), dim3(256), 0, st, q, skip_above, guard);
  else hipLaunchKernelGGL(opt_apply_kernel, dim3(blocks), dim3(256), 0, st, q);
  CK(hipGetLastError());
  return MACX_OK;
}
// what the guarded exports check on top of their namesakes (skip_above: 0 = no threshold; !(x >= 0) also catches NaN)
bool guard_args_bad(float skip_above, const uint32_t* guard) { return !guard || ((uintptr_t)guard & 3) || !(skip_above >= 0.f); }
}  // namespace

int macx_adam_ema_step(size_t n, float* params, const float* grads, float* m, float* v, float* ema, float lr, float beta1,
                       float beta2, float eps, int step, float clip_norm, float ema_decay, float* ws, float* norm_out,
                       void* stream) {
  if (!params || !grads || !m || !v || !ws || n == 0 || step < 1) return MACX_EINVAL;
  if (ema_decay >= 0.f && !ema) return MACX_EINVAL;
  // tf.train.AdamOptimizer: lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t)
  const float lr_t = (float)((double)lr * sqrt(1.0 - pow((double)beta2, step)) / (1.0 - pow((double)beta1, step)));
  return adam_ema_launch(n, params, grads, m, v, ema, lr_t, nullptr, beta1, beta2, eps, clip_norm, ema_decay, ws, norm_out, stream);
}

int macx_adam_ema_step_p(size_t n, float* params, const float* grads, float* m, float* v, float* ema, const float* lr_t_dev,
                         float beta1, float beta2, float eps, float clip_norm, float ema_decay, float* ws, float* norm_out,
                         void* stream) {
  if (!params || !grads || !m || !v || !ws || !lr_t_dev || n == 0) return MACX_EINVAL;
  if (ema_decay >= 0.f && !ema) return MACX_EINVAL;
  return adam_ema_launch(n, params, grads, m, v, ema, 0.f, lr_t_dev, beta1, beta2, eps, clip_norm, ema_decay, ws, norm_out, stream);
}

int macx_adam_ema_step_g(size_t n, float* params, const float* grads, float* m, float* v, float* ema, float lr, float beta1,
                         float beta2, float eps, int step, float clip_norm, float ema_decay, float skip_above, uint32_t* guard,
                         float* ws, float* norm_out, void* stream) {
  if (!params || !grads || !m || !v || !ws || n == 0 || step < 1) return MACX_EINVAL;
  if (ema_decay >= 0.f && !ema) return MACX_EINVAL;
  if (guard_args_bad(skip_above, guard)) return MACX_EINVAL;
  const float lr_t = (float)((double)lr * sqrt(1.0 - pow((double)beta2, step)) / (1.0 - pow((double)beta1, step)));
  return adam_ema_launch(n, params, grads, m, v, ema, lr_t, nullptr, beta1, beta2, eps, clip_norm, ema_decay, ws, norm_out, stream,
                         skip_above, guard);
}

int macx_adam_ema_step_pg(size_t n, float* params, const float* grads, float* m, float* v, float* ema, const float* lr_t_dev,
                          float beta1, float beta2, float eps, float clip_norm, float ema_decay, float skip_above, uint32_t* guard,
                          float* ws, float* norm_out, void* stream) {
  if (!params || !grads || !m || !v || !ws || !lr_t_dev || n == 0) return MACX_EINVAL;
  if (ema_decay >= 0.f && !ema) return MACX_EINVAL;
  if (guard_args_bad(skip_above, guard)) return MACX_EINVAL;
  return adam_ema_launch(n, params, grads, m, v, ema, 0.f, lr_t_dev, beta1, beta2, eps, clip_norm, ema_decay, ws, norm_out, stream,
                         skip_above, guard);
}

int macx_gather_flat(const macx_gather_entry* table_dev, int entries, float* flat, void* stream) {
  static_assert(sizeof(macx_gather_entry) == sizeof(GatherEntry) && sizeof(GatherEntry) == 24, "gather table entry layout");
  if (!table_dev || !flat || entries < 0 || ((uintptr_t)table_dev & 7) || ((uintptr_t)flat & 3)) return MACX_EINVAL;
  if (entries == 0) return MACX_OK;
  hipLaunchKernelGGL(gather_flat_kernel, dim3(GATHER_BLOCKS), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const GatherEntry*>(table_dev), entries, flat);
  CK(hipGetLastError());
  return MACX_OK;
}

int macx_kb_gather(const float* kb_images, const int32_t* image_index, int G, int B, int N, int d, float* kb, void* stream) {
  if (!kb_images || !image_index || !kb || G < 1 || B < 1 || N < 1 || d < 1 || ((size_t)N * d) % 4) return MACX_EINVAL;
  if (misaligned(kb_images) || misaligned(kb) || ((uintptr_t)image_index & 3)) return MACX_EINVAL;
  const size_t quads = (size_t)N * d / 4;
  hipLaunchKernelGGL(kb_gather_kernel, kbg_grid(quads, KBG_CHUNK, B), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const f32x4*>(kb_images), image_index, G, B, quads, reinterpret_cast<f32x4*>(kb));
  CK(hipGetLastError());
  return MACX_OK;
}

int macx_kb_gather_bwd(const float* dkb, const int32_t* image_index, int G, int B, int N, int d, float* dkb_images, void* stream) {
  if (!dkb || !image_index || !dkb_images || G < 1 || B < 1 || N < 1 || d < 1 || ((size_t)N * d) % 4) return MACX_EINVAL;
  if (misaligned(dkb) || misaligned(dkb_images) || ((uintptr_t)image_index & 3)) return MACX_EINVAL;
  const size_t quads = (size_t)N * d / 4;
  hipLaunchKernelGGL(kb_gather_bwd_kernel, kbg_grid(quads, 256, G), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const f32x4*>(dkb), image_index, G, B, quads, reinterpret_cast<f32x4*>(dkb_images));
  CK(hipGetLastError());
  return MACX_OK;
}

int macx_kb_gather_l(const float* kb_images, const int32_t* image_index, const int32_t* image_lengths, int G, int B, int N, int d,
                     float* kb, int32_t* kb_lengths_out, void* stream) {
  if (!image_lengths) return macx_kb_gather(kb_images, image_index, G, B, N, d, kb, stream);
  if (!kb_images || !image_index || !kb || !kb_lengths_out || G < 1 || B < 1 || N < 1 || d < 1 || d % 4) return MACX_EINVAL;
  if (misaligned(kb_images) || misaligned(kb)) return MACX_EINVAL;
  if (((uintptr_t)image_index | (uintptr_t)image_lengths | (uintptr_t)kb_lengths_out) & 3) return MACX_EINVAL;
  const size_t quads = (size_t)N * d / 4;
  hipLaunchKernelGGL(kb_gather_l_kernel, kbg_grid(quads, KBG_CHUNK, B), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const f32x4*>(kb_images), image_index, image_lengths, G, B, N, (size_t)d / 4,
                     reinterpret_cast<f32x4*>(kb), kb_lengths_out);
  CK(hipGetLastError());
  return MACX_OK;
}

int macx_kb_gather_bwd_l(const float* dkb, const int32_t* image_index, const int32_t* image_lengths, int G, int B, int N, int d,
                         float* dkb_images, void* stream) {
  if (!image_lengths) return macx_kb_gather_bwd(dkb, image_index, G, B, N, d, dkb_images, stream);
  if (!dkb || !image_index || !dkb_images || G < 1 || B < 1 || N < 1 || d < 1 || d % 4) return MACX_EINVAL;
  if (misaligned(dkb) || misaligned(dkb_images) || (((uintptr_t)image_index | (uintptr_t)image_lengths) & 3)) return MACX_EINVAL;
  const size_t quads = (size_t)N * d / 4;
  hipLaunchKernelGGL(kb_gather_bwd_l_kernel, kbg_grid(quads, 256, G), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<const f32x4*>(dkb), image_index, image_lengths, G, B, N, (size_t)d / 4,
                     reinterpret_cast<f32x4*>(dkb_images));
  CK(hipGetLastError());
  return MACX_OK;
}

// ---- image features resident in device memory (macx_features.hip.h) ----
namespace {
// what both calls refuse before anything else: sizes, dtype, the quad rule, rows < 2^31 (row0 and rows travel as size_t: a negative
// 64-bit value arrives as 2^63 or more and fails the range test)
inline bool features_ok(int C, int HW, int dtype, size_t rows) {
  return C >= 1 && HW >= 1 && (dtype == MACX_FEATURES_F32 || dtype == MACX_FEATURES_F16) && ((size_t)C * HW) % 4 == 0 && rows >= 1 &&
         rows < ((size_t)1 << 31);
}
}  // namespace

int macx_features_pack(const float* src, int layout, int n, int C, int HW, void* table, int dtype, size_t row0, size_t rows,
                       int32_t* overflow, void* stream) {
  if (!src || !table || n < 1 || (layout != 0 && layout != 1) || !features_ok(C, HW, dtype, rows)) return MACX_EINVAL;
  if (row0 > rows || (size_t)n > rows - row0) return MACX_EINVAL;
  if (misaligned(src) || misaligned(table) || ((uintptr_t)overflow & 3)) return MACX_EINVAL;
  if (((size_t)C + FT_TILE - 1) / FT_TILE > 65535 || HW > 0x7FFFFFFF - FT_TILE) return MACX_EINVAL;   // (grid y; int tile edges)
  const hipStream_t st = (hipStream_t)stream;
  if (dtype == MACX_FEATURES_F16)
    CK(feat_pack_launch(src, layout, n, C, HW, reinterpret_cast<_Float16*>(table), row0, overflow, st));
  else
    CK(feat_pack_launch(src, layout, n, C, HW, reinterpret_cast<float*>(table), row0, overflow, st));
  return MACX_OK;
}

int macx_features_gather(const void* table, int dtype, size_t rows, const int32_t* ids, int G, int C, int HW, float* out, void* stream) {
  if (!table || !ids || !out || G < 1 || !features_ok(C, HW, dtype, rows)) return MACX_EINVAL;
  if (misaligned(table) || misaligned(out) || ((uintptr_t)ids & 3)) return MACX_EINVAL;
  const size_t image = (size_t)C * HW;
  const hipStream_t st = (hipStream_t)stream;
  if (dtype == MACX_FEATURES_F32) {                      // the copy macx_kb_gather launches: table rows are its images
    const size_t quads = image / 4;
    hipLaunchKernelGGL(kb_gather_kernel, kbg_grid(quads, KBG_CHUNK, G), dim3(256), 0, st, reinterpret_cast<const f32x4*>(table), ids,
                       (int)rows, G, quads, reinterpret_cast<f32x4*>(out));
  } else if (image % 8 == 0) {
    hipLaunchKernelGGL(feat_gather_h_kernel<2>, kbg_grid(image / 8, FT_CHUNK, G), dim3(256), 0, st,
                       reinterpret_cast<const _Float16*>(table), ids, (int)rows, G, image / 8, reinterpret_cast<f32x4*>(out));
  } else {
    hipLaunchKernelGGL(feat_gather_h_kernel<1>, kbg_grid(image / 4, FT_CHUNK, G), dim3(256), 0, st,
                       reinterpret_cast<const _Float16*>(table), ids, (int)rows, G, image / 4, reinterpret_cast<f32x4*>(out));
  }
  CK(hipGetLastError());
  return MACX_OK;
}

// ---- questions resident in device memory (macx_questions.hip.h) ----
int macx_questions_gather(const int32_t* q_words, const int32_t* q_lengths, const int32_t* q_answers, const int32_t* q_images,
                          const int32_t* q_kb_len, const float* q_weights, int Q, int S_tab, const int32_t* ids, int B, int S,
                          int32_t* questions, int32_t* lengths, int32_t* answers, int32_t* image_ids, int32_t* kb_lengths, float* weights,
                          int32_t* image_index, int G, int32_t* bad, void* stream) {
  if (!q_words || !q_lengths || !ids || !questions || !lengths) return MACX_EINVAL;
  if (Q < 1 || S_tab < 1 || B < 1 || S < S_tab || (size_t)Q >= ((size_t)1 << 31)) return MACX_EINVAL;
  // an output column needs its table (weights alone has a default: ones)
  if ((answers && !q_answers) || (image_ids && !q_images) || (kb_lengths && !q_kb_len)) return MACX_EINVAL;
  if (image_index && (!q_images || !image_ids || G < 1 || B > QG_MAX_GROUP_B)) return MACX_EINVAL;
  const uintptr_t all = (uintptr_t)q_words | (uintptr_t)q_lengths | (uintptr_t)q_answers | (uintptr_t)q_images | (uintptr_t)q_kb_len |
                        (uintptr_t)q_weights | (uintptr_t)ids | (uintptr_t)questions | (uintptr_t)lengths | (uintptr_t)answers |
                        (uintptr_t)image_ids | (uintptr_t)kb_lengths | (uintptr_t)weights | (uintptr_t)image_index | (uintptr_t)bad;
  if (all & 3) return MACX_EINVAL;
  QuestionsP a{q_words, q_lengths, q_answers, q_images, q_kb_len, q_weights, Q, S_tab, ids, B, S, questions, lengths, answers, image_ids,
               kb_lengths, weights, image_index, G, bad};
  // the widest access both row pitches and both base pointers allow; a narrower path serves what a wider one cannot
  const uintptr_t rows = (uintptr_t)q_words | (uintptr_t)questions;
  const hipStream_t st = (hipStream_t)stream;
  if (S_tab % 4 == 0 && S % 4 == 0 && !(rows & 15)) CK(questions_gather_launch<4>(a, st));
  else if (S_tab % 2 == 0 && S % 2 == 0 && !(rows & 7)) CK(questions_gather_launch<2>(a, st));
  else CK(questions_gather_launch<1>(a, st));
  return MACX_OK;
}

int macx_preds_scatter(const int32_t* pred, const int32_t* ids, int B, int Q, int32_t* table, void* stream) {
  if (!pred || !ids || !table || B < 1 || Q < 1) return MACX_EINVAL;
  if (((uintptr_t)pred | (uintptr_t)ids | (uintptr_t)table) & 3) return MACX_EINVAL;
  hipLaunchKernelGGL(preds_scatter_kernel, dim3(qg_blocks((size_t)B)), dim3(256), 0, (hipStream_t)stream, pred, ids, B, Q, table);
  CK(hipGetLastError());
  return MACX_OK;
}

// ---- evaluation records resident in device memory (macx_records.hip.h) ----
int macx_records_scatter(const macx_record_desc* descs, int count, const int32_t* ids, int B, int Q, void* stream) {
  if (!descs || !ids || count < 1 || count > MACX_RECORDS_MAX || B < 1 || Q < 1 || (size_t)Q >= ((size_t)1 << 31)) return MACX_EINVAL;
  if ((uintptr_t)ids & 3) return MACX_EINVAL;
  RecordList L{};
  size_t units = 0;
  for (int k = 0; k < count; ++k) {                      // every descriptor is checked before anything is launched
    const macx_record_desc& d = descs[k];
    if (!d.src || !d.table || d.steps < 1 || d.n < 1 || (d.dtype != MACX_FEATURES_F32 && d.dtype != MACX_FEATURES_F16)) return MACX_EINVAL;
    const uintptr_t esize = d.dtype == MACX_FEATURES_F16 ? 2 : 4, s = (uintptr_t)d.src, t = (uintptr_t)d.table;
    if ((s & 3) || (t & (esize - 1))) return MACX_EINVAL;
    // the widest access n and both base pointers allow; a narrower path serves what a wider one cannot
    const int vec = (d.n % 4 == 0 && !(s & 15) && !(t & (4 * esize - 1))) ? 4 : (d.n % 2 == 0 && !(s & 7) && !(t & (2 * esize - 1))) ? 2 : 1;
    L.d[k] = RecordDesc{d.src, d.table, d.steps, d.n, d.dtype, vec};
    const size_t u = (size_t)d.steps * (size_t)B;
    units = u > units ? u : units;
  }
  const size_t blocks = (units + 3) / 4;                 // one wave per row unit, four waves a workgroup
  const dim3 grid((unsigned)(blocks < (size_t)REC_MAX_BLOCKS ? blocks : (size_t)REC_MAX_BLOCKS), (unsigned)count);
  hipLaunchKernelGGL(records_scatter_kernel, grid, dim3(256), 0, (hipStream_t)stream, L, ids, B, Q);
  CK(hipGetLastError());
  return MACX_OK;
}

/* test/tuning hook: key 0 = waves per workgroup of the kb GEMM (4 or 8) */
int macx_gemm_mode(int mode) {
  if (mode == MACX_GEMM_NATIVE || mode == MACX_GEMM_SPLIT || mode == MACX_GEMM_H2) gemm_default_mode() = mode;
  return gemm_split_mode();
}

size_t macx_h2_floats(size_t rows, size_t cols) { return (cols % 128) ? 0 : al4(h2_floats(rows, cols)); }

int macx_h2_from_f32(const float* src, int B, int N, int C, float* h2, void* stream) {
  if (!src || !h2 || B < 1 || N < 1 || C < 128 || C % 128 || misaligned(src) || misaligned(h2)) return MACX_EINVAL;
  H2FromP f;
  memset(&f, 0, sizeof(f));
  f.src = src; f.B = B; f.N = N; f.C = C; f.out = h2_view(h2, B * N, C);
  f.thr24 = 1u << 24; f.inv_keep = 1.0f; f.thr24_2 = 1u << 24;
  CK(h2_from_f32(f, (hipStream_t)stream));
  return MACX_OK;
}

int macx_h2_to_f32(const float* h2, int rows, int C, float* out, void* stream) {
  if (!h2 || !out || rows < 1 || C < 128 || C % 128) return MACX_EINVAL;
  hipLaunchKernelGGL(h2_to_f32_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, h2_view(h2, rows, C), out);
  CK(hipGetLastError());
  return MACX_OK;
}

int macx_h2_pack_weight(const float* Wm, int K, int n_out, int transpose, float* out, void* stream) {
  if (!Wm || !out || K < 128 || K % 128 || n_out < 128 || n_out % 128 || misaligned(Wm) || misaligned(out)) return MACX_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  float* wmax = out + al4((size_t)K * n_out + 4);
  CK(absmax4(Wm, (size_t)K * n_out, Wm, 1, Wm, 1, Wm, 1, wmax, nullptr, st));
  Packer pk;
  if (transpose) pk.add(Wm, 1, K, K, n_out, out, -1, -1, 3, wmax);
  else pk.add(Wm, n_out, 1, K, n_out, out, -1, -1, 3, wmax);
  CK(pk.run(st));
  return MACX_OK;
}

int macx_h2_gemm_planes(const float* hA, int B, int N, int K, const float* Wh, int n_out, const float* bias, int act, float* hO,
                        void* stream) {
  if (!hA || !Wh || !bias || !hO || B < 1 || N < 1 || N > K_MAXN || K < 128 || K % 128 || n_out < 128 || n_out % 128)
    return MACX_EINVAL;
  GemmH2P g;
  memset(&g, 0, sizeof(g));
  g.B = B; g.N = N; g.K = K; g.Nout = n_out;
  g.A = h2_view(hA, B * N, K);
  set_h2_weight(g, Wh, (size_t)K * n_out);
  g.out = h2_view(hO, B * N, n_out); g.bias = bias; g.act = act; g.e_inv_keep = 1.0f;
  g.dbg = kb_gemm_dbg();
  static const int reps = getenv("MACX_H2_DEBUG_REPS") ? atoi(getenv("MACX_H2_DEBUG_REPS")) : 1;   // timing aid (tools/h2_gemm_time.py)
  for (int r = 0; r < reps; ++r) CK((kb_gemm_h2_launch<B_PLAIN, E_BIAS_ACT, false>(g, (hipStream_t)stream)));
  return MACX_OK;
}

int macx_h2_gemm(const float* A, int B, int N, int K, const float* Wm, int n_out, const float* bias, int act, float* out,
                 float* ws, size_t ws_floats, void* stream) {
  if (!A || !Wm || !bias || !out || !ws || B < 1 || N < 1 || N > K_MAXN || K < 128 || K % 128 || n_out < 128 || n_out % 128)
    return MACX_EINVAL;
  const size_t fa = al4(h2_floats((size_t)B * N, K)), fo = al4(h2_floats((size_t)B * N, n_out));
  const size_t fw = al4((size_t)K * n_out + 4);
  if (ws_floats < fa + fo + fw + 8) return MACX_ESMALL;
  float* hA = ws; float* hO = ws + fa; float* wp = hO + fo;
  CKI(macx_h2_from_f32(A, B, N, K, hA, stream));
  CKI(macx_h2_pack_weight(Wm, K, n_out, 0, wp, stream));
  CKI(macx_h2_gemm_planes(hA, B, N, K, wp, n_out, bias, act, hO, stream));
  return macx_h2_to_f32(hO, B * N, n_out, out, stream);
}

size_t macx_h2_wgrad_ws_floats(const macx_opts* o, int nt, int R, int Kd, int Jd, int nsplit, int pair) {
  if (o && o->abi_version != MACX_ABI_VERSION) return 0;
  H2Scope sc(o);
  H2WgradWs w;
  return h2_wgrad_plan(nt, R, Kd, Jd, nsplit, pair != 0, &w) ? w.total : 0;
}

// h2_wgrad, which is CellBwd::read_weight_contractions' H2 branch, on the caller's operands (minima, factor tables,
// contraction(s)), then a slab reduction per contraction
int macx_h2_wgrad(const macx_opts* o, int nt, int R, int Kd, int Jd, int nsplit, const float* hA, size_t a_stride, int a_shared,
                  const float* hG, size_t g_stride, float* out, const float* hA2, size_t a2_stride, int a2_shared, const float* hG2,
                  size_t g2_stride, float* out2, float* ws, size_t ws_floats, void* stream) {
  if (o && o->abi_version != MACX_ABI_VERSION) return MACX_EINVAL;
  H2Scope sc(o);
  const bool pair = hA2 || hG2 || out2;
  H2WgradWs w;
  if (!h2_wgrad_plan(nt, R, Kd, Jd, nsplit, pair, &w)) return MACX_EINVAL;
  if (!hA || !hG || !out || !ws || (pair && (!hA2 || !hG2 || !out2 || out2 == out))) return MACX_EINVAL;
  if (misaligned(hA) || misaligned(hG) || misaligned(out) || misaligned(ws) || misaligned(hA2) || misaligned(hG2) || misaligned(out2))
    return MACX_EINVAL;
  if ((a_shared != 0 && a_shared != 1) || (a2_shared != 0 && a2_shared != 1)) return MACX_EINVAL;
  if (!h2x_stride_ok(a_stride, a_shared ? 1 : nt, R, Kd) || !h2x_stride_ok(g_stride, nt, R, Jd)) return MACX_EINVAL;
  if (pair && (!h2x_stride_ok(a2_stride, a2_shared ? 1 : nt, R, Kd) || !h2x_stride_ok(g2_stride, nt, R, Jd))) return MACX_EINVAL;
  if (ws_floats < w.total) return MACX_ESMALL;
  const hipStream_t st = (hipStream_t)stream;
  const H2WgradOp op[2] = {{hA, a_stride, a_shared != 0, hG, g_stride, ws + w.ftab[0], ws + w.slab[0]},
                           {hA2, a2_stride, a2_shared != 0, hG2, g2_stride, ws + w.ftab[1], ws + w.slab[1]}};
  CKI(h2_wgrad(op, pair ? 2 : 1, nt, R, Kd, Jd, nsplit, w.rows_per_split, reinterpret_cast<int*>(ws + w.ecom), st));
  CK(slab_reduce_launch(ws + w.slab[0], nsplit, (size_t)Kd * Jd, out, 0, st));
  if (pair) CK(slab_reduce_launch(ws + w.slab[1], nsplit, (size_t)Kd * Jd, out2, 0, st));
  return MACX_OK;
}

size_t macx_h2_sb_ws_floats(const macx_opts* o, int B, int N, int d, int nsteps, int qpg, int wide) {
  if (o && o->abi_version != MACX_ABI_VERSION) return 0;
  H2Scope sc(o);
  H2SbWs w;
  return h2_sb_plan(B, N, d, nsteps, qpg, wide, 0, &w) ? w.total : 0;
}

// sb_h2, the S_b launch of CellBwd (per step with dy, or deferred over all steps), on the caller's operands, and its slab reductions
int macx_h2_sb(const macx_opts* o, int B, int N, int d, int nsteps, int qpg, int wide, const float* hX, size_t x_stride,
               const float* hdI1, size_t g_stride, const float* y, const float* W1a, float* dW1a, float* dW1b, float* dy_part,
               float* ws, size_t ws_floats, void* stream) {
  if (o && o->abi_version != MACX_ABI_VERSION) return MACX_EINVAL;
  H2Scope sc(o);
  H2SbWs w;
  if (!h2_sb_plan(B, N, d, nsteps, qpg, wide, dy_part != nullptr, &w)) return MACX_EINVAL;
  if (!hX || !hdI1 || !y || !dW1a || !dW1b || !ws || dW1a == dW1b || (dy_part && !W1a)) return MACX_EINVAL;
  if (misaligned(hX) || misaligned(hdI1) || misaligned(y) || misaligned(W1a) || misaligned(dW1a) || misaligned(dW1b) ||
      misaligned(dy_part) || misaligned(ws))
    return MACX_EINVAL;
  const size_t rows = (size_t)B * N;
  if (!h2x_stride_ok(x_stride, nsteps, rows, d) || !h2x_stride_ok(g_stride, nsteps, rows, d)) return MACX_EINVAL;
  if (ws_floats < w.total) return MACX_ESMALL;
  const hipStream_t st = (hipStream_t)stream;
  CKI(sb_h2(B, N, d, nsteps, w.qpg, wide != 0, hX, x_stride, hdI1, g_stride, y, (size_t)B * d, W1a, ws + w.slab_a, ws + w.slab_b, dy_part, st));
  const size_t dd = (size_t)d * d;
  CK(slab_reduce_launch(ws + w.slab_a, w.ngroup, dd, dW1a, 0, st));
  CK(slab_reduce_launch(ws + w.slab_b, w.ngroup, dd, dW1b, 0, st));
  return MACX_OK;
}

/* bench / profiling hook: the read unit's forward chain kernel of `step`, re-launched `reps` times on `stream` between two HIP
   events; *ms_out = average milliseconds per launch.  `saved` must come from macx_cell_begin + macx_cell_step(.., step) with
   keep = 1 (the step's y and control exist then); the outputs of launch r go to the buffers of step (step + r) % p, so the run
   must not be differentiated afterwards. */
int macx_read_chain_time(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                         const macx_inputs* in, float* saved, size_t saved_floats, int step, int reps, float* ms_out,
                         void* stream) {
  ModeScope ms(o);
  CKI(check_impl(o, s));
  if (!dp || !P || !in || !saved || !ms_out || reps < 1 || step < 0 || step >= s->p) return MACX_EINVAL;
  const CellRoute R = plan_route(o, s, dp, 1, NCU_ASK);
  if (!R.chain) return MACX_EUNSUPPORTED;
  const SavedLayout L = make_saved(o, s, 1, R);
  if (saved_floats < L.total) return MACX_ESMALL;
  hipStream_t st = (hipStream_t)stream;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  CK(chain_fwd_launch(make_chain_fwd(o, s, dp, P, in, saved, L, R, 1, step, step), st));      // untimed: code object, LDS attribute
  CK(hipEventRecord(e0, st));
  for (int r = 0; r < reps; ++r) CK(chain_fwd_launch(make_chain_fwd(o, s, dp, P, in, saved, L, R, 1, step, (step + r) % s->p), st));
  CK(hipEventRecord(e1, st));
  CK(hipEventSynchronize(e1));
  float t = 0.f;
  CK(hipEventElapsedTime(&t, e0, e1));
  *ms_out = t / reps;
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  return MACX_OK;
}

/* The same kernel timed IN A RUNNING FORWARD PASS: one macx_cell_forward (keep = 1) on `stream`, each of its p chain launches issued
   through hipExtLaunchKernelGGL with a start and a stop event -- the kernel's own dispatch timestamps, what a kernel trace reports;
   in front of a launch sits the step's [B,d] linear, behind it the attention kernel, as in a training step.  *ms_out = average
   milliseconds per launch (synchronises `stream`).  What bench.py's roofline.kernel_ms reports. */
int macx_cell_forward_chain_time(const macx_opts* o, const macx_shapes* s, const macx_dropout* dp, const macx_params* P,
                                 const macx_inputs* in, float* saved, size_t saved_floats, float* ws, size_t ws_floats, float* ms_out,
                                 void* stream) {
  ModeScope ms(o);
  CKI(check_impl(o, s));
  if (!ms_out) return MACX_EINVAL;
  if (!plan_route(o, s, dp, 1, NCU_NONE).chain) return MACX_EUNSUPPORTED;
  ChainProbe& cp = *chain_probe();
  if (cp.on) return MACX_EINVAL;
  const int ne = 2 * (s->p < 64 ? s->p : 64);
  for (int i = 0; i < ne; ++i) CK(hipEventCreate(&cp.ev[i]));
  // three untimed passes in front of the timed one, nothing but launches in between: the timed pass runs on a chip that has been
  // busy for milliseconds, like a pass inside a training loop (a lone pass after a host synchronisation measured 10 % slow: clocks)
  int rc = MACX_OK;
  for (int w = 0; w < 3 && rc == MACX_OK; ++w) rc = macx_cell_forward(o, s, dp, P, in, saved, saved_floats, ws, ws_floats, 1, stream);
  cp.n = 0; cp.on = true;
  if (rc == MACX_OK) rc = macx_cell_forward(o, s, dp, P, in, saved, saved_floats, ws, ws_floats, 1, stream);
  cp.on = false;
  int err = rc;
  if (rc == MACX_OK && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) err = MACX_EINVAL;
  double total = 0.0;
  for (int k = 0; err == MACX_OK && k < cp.n; ++k) {
    float t = 0.f;
    if (hipEventElapsedTime(&t, cp.ev[2 * k], cp.ev[2 * k + 1]) != hipSuccess) err = MACX_EINVAL;
    total += t;
  }
  for (int i = 0; i < ne; ++i) (void)hipEventDestroy(cp.ev[i]);
  if (err != MACX_OK) return err;
  if (cp.n < 1) return MACX_EUNSUPPORTED;
  *ms_out = (float)(total / cp.n);
  return MACX_OK;
}

// ---- the control unit's question projections (mac_cell.py:442-448) behind a contract of their own -----------------
//   t = act(vecQ Wq + bq)  [B,d]  (controlInputAct);   cI_i = t WqU_i + bqU_i  [p,B,d]  (one matrix per step with
//   controlInputUnshared, else the same one p times): ctrl_inputs_fwd, which macx_cell_begin calls, on weights packed here.
// The workspace: the packed weights (the backward call: their transposes) [1 + nU][d,d], then the backward pass's dt, du and summed
// d_ctrl_inputs [3][B,d], with unshared inputs dt_part [p,B,d], and a SmallWgradBatch's eight slab sets.
namespace {
inline size_t ctrl_inputs_slab_stride(const macx_shapes* s) { return al4((size_t)wgrad_splits(s->B, s->d, s->d) * s->d * s->d); }
// packs qInput_W and the nU matrices of qInputU_W (T: their transposes) into ws
int ctrl_inputs_pack(const macx_params* P, bool T, int d, int nU, float* ws, hipStream_t st) {
  const size_t dd = (size_t)d * d;
  Packer pk;
  add_pack(pk, T, P->qInput_W, d, d, ws);
  for (int i = 0; i < nU; ++i) {
    if (pk.n == PACK_MAX) CK(pk.run(st));
    add_pack(pk, T, P->qInputU_W + (size_t)i * dd, d, d, ws + (1 + i) * dd);
  }
  CK(pk.run(st));
  return MACX_OK;
}
}  // namespace

size_t macx_ctrl_inputs_ws_floats(const macx_opts* o, const macx_shapes* s) {
  if (!o || !s || s->d < 1 || s->B < 1 || s->p < 1) return 0;
  const size_t dd = (size_t)s->d * s->d, Bd = (size_t)s->B * s->d, nU = o->control_input_unshared ? s->p : 1;
  return (1 + nU) * dd + (3 + (o->control_input_unshared ? s->p : 0)) * Bd + 8 * ctrl_inputs_slab_stride(s) + 64;
}

int macx_ctrl_inputs_fwd(const macx_opts* o, const macx_shapes* s, const macx_params* P, const float* vecQuestions, float* ctrl_t,
                         float* ctrl_inputs, float* ws, size_t ws_floats, void* stream) {
  ModeScope ms(o);
  CKI(check_impl(o, s));
  if (!P || !vecQuestions || !ctrl_t || !ctrl_inputs || !ws || !P->qInput_W || !P->qInputU_W) return MACX_EINVAL;
  if (misaligned(vecQuestions) || misaligned(ctrl_t) || misaligned(ctrl_inputs) || misaligned(ws)) return MACX_EINVAL;
  if (ws_floats < macx_ctrl_inputs_ws_floats(o, s)) return MACX_ESMALL;
  hipStream_t st = (hipStream_t)stream;
  const int d = s->d;
  CKI(ctrl_inputs_pack(P, false, d, o->control_input_unshared ? s->p : 1, ws, st));
  return ctrl_inputs_fwd(vecQuestions, ws, P->qInput_b, ws + (size_t)d * d, P->qInputU_b, o->control_input_unshared,
                         o->control_input_act, s->B, d, s->p, ctrl_t, ctrl_inputs, st);
}

// backward of the above: d_ctrl_inputs [p,B,d] -> d_vecQuestions [B,d] and the gradients of qInput / qInputU (the non-NULL fields of
// `GP`: qInput_W [d,d], qInput_b [d], qInputU_W [nU,d,d], qInputU_b [nU,d]) -- ctrl_inputs_bwd, which CellBwd::control_inputs_bwd
// calls (SURVEY appendix A rows "qInput", "qInput{i}"), with batches of this call's own that run before it returns.
int macx_ctrl_inputs_bwd(const macx_opts* o, const macx_shapes* s, const macx_params* P, const float* vecQuestions, const float* ctrl_t,
                         const float* d_ctrl_inputs, const macx_param_grads* GP, float* d_vecQuestions, float* ws, size_t ws_floats,
                         void* stream) {
  ModeScope ms(o);
  CKI(check_impl(o, s));
  if (!P || !vecQuestions || !ctrl_t || !d_ctrl_inputs || !GP || !d_vecQuestions || !ws || !P->qInput_W || !P->qInputU_W) return MACX_EINVAL;
  if (misaligned(vecQuestions) || misaligned(ctrl_t) || misaligned(d_ctrl_inputs) || misaligned(d_vecQuestions) || misaligned(ws)) return MACX_EINVAL;
  if (ws_floats < macx_ctrl_inputs_ws_floats(o, s)) return MACX_ESMALL;
  hipStream_t st = (hipStream_t)stream;
  const int B = s->B, d = s->d, p = s->p;
  const size_t dd = (size_t)d * d, Bd = (size_t)B * d;
  const bool unshared = o->control_input_unshared != 0;
  const int nU = unshared ? p : 1;
  CKI(ctrl_inputs_pack(P, true, d, nU, ws, st));
  float* dt = ws + (1 + nU) * dd;
  float* slab = dt + (3 + (unshared ? p : 0)) * Bd;
  const CtrlInputsScratch x{dt + 3 * Bd, dt, dt + Bd, dt + 2 * Bd, slab};
  RowsumBatch rs;
  SmallWgradBatch wb(slab, ctrl_inputs_slab_stride(s));
  CKI(ctrl_inputs_bwd(unshared, o->control_input_act, B, d, p, vecQuestions, ctrl_t, d_ctrl_inputs, ws, ws + dd, nullptr, x,
                      d_vecQuestions, GP, rs, wb, st));
  CKI(wb.run(st));
  CK(rs.run(st));
  return MACX_OK;
}

// One of the read unit's kept [B*N, d] activations of step `step` as fp32 row-major: which = 0 dropout(KB) (ops.py:678), 1 X
// (ops.py:688), 2 H1 (ops.py:718), 3 I2 (ops.py:326) -- what the forward pass left in `saved` (keep = 1) for the backward pass,
// whatever format the kernel family keeps it in (H2 planes in the default family).  Inspection / tests: the chain kernel's
// intermediate products are checked against fp64 through this (tests/test_gpu_h2.py).
int macx_saved_activation(const macx_opts* o, const macx_shapes* s, int which, int step, const float* saved, size_t saved_floats,
                          float* out, void* stream) {
  ModeScope ms(o);
  CKI(check_impl(o, s));
  if (!saved || !out || which < 0 || which > 3 || step < 0 || step >= s->p || misaligned(out)) return MACX_EINVAL;
  const CellRoute route = plan_route(o, s, nullptr, 1, NCU_NONE);
  const SavedLayout L = make_saved(o, s, 1, route);
  if (saved_floats < L.total) return MACX_ESMALL;
  const size_t base = which == 0 ? L.KBd : (which == 1 ? L.X : (which == 2 ? L.H1 : L.I2));
  const float* src = saved + base + (size_t)step * L.act_stride;
  hipStream_t st = (hipStream_t)stream;
  const size_t R = (size_t)s->B * s->N;
  if (route.h2) {
    hipLaunchKernelGGL(h2_to_f32_kernel, dim3(1024), dim3(256), 0, st, h2_view(src, (int)R, s->d), out);
    CK(hipGetLastError());
  } else {
    CK(dev_copy(out, src, R * s->d * sizeof(float), st));
  }
  return MACX_OK;
}

int macx_wgrad_splits(int M, int Kd, int Jd) {
  if (M < 1 || Kd < 128 || Jd < 128 || Kd % 128 || Jd % 128) return MACX_EINVAL;
  return wgrad_splits(M, Kd, Jd);
}

int macx_wgrad(const float* A, int lda, const float* G, int ldg, int M, int Kd, int Jd, float* out, float* ws, void* stream) {
  if (!A || !G || !out || !ws) return MACX_EINVAL;
  if (M < 1 || Kd < 128 || Jd < 128 || Kd % 128 || Jd % 128 || lda % 4 || ldg % 4) return MACX_EINVAL;
  return wgrad_impl(A, lda, G, ldg, M, Kd, Jd, out, ws, (hipStream_t)stream);
}

}  // extern "C"
