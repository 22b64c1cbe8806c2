/* macx.h -- C ABI of libmacx.so: the MI355X-native MAC reasoning cell.
 *
 * The reference (stanfordnlp/mac-network) has no FFI: its hot path is the Python class
 * MACCell (mac_cell.py:30-592) driven by MACnet.MACnetwork (model.py:428-489), and all
 * arithmetic lives in the TensorFlow-1.x runtime.  This header is the boundary a maintainer
 * would bind to replace that class's arithmetic (ctypes stub in INTEGRATION.md).  Every entry
 * point names the reference code it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; all tensors fp32, row-major, contiguous, 16-byte aligned;
 *     question lengths int32.  All pointers are DEVICE pointers unless marked host.
 *   - ownership: the caller owns every buffer (parameters, inputs, `saved`, `ws`, gradients).
 *     The library never allocates, frees or retains device memory.
 *   - asynchronous: work is enqueued on `stream`; nothing synchronises the device (the timing hooks, macx_run_status and
 *     macx_handoff_selftest say so where they do).
 *   - errors: 0 on success, a negative MACX_E* code for a rejected call, or the positive
 *     hipError_t of a failed launch.  No exceptions, no abort().
 *   - determinism: no floating-point atomics anywhere; weight gradients use fixed-order
 *     slab reductions, so two runs on the same inputs are bit-identical.
 */
#ifndef MACX_H
#define MACX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MACX_ABI_VERSION 5

enum {
  MACX_OK = 0,
  MACX_EINVAL = -1,      /* malformed shapes / null pointer / misaligned pointer            */
  MACX_EUNSUPPORTED = -2,/* legal reference option combination without a HIP path yet       */
  MACX_EREJECTED = -3,   /* option value that raises in the reference   */
  MACX_ESMALL = -4,      /* `saved` or `ws` smaller than macx_saved_floats / macx_ws_floats */
  MACX_EWAIT = -5        /* macx_run_status: a workgroup gave up waiting for another one of its own launch; the run is poisoned */
};

/* activation codes (ops.py:181-187; "RELU" resolves through config.relu, ops.py:161-179) */
enum { MACX_ACT_NON = 0, MACX_ACT_TANH = 1, MACX_ACT_SIGMOID = 2, MACX_ACT_ELU = 3, MACX_ACT_RELU = 4 };
/* state initialisation (mac_cell.py:496-505) */
enum { MACX_INIT_PRM = 0, MACX_INIT_ZERO = 1, MACX_INIT_Q = 2 };
/* write-unit inputs (mac_cell.py:333-340) */
enum { MACX_WRITE_MEM = 0, MACX_WRITE_INFO = 1, MACX_WRITE_SUM = 2, MACX_WRITE_BOTH = 3 };

/* Frozen option surface: the subset of config.py flags (config.py:194-223, 292-387) the cell
 * branches on, resolved to integers by the host (mac-network_amd/options.py). */
typedef struct macx_opts {
  int32_t abi_version;              /* MACX_ABI_VERSION                                        */
  int32_t init_ctrl, init_mem;      /* --initCtrl / --initMem                                  */
  int32_t control_input_unshared;   /* --controlInputUnshared     (mac_cell.py:430-432)        */
  int32_t control_input_act;        /* --controlInputAct          (mac_cell.py:445)            */
  int32_t control_feed_prev;        /* --controlFeedPrev          (mac_cell.py:142)            */
  int32_t control_feed_prev_att;    /* --controlFeedPrevAtt       (mac_cell.py:143)            */
  int32_t control_feed_inputs;      /* --controlFeedInputs        (mac_cell.py:144-146)        */
  int32_t control_cont_act;         /* --controlContAct           (mac_cell.py:149-150)        */
  int32_t read_mem_act;             /* --readMemAct resolved      (mac_cell.py:237)            */
  int32_t read_ctrl_act;            /* --readCtrlAct resolved     (mac_cell.py:262)            */
  int32_t write_inputs;             /* --writeInputs              (mac_cell.py:333-340)        */
  int32_t write_self_att;           /* --writeSelfAtt             (mac_cell.py:316-330)        */
  int32_t write_self_att_cont;      /* --writeSelfAttMod == CONT  (mac_cell.py:318-319)        */
  int32_t write_mem_act;            /* --writeMemAct resolved     (mac_cell.py:355)            */
  int32_t write_gate;               /* --writeGate                (mac_cell.py:358-367)        */
  int32_t write_gate_shared;        /* --writeGateShared          (mac_cell.py:360-361)        */
  float   write_gate_bias;          /* --writeGateBias            (mac_cell.py:363)            */
  int32_t memory_variational_dropout; /* --memoryVariationalDropout (mac_cell.py:214-217)      */
  int32_t gemm_family;              /* kernel family of the knowledge-base GEMMs for EVERY call made with these options
                                       (sizing, begin, step, backward): 0 = the process default (macx_gemm_mode),
                                       1 + MACX_GEMM_NATIVE / _SPLIT / _H2 = that family.  Per call and per thread: two
                                       cells of one process can run on different families side by side               */
  int32_t tune[16];                 /* PER-CALL tuning table (ABI 5; replaces the process-global `macx_debug_set` of ABI <= 4): the A/B
                                       hook of each live kernel-selection decision and the phase masks of the profiling tools.
                                       All zero = the shipped configuration.  tune[k] = 0: the default of key k; else the value
                                       v is passed as v + 1 (MACX_TUNE(v)).  Read when a call is enqueued, from the opts of THAT
                                       call (forward and backward of one run must see the same table): no state lives in the
                                       library, calls on different threads or with different opts never see each other's table.
                                       Keys: MACX_TUNE_* below.  Never needed for correct results. */
} macx_opts;
#define MACX_TUNE(v) ((v) + 1)
enum {
  MACX_TUNE_NATIVE_WAVES = 0, /* waves per workgroup of the NATIVE knowledge-base GEMM: 4 | 8 (default)                        */
  MACX_TUNE_PHASE_MASK = 1,   /* bit mask of TIMING experiments (results are wrong under a non-zero mask; tools/mask_steps.py):
                                 1 skip the GEMM epilogue, 2 skip the in-loop staging, 8 epilogue without its global stores,
                                 32 / 64 re-read K-slice 0 of A / of the weights (cache-hot), 128 weight-gradient contractions on
                                 the f32 TN kernel, 256 S_b kernel on the f32 kernel, 512 / 1024 / 2048 the deferred contractions
                                 without their folds / products / in-loop DMA, bits 12-16 stop chain_fwd after a stage, bits
                                 17-21 chain_bwd                                                                              */
  MACX_TUNE_ROW_TILES = 2,    /* forced row tiles per GEMM workgroup (0 = automatic | 1 | 2 | 4 | 7 | 13)                      */
  MACX_TUNE_CHAIN = 4,        /* 0: the read unit's products as separate launches (what also runs for d > 512 or N < 16);
                                 1 (default): the chain kernels of macx_chain_h2.hip.h                                        */
  MACX_TUNE_SB_DEFER = 5,     /* 0: the per-question contraction S_b = X_b^T dI1_b once per step (it then also delivers dy; what
                                 also runs for N < 32); 1 (default): dy from the chain kernel, S_b of all steps in one launch   */
  MACX_TUNE_CHAIN_KV = 7,     /* K loop of the d = 512 chain kernels: 0 activation fragments requested in front of a slice's
                                 products; -1 (default): in mid-slice                                                         */
  MACX_TUNE_SB_WIDE = 8,      /* dW1a / dW1b: 0 the 128 x 128 per-question S_b kernel; 1 (default) the 128 x 256 one            */
  MACX_TUNE_WGRAD_PIPE = 10,  /* wgrad_h2_kernel<2,2>: 0 a stage requested one iteration ahead; 1 a buffer's halves re-requested
                                 inside the iteration; 2 = 1 + dW2 and dWx as ONE launch; 3 (default) = 2 with half the splits  */
  MACX_TUNE_SB_CONT = 13,     /* sb_h2w_kernel: 1 (default) one stage stream over all steps; 0 drained and re-primed per step    */
  MACX_TUNE_DKB_UNI = 14,     /* merged dKB launch: 1 (default) one fold of the block accumulator per step; 0 per 128-wide K block */
  MACX_TUNE_PRE_FILL = 3,     /* what the filler workgroups of a d = 512 chain_fwd launch do on the CUs its tile grid leaves idle (runs
                                 of macx_cell_forward; 196 tiles on 256 CUs at B = 64): 1 (default) the previous step's write-unit
                                 linear, this step's y = md Wy + by, and stage 0 (dropout(KB) -> fp16 planes, keep bits) of the next
                                 step; 2 the same without the write unit; 0 no fillers: every piece is a launch / a stage of its own */
  MACX_TUNE_DKB_FILL = 15     /* dKB on the CUs a d = 512 chain_bwd launch leaves idle (196 tiles on 256 CUs at B = 64): jobs per
                                 filler workgroup, default 3; 0: all of dKB in the merged launch after the last step            */
};

typedef struct macx_shapes {
  int32_t B;     /* questions in this (shard of the) batch                                     */
  int32_t S;     /* padded question length                                                     */
  int32_t N;     /* knowledge-base cells per question (H*W, model.py:202)                      */
  int32_t d;     /* memDim == ctrlDim == attDim (config.py:294-296); multiple of 128           */
  int32_t p;     /* netLength (config.py:292)                                                  */
  int32_t b0;    /* global index of question 0: data-parallel shard offset (model.py:139-149)  */
  int32_t d_logical; /* 0 (or d): the cell is d wide.  Else: the caller runs a d_logical-wide cell (config.py:294-296 takes
                      * any width) zero-padded to d columns -- weights, biases, inputs -- and the dropout element indices are
                      * taken at the LOGICAL width ((row * d_logical + column): the masks of the unpadded cell); d_logical % 8
                      * == 0, d - 128 < d_logical < d.  The padded columns of every state and gradient are exact zeros. */
} macx_shapes;

/* Dropout of one cell run.  keep == 1 (evaluation, model.py:118-125) is the exact identity. */
typedef struct macx_dropout {
  float keep_memory, keep_read, keep_write;   /* config.py:213-215                              */
  uint32_t seed;                              /* stateless mask stream, see macx_dropout_mask  */
  const uint32_t* mask_word;                  /* NULL, or ONE 32-bit word in DEVICE memory that every dropout site of the run
                                               * XORs into its key when the kernel RUNS (not when it is enqueued):
                                               *   mask(seed, word, site, step, i) = stream keyed site_key(seed, site, step) ^ word.
                                               * The seed travels by value in kernel arguments, so a captured HIP graph would
                                               * replay the masks of the captured seed for ever; the word is read on every
                                               * replay, so ONE capture of a training step draws fresh masks per replay
                                               * (write the word between replays -- e.g. a hash of the iteration number).
                                               * Forward and backward of one run must see the same word.  NULL == word 0 ==
                                               * the masks of ABI <= 3. */
} macx_dropout;

/* Parameters, keyed by the reference's variable names under macModel/MACnetwork/ (SURVEY 8b).
 * Matrices are [in, out] row-major exactly as tf.get_variable stores them. */
typedef struct macx_params {
  const float* initMem;        /* initMem [d]                         (mac_cell.py:498)         */
  const float* initCtrl;       /* initCtrl [d]           (PRM only)                             */
  const float* qInput_W;       /* MACCell/linearLayerqInput/weights/weight [d,d]                */
  const float* qInput_b;       /*                       .../biases/bias [d]                     */
  const float* qInputU_W;      /* linearLayerqInput{i} stacked [p,d,d] (or [1,d,d] if shared)   */
  const float* qInputU_b;      /* [p,d] / [1,d]                                                 */
  const float* ctrlLogits_w;   /* control/inter2logits/linearLayerlogits/weights/weight [d]     */
  const float* ctrlLogits_b;   /* .../biases/bias []                                            */
  const float* contControl_W;  /* control/linearLayercontControl [d or 2d, d]   (args1)         */
  const float* contControl_b;
  const float* contControl2_W; /* .../linearLayercontControl_2 [d,d]   (controlContAct != NON)  */
  const float* contControl2_b;
  const float* projX_W;        /* read/mulmemInter/linearLayerprojX [d,d]                       */
  const float* projX_b;
  const float* projY_W;        /* read/mulmemInter/linearLayerprojY [d,d]                       */
  const float* projY_b;
  const float* memKbProj_W;    /* read/linearLayermemKbProj [2d,d]: rows [0,d) x*y, [d,2d) x    */
  const float* memKbProj_b;
  const float* memKbProj2_W;   /* read/linearLayermemKbProj/linearLayermemKbProj_2 [d,d]        */
  const float* memKbProj2_b;
  const float* kbLogits_w;     /* read/inter2att/inter2logits/linearLayerlogits [d]             */
  const float* kbLogits_b;
  const float* newMemory_W;    /* write/linearLayernewMemory [2d or 3d, d]                      */
  const float* newMemory_b;
  const float* selfCtrl_W;     /* write/linearLayerctrlProj [d,d]               (args3)         */
  const float* selfCtrl_b;
  const float* selfLogits_w;   /* write/inter2attselfAttention/.../linearLayerlogits [d]        */
  const float* selfLogits_b;
  const float* gate_W;         /* write/linearLayergate [d, d or 1]             (args4)         */
  const float* gate_b;
} macx_params;

/* Gradients: same fields, written (not accumulated) by macx_cell_backward. */
typedef struct macx_param_grads {
  float* initMem; float* initCtrl;
  float* qInput_W; float* qInput_b; float* qInputU_W; float* qInputU_b;
  float* ctrlLogits_w; float* ctrlLogits_b;
  float* contControl_W; float* contControl_b; float* contControl2_W; float* contControl2_b;
  float* projX_W; float* projX_b; float* projY_W; float* projY_b;
  float* memKbProj_W; float* memKbProj_b; float* memKbProj2_W; float* memKbProj2_b;
  float* kbLogits_w; float* kbLogits_b;
  float* newMemory_W; float* newMemory_b;
  float* selfCtrl_W; float* selfCtrl_b; float* selfLogits_w; float* selfLogits_b;
  float* gate_W; float* gate_b;
} macx_param_grads;

/* Cell inputs: the tensors MACCell.__init__ stores (mac_cell.py:59-79). */
typedef struct macx_inputs {
  const float* vecQuestions;     /* [B,d]                                                        */
  const float* words;            /* [B,S,d]  questionCntxWords or questionWords (mac_cell.py:570) */
  const int32_t* questionLengths;/* [B]                                                          */
  const float* knowledgeBase;    /* [B,N,d]  stem output (model.py:202)                          */
  const int32_t* kbLengths;      /* [B] device, or NULL */
  /* kbLengths (appended; a zero-initialised struct keeps the old behaviour): question b's knowledge base is its first
   * kbLengths[b] cells (clamped to [1, N]); the rest is padding.  The read unit's softmax and summary run over the live cells
   * only, att_kb[b][n >= kbLengths[b]] is exactly 0, and the forward pass does not depend on what the padded rows hold.  The
   * backward pass multiplies them by that 0, so padded rows must be FINITE (zeros recommended) when gradients are taken; the
   * gradient of a padded row is exactly 0.  The padded rows are still computed: the mask changes results, not time.
   * With shared images, macx_kb_gather_l makes both on the device: this array from the sizes per image, and the zero padding. */
} macx_inputs;

typedef struct macx_input_grads {
  float* vecQuestions;           /* [B,d]                                                        */
  float* words;                  /* [B,S,d]                                                      */
  float* knowledgeBase;          /* [B,N,d]                                                      */
} macx_input_grads;

/* Segments of the `saved` buffer that the host may view (offsets in floats). */
enum {
  MACX_SEG_CONTROLS = 0,   /* [p+1,B,d]  controls history, entry 0 = initial (mac_cell.py:549,472) */
  MACX_SEG_MEMORIES = 1,   /* [p+1,B,d]  memories history                     (mac_cell.py:550,473) */
  MACX_SEG_INFOS = 2,      /* [p,B,d]    retrieved information per step       (mac_cell.py:474)     */
  MACX_SEG_ATT_QUESTION = 3,/* [p,B,S]   attentions["question"]               (mac_cell.py:176)     */
  MACX_SEG_ATT_KB = 4,     /* [p,B,N]    attentions["kb"]                     (mac_cell.py:268)     */
  MACX_SEG_ATT_SELF = 5,   /* [p,B,p]    attentions["self"], row i uses i+1   (mac_cell.py:329)     */
  MACX_SEG_ATT_GATE = 6,   /* [p,B,d|1]  attentions["gate"]                   (mac_cell.py:365)     */
  MACX_SEG_STATUS = 7,     /* 16 uint32 words (not floats): the run's hand-off status, see macx_run_status           */
  MACX_SEG_COUNT = 8
};

/* ---- sizing -------------------------------------------------------------------------------- */
/* floats the caller must provide in `saved` (kept from forward to backward) and `ws` (scratch).
 * keep_activations = 1 keeps the per-step [B,N,d] read-unit activations needed by backward. */
size_t macx_saved_floats(const macx_opts*, const macx_shapes*, int keep_activations);
size_t macx_ws_floats(const macx_opts*, const macx_shapes*, int for_backward);
/* offset (floats) and element count of a viewable segment of `saved`; returns MACX_OK or error */
int macx_saved_segment(const macx_opts*, const macx_shapes*, int keep_activations, int segment,
                       size_t* offset, size_t* count);
/* validates an option/shape combination exactly as macx_cell_begin would */
int macx_check(const macx_opts*, const macx_shapes*);

/* The launch route of a fused-cell call: which of its kernels the library runs for these options, shapes and dropout on a device of
 * `ncu` compute units, and how it sizes what they share.  The library plans this once per call, with the same function; this export
 * only reads the plan (nothing is launched), for tests, tools and records.  Fields 0 / 1 unless a range is given. */
typedef struct macx_route {
  int32_t family;             /* kernel family the call runs on: MACX_GEMM_NATIVE / _SPLIT / _H2                               */
  int32_t chain;              /* the read unit's products as ONE kernel per direction, chain_fwd / chain_bwd<d> (H2 family, d <= 512,
                                 N >= 16, MACX_TUNE_CHAIN); 0: one launch per product                                             */
  int32_t tile_rows, tiles;   /* chain: rows of a tile (16 | 32 | 64) and tiles of a launch; else 0                              */
  int32_t chain_sums;         /* chain_bwd leaves per-tile partials of what is summed per question (N >= 32)                     */
  int32_t sb_deferred;        /* dy from chain_bwd, S_b = X_b^T dI1_b of all steps in ONE launch at the end (MACX_TUNE_SB_DEFER); 0:
                                 the S_b kernel once per step, which then also delivers dy                                        */
  int32_t dy_in_linear;       /* sb_deferred: the dy linear sums the per-tile partials of dy itself (B <= 128, <= 6 tiles a question) */
  int32_t dc_reduce_per_step; /* sb_deferred: ... or a reduction launch behind every chain_bwd launch does (a recurrent control unit
                                 makes the whole-cell backward pass reduce per step whatever this says)                           */
  int32_t sb_wide;            /* sb_deferred: the 128 x 256 S_b kernel (MACX_TUNE_SB_WIDE); 0: the 128 x 128 one                    */
  int32_t sb_qpg, sb_groups;  /* questions per workgroup group of the S_b kernel in use, and groups per launch                   */
  int32_t sb_slabs;           /* [d,d] partial slabs of dW1a (and of dW1b) the closing reduction sums                             */
  int32_t wgrad_splits;       /* reduction splits the dW2 / dWx slabs are sized for                                              */
  int32_t wgrad_kw;           /* H2 family: 128-column blocks per tile side (kw = jw) of those contractions, 1 | 2; else 0        */
  int32_t db_rows, dwk_rows;  /* rows per step of the bias-gradient partials of dI1 / dX, and of dw_k / db2                       */
  int32_t wfmt_plain, wfmt_ymix; /* internal pack format of a plain weight (0 f32 MFMA order | 1 bf16 planes | 3 fp16 planes +
                                 exponent) and of one mixed with a per-question vector (0 | 2 fp32 k-major tiles)                */
  /* what depends on `ncu` and on the dropout, never on anything above: work on the compute units a chain launch's tiles leave idle */
  int32_t fwd_fillers;        /* filler workgroups of each chain_fwd launch of macx_cell_forward (MACX_TUNE_PRE_FILL); 0: none       */
  int32_t fill_y;             /* ... they compute the step's y = md Wy + by                                                       */
  int32_t fill_stage0;        /* ... and stage 0 (dropout(KB) -> fp16 planes) of the next step: keep_activations and keep_read < 1  */
  int32_t fill_write;         /* ... and the previous step's write linear: no gate, no self-attention, no recurrent control, no write
                                 dropout                                                                                          */
  int32_t dkb_jobs, dkb_fillers, dkb_skip; /* dKB on chain_bwd's idle compute units (MACX_TUNE_DKB_FILL): jobs per filler workgroup
                                 (0: the merged dKB launch), filler workgroups, tiles a launch leaves to the closing launch        */
} macx_route;
/* dropout NULL: no dropout.  ncu <= 0: the current device's compute units, exactly as a launch plans (0 without a device, hence no
 * fillers); ncu > 0: plan for that many.  No field above the filler block depends on ncu or the dropout.  The step-wise and unit
 * entry points follow the same route but never use forward fillers.  Returns what macx_check returns. */
int macx_cell_route(const macx_opts*, const macx_shapes*, const macx_dropout*, int keep_activations, int ncu, macx_route* out);

/* ---- did the run's in-launch hand-offs complete? ------------------------------------------------ */
/* In the default d = 512 path (macx_cell_forward, MACX_TUNE_PRE_FILL) workgroups of ONE launch hand results to each other through
 * counters; the waits are bounded.  A workgroup whose wait runs out does not use the unfinished data: it computes on quiet NaNs, so
 * the run's final memory and every gradient derived from it are NaN, and it reports into 16 status words of `saved`
 * (MACX_SEG_STATUS, directly in front of the run's counters):
 *   word 0  bits: 1 = a tile gave up waiting for its step's projected memory y, 2 = a filler workgroup gave up waiting for the
 *           previous step's write unit;   word 1  1 + the step of the first give-up (0: none);   the rest: spare.
 * The words are STICKY: macx_cell_begin does not touch them (a captured step replayed on one `saved` keeps the evidence), nothing
 * but the reset call clears them.  Contract: reset once after allocating `saved` and again after handling an error.
 * The arguments before `saved` are those of the sizing calls (they locate the words); `saved` smaller than macx_saved_floats is
 * MACX_ESMALL, a null `saved` MACX_EINVAL.
 *   macx_run_status        copies the words to the host on `stream` and SYNCHRONISES that stream (the one cell entry point that
 *                          does): MACX_OK when word 0 is 0, else MACX_EWAIT.  *host_status = word 0, *host_first_step = the step or
 *                          -1; either pointer may be NULL.  On a stream that is being captured: the hipError_t of the refusal.
 *   macx_run_status_reset  zeroes the words: one launch, asynchronous, capturable.
 *   macx_handoff_selftest  runs the kernels' wait routine on words of its own (allocated and freed inside the call -- the one
 *                          exception to "never allocates"), twice, and synchronises: a counter that already holds the wanted value,
 *                          then one that holds less, waited for with a budget of 0 polls.  host_out[8] = per call {arrived,
 *                          status bits, step word (1 + step), every thread of the workgroup was told to poison}: {1,0,0,0} and
 *                          {0,2,7,1}.  The give-up branch of a real run cannot be tested without making a run fail. */
int macx_run_status(const macx_opts*, const macx_shapes*, int keep_activations, const float* saved, size_t saved_floats,
                    void* stream, uint32_t* host_status, int32_t* host_first_step);
int macx_run_status_reset(const macx_opts*, const macx_shapes*, int keep_activations, float* saved, size_t saved_floats,
                          void* stream);
int macx_handoff_selftest(void* stream, uint32_t* host_out /* host, [8] */);

/* ---- the cell ------------------------------------------------------------------------------ */
/* Replaces MACCell.zero_state (mac_cell.py:539-592): initial control/memory, histories, memory
 * variational-dropout stream; additionally packs the weights for the MFMA kernels and, when the
 * control is not recurrent (controlFeedPrev off), computes all p control states up front
 * (mac_cell.py:442-451, :133-187). */
int macx_cell_begin(const macx_opts*, const macx_shapes*, const macx_dropout*, const macx_params*,
                    const macx_inputs*, float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                    int keep_activations, void* stream);

/* Replaces one MACCell.__call__ (mac_cell.py:420-480) for iteration `step`: control (if
 * recurrent), read, write, history append.  Must be called with step = 0..p-1 in order. */
int macx_cell_step(const macx_opts*, const macx_shapes*, const macx_dropout*, const macx_params*,
                   const macx_inputs*, float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                   int keep_activations, int step, void* stream);

/* begin + p steps in one call (the loop of model.py:453-458). */
int macx_cell_forward(const macx_opts*, const macx_shapes*, const macx_dropout*, const macx_params*,
                      const macx_inputs*, float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                      int keep_activations, void* stream);

/* Gradient of the whole p-step run (what tf.gradients builds for model.py:453-458).
 * d_memory / d_control: [B,d] gradients of the final state (either may be NULL = zero).
 * Requires `saved` from a forward run with keep_activations = 1, the same dropout struct, the same macx_opts (kernel family and
 * tuning table included) and the SAME PARAMETER VALUES: the weight matrices are read from the transposed / H2 packs the forward
 * call's pack launch left in `saved`, only biases and the attention vectors are read live from macx_params -- a run whose
 * parameters change between its forward and its backward call mixes old and new weights. */
int macx_cell_backward(const macx_opts*, const macx_shapes*, const macx_dropout*, const macx_params*,
                       const macx_inputs*, const float* saved, size_t saved_floats,
                       float* ws, size_t ws_floats,
                       const float* d_memory, const float* d_control,
                       const macx_param_grads*, const macx_input_grads*, void* stream);
/* The same in two parts for data-parallel overlap: phase 1 = everything except the read unit's deferred weight contractions
 * (dW2, dWx over all p*B*N rows, the S_b slab sums for dW1 and their bias sums), phase 2 = only those, on the buffers of a
 * phase-1 call; phase 0 = both (= macx_cell_backward).  After phase 1 every other parameter gradient and all input
 * gradients are final, so a host can all-reduce them on a side stream while phase 2 runs (mac-network_amd/dp.py). */
int macx_cell_backward_phase(const macx_opts*, const macx_shapes*, const macx_dropout*, const macx_params*,
                       const macx_inputs*, const float* saved, size_t saved_floats,
                       float* ws, size_t ws_floats,
                       const float* d_memory, const float* d_control,
                       const macx_param_grads*, const macx_input_grads*, int phase, void* stream);

/* Gradients that a loss sends to the run's attention maps and step states themselves (attention supervision, entropy
 * regularisers, per-step heads): dL/d of the viewable segments of `saved`, in the layouts of the MACX_SEG_* segments.  Every
 * field may be NULL = zero.  They are ADDED to what arrives through the final state: d_memory / d_control keep their meaning
 * (slot p of the histories takes both).  d_att_self needs write_self_att, d_att_gate needs write_gate: MACX_EINVAL otherwise,
 * before anything is launched.  There is no d_infos.
 * Contract, as for the padded rows of the knowledge base (macx_inputs.kbLengths): the values must be FINITE.  The softmax
 * backward multiplies them by the attention, so entries at masked words and padded cells (att == 0) contribute exact zeros and the
 * gradients there stay exact zeros -- but 0 * NaN or 0 * Inf would poison the whole row's sum. */
typedef struct macx_state_grads {
  const float* d_controls;      /* [p+1,B,d]  dL/d controls history (slot 0 = initial control)  */
  const float* d_memories;      /* [p+1,B,d]  dL/d memories history                              */
  const float* d_att_question;  /* [p,B,S]                                                       */
  const float* d_att_kb;        /* [p,B,N]                                                       */
  const float* d_att_self;      /* [p,B,p]    row i uses entries 0..i; only with write_self_att  */
  const float* d_att_gate;      /* [p,B,d]    only with write_gate                               */
} macx_state_grads;
/* macx_cell_backward / macx_cell_backward_phase with those gradients.  A NULL struct, or one whose fields are all NULL, IS the
 * plain call: the same launches, the same arithmetic order, bit-identical results (the plain exports forward here with NULL).
 * A non-NULL d_memories costs one small launch per step where the option set has neither self attention nor a gate (the
 * step's dL/dm_{i-1} is accumulated into its slot instead of written); the other fields ride launches that run anyway. */
int macx_cell_backward_x(const macx_opts*, const macx_shapes*, const macx_dropout*, const macx_params*,
                       const macx_inputs*, const float* saved, size_t saved_floats,
                       float* ws, size_t ws_floats,
                       const float* d_memory, const float* d_control,
                       const macx_param_grads*, const macx_input_grads*, const macx_state_grads*, void* stream);
int macx_cell_backward_phase_x(const macx_opts*, const macx_shapes*, const macx_dropout*, const macx_params*,
                       const macx_inputs*, const float* saved, size_t saved_floats,
                       float* ws, size_t ws_floats,
                       const float* d_memory, const float* d_control,
                       const macx_param_grads*, const macx_input_grads*, const macx_state_grads*, int phase, void* stream);

/* ---- output unit + classifier (consumer of the final memory) ------------------ */
/* outputOp (model.py:512-528, --outQuestion) + classifier (model.py:547-576 -> ops.FCLayer
 * ops.py:349-359) for outClassifierDims = [hidden]:
 *   logits = dropout(act(dropout(concat([memory, vecQ Woq + boq])) W0 + b0)) W1 + b1
 * Variables: outputUnit/linearLayeroutQuestion, classifier/linearLayerfc_0, classifier/linearLayerfc_1. */
typedef struct macx_out_shapes {
  int32_t B, d, hidden, answers;  /* batch, memDim == ctrlDim, outClassifierDims[0], answerWordsNum */
  int32_t b0;                     /* global index of question 0 (dropout stream) */
} macx_out_shapes;
typedef struct macx_out_params {
  const float* outQuestion_W; const float* outQuestion_b;   /* [d,d], [d]              */
  const float* fc0_W; const float* fc0_b;                   /* [2d,hidden], [hidden]   */
  const float* fc1_W; const float* fc1_b;                   /* [hidden,answers], [answers] */
} macx_out_params;
typedef struct macx_out_grads {
  float* outQuestion_W; float* outQuestion_b; float* fc0_W; float* fc0_b; float* fc1_W; float* fc1_b;
} macx_out_grads;
size_t macx_output_saved_floats(const macx_out_shapes*);
size_t macx_output_ws_floats(const macx_out_shapes*);
/* act: resolved activation of "RELU" (config.relu); keep: outputDropout (1.0 in evaluation). */
int macx_output_forward(const macx_out_shapes*, int act, float keep, uint32_t seed, const macx_out_params*,
                        const float* memory, const float* vecQuestions, float* logits,
                        float* saved, size_t saved_floats, void* stream);
int macx_output_backward(const macx_out_shapes*, int act, float keep, uint32_t seed, const macx_out_params*,
                         const float* memory, const float* vecQuestions, const float* saved, size_t saved_floats,
                         float* ws, size_t ws_floats, const float* d_logits, const macx_out_grads*,
                         float* d_memory, float* d_vecQuestions, void* stream);
/* The same two calls under a run's mask word.  mask_word: one 32-bit word in DEVICE memory (NULL == 0), XORed into the site key of
 * both layer-input dropouts (sites 7, 8) when the kernels RUN, exactly as macx_dropout.mask_word inside the cell: a captured
 * graph bakes `seed` but draws the masks of (seed, *mask_word) on every replay.  The backward call must see the word the
 * forward call saw.  NULL, or a word holding 0, gives the bits of the calls above (which forward here with NULL). */
int macx_output_forward_w(const macx_out_shapes*, int act, float keep, uint32_t seed, const macx_out_params*,
                          const float* memory, const float* vecQuestions, float* logits,
                          float* saved, size_t saved_floats, const uint32_t* mask_word, void* stream);
int macx_output_backward_w(const macx_out_shapes*, int act, float keep, uint32_t seed, const macx_out_params*,
                           const float* memory, const float* vecQuestions, const float* saved, size_t saved_floats,
                           float* ws, size_t ws_floats, const float* d_logits, const macx_out_grads*,
                           float* d_memory, float* d_vecQuestions, const uint32_t* mask_word, void* stream);

/* ---- stem CNN (producer of the knowledge base) -------------------------------- */
/* MACnet.stem (model.py:165-204) -> ops.CNNLayer / ops.cnn (ops.py:380-438) for the default
 * stemNumLayers = 2, stemKernelSize = 3, stride 1, no batch norm:
 *   KB = act(conv3x3_SAME(dropout(act(conv3x3_SAME(dropout(images), K0) + b0)), K1) + b1)
 * images [B, H*W, Cin] NHWC (config.imageDims = 14 x 14 x 1024), KB [B, H*W, Cout] (model.py:202).
 * Variables: stem/cnnLayercnn_{0,1}/kernels/kernel [3,3,in,out] (HWIO), .../biases/bias [out].
 * Cin, Cmid, Cout multiples of 128.  No gradient is returned for `images` (pre-extracted features).
 * Limits (anything else: the size calls return 0, the others MACX_EINVAL): W >= 2, H W <= 1024, (b0 + B) H W max(Cin, Cmid) < 2^32
 * (the dropout's element index), and, with N = H W and e = ceil(2^32 / N) N - 2^32, (B N - 1) e < 2^32 unless e = 0 (the kernel
 * gradients divide a flattened row by N with one 32-bit multiply: about 4,100 images at N = 1023, 6,100 at N = 1000). */
typedef struct macx_stem_shapes { int32_t B, H, W, Cin, Cmid, Cout, b0; } macx_stem_shapes;
typedef struct macx_stem_params { const float* kernel0; const float* bias0; const float* kernel1; const float* bias1; } macx_stem_params;
typedef struct macx_stem_grads { float* kernel0; float* bias0; float* kernel1; float* bias1; } macx_stem_grads;
size_t macx_stem_saved_floats(const macx_stem_shapes*);
size_t macx_stem_ws_floats(const macx_stem_shapes*);
int macx_stem_forward(const macx_stem_shapes*, int act, float keep, uint32_t seed, const macx_stem_params*,
                      const float* images, float* kb, float* saved, size_t saved_floats, void* stream);
int macx_stem_backward(const macx_stem_shapes*, int act, float keep, uint32_t seed, const macx_stem_params*,
                       const float* kb, const float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                       const float* d_kb, const macx_stem_grads*, void* stream);
/* Under a run's mask word (device memory, NULL == 0; see macx_output_forward_w): XORed into the keys of both layer-input dropouts
 * (sites 9, 10) when the forward kernels run.  The backward pass hashes nothing -- layer 0's dropped input and layer 1's keep
 * bits are in `saved` -- so macx_stem_backward_w takes the word for symmetry and ignores it. */
int macx_stem_forward_w(const macx_stem_shapes*, int act, float keep, uint32_t seed, const macx_stem_params*,
                        const float* images, float* kb, float* saved, size_t saved_floats, const uint32_t* mask_word, void* stream);
int macx_stem_backward_w(const macx_stem_shapes*, int act, float keep, uint32_t seed, const macx_stem_params*,
                         const float* kb, const float* saved, size_t saved_floats, float* ws, size_t ws_floats,
                         const float* d_kb, const macx_stem_grads*, const uint32_t* mask_word, void* stream);

/* ---- general convolution (the generic stem: any --stemNumLayers / --stemKernelSize(s) / --stemStrideSizes) ---------- */
/* ops.cnn's tf.nn.conv2d(inp, kernel, strides = [1, s, s, 1], padding = "SAME") (ops.py:380-411) for any kernel size k >= 1
 * and stride s >= 1, as implicit GEMMs on exact-fp32 MFMA (no im2col buffer):
 *   Ho = ceil(H / s), pad_total = max((Ho - 1) s + k - H, 0), pad_top = pad_total / 2 (the odd row at the bottom); same along W.
 *   macx_conv2d_fwd       y [B,Ho,Wo,Cout] = conv(x [B,H,W,Cin], w [k,k,Cin,Cout] (HWIO)) (+ bias [Cout] unless NULL)
 *   macx_conv2d_bwd_data  dx [B,H,W,Cin] = d conv / dx applied to dy [B,Ho,Wo,Cout]
 *   macx_conv2d_wgrad     dw [k,k,Cin,Cout] = d conv / dw applied to dy; ws >= macx_conv2d_ws_floats floats (may be 0 / NULL).
 *                         Fixed-order split-K reduction: identical calls give identical bits.
 * Cin and Cout multiples of 4, every pointer 16-byte aligned, B*H*W and B*Ho*Wo < 2^31; anything else is MACX_EINVAL and
 * nothing is launched.  The bias gradient is a column sum of dy (macx_op_reduce ROWS). */
typedef struct macx_conv_shapes { int32_t B, H, W, Cin, Cout, k, stride; } macx_conv_shapes;
size_t macx_conv2d_ws_floats(const macx_conv_shapes*);
int macx_conv2d_fwd(const macx_conv_shapes*, const float* x, const float* w, const float* bias, float* y, void* stream);
int macx_conv2d_bwd_data(const macx_conv_shapes*, const float* dy, const float* w, float* dx, void* stream);
int macx_conv2d_wgrad(const macx_conv_shapes*, const float* x, const float* dy, float* dw, float* ws, size_t ws_floats,
                      void* stream);

/* Feed-dict image layout (model.py:67-68): the h5 features are [B, C, H, W] (extract_features.py) and the graph
 * transposes them to NHWC before the stem.  nhwc[b][hw][c] = nchw[b][c][hw]. */
int macx_images_to_nhwc(const float* nchw, int B, int C, int HW, float* nhwc, void* stream);

/* ---- question encoder (producer of vecQuestions / questionCntxWords) ---------- */
/* qEmbeddingsOp (model.py:208-221) + encoder (model.py:255-307) for encType = LSTM, encBi,
 * encNumLayers = 1: embedding lookup (index 0 = zero pad row), dropout(encInputDropout), a
 * bidirectional BasicLSTMCell(h = encDim/2) under tf.nn.bidirectional_dynamic_rnn semantics,
 * questionCntxWords = concat(fw, bw) [B,S,2h], vecQuestions = dropout(concat(final h), qDropout).
 * Variables: qEmbeddings/emb [V,E]; encoder/birnnLayer/bidirectional_rnn/{fw,bw}/basic_lstm_cell/
 * {kernel [E+h,4h], bias [4h]} (gate order i, j, f, o; forget bias 1).  h % 128 == 0 (else MACX_EINVAL) and h <= 512:
 * the backward step holds the gate gradients of 16 questions in LDS, (16 (4h + 4) + 4608) * 4 bytes, which passes a CU's
 * 160 KB (163,840 B) at h = 640.  A wider h is MACX_EUNSUPPORTED in every call below, and both sizing calls return 0. */
typedef struct macx_enc_shapes { int32_t B, S, V, E, h, b0; } macx_enc_shapes;   /* V rows in emb (ids 1..V) */
typedef struct macx_enc_params { const float* emb; const float* fw_kernel; const float* fw_bias; const float* bw_kernel; const float* bw_bias; } macx_enc_params;
typedef struct macx_enc_grads { float* emb; float* fw_kernel; float* fw_bias; float* bw_kernel; float* bw_bias; } macx_enc_grads;
size_t macx_encoder_saved_floats(const macx_enc_shapes*);
size_t macx_encoder_ws_floats(const macx_enc_shapes*);
int macx_encoder_forward(const macx_enc_shapes*, float keep_input, float keep_question, uint32_t seed, const macx_enc_params*,
                         const int32_t* questions /*[B,S]*/, const int32_t* lengths /*[B]*/, float* words /*[B,S,2h]*/,
                         float* vecQuestions /*[B,2h]*/, float* saved, size_t saved_floats, void* stream);
int macx_encoder_backward(const macx_enc_shapes*, float keep_input, float keep_question, uint32_t seed, const macx_enc_params*,
                          const int32_t* questions, const int32_t* lengths, const float* saved, size_t saved_floats,
                          float* ws, size_t ws_floats, const float* d_words, const float* d_vecQuestions,
                          const macx_enc_grads*, void* stream);
/* Under a run's mask word (device memory, NULL == 0; see macx_output_forward_w): XORed into the keys of the input dropout
 * (site 11) and the question dropout (site 12) when the kernels run.  Both sites are re-hashed by the backward pass (the
 * embedding gradient and d vecQuestions), which must therefore see the word the forward pass saw. */
int macx_encoder_forward_w(const macx_enc_shapes*, float keep_input, float keep_question, uint32_t seed, const macx_enc_params*,
                           const int32_t* questions /*[B,S]*/, const int32_t* lengths /*[B]*/, float* words /*[B,S,2h]*/,
                           float* vecQuestions /*[B,2h]*/, float* saved, size_t saved_floats, const uint32_t* mask_word,
                           void* stream);
int macx_encoder_backward_w(const macx_enc_shapes*, float keep_input, float keep_question, uint32_t seed, const macx_enc_params*,
                            const int32_t* questions, const int32_t* lengths, const float* saved, size_t saved_floats,
                            float* ws, size_t ws_floats, const float* d_words, const float* d_vecQuestions,
                            const macx_enc_grads*, const uint32_t* mask_word, void* stream);

/* ---- question encoder, every cell ops.createCell builds with an activation (ops.py:749-772) ------ */
/* The encoder above for encType RNN | GRU | LSTM in one direction (ops.fwRNNLayer: tf.nn.dynamic_rnn, h = encDim) or two
 * (ops.biRNNLayer, h = encDim/2); (MACX_RNN_LSTM, 2) runs macx_encoder_*'s launches and returns their bits.
 *   MACX_RNN_BASIC  BasicRNNCell   h' = tanh([x, h] kernel + bias)                       kernel [E+h, h]
 *   MACX_RNN_GRU    GRUCell        r, u = split(sigmoid([x, h] kernel + bias))           kernel [E+h, 2h]  (gru_cell/gates)
 *                                  c = tanh([x, r h] candidate_kernel + candidate_bias)  candidate_kernel [E+h, h]
 *                                  h' = u h + (1 - u) c
 *   MACX_RNN_LSTM   BasicLSTMCell  as macx_encoder_*                                     kernel [E+h, 4h]
 * words [B,S,dirs h] (+0 past a question's end), vecQuestions [B,dirs h] = dropout(concat of the final h).  One launch per
 * time step and pass for all directions; the GRU two (gates, then candidate: r h of all units; backward: d(r h), then the gates).
 * Pointers the cell or the direction count does not use (bw_* with dirs == 1, *candidate* outside the GRU) are ignored and may
 * be NULL; a NULL one among those it needs is MACX_EINVAL, as are cell / dirs out of range and h % 128 != 0.  h > 512 is
 * MACX_EUNSUPPORTED in every call and both sizing calls return 0 (one bound for all cells: the LSTM's backward LDS tile).
 * The argument lists are macx_encoder_forward_w's / _backward_w's. */
enum { MACX_RNN_BASIC = 0, MACX_RNN_GRU = 1, MACX_RNN_LSTM = 2 };
typedef struct macx_rnn_shapes { int32_t B, S, V, E, h, b0, cell, dirs; } macx_rnn_shapes;   /* V rows in emb (ids 1..V) */
typedef struct macx_rnn_params {
  const float* emb; const float* fw_kernel; const float* fw_bias; const float* bw_kernel; const float* bw_bias;
  const float* fw_candidate_kernel; const float* fw_candidate_bias; const float* bw_candidate_kernel; const float* bw_candidate_bias;
} macx_rnn_params;
typedef struct macx_rnn_grads {
  float* emb; float* fw_kernel; float* fw_bias; float* bw_kernel; float* bw_bias;
  float* fw_candidate_kernel; float* fw_candidate_bias; float* bw_candidate_kernel; float* bw_candidate_bias;
} macx_rnn_grads;
size_t macx_rnn_encoder_saved_floats(const macx_rnn_shapes*);
size_t macx_rnn_encoder_ws_floats(const macx_rnn_shapes*);
int macx_rnn_encoder_forward_w(const macx_rnn_shapes*, float keep_input, float keep_question, uint32_t seed, const macx_rnn_params*,
                               const int32_t* questions /*[B,S]*/, const int32_t* lengths /*[B]*/, float* words /*[B,S,dirs h]*/,
                               float* vecQuestions /*[B,dirs h]*/, float* saved, size_t saved_floats, const uint32_t* mask_word,
                               void* stream);
int macx_rnn_encoder_backward_w(const macx_rnn_shapes*, float keep_input, float keep_question, uint32_t seed, const macx_rnn_params*,
                                const int32_t* questions, const int32_t* lengths, const float* saved, size_t saved_floats,
                                float* ws, size_t ws_floats, const float* d_words, const float* d_vecQuestions,
                                const macx_rnn_grads*, const uint32_t* mask_word, void* stream);

/* ---- optimizer step ---------------------------------------------------------- */
/* addTrainingOp (model.py:639-669) over ONE flat fp32 buffer of n elements:
 *   norm = ||g||_2 ; g *= clip / max(norm, clip)      tf.clip_by_global_norm, clip_norm <= 0 disables
 *   Adam (tf.train.AdamOptimizer): m, v, p -= lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)
 *   ema -= (1 - decay) * (ema - p)                    tf.train.ExponentialMovingAverage, decay < 0 disables
 * `step` is 1-based; `ws` >= 1024 floats; `norm_out` (device, may be NULL) receives the pre-clip norm. */
int macx_adam_ema_step(size_t n, float* params, const float* grads, float* m, float* v, float* ema,
                       float lr, float beta1, float beta2, float eps, int step, float clip_norm, float ema_decay,
                       float* ws, float* norm_out, void* stream);
/* The same step with the bias-corrected rate in DEVICE memory: lr_t_dev[0] = (float)(lr * sqrt(1 - b2^t) / (1 - b1^t)), computed
 * by the caller in double as the call above computes it, read by the update kernel when it RUNS.  A captured graph therefore
 * follows the step count and a changed learning rate: write the 4 bytes between replays, outside the graph.  With the same
 * rate the result is bit-identical to macx_adam_ema_step. */
int macx_adam_ema_step_p(size_t n, float* params, const float* grads, float* m, float* v, float* ema,
                         const float* lr_t_dev, float beta1, float beta2, float eps, float clip_norm, float ema_decay,
                         float* ws, float* norm_out, void* stream);
/* The two steps above under a guard: the arguments of the namesake with `skip_above` and `guard` in front of `ws`.  The same two
 * launches; the update kernel decides from the norm it has just folded, every workgroup from the same partials in the same
 * order, so all of them decide alike.
 *   The step is SKIPPED iff  !(norm <= FLT_MAX) || (skip_above > 0 && norm > skip_above)
 * The first clause covers a NaN or an infinity anywhere in `grads` and a sum of squares that overflows fp32 (one finite element
 * of 3e19 is enough: its square is no float); skip_above == 0 means no threshold, and the comparison is strictly greater.
 * A skipped step leaves all state untouched: no byte of params, m, v, ema is written; norm_out[0] still receives the norm (the
 * non-finite value, or the one above the threshold).  An applied step writes exactly the bits of the unguarded call.
 * guard: four uint32 words in DEVICE memory, 4-byte aligned, zeroed by the caller before the first step:
 *   [0] steps applied   [1] steps skipped   [2] attempt index of the first skipped step (1-based, 0: none)   [3] of the last
 * The attempt index of a step is guard[0] + guard[1] + 1 as read before its update.  The words are written by one thread with plain
 * loads and stores (no atomics): steps that share them must be ordered on one stream, as steps that share params are anyway.
 * `step` and lr_t_dev stay the caller's and count attempts; guard[0] is the number of updates m and v have seen.
 * MACX_EINVAL (nothing is launched): what the namesake refuses, guard NULL or off a 4-byte boundary, skip_above < 0 or NaN. */
int macx_adam_ema_step_g(size_t n, float* params, const float* grads, float* m, float* v, float* ema,
                         float lr, float beta1, float beta2, float eps, int step, float clip_norm, float ema_decay,
                         float skip_above, uint32_t* guard, float* ws, float* norm_out, void* stream);
int macx_adam_ema_step_pg(size_t n, float* params, const float* grads, float* m, float* v, float* ema,
                          const float* lr_t_dev, float beta1, float beta2, float eps, float clip_norm, float ema_decay,
                          float skip_above, uint32_t* guard, float* ws, float* norm_out, void* stream);

/* ---- flat gather -------------------------------------------------------------------------------- */
/* ONE launch copies `entries` tensors into their slices of a flat buffer: flat[dst_offset .. dst_offset + count) = src[0 .. count)
 * per table entry; src == NULL zero-fills the slice (a parameter that received no gradient).  The table lives in device memory
 * (8-byte aligned) and is read when the kernel runs.  Slices must not overlap each other or a source; floats of `flat` outside
 * every slice (the pad between 16-byte aligned segments) are not written.  Entries whose source and destination are both 16-byte
 * aligned move as dwordx4, the others and every tail float by float.  The workgroup-to-chunk mapping is a function of the table
 * alone (chunks of 1024 floats, dealt round-robin); no atomics.  The caller guarantees that every slice lies inside `flat`. */
typedef struct macx_gather_entry { const float* src; uint64_t dst_offset; uint64_t count; } macx_gather_entry;
int macx_gather_flat(const macx_gather_entry* table_dev, int entries, float* flat, void* stream);

/* ---- questions that share images ---------------------------------------------------------------- */
/* A batch of B questions about G images (an evaluation set has many questions per image): the stem runs on the G images and each
 * question's knowledge-base block [N, d] is a copy of its image's block.
 *   macx_kb_gather      kb[b] = kb_images[image_index[b]]
 *   macx_kb_gather_bwd  dkb_images[g] = sum over {b : image_index[b] == g} of dkb[b]
 * image_index: [B] int32 in DEVICE memory, read when the kernel runs (a captured graph follows an index rewritten between replays).
 * Forward: an index outside [0, G) is never dereferenced; that question's block is filled with quiet NaN (the call still returns
 * MACX_OK: the index is device data), every other block is exact.  Nothing outside kb[0 .. B*N*d) is written.
 * Backward: no atomics.  Each output element is summed by one thread over b = 0 .. B-1 in ascending order with plain fp32 adds
 * starting from +0, so identical calls give identical bits; an image that no question names gets zeros; every element of
 * dkb_images is written (no clearing beforehand); an index outside [0, G) contributes nowhere.
 * MACX_EINVAL (nothing is launched): G, B, N or d < 1, N*d % 4 != 0, a NULL pointer, a float pointer off a 16-byte boundary.
 * Like every call here: no allocation, no memcpy / memset, stream-ordered only. */
int macx_kb_gather(const float* kb_images /*[G,N,d]*/, const int32_t* image_index /*[B], device*/, int G, int B, int N, int d,
                   float* kb /*[B,N,d]*/, void* stream);
int macx_kb_gather_bwd(const float* dkb /*[B,N,d]*/, const int32_t* image_index /*[B], device*/, int G, int B, int N, int d,
                       float* dkb_images /*[G,N,d]*/, void* stream);
/* The same two with a knowledge-base SIZE per image (object features padded to a common N, grids of mixed sizes): with shared images
 * the size belongs to the image, and the size of question b's knowledge base is that of the image it names.
 * image_lengths: [G] int32 in DEVICE memory, read when the kernel runs like the index; L_g = clamp(image_lengths[g], 1, N), the
 * clamp of macx_kb_attend_fwd_l.  NULL: exactly the plain call above (same kernel, same bits; kb_lengths_out is not written).
 * Forward: rows n < L_g of question b are the copy of its image's rows; rows n >= L_g are written as +0.0f WITHOUT reading the
 * source (what the stem computed in padded rows never reaches the cell, whose backward pass wants finite padding);
 * kb_lengths_out[b] = L_g -- the per-question lengths the cell takes (macx_inputs.kbLengths), made on the device so that a captured
 * graph follows an index and lengths rewritten between replays.  An index outside [0, G) gives the all-NaN block of the plain call
 * and kb_lengths_out[b] = N, so the poison reaches the result.
 * Backward: rows n < L_g of image g are the ascending-b fp32 sum of the plain call; rows n >= L_g are written as zeros without
 * reading dkb; an image that no question names is all zeros; no atomics.
 * MACX_EINVAL as above, and for d % 4 != 0 (a row is d/4 16-byte quads) or an int32 pointer off a 4-byte boundary. */
int macx_kb_gather_l(const float* kb_images /*[G,N,d]*/, const int32_t* image_index /*[B], device*/,
                     const int32_t* image_lengths /*[G], device, or NULL*/, int G, int B, int N, int d, float* kb /*[B,N,d]*/,
                     int32_t* kb_lengths_out /*[B], device*/, void* stream);
int macx_kb_gather_bwd_l(const float* dkb /*[B,N,d]*/, const int32_t* image_index /*[B], device*/,
                         const int32_t* image_lengths /*[G], device, or NULL*/, int G, int B, int N, int d,
                         float* dkb_images /*[G,N,d]*/, void* stream);

/* ---- image features resident in device memory ------------------------------------------------- */
/* The whole feature set of a dataset as ONE device table [rows][HW][C] (NHWC rows, what macx_stem_forward reads), fp32 or fp16,
 * filled once from the feature file's chunks; a batch then names its images by row id.
 *   macx_features_pack    table[row0 + i] = convert(src[i]), i = 0 .. n-1, and nothing else is written
 *   macx_features_gather  out[g] = (float) table[ids[g]]
 * dtype: MACX_FEATURES_F32 | MACX_FEATURES_F16.  layout: 0 = src is [n][C][HW] (the h5 file's; the transpose of
 * macx_images_to_nhwc per image, tiled through LDS), 1 = src is [n][HW][C].  rows < 2^31; row0 and rows are 64-bit and travel as
 * size_t: a negative value of a signed caller arrives as 2^63 or more and is refused like any other row0 + n > rows.
 * Pack: fp32 -> fp16 is round-to-nearest-even with subnormals kept and the sign of zero preserved; an fp32 table takes the source
 * bits.  overflow (int32 in DEVICE memory, or NULL): a source value that is NaN or infinite, or that rounds to an infinity, is
 * stored as such AND the constant 1 is written to overflow[0] (a plain store from every thread that sees one, no atomics).  The
 * call never clears the word: zero it once, pack every chunk, read it once.
 * Gather: ids [G] int32 in DEVICE memory, read when the kernel runs (a captured graph follows ids rewritten between replays).  An
 * id outside [0, rows) is never dereferenced; that image's block is filled with quiet NaN (the call still returns MACX_OK: the id
 * is device data), every other block is exact (fp16 -> fp32 loses nothing).  Nothing outside out[0 .. G*HW*C) is written.  For an
 * fp32 table this is the copy kernel of macx_kb_gather, bit for bit.
 * MACX_EINVAL (nothing is launched): a NULL table, src, out or ids; n, G, C, HW or rows < 1; C*HW % 4 != 0; rows >= 2^31;
 * row0 + n > rows; a dtype or layout other than the listed values; a float or table pointer off a 16-byte boundary, an int32
 * pointer off a 4-byte boundary.  Like every call here: no allocation, no memcpy / memset, stream-ordered only. */
enum { MACX_FEATURES_F32 = 0, MACX_FEATURES_F16 = 1 };
int macx_features_pack(const float* src, int layout, int n, int C, int HW, void* table, int dtype, size_t row0, size_t rows,
                       int32_t* overflow /*[1], device, or NULL*/, void* stream);
int macx_features_gather(const void* table, int dtype, size_t rows, const int32_t* ids /*[G], device*/, int G, int C, int HW,
                         float* out /*[G,HW,C]*/, void* stream);

/* ---- questions resident in device memory ------------------------------------------------------- */
/* A question set as per-question DEVICE tables (a CLEVR split: 700 k x 50 int32 = 140 MB), validated once on the host; a batch then
 * names its questions by id, and ONE launch fills every per-question static input of the tower's captured graphs:
 *   macx_questions_gather  slot b of every output <- question ids[b]
 *   macx_preds_scatter     table[ids[b]] = pred[b]
 * ids: [B] int32 in DEVICE memory, read when the kernel runs (a captured graph follows ids rewritten between replays).
 * Tables: q_words [Q,S_tab] and q_lengths [Q] are required; q_answers, q_images (rows of a feature table), q_kb_len and q_weights may
 * be NULL.  An output column (answers, image_ids, kb_lengths) whose table is NULL is refused; `weights` without q_weights is taken:
 * live slots then get 1.0f.  An output that is NULL is not written.  Per slot b, id = ids[b]:
 *   live   0 <= id < Q     questions[b] = q_words[id] in columns 0 .. S_tab-1 and 0 (the pad id) in columns S_tab .. S-1; every scalar
 *                          column from its table; weights[b] = q_weights[id], or 1.0f without a table.
 *   dead   id == -1        every integer column is that of slot 0's question -- finite, in range, the same launches downstream --
 *                          and weights[b] = +0.0f.  If slot 0 is not live itself: the pad question (words 0, length 0, answer 0,
 *                          image row 0, kb length 1).
 *   other  any other id    is never dereferenced (it is compared before it is used as an offset).  Poison, never silently wrong:
 *                          words 0, length 0, answer -1 (a NaN loss and NaN totals in the weighted answer loss), image row -1 (a NaN
 *                          block in the feature gather), kb length 1, weight 1.0f -- not NaN, which the loss kernel counts as dead --
 *                          and the constant 1 is written to bad[0] (int32 in DEVICE memory, or NULL): a plain store from every thread
 *                          that sees such an id, no atomics.  The call never clears the word.  The call still returns MACX_OK.
 * Grouping (image_index != NULL; needs q_images and image_ids, G >= 1, B <= 1024): image_ids is [G] and the batch's images are
 * grouped on the device.  The distinct image rows of the LIVE slots are numbered in order of first appearance by slot;
 * image_ids[g] = the g-th distinct row; image_index[b] = the group of slot b's row.  Dead slots take slot 0's group, which is 0 (a
 * live slot 0 opens group 0; without one, group 0 still names a valid image).  Image slots beyond the D distinct rows are copies of
 * image_ids[0] (no live slot at all: row 0).  D > G: the slots whose row did not fit get image_index = -1 (a NaN block in the
 * knowledge-base gather) and bad[0] = 1.  A slot of the `other` kind joins no group: image_index = -1.
 * One workgroup holds the whole batch in LDS and finds first occurrences by linear search -- quadratic in B, fine for the intended
 * range of a few hundred questions (B = 1024: about 4 k LDS reads per thread), which is why B is capped.
 * Rows move as 16-byte accesses where S_tab % 4 == 0, S % 4 == 0 and q_words and questions sit on 16-byte boundaries, as 8-byte
 * accesses where both are even and the pointers sit on 8-byte boundaries, dword by dword otherwise: a pointer a vector path would
 * need aligned is not refused but sent to the next narrower path.  Offsets are 64-bit; any B is covered by a capped grid-stride
 * grid.  Identical calls give identical bits; nothing outside the outputs' [B] / [B,S] / [G] extents is written.
 * macx_preds_scatter: for every slot with 0 <= ids[b] < Q, table[ids[b]] = pred[b]; dead and other slots write nothing; the rest of
 * the table is not touched.  An id that appears twice in a batch takes the HIGHEST slot's value: a slot stores only if no later slot
 * names its id (a linear search: quadratic in B, meant for batches up to a few thousand), so the result does not depend on the
 * order in which stores retire.
 * MACX_EINVAL (nothing is launched or written): a NULL q_words, q_lengths, ids, questions or lengths (scatter: pred, ids or table);
 * Q, S_tab or B < 1; S < S_tab; Q >= 2^31; an output column without its table; grouping without q_images or image_ids, with G < 1 or
 * B > 1024; an int32 or float pointer off a 4-byte boundary.  Like every call here: no allocation, no memcpy / memset,
 * stream-ordered only. */
int macx_questions_gather(const int32_t* q_words /*[Q,S_tab]*/, const int32_t* q_lengths /*[Q]*/, const int32_t* q_answers /*[Q] or NULL*/,
                          const int32_t* q_images /*[Q] or NULL*/, const int32_t* q_kb_len /*[Q] or NULL*/,
                          const float* q_weights /*[Q] or NULL*/, int Q, int S_tab, const int32_t* ids /*[B], device*/, int B,
                          int S /* >= S_tab */, int32_t* questions /*[B,S]*/, int32_t* lengths /*[B]*/, int32_t* answers /*[B] or NULL*/,
                          int32_t* image_ids /*[B], [G] when grouping, or NULL*/, int32_t* kb_lengths /*[B] or NULL*/,
                          float* weights /*[B] or NULL*/, int32_t* image_index /*[B] or NULL: grouping*/, int G,
                          int32_t* bad /*[1], device, or NULL*/, void* stream);
int macx_preds_scatter(const int32_t* pred /*[B]*/, const int32_t* ids /*[B], device*/, int B, int Q, int32_t* table /*[Q]*/,
                       void* stream);

/* ---- evaluation records resident in device memory ---------------------------------------------- */
/* A run's attention maps and logits filed by question id, as macx_preds_scatter files its predictions: per-question DEVICE tables
 * [Q][steps][n] (fp32 or fp16), and ONE launch that files a batch into up to MACX_RECORDS_MAX of them.  The descriptors are a HOST
 * array, taken by value when the call is made (they travel in the kernel argument; the array may be reused at once):
 *   src     [steps][B][n] fp32, contiguous: a viewable segment of a run's `saved` (MACX_SEG_ATT_KB, MACX_SEG_ATT_QUESTION,
 *           MACX_SEG_ATT_SELF through macx_saved_segment), or the logits as [1][B][answers]
 *   table   [Q][steps][n] of dtype, contiguous;  dtype: MACX_FEATURES_F32 | MACX_FEATURES_F16
 * ids: [B] int32 in DEVICE memory, read when the kernel runs (a captured graph follows ids rewritten between replays); B and Q are
 * shared by the tables of a call.
 * Live slots: for every slot b with 0 <= ids[b] < Q, table[ids[b]][i][j] = convert(src[i][b][j]) for all i < steps, j < n -- a
 * transpose from step-major to question-major.
 * Other slots: a dead slot (-1) and any other id write nothing and are never used as an offset (the id is compared first).  Table
 * rows that no slot names are not touched.
 * Repeated ids: an id named by several slots takes the HIGHEST slot's rows.  A slot stores only if no later slot names its id; that
 * is decided by comparison (one strided scan of ids[b+1 .. B) by the wave that owns the row, and a wave vote), never by the order
 * in which stores retire.  No atomics.  Identical calls give identical bits.
 * Conversion: fp32 -> fp32 copies the bits.  fp32 -> fp16 is the hardware's round-to-nearest-even with subnormals kept and the
 * sign of zero preserved; NaN stays NaN (a poisoned question's map stays loud); a value that rounds past 65504 becomes an
 * infinity -- torch's CPU .to(torch.float16) bit for bit, as macx_features_pack promises.
 * Access: offsets are 64-bit; the grid is capped and grid-stride.  Rows move as 16-byte source accesses (four elements) where
 * n % 4 == 0, src sits on a 16-byte boundary and table on a boundary of four of its elements, as 8-byte source accesses (two
 * elements) where n % 2 == 0 and the pointers allow that, element by element otherwise: a pointer off the vector boundary takes
 * the narrower path, it is not refused.  Nothing outside the tables' [Q][steps][n] extents is written.
 * MACX_EINVAL (nothing is launched or written): count outside [1, MACX_RECORDS_MAX]; a NULL descs, ids, src or table; steps, n, B
 * or Q < 1; Q >= 2^31; a dtype other than the listed values; a src or ids off a 4-byte boundary, a table off its element size.
 * Like every call here: no allocation, no memcpy / memset, stream-ordered only. */
enum { MACX_RECORDS_MAX = 4 };
typedef struct macx_record_desc {
  const float* src;
  void* table;
  int32_t steps, n, dtype;
} macx_record_desc;
int macx_records_scatter(const macx_record_desc* descs /*[count], host*/, int count, const int32_t* ids /*[B], device*/, int B, int Q,
                         void* stream);

/* ---- unit-level entry points (the ops.py primitives; used by the parity tests) -------------- */
/* out[r, :] = act(concat(x1[r], x2[r]) @ W + b + bias_const)     ops.linear (ops.py:298-333)
 * on fp32 MFMA; `W_packed` from macx_pack_weight(W, k1 + k2, n_out, 0); k1, k2, n_out % 16 == 0. */
int macx_linear(const float* x1, int k1, const float* x2, int k2, int rows,
                const float* W_packed, const float* b, float bias_const, int n_out, int act,
                float* out, void* stream);
/* The same linear with its input row r given as per-tile partial sums, as the backward recurrence's dy linear runs it:
 * x[r] = ((p0 + p1) + p2) + ... over the tiles of 2^part_shift rows (4 .. 6) that rows [r * part_N, (r + 1) * part_N) of a
 * [rows * part_N]-row matrix touch, in ascending order; part[tile][3][k], a tile's slot for row r being r minus the first r
 * whose range reaches into the tile.  part_sum[rows][k] receives x.  rows <= 128, ((part_N - 2) >> part_shift) + 2 <= 6,
 * 2^part_shift <= 2 part_N (three slots per tile), k, n_out % 16 == 0. */
int macx_linear_part(const float* part, int part_N, int part_shift, int k, int rows,
                     const float* W_packed, const float* b, float bias_const, int n_out, int act,
                     float* part_sum, float* out, void* stream);
/* Re-lays a [K, n_out] weight (flags bit 0 = 0) or the transpose of a [n_out, K] weight (bit 0 = 1) into the operand
 * order a kernel reads; flags bits 1-2 select the format:
 *   MACX_PACK_F32MFMA (0)  out[Q][g][j][e] = W[16Q + 4g + e][j]            fp32, K*n_out floats   (macx_linear, native GEMM)
 *   MACX_PACK_BF16X3  (1)  out[K/32][3][n_out][32] bf16: the exact split W = W1 + W2 + W3 of every element into three
 *                          bf16 pieces (round-to-nearest residual chain), K*n_out*3/2 floats      (split GEMM)
 *   MACX_PACK_KMAJOR  (2)  out[K/32][n_out][32] fp32 k-major tiles, K*n_out floats
 * K % 16 == 0 (K % 32 for formats 1, 2), n_out % 16 == 0. */
#define MACX_PACK_TRANSPOSE 1
#define MACX_PACK_F32MFMA (0 << 1)
#define MACX_PACK_BF16X3 (1 << 1)
#define MACX_PACK_KMAJOR (2 << 1)
int macx_pack_weight(const float* W, int K, int n_out, int flags, float* out, void* stream);
/* Which kernel family runs the knowledge-base GEMMs (projX, memKbProj, memKbProj_2, their backward-data products, the
 * weight-gradient contractions and the stem's implicit-GEMM convolutions).  gfx950 issues f32-input MFMA at 1/16 of the
 * 16-bit rate and has no TF32 form, so the large contractions run on the 16-bit matrix pipe at fp32-class accuracy:
 *   MACX_GEMM_H2 (default)  every [B,N,d] activation is stored ONCE, by its producer, as x 2^e = hi + lo (two fp16 planes,
 *                           |error| <= 2^-24, one int8 exponent per row and 128 columns); a product is 3 MFMA terms on
 *                           v_mfma_f32_16x16x32_f16 with fp32 accumulation (see "the H2 tensor format" below)
 *   MACX_GEMM_SPLIT         every fp32 operand is split exactly into three bf16 pieces while it is staged, 6 terms on
 *                           v_mfma_f32_16x16x32_bf16
 *   MACX_GEMM_NATIVE        v_mfma_f32_16x16x4_f32 (bit-equal to an fmaf chain)
 * Measured error against fp64 of all three: tests/test_gpu_h2.py, tests/test_gpu_units.py.
 * This call sets / queries (mode < 0) the PROCESS DEFAULT and returns it; a run selects its own family with
 * macx_opts.gemm_family, which is applied per call on the calling thread.  Packed-weight formats and buffer sizes differ
 * between families: use one family for the sizing, forward and backward calls of a run. */
#define MACX_GEMM_NATIVE 0
#define MACX_GEMM_SPLIT 1
#define MACX_GEMM_H2 2
int macx_gemm_mode(int mode);

/* ---- the H2 tensor format (mode MACX_GEMM_H2, the default; mac-network_amd/csrc/macx_h2.hip.h) ---------------------
 * An fp32 [rows, cols] tensor (cols % 128 == 0) held as two fp16 planes in slot order + one int8 exponent per (row, 128
 * columns): x * 2^e = hi + lo to 2^-24.  Inside the cell every [B,N,d] activation lives in HBM in this format; these
 * entry points expose the conversions and one GEMM on it so that the format and its numerics are testable in isolation.
 *   macx_h2_floats      floats a caller-owned buffer needs for one H2 tensor (0 if cols % 128)
 *   macx_h2_from_f32    src [B][N][C] fp32 row-major -> h2
 *   macx_h2_to_f32      h2 -> out [rows][C] fp32 row-major
 *   macx_h2_pack_weight W [K, n_out] (or its transpose, from [n_out, K]) -> H2 weight planes + exponent; out >= K*n_out + 16 floats
 *   macx_h2_gemm_planes hO = act(hA @ Wh + bias) on operands already in the format (what the cell launches per step; timed by
 *                       bench.py's roofline probe)
 *   macx_h2_gemm        out[B*N, n_out] = act(A[B*N, K] @ W[K, n_out] + bias): from_f32 + pack + gemm_planes + to_f32 (three fp16
 *                       MFMA terms per product, fp32 accumulate); ws >= h2_floats(B*N,K) + h2_floats(B*N,n_out) + K*n_out + 16 */
size_t macx_h2_floats(size_t rows, size_t cols);
int macx_h2_from_f32(const float* src, int B, int N, int C, float* h2, void* stream);
int macx_h2_to_f32(const float* h2, int rows, int C, float* out, void* stream);
int macx_h2_pack_weight(const float* W, int K, int n_out, int transpose, float* out, void* stream);
int macx_h2_gemm_planes(const float* hA, int B, int N, int K, const float* Wh, int n_out, const float* bias, int act, float* hO,
                        void* stream);
int macx_h2_gemm(const float* A, int B, int N, int K, const float* W, int n_out, const float* bias, int act, float* out,
                 float* ws, size_t ws_floats, void* stream);
/* The backward pass's contractions over the ROWS of H2 tensors (mac-network_amd/csrc/macx_wgrad_h2.hip.h), each on its own: the
 * functions that fill the kernels' parameter blocks and launch them for the fused cell's backward pass, called on the caller's
 * operands, plus a slab reduction per output (the cell reduces its four slab sets in one launch of its own) -- so that the kernels
 * and their launch code are testable against fp64 in isolation (tests/test_gpu_h2_contractions.py).  Operands are H2 tensors made with macx_h2_from_f32; a sequence of tensors lies `*_stride`
 * FLOATS apart (a multiple of 4, >= macx_h2_floats of one tensor).  `o`: NULL = defaults; its tune table selects the kernel forms
 * (MACX_TUNE_WGRAD_PIPE, MACX_TUNE_SB_CONT, MACX_TUNE_PHASE_MASK); the calls run in the H2 family whatever gemm_family says.
 * Dimensions are multiples of 128 up to 1024, at most 2^24 rows per call.  A refused call (MACX_EINVAL; MACX_ESMALL: ws_floats
 * below the sizing call's answer) launches nothing; the sizing calls return 0 for a shape the entry point refuses.
 *   macx_h2_wgrad   out[Kd][Jd] = sum_m A[m][k] G[m][j] over M = nt * R rows: reduction row m is row m % R of tensor m / R of A
 *                   (nt tensors [R][Kd]) and of G (nt tensors [R][Jd]); a_shared = 1: A is ONE tensor, row m % R of it for every
 *                   tensor of G.  nsplit >= 1 reduction splits of the library's own rows per split (a multiple of 32; a split
 *                   that starts at or behind M is empty and adds exact zeros).  hA2 / hG2 / out2: NULL all three, or a second
 *                   contraction of the same shape; at Kd % 256 == Jd % 256 == 0 and MACX_TUNE_WGRAD_PIPE >= 2 the two run as one
 *                   launch, as in the cell.  Launches: row-exponent minima (one launch at Kd == Jd, as in the cell; else one per
 *                   column count), factor tables, contraction(s), slab reduction.
 *   macx_h2_sb      per question b of each of nsteps steps S_b = X_b^T dI1_b (X, dI1: nsteps tensors [B*N][d]) and
 *                     dW1b[k][j] = sum S_b[k][j],   dW1a[k][j] = sum y[step][b][k] S_b[k][j]       (sums over steps and questions)
 *                   y [nsteps][B][d] fp32.  wide = 0: sb_h2_kernel (128 x 128 tiles); wide = 1: sb_h2w_kernel (128 x 256 tiles,
 *                   summation by parts; d % 256 == 0, N <= 512).  qpg: questions per workgroup, 0 = the route plan's own choice;
 *                   narrow: qpg <= 32 and qpg * roundup(N, 32) <= 4096, wide: qpg <= 4 and qpg * roundup(N, 32) <= 512.
 *                   dy_part (NULL, or wide = 0 and nsteps = 1 only; needs W1a [d][d] row-major (k, j)): the kernel's partials of
 *                   dy[b][k] = sum_j W1a[k][j] S_b[k][j] as it leaves them, [4 * d / 128][B][d]: partial 4 * tj + c holds the
 *                   sum over columns j in [128 tj + 32 c, 128 tj + 32 c + 32); dy is the sum over the 4 * d / 128 partials. */
size_t macx_h2_wgrad_ws_floats(const macx_opts* o, int nt, int R, int Kd, int Jd, int nsplit, int pair);
int macx_h2_wgrad(const macx_opts* o, int nt, int R, int Kd, int Jd, int nsplit, const float* hA, size_t a_stride, int a_shared,
                  const float* hG, size_t g_stride, float* out, const float* hA2, size_t a2_stride, int a2_shared, const float* hG2,
                  size_t g2_stride, float* out2, float* ws, size_t ws_floats, void* stream);
size_t macx_h2_sb_ws_floats(const macx_opts* o, int B, int N, int d, int nsteps, int qpg, int wide);
int macx_h2_sb(const macx_opts* o, int B, int N, int d, int nsteps, int qpg, int wide, const float* hX, size_t x_stride,
               const float* hdI1, size_t g_stride, const float* y, const float* W1a, float* dW1a, float* dW1b, float* dy_part,
               float* ws, size_t ws_floats, void* stream);
/* bench / profiling hook (mode MACX_GEMM_H2, d <= 512, N >= 16): the kernel that runs the read unit's three knowledge-base
 * products of one step -- dropout(KB) -> X -> H1 -> I2 -> attention logits (mac_cell.py:230-266, ops.py:668-725;
 * mac-network_amd/csrc/macx_chain_h2.hip.h) -- re-launched `reps` times on `stream` between two HIP events; *ms_out = average
 * milliseconds per launch.  `saved` comes from macx_cell_begin + macx_cell_step(.., step) with keep = 1; launch r writes the
 * buffers of step (step + r) % p, so the run must not be differentiated afterwards.  MACX_EUNSUPPORTED when this shape /
 * family does not run on that kernel. */
int macx_read_chain_time(const macx_opts*, const macx_shapes*, const macx_dropout*, const macx_params*, const macx_inputs*,
                         float* saved, size_t saved_floats, int step, int reps, float* ms_out, void* stream);
/* ... and IN A RUNNING FORWARD PASS: one macx_cell_forward (keep = 1) on `stream`, each of its p chain launches issued with a start
 * and a stop HIP event that receive the kernel's own dispatch timestamps (the step's [B,d] linear in front of a launch, the
 * attention kernel behind it, as in a training step), behind three untimed passes so that the chip is as busy as inside a training
 * loop; *ms_out = average milliseconds per launch of the timed pass.  Synchronises `stream`.
 * bench.py's roofline.kernel_ms. */
int macx_cell_forward_chain_time(const macx_opts*, const macx_shapes*, const macx_dropout*, const macx_params*, const macx_inputs*,
                                 float* saved, size_t saved_floats, float* ws, size_t ws_floats, float* ms_out, void* stream);
/* One of the read unit's kept [B*N, d] activations of step `step`, as fp32 row-major, from the `saved` buffer of a forward pass with
 * keep = 1: which = 0 dropout(KB) (ops.py:678), 1 X = dropout(KB) Wx + bx (ops.py:688), 2 H1 (ops.py:718, mac_cell.py:237), 3 I2
 * (ops.py:326) -- whatever format the kernel family keeps them in (H2 planes in the default family).  Inspection and tests: the chain
 * kernel's intermediate products are checked against fp64 through this.  out: [B*N][d] floats, 16-byte aligned. */
int macx_saved_activation(const macx_opts*, const macx_shapes*, int which, int step, const float* saved, size_t saved_floats,
                          float* out, void* stream);
/* The control unit's question projections on their own (mac_cell.py:442-448; SURVEY 8b's `ctrl_inputs` unit):
 *   fwd:  ctrl_t[B,d] = controlInputAct(vecQuestions Wq + bq);  ctrl_inputs[p,B,d]: step i = ctrl_t WqU_i + bqU_i (one matrix per
 *         step with controlInputUnshared, else the shared one) -- the function macx_cell_begin calls for its two launches;
 *   bwd:  d_ctrl_inputs[p,B,d] -> d_vecQuestions[B,d] and the non-NULL ones of GP->qInput_W / qInput_b / qInputU_W / qInputU_b
 *         (a NULL one is neither computed nor written) -- the function the cell's backward pass calls for this unit, launch for
 *         launch: with controlInputUnshared the p products of dt as one batched launch and a fixed-order sum that also applies
 *         act', and in the split family the p gradients of qInputU_W as one batched contraction.  The row sums and qInput_W's
 *         contraction, which the cell collects into its end-of-pass batches, run in batches of this call's own before it returns.
 * Only the qInput / qInputU fields of macx_params / macx_param_grads are touched.  ws >= macx_ctrl_inputs_ws_floats() floats:
 * the packed weights (bwd: their transposes) [1 + nU][d,d] with nU = p or 1 matrices of qInputU, three [B,d] temporaries (dt, du,
 * the summed d_ctrl_inputs), with controlInputUnshared the per-step products dt_part [p,B,d], and the eight slab sets of a batch of
 * small weight gradients.  Nothing survives from fwd to bwd in it -- pass ctrl_t back in. */
size_t macx_ctrl_inputs_ws_floats(const macx_opts*, const macx_shapes*);
int macx_ctrl_inputs_fwd(const macx_opts*, const macx_shapes*, const macx_params*, const float* vecQuestions, float* ctrl_t,
                         float* ctrl_inputs, float* ws, size_t ws_floats, void* stream);
int macx_ctrl_inputs_bwd(const macx_opts*, const macx_shapes*, const macx_params*, const float* vecQuestions, const float* ctrl_t,
                         const float* d_ctrl_inputs, const macx_param_grads*, float* d_vecQuestions, float* ws, size_t ws_floats,
                         void* stream);
/* X = dropout(KB) @ Wx + bx: the projX half of ops.mul (ops.py:678,688) on the knowledge-base GEMM.
 * `W_packed` from macx_pack_weight(Wx, d, d, macx_gemm_mode(-1) ? MACX_PACK_BF16X3 : MACX_PACK_F32MFMA);
 * `drop_ws` >= B*N*d + B*N*d/32 floats of scratch for the dropped KB and its keep bits (may be NULL when keep_read == 1). */
int macx_kb_project(const macx_shapes*, const macx_dropout*, int step, const float* kb,
                    const float* W_packed, const float* b, float* out, float* drop_ws, void* stream);
/* softmax(expMask(logits)) + att2Smry over the question words for one step
 * (mac_cell.py:155-181; ops.py:114-150, 243-247).  cc: continuous control [B,d].  The launcher the cell calls, for one step. */
int macx_control_attend(const macx_shapes*, const float* cc, const float* words, const int32_t* lengths,
                        const float* w, const float* b, float* att, float* control, void* stream);
/* its backward: d_control[B,d] -> d_cc[B,d], d_words[B,S,d] (written), d_w[d], d_b[1]; `att` is what the forward call
 * returned; ws >= macx_control_attend_bwd_ws_floats(shapes) floats.  d % 64 == 0.  The cell's launcher of the two backward
 * kernels for one step, then the two row sums of the parameter partials. */
size_t macx_control_attend_bwd_ws_floats(const macx_shapes*);
int macx_control_attend_bwd(const macx_shapes*, const float* d_control, const float* cc, const float* att, const float* words,
                            const float* w, float* ws, size_t ws_floats, float* d_cc, float* d_words, float* d_w, float* d_b,
                            void* stream);
/* Materialises the 0/1 keep mask of a dropout site for n elements starting at flat index
 * `first` (test hook for the stateless stream; site numbers in macx_common.hip.h). */
int macx_dropout_mask(uint32_t seed, uint32_t site, uint32_t step, float keep, uint32_t first,
                      size_t n, float* out, void* stream);
/* ... under a run's mask word (macx_dropout.mask_word: device pointer or NULL) */
int macx_dropout_mask_w(uint32_t seed, uint32_t site, uint32_t step, float keep, uint32_t first,
                        size_t n, const uint32_t* mask_word, float* out, void* stream);
/* weight-gradient contraction out[k][j] = sum_m A[m][k] G[m][j]  (fixed-order split reduction).
 * `ws` >= nsplit*Kd*Jd floats where nsplit = macx_wgrad_splits(M, Kd, Jd). */
int macx_wgrad_splits(int M, int Kd, int Jd);
int macx_wgrad(const float* A, int lda, const float* G, int ldg, int M, int Kd, int Jd,
               float* out, float* ws, void* stream);

/* ---- answer loss and prediction (addAnswerLossOp model.py:593-599, addPredOp model.py:603-612) ----
 * loss_rows[b] = -log softmax(logits[b])[answers[b]]  (tf.nn.sparse_softmax_cross_entropy_with_logits; the model's loss is
 * their mean), pred[b] = argmax_c logits[b][c] (first maximum, tf.argmax), dlogits (may be NULL) = (softmax - onehot) *
 * grad_scale -- grad_scale = 1/B is the gradient of the mean loss.  logits [B][A] fp32 contiguous, answers / pred int32. */
int macx_answer_loss(const float* logits, const int32_t* answers, int B, int A, float* loss_rows, int32_t* pred,
                     float* dlogits, float grad_scale, void* stream);

/* ---- a loss on a run's attention maps (attention supervision, entropy regularisers) --------------------------------
 * One launch turns a stacked map `att` [p,B,n] (a viewable segment of `saved`: MACX_SEG_ATT_KB, n = N; MACX_SEG_ATT_QUESTION,
 * n = S) into loss rows [p,B] and the gradient d_att [p,B,n] (may be NULL: rows only) in the layout macx_state_grads takes, so the
 * call can sit between macx_cell_forward and macx_cell_backward[_phase]_x -- inside a captured graph as well.
 * With w = scale * step_weights[i] * row_weights[b] (NULL weights = 1) and L = clamp(lengths[b], 1, n) (NULL = n; the clamp of
 * macx_kb_attend_fwd_l):
 *   MACX_ATT_LOSS_CE       loss_rows[i,b] = -w sum_{j<L} t[j] log(a[j] + eps);   d_att[i,b,j] = -w t[j] / (a[j] + eps)
 *                          t = target[b] ([B,n], target_steps 0) or target[i,b] ([p,B,n], target_steps 1)
 *   MACX_ATT_LOSS_ENTROPY  loss_rows[i,b] =  w sum_{j<L} a[j] log(a[j] + eps)   (the NEGATIVE entropy: the sign of `scale` chooses);
 *                          d_att[i,b,j] = w (log(a[j] + eps) + a[j] / (a[j] + eps));   target is not read (NULL)
 * d_att[i,b,j >= L] = +0.0f and neither att nor target is read there (they may hold NaN); a row with w == 0 (row_weights[b] = 0: the
 * question is unsupervised) is exactly 0 with an all +0.0f d_att row, whatever att and target hold -- the finite-gradient contract
 * of macx_state_grads.  (A live cell with t[j] == 0 gets CE's -0.0f under w > 0: +0.0f is promised for j >= L and w == 0 only.)  lengths (int32), step_weights [p] and row_weights [B] are device memory read when the kernel runs; eps and
 * scale travel by value.  Identical calls give identical bits (fixed-order reduction, no atomics).
 * MACX_EINVAL, and nothing is launched: eps <= 0 or not finite, an unknown kind, kind CE without a target. */
enum { MACX_ATT_LOSS_CE = 0, MACX_ATT_LOSS_ENTROPY = 1 };
int macx_att_loss(const float* att, const float* target, const int32_t* lengths, const float* step_weights,
                  const float* row_weights, int p, int B, int n, int kind, int target_steps, float eps, float scale,
                  float* loss_rows, float* d_att, void* stream);

/* ---- the answer loss under per-question weights: partial batches, re-weighted samples, evaluation totals ----------
 * macx_answer_loss with a weight per question that is DEVICE data, read when the kernel runs -- a captured graph of batch size B
 * serves n < B questions (weights of 0 behind them) and any re-weighting, one graph for all of them.  (It stands behind
 * macx_att_loss here, not beside macx_answer_loss, which it leaves as it is: the binding table follows the header's order.)
 * weights: [B] fp32 or NULL (= all ones).  Question b is LIVE iff weights[b] > 0; everything else -- 0, negative, NaN -- is weight 0.
 * W = sum of the live weights, summed in fp64 in one fixed order.
 *   live row   loss_rows[b] = -log softmax(logits[b])[answers[b]], UNWEIGHTED: the bits macx_answer_loss writes; pred[b] = argmax (first
 *              maximum); dlogits[b] = grad_scale * (w_b / W) * (softmax - onehot).  A label outside [0, A): NaN loss row, zero
 *              gradient row, as in macx_answer_loss; that NaN reaches loss_out and totals.
 *   dead row   neither logits[b] nor answers[b] is read (they may hold NaN or garbage): loss_rows[b] = +0.0f, pred[b] = -1,
 *              dlogits[b] all +0.0f -- downstream the finite-gradient contract macx_att_loss states for w == 0.
 *   loss_out   (may be NULL) loss_out[0] = sum_live w_b loss_rows[b] / W, the products and the sum in fp64, rounded once; W == 0: +0.0f,
 *              and every gradient is +0.0f -- no division by zero, no NaN.
 *   totals     (may be NULL) three doubles in device memory to which the call ADDS sum w_b loss_rows[b], sum w_b [pred[b] == answers[b]]
 *              and W: fp64 products and sums in a fixed order, added by one thread with a plain load and store -- no atomics.  They
 *              run on across calls and graph replays until the host clears them; calls that share a `totals` must be stream-ordered.
 *   dlogits    (may be NULL) rows, pred, loss_out and totals only.
 * With weights == NULL, W = B: rows and pred are macx_answer_loss's bit for bit; dlogits * B is its dlogits at grad_scale 1 within
 * 2 ulp per entry (one division and one product in fp32; bit for bit when B is a power of two).
 * One workgroup walks the batch, 16 questions per pass: no hand-off between workgroups.  Any B >= 1 is accepted and correct; the
 * intended range is a training or evaluation batch, B up to a few hundred (4 passes at B = 64), and the time grows with B / 16, so a
 * loss over many thousands of rows belongs in several calls.  W is rounded once to fp32 for w_b / W.  Identical calls give identical bits.
 * MACX_EINVAL, and nothing is launched: B < 1, A < 1, a NULL logits, answers, loss_rows or pred. */
int macx_answer_loss_weighted(const float* logits, const int32_t* answers, const float* weights, int B, int A,
                              float* loss_rows, int32_t* pred, float* dlogits, float* loss_out, double* totals,
                              float grad_scale, void* stream);

/* ---- the knowledge-base attention unit on its own (mac_cell.py:266-272: inter2att's softmax + att2Smry) ------------
 * The fused cell's own kernels behind a per-unit contract, so that the unit is testable in isolation:
 *   macx_kb_attend_fwd   att[B,N] = softmax_n(logits[B,N] + bias[0]);  info[B,d] = sum_n att KB        (ops.py:140-150)
 *   macx_kb_attend_bwd   da = dinfo . KB;  dlogits = att (da - sum_n att da);  dkb (= | +=) att (x) dinfo (dkb may be NULL);
 *                        ws >= macx_kb_attend_bwd_ws_floats(B, N, d) floats
 *   macx_kb_attend_fwd_l the same over the first kb_lengths[b] cells of question b (int32 [B] on the device, clamped to [1, N]; NULL =
 *                        macx_kb_attend_fwd, bit for bit): att[b][n >= kb_lengths[b]] = 0 exactly; logits and kb rows of those cells
 *                        are never used (they may hold NaN).  macx_kb_attend_bwd needs no lengths: it multiplies by that 0, so for
 *                        it the padded kb rows must be finite
 * N <= 1024, d % 128 == 0. */
int macx_kb_attend_fwd(int B, int N, int d, const float* logits, const float* bias, const float* kb, float* att, float* info,
                       void* stream);
int macx_kb_attend_fwd_l(int B, int N, int d, const float* logits, const float* bias, const float* kb, const int32_t* kb_lengths,
                         float* att, float* info, void* stream);
size_t macx_kb_attend_bwd_ws_floats(int B, int N, int d);
int macx_kb_attend_bwd(int B, int N, int d, const float* att, const float* kb, const float* dinfo, float* dlogits, float* dkb,
                       int accumulate, float* ws, size_t ws_floats, void* stream);

/* ---- the read unit and the write unit as wholes (macx_<unit>_{fwd,bwd}) ----------------------------------
 * ONE unit of the fused cell on caller-owned buffers -- the cell's own step code restricted to that unit, so per-unit
 * parity against mac_cell.py:209-277 (read) and :305-375 (write) is testable without running a cell.
 *   shapes->p must be 1: it is the unit of step 0 (dropout streams are keyed by (seed, site, step 0)); S is ignored.
 *   saved >= macx_saved_floats(opts, shapes, 1) floats, written by *_fwd and read by the matching *_bwd;
 *   ws >= macx_workspace_bytes(opts, shapes, 1) bytes (= 4 * macx_ws_floats).  Only the unit's fields of macx_params /
 *   macx_param_grads are read / written (read: projX, projY, memKbProj, memKbProj2, kbLogits; write: newMemory, gate).
 *   read:  info[B,d], att[B,N] = read(knowledgeBase[B,N,d], memory[B,d], control[B,d]); memory / read dropout per macx_dropout
 *          bwd: d_info -> d_knowledgeBase[B,N,d], d_memory, d_control and the unit's parameter gradients
 *          macx_read_fwd_l: the same with macx_inputs.kbLengths (kb_lengths: [B] int32 on the device, clamped to [1, N]; NULL =
 *          macx_read_fwd, which forwards here).  No backward twin: every backward consumer multiplies by att, which is exactly 0
 *          in the padded cells, so macx_read_bwd on this call's `saved` gives exact zeros in the padded rows of d_knowledgeBase
 *          (the padded rows of knowledgeBase must be finite for that).
 *   write: new_memory[B,d] = write(memory, info, control); the write dropout (mac_cell.py:461-463) is applied to `info`
 *          bwd: d_new_memory -> d_memory, d_info, d_control (the gate's; zeros without --writeGate) + parameter gradients
 *          opts->write_self_att needs the histories of a running cell: MACX_EUNSUPPORTED here (use macx_cell_step). */
size_t macx_workspace_bytes(const macx_opts*, const macx_shapes*, int for_backward);
int macx_read_fwd(const macx_opts*, const macx_shapes*, const macx_dropout*, const macx_params*, const float* knowledgeBase,
                  const float* memory, const float* control, float* saved, size_t saved_floats, float* info, float* att,
                  void* stream);
int macx_read_fwd_l(const macx_opts*, const macx_shapes*, const macx_dropout*, const macx_params*, const float* knowledgeBase,
                    const int32_t* kb_lengths, const float* memory, const float* control, float* saved, size_t saved_floats,
                    float* info, float* att, void* stream);
int macx_read_bwd(const macx_opts*, const macx_shapes*, const macx_dropout*, const macx_params*, const float* knowledgeBase,
                  const float* saved, size_t saved_floats, float* ws, size_t ws_floats, const float* d_info,
                  const macx_param_grads*, float* d_knowledgeBase, float* d_memory, float* d_control, void* stream);
int macx_write_fwd(const macx_opts*, const macx_shapes*, const macx_dropout*, const macx_params*, const float* memory,
                   const float* info, const float* control, float* saved, size_t saved_floats, float* new_memory, void* stream);
int macx_write_bwd(const macx_opts*, const macx_shapes*, const macx_dropout*, const macx_params*, const float* saved,
                   size_t saved_floats, float* ws, size_t ws_floats, const float* d_new_memory, const macx_param_grads*,
                   float* d_memory, float* d_info, float* d_control, void* stream);

/* ---- embedding lookup on its own (model.py:207-219 qEmbeddingsOp + the input dropout of ops.py:812 / :880) --------------
 *   macx_embed_lookup      x[r][0..E) = dropout(table[ids[r]]), table row 0 = zeros (padding), row i = emb[i - 1]; columns
 *                          [E, ld) of x are written as zeros.  Dropout site SITE_ENC_INPUT on the stateless stream, element
 *                          index (first_row + r) * E + c (first_row = b0 * S for a data-parallel shard); keep = 1: none.
 *   macx_embed_lookup_bwd  d_emb[V][E] (written) = sum over the rows that looked a word up of dropout'(dx[r]); one workgroup
 *                          per vocabulary row, fixed order, no atomics.
 * The generic question encoder (mac-network_amd/encoder.py GenericQuestionEncoder) is built from these, macx_linear / macx_wgrad
 * and the macx_op_* kernels. */
int macx_embed_lookup(const int32_t* ids, const float* emb, int rows, int E, int ld, float keep, uint32_t seed,
                      uint32_t first_row, float* x, void* stream);
int macx_embed_lookup_bwd(const int32_t* ids, const float* dx, int rows, int E, int ld, int V, float keep, uint32_t seed,
                          uint32_t first_row, float* d_emb, void* stream);

/* ---- the ops.py primitives as single kernels (mac-network_amd/csrc/macx_ops.hip.h) -------------------------------
 * The building blocks of the GENERIC option path (mac-network_amd/generic.py): every legal option combination the fused
 * cell kernels above answer with MACX_EUNSUPPORTED runs as one kernel per reference op -- these, macx_linear / macx_h2_gemm
 * and macx_wgrad -- chained by the host exactly as mac_cell.py chains ops.py.  fp32, contiguous, device pointers.
 *   macx_op_act      out = act(x); act = MACX_ACT_* or MACX_OP_PRELU (relu(x) - alpha[c] relu(-x), c = index % inner; ops.py:171-173)
 *   macx_op_act_bwd  dx = dy act'(x); PRELU also writes dalpha_elem = dy min(x, 0) for the caller to reduce over rows
 *   macx_op_binary   out = scale (a + b) or scale (a * b); a, out hold n floats viewed [.., mid, inner]; b by `bmode`:
 *                    SAME [n] | MID [n / (mid inner)][inner], broadcast over the middle axis (ops.mul's extendY, ops.py:693-695) |
 *                    CHANNEL [inner] | ROW [n / inner], one scalar per row (ops.att2Smry, ops.py:150)
 *   macx_op_reduce   MID: x [outer][mid][inner] -> out [outer][inner];  LAST: x [outer][inner] -> out [outer];
 *                    ROWS: x [outer][inner] -> out [inner], ws >= 64 inner floats.  Fixed summation order.
 *   macx_op_softmax  softmax over the last axis of [rows][n]; with `lengths`, columns >= lengths[row / rows_per_len] are
 *                    masked to -inf first (ops.expMask, ops.py:243-247; mac_cell.py:176)
 *   macx_op_softmax_bwd  dx = a (da - sum a da)
 *   macx_op_dropout  out = x / keep * mask(seed, site, step, first + index): tf.nn.dropout on the stateless stream of
 *                    macx_dropout_mask (ops.py:312, mac_cell.py:217,463); its own backward (apply it to dy) */
#define MACX_OP_PRELU 16
#define MACX_OP_RSQRT_EPS 17   /* out = 1 / sqrt(x + alpha[0]): batch-norm normaliser (mac_cell.py:370-373); no dalpha */
enum { MACX_OP_ADD = 0, MACX_OP_MUL = 1 };
enum { MACX_OP_B_SAME = 0, MACX_OP_B_MID = 1, MACX_OP_B_CHANNEL = 2, MACX_OP_B_ROW = 3 };
enum { MACX_OP_R_MID = 0, MACX_OP_R_LAST = 1, MACX_OP_R_ROWS = 2 };
int macx_op_act(int act, const float* x, const float* alpha, size_t n, int inner, float* out, void* stream);
int macx_op_act_bwd(int act, const float* x, const float* alpha, const float* dy, size_t n, int inner, float* dx,
                    float* dalpha_elem, void* stream);
int macx_op_binary(int op, int bmode, const float* a, const float* b, size_t n, int mid, int inner, float scale, float* out,
                   void* stream);
int macx_op_reduce(int mode, const float* x, size_t outer, int mid, int inner, float* out, float* ws, void* stream);
int macx_op_softmax(const float* x, const int32_t* lengths, int rows_per_len, size_t rows, int n, float* out, void* stream);
int macx_op_softmax_bwd(const float* a, const float* da, size_t rows, int n, float* dx, void* stream);
int macx_op_dropout(const float* x, size_t n, uint32_t seed, uint32_t site, uint32_t step, float keep, uint32_t first,
                    float* out, void* stream);
/* ... under a run's mask word (macx_dropout.mask_word: device pointer or NULL) */
int macx_op_dropout_w(const float* x, size_t n, uint32_t seed, uint32_t site, uint32_t step, float keep, uint32_t first,
                      const uint32_t* mask_word, float* out, void* stream);

/* (ABI <= 4 had a `macx_debug_set` entry point here: fifteen process-global integers.  ABI 5 removed it -- the live A/B hooks travel per
 * call in macx_opts.tune, the variants that were measured slower in rounds 4-5 (side-queue modes, pair launches, the dual-A
 * contraction, 8-wave linears, the 32 x 32 x 16 K loop, write-through stores) and the kernels only they instantiated are gone.
 * What is left of process-wide state is macx_gemm_mode's default kernel FAMILY for the entry points that carry no macx_opts;
 * no product module sets it: tests/test_host.py::test_product_code_never_touches_the_debug_knobs.) */

const char* macx_strerror(int code);
int macx_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MACX_H */
