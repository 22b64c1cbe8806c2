"""ctypes binding of libmacx.so -- the C ABI declared in include/macx.h.

The product path has NO CPU fallback: if the library is missing or does not export the ABI this
module raises, and every op built on it fails loudly.
"""
import ctypes as C
import os

import torch

from . import build as _build

ABI_VERSION = 5

MACX_OK, MACX_EINVAL, MACX_EUNSUPPORTED, MACX_EREJECTED, MACX_ESMALL, MACX_EWAIT = 0, -1, -2, -3, -4, -5
# macx_run_status word 0 (include/macx.h): which in-launch hand-off wait gave up
HANDOFF_BITS = {1: "a chain tile gave up waiting for its step's y", 2: "a filler workgroup gave up waiting for the previous step's write unit"}
STATUS_WORDS = 16
ACT = {"NON": 0, "TANH": 1, "SIGMOID": 2, "ELU": 3, "RELU": 4}
INIT = {"PRM": 0, "ZERO": 1, "Q": 2}
WRITE_INPUTS = {"MEM": 0, "INFO": 1, "SUM": 2, "BOTH": 3}
SEG = {"controls": 0, "memories": 1, "infos": 2, "att_question": 3, "att_kb": 4, "att_self": 5, "att_gate": 6,
       "status": 7}


class MacxOpts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "abi_version", "init_ctrl", "init_mem", "control_input_unshared", "control_input_act", "control_feed_prev",
        "control_feed_prev_att", "control_feed_inputs", "control_cont_act", "read_mem_act", "read_ctrl_act",
        "write_inputs", "write_self_att", "write_self_att_cont", "write_mem_act", "write_gate", "write_gate_shared")]
    _fields_ += [("write_gate_bias", C.c_float), ("memory_variational_dropout", C.c_int32), ("gemm_family", C.c_int32),
                 ("tune", C.c_int32 * 16)]


# macx_opts.tune keys (include/macx.h MACX_TUNE_*): the per-call A/B hooks and the profiling tools' phase mask.  A value v travels
# as v + 1; 0 = the shipped default of that key.
TUNE = {"native_waves": 0, "phase_mask": 1, "row_tiles": 2, "pre_fill": 3, "chain": 4, "sb_defer": 5, "chain_kv": 7, "sb_wide": 8,
        "wgrad_pipe": 10, "sb_cont": 13, "dkb_uni": 14, "dkb_fill": 15}


def set_tune(opts, key, value):
    """opts.tune[key] = value (None: back to the default).  key: a name of TUNE or its number."""
    k = TUNE[key] if isinstance(key, str) else int(key)
    if k not in TUNE.values():
        raise KeyError("no tuning key %r (have %s)" % (key, sorted(TUNE)))
    opts.tune[k] = 0 if value is None else int(value) + 1


class MacxShapes(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "S", "N", "d", "p", "b0", "d_logical")]


class MacxDropout(C.Structure):
    _fields_ = [("keep_memory", C.c_float), ("keep_read", C.c_float), ("keep_write", C.c_float), ("seed", C.c_uint32),
                ("mask_word", C.c_void_p)]


class MacxRoute(C.Structure):
    """macx_route: the launch route macx_cell_route reports (include/macx.h)"""
    _fields_ = [(n, C.c_int32) for n in (
        "family", "chain", "tile_rows", "tiles", "chain_sums", "sb_deferred", "dy_in_linear", "dc_reduce_per_step", "sb_wide", "sb_qpg",
        "sb_groups", "sb_slabs", "wgrad_splits", "wgrad_kw", "db_rows", "dwk_rows", "wfmt_plain", "wfmt_ymix", "fwd_fillers", "fill_y",
        "fill_stage0", "fill_write", "dkb_jobs", "dkb_fillers", "dkb_skip")]


PARAM_FIELDS = (
    "initMem", "initCtrl", "qInput_W", "qInput_b", "qInputU_W", "qInputU_b", "ctrlLogits_w", "ctrlLogits_b",
    "contControl_W", "contControl_b", "contControl2_W", "contControl2_b", "projX_W", "projX_b", "projY_W", "projY_b",
    "memKbProj_W", "memKbProj_b", "memKbProj2_W", "memKbProj2_b", "kbLogits_w", "kbLogits_b", "newMemory_W",
    "newMemory_b", "selfCtrl_W", "selfCtrl_b", "selfLogits_w", "selfLogits_b", "gate_W", "gate_b")


class MacxParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in PARAM_FIELDS]


class MacxParamGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in PARAM_FIELDS]


class MacxOutShapes(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "d", "hidden", "answers", "b0")]


OUT_FIELDS = ("outQuestion_W", "outQuestion_b", "fc0_W", "fc0_b", "fc1_W", "fc1_b")


class MacxOutParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in OUT_FIELDS]


class MacxOutGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in OUT_FIELDS]


class MacxStemShapes(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "H", "W", "Cin", "Cmid", "Cout", "b0")]


STEM_FIELDS = ("kernel0", "bias0", "kernel1", "bias1")


class MacxStemParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in STEM_FIELDS]


class MacxStemGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in STEM_FIELDS]


class MacxConvShapes(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "H", "W", "Cin", "Cout", "k", "stride")]


class MacxEncShapes(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "S", "V", "E", "h", "b0")]


ENC_FIELDS = ("emb", "fw_kernel", "fw_bias", "bw_kernel", "bw_bias")


class MacxEncParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ENC_FIELDS]


class MacxEncGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ENC_FIELDS]


RNN_CELL = {"RNN": 0, "GRU": 1, "LSTM": 2}                                    # MACX_RNN_BASIC | _GRU | _LSTM


class MacxRnnShapes(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "S", "V", "E", "h", "b0", "cell", "dirs")]


RNN_FIELDS = ENC_FIELDS + ("fw_candidate_kernel", "fw_candidate_bias", "bw_candidate_kernel", "bw_candidate_bias")


class MacxRnnParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in RNN_FIELDS]


class MacxRnnGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in RNN_FIELDS]


class MacxGatherEntry(C.Structure):
    """macx_gather_entry: one row of macx_gather_flat's device table (24 bytes = three int64 of a torch tensor)"""
    _fields_ = [("src", C.c_void_p), ("dst_offset", C.c_uint64), ("count", C.c_uint64)]


class MacxInputs(C.Structure):
    _fields_ = [("vecQuestions", C.c_void_p), ("words", C.c_void_p), ("questionLengths", C.c_void_p),
                ("knowledgeBase", C.c_void_p), ("kbLengths", C.c_void_p)]     # kbLengths: int32 [B] on the device, or NULL


class MacxInputGrads(C.Structure):
    _fields_ = [("vecQuestions", C.c_void_p), ("words", C.c_void_p), ("knowledgeBase", C.c_void_p)]


class MacxRecordDesc(C.Structure):
    """macx_record_desc: one table of a macx_records_scatter call -- src [steps][B][n] fp32, table [Q][steps][n] of dtype
    (FEATURES_DTYPE's codes)"""
    _fields_ = [("src", C.c_void_p), ("table", C.c_void_p), ("steps", C.c_int32), ("n", C.c_int32), ("dtype", C.c_int32)]


RECORDS_MAX = 4                                                               # MACX_RECORDS_MAX

STATE_GRAD_FIELDS = ("d_controls", "d_memories", "d_att_question", "d_att_kb", "d_att_self", "d_att_gate")


class MacxStateGrads(C.Structure):
    """macx_state_grads: gradients a loss sends to the run's histories and attention maps themselves (device pointers in the layouts
    of the MACX_SEG_* segments; NULL = zero).  Finite values only (include/macx.h)."""
    _fields_ = [(n, C.c_void_p) for n in STATE_GRAD_FIELDS]


# ---------------------------------------------------------------------------------------------------------------------------
# The binding: export -> (restype, argtypes), in the order and under the section titles of include/macx.h.  This table is the ONE
# place an export is declared on the Python side; lib() applies it and nothing else sets a restype or argtypes.  It is plain data
# (importable without libmacx.so), and tests/test_abi_host.py holds it to the header: every prototype's arity and every
# parameter's class (pointer | int | uint32 | size_t | float), every struct's size and field offsets.
# A pointer is POINTER(Struct) where callers pass byref(struct) / None, c_void_p where they pass addresses (tensor.data_ptr()).
# ---------------------------------------------------------------------------------------------------------------------------
_P = C.POINTER
_I, _U, _Z, _F, _V = C.c_int, C.c_uint32, C.c_size_t, C.c_float, C.c_void_p


def _masked(sig):
    """the `_w` twin of an entry point: the plain signature + the device mask word in front of the stream"""
    restype, a = sig
    return restype, a[:-1] + (_V, a[-1])


_OS = (_P(MacxOpts), _P(MacxShapes))
# what every call on a cell run starts with: opts, shapes, dropout, params, inputs, saved, saved_floats, ws, ws_floats
_RUN = _OS + (_P(MacxDropout), _P(MacxParams), _P(MacxInputs), _V, _Z, _V, _Z)
# ... and a backward call goes on with: d_memory, d_control, parameter gradients, input gradients
_BWD = _RUN + (_V, _V, _P(MacxParamGrads), _P(MacxInputGrads))
# a single unit (read / write) starts with: opts, shapes, dropout, params
_UNIT = _OS + (_P(MacxDropout), _P(MacxParams))
_STEM = (_P(MacxStemShapes), _I, _F, _U, _P(MacxStemParams))        # shapes, act, keep, seed, params
_OUT = (_P(MacxOutShapes), _I, _F, _U, _P(MacxOutParams))
_ENC = (_P(MacxEncShapes), _F, _F, _U, _P(MacxEncParams))           # shapes, keep_input, keep_question, seed, params
_GATHER = (_V, _V, _I, _I, _I, _I, _V, _V)                          # source, index, G, B, N, d, destination, stream

TABLE = {}
# ---- sizing
TABLE.update(
    macx_saved_floats=(_Z, _OS + (_I,)),
    macx_ws_floats=(_Z, _OS + (_I,)),
    macx_saved_segment=(_I, _OS + (_I, _I, _P(_Z), _P(_Z))),
    macx_check=(_I, _OS),
    macx_cell_route=(_I, _OS + (_P(MacxDropout), _I, _I, _P(MacxRoute))))
# ---- did the run's in-launch hand-offs complete?
TABLE.update(
    macx_run_status=(_I, _OS + (_I, _V, _Z, _V, _P(_U), _P(C.c_int32))),
    macx_run_status_reset=(_I, _OS + (_I, _V, _Z, _V)),
    macx_handoff_selftest=(_I, (_V, _P(_U))))
# ---- the cell
TABLE.update(
    macx_cell_begin=(_I, _RUN + (_I, _V)),
    macx_cell_step=(_I, _RUN + (_I, _I, _V)),
    macx_cell_forward=(_I, _RUN + (_I, _V)),
    macx_cell_backward=(_I, _BWD + (_V,)),
    macx_cell_backward_phase=(_I, _BWD + (_I, _V)),
    # (... + macx_state_grads* behind the input gradients; NULL = the plain call)
    macx_cell_backward_x=(_I, _BWD + (_P(MacxStateGrads), _V)),
    macx_cell_backward_phase_x=(_I, _BWD + (_P(MacxStateGrads), _I, _V)))
# ---- output unit + classifier
TABLE.update(
    macx_output_saved_floats=(_Z, (_P(MacxOutShapes),)),
    macx_output_ws_floats=(_Z, (_P(MacxOutShapes),)),
    macx_output_forward=(_I, _OUT + (_V, _V, _V, _V, _Z, _V)),
    macx_output_backward=(_I, _OUT + (_V, _V, _V, _Z, _V, _Z, _V, _P(MacxOutGrads), _V, _V, _V)))
TABLE.update(macx_output_forward_w=_masked(TABLE["macx_output_forward"]),
             macx_output_backward_w=_masked(TABLE["macx_output_backward"]))
# ---- stem CNN
TABLE.update(
    macx_stem_saved_floats=(_Z, (_P(MacxStemShapes),)),
    macx_stem_ws_floats=(_Z, (_P(MacxStemShapes),)),
    macx_stem_forward=(_I, _STEM + (_V, _V, _V, _Z, _V)),
    macx_stem_backward=(_I, _STEM + (_V, _V, _Z, _V, _Z, _V, _P(MacxStemGrads), _V)))
TABLE.update(macx_stem_forward_w=_masked(TABLE["macx_stem_forward"]),
             macx_stem_backward_w=_masked(TABLE["macx_stem_backward"]))
# ---- general convolution
TABLE.update(
    macx_conv2d_ws_floats=(_Z, (_P(MacxConvShapes),)),
    macx_conv2d_fwd=(_I, (_P(MacxConvShapes), _V, _V, _V, _V, _V)),
    macx_conv2d_bwd_data=(_I, (_P(MacxConvShapes), _V, _V, _V, _V)),
    macx_conv2d_wgrad=(_I, (_P(MacxConvShapes), _V, _V, _V, _V, _Z, _V)),
    macx_images_to_nhwc=(_I, (_V, _I, _I, _I, _V, _V)))
# ---- question encoder
TABLE.update(
    macx_encoder_saved_floats=(_Z, (_P(MacxEncShapes),)),
    macx_encoder_ws_floats=(_Z, (_P(MacxEncShapes),)),
    macx_encoder_forward=(_I, _ENC + (_V, _V, _V, _V, _V, _Z, _V)),
    macx_encoder_backward=(_I, _ENC + (_V, _V, _V, _Z, _V, _Z, _V, _V, _P(MacxEncGrads), _V)))
TABLE.update(macx_encoder_forward_w=_masked(TABLE["macx_encoder_forward"]),
             macx_encoder_backward_w=_masked(TABLE["macx_encoder_backward"]))
# ---- question encoder, every cell
# (macx_encoder_*_w's argument lists on the rnn structs: unit._FusedCall drives both)
_RNN = (_P(MacxRnnShapes), _F, _F, _U, _P(MacxRnnParams))
TABLE.update(
    macx_rnn_encoder_saved_floats=(_Z, (_P(MacxRnnShapes),)),
    macx_rnn_encoder_ws_floats=(_Z, (_P(MacxRnnShapes),)),
    macx_rnn_encoder_forward_w=(_I, _RNN + (_V, _V, _V, _V, _V, _Z, _V, _V)),
    macx_rnn_encoder_backward_w=(_I, _RNN + (_V, _V, _V, _Z, _V, _Z, _V, _V, _P(MacxRnnGrads), _V, _V)))
# ---- optimizer step
TABLE.update(
    macx_adam_ema_step=(_I, (_Z, _V, _V, _V, _V, _V, _F, _F, _F, _F, _I, _F, _F, _V, _V, _V)),
    # (the rate in device memory instead of lr and step)
    macx_adam_ema_step_p=(_I, (_Z, _V, _V, _V, _V, _V, _V, _F, _F, _F, _F, _F, _V, _V, _V)),
    # (guarded: skip_above and the four guard words in front of ws)
    macx_adam_ema_step_g=(_I, (_Z, _V, _V, _V, _V, _V, _F, _F, _F, _F, _I, _F, _F, _F, _V, _V, _V, _V)),
    macx_adam_ema_step_pg=(_I, (_Z, _V, _V, _V, _V, _V, _V, _F, _F, _F, _F, _F, _F, _V, _V, _V, _V)))
# ---- flat gather
TABLE.update(macx_gather_flat=(_I, (_V, _I, _V, _V)))             # (the table of MacxGatherEntry rows lives in device memory)
# ---- questions that share images
TABLE.update(
    macx_kb_gather=(_I, _GATHER),
    macx_kb_gather_bwd=(_I, _GATHER),
    # (the sizes per image, [G] int32 or NULL, behind the index; the forward call also writes kb_lengths_out [B] in front of the stream)
    macx_kb_gather_l=(_I, _GATHER[:2] + (_V,) + _GATHER[2:-1] + (_V, _GATHER[-1])),
    macx_kb_gather_bwd_l=(_I, _GATHER[:2] + (_V,) + _GATHER[2:]))
# ---- image features resident in device memory
TABLE.update(
    # (src, layout, n, C, HW; table, dtype, row0, rows; overflow, stream)
    macx_features_pack=(_I, (_V, _I, _I, _I, _I, _V, _I, _Z, _Z, _V, _V)),
    # (table, dtype, rows; ids, G, C, HW; out, stream)
    macx_features_gather=(_I, (_V, _I, _Z, _V, _I, _I, _I, _V, _V)))
FEATURES_DTYPE = {torch.float32: 0, torch.float16: 1}                       # MACX_FEATURES_*
# ---- questions resident in device memory
TABLE.update(
    # (the six tables, Q, S_tab; ids, B, S; the six outputs; image_index, G; bad, stream)
    macx_questions_gather=(_I, (_V,) * 6 + (_I, _I, _V, _I, _I) + (_V,) * 6 + (_V, _I, _V, _V)),
    # (pred, ids, B, Q; table, stream)
    macx_preds_scatter=(_I, (_V, _V, _I, _I, _V, _V)))
# ---- evaluation records resident in device memory
# (descs: a host array of MacxRecordDesc, count; ids, B, Q; stream)
TABLE.update(macx_records_scatter=(_I, (_P(MacxRecordDesc), _I, _V, _I, _I, _V)))
# ---- unit-level entry points
TABLE.update(
    macx_linear=(_I, (_V, _I, _V, _I, _I, _V, _V, _F, _I, _I, _V, _V)),
    # (part, part_N, part_shift, k, rows; W_packed, b, bias_const, n_out, act; part_sum, out, stream)
    macx_linear_part=(_I, (_V, _I, _I, _I, _I, _V, _V, _F, _I, _I, _V, _V, _V)),
    macx_pack_weight=(_I, (_V, _I, _I, _I, _V, _V)),
    macx_gemm_mode=(_I, (_I,)))
# ---- the H2 tensor format
TABLE.update(
    macx_h2_floats=(_Z, (_Z, _Z)),
    macx_h2_from_f32=(_I, (_V, _I, _I, _I, _V, _V)),
    macx_h2_to_f32=(_I, (_V, _I, _I, _V, _V)),
    macx_h2_pack_weight=(_I, (_V, _I, _I, _I, _V, _V)),
    macx_h2_gemm_planes=(_I, (_V, _I, _I, _I, _V, _I, _V, _I, _V, _V)),
    macx_h2_gemm=(_I, (_V, _I, _I, _I, _V, _I, _V, _I, _V, _V, _Z, _V)),
    # (opts; nt, R, Kd, Jd, nsplit; [A, stride, shared, G, stride, out] x 2; ws, ws_floats, stream)
    macx_h2_wgrad_ws_floats=(_Z, (_P(MacxOpts),) + (_I,) * 6),
    macx_h2_wgrad=(_I, (_P(MacxOpts),) + (_I,) * 5 + (_V, _Z, _I, _V, _Z, _V) * 2 + (_V, _Z, _V)),
    # (opts; B, N, d, nsteps, qpg, wide; X, stride, dI1, stride; y, W1a, dW1a, dW1b, dy_part; ws, ws_floats, stream)
    macx_h2_sb_ws_floats=(_Z, (_P(MacxOpts),) + (_I,) * 6),
    macx_h2_sb=(_I, (_P(MacxOpts),) + (_I,) * 6 + (_V, _Z, _V, _Z) + (_V,) * 5 + (_V, _Z, _V)),
    macx_read_chain_time=(_I, _RUN[:7] + (_I, _I, _P(_F), _V)),
    macx_cell_forward_chain_time=(_I, _RUN + (_P(_F), _V)),
    macx_saved_activation=(_I, _OS + (_I, _I, _V, _Z, _V, _V)),
    macx_ctrl_inputs_ws_floats=(_Z, _OS),
    macx_ctrl_inputs_fwd=(_I, _OS + (_P(MacxParams), _V, _V, _V, _V, _Z, _V)),
    macx_ctrl_inputs_bwd=(_I, _OS + (_P(MacxParams), _V, _V, _V, _P(MacxParamGrads), _V, _V, _Z, _V)),
    macx_kb_project=(_I, (_P(MacxShapes), _P(MacxDropout), _I, _V, _V, _V, _V, _V, _V)),
    macx_control_attend=(_I, (_P(MacxShapes),) + (_V,) * 8),
    macx_control_attend_bwd_ws_floats=(_Z, (_P(MacxShapes),)),
    macx_control_attend_bwd=(_I, (_P(MacxShapes),) + (_V,) * 6 + (_Z,) + (_V,) * 5),
    macx_dropout_mask=(_I, (_U, _U, _U, _F, _U, _Z, _V, _V)),
    macx_dropout_mask_w=(_I, (_U, _U, _U, _F, _U, _Z, _V, _V, _V)),          # (the word in front of `out`)
    macx_wgrad_splits=(_I, (_I, _I, _I)),
    macx_wgrad=(_I, (_V, _I, _V, _I, _I, _I, _I, _V, _V, _V)))
# ---- answer loss and prediction
TABLE.update(macx_answer_loss=(_I, (_V, _V, _I, _I, _V, _V, _V, _F, _V)))
# ---- a loss on a run's attention maps
# (att, target, lengths, step_weights, row_weights; p, B, n, kind, target_steps; eps, scale; loss_rows, d_att, stream)
TABLE.update(macx_att_loss=(_I, (_V,) * 5 + (_I,) * 5 + (_F, _F) + (_V, _V, _V)))
ATT_LOSS_KINDS = {"ce": 0, "entropy": 1}                                      # MACX_ATT_LOSS_*
# ---- the answer loss under per-question device weights
# (logits, answers, weights; B, A; loss_rows, pred, dlogits, loss_out, totals; grad_scale; stream)
TABLE.update(macx_answer_loss_weighted=(_I, (_V,) * 3 + (_I, _I) + (_V,) * 5 + (_F, _V)))
# ---- the knowledge-base attention unit on its own
TABLE.update(
    macx_kb_attend_fwd=(_I, (_I, _I, _I) + (_V,) * 6),
    macx_kb_attend_fwd_l=(_I, (_I, _I, _I) + (_V,) * 7),                       # (+ kb_lengths behind kb)
    macx_kb_attend_bwd_ws_floats=(_Z, (_I, _I, _I)),
    macx_kb_attend_bwd=(_I, (_I, _I, _I) + (_V,) * 5 + (_I, _V, _Z, _V)))
# ---- the read unit and the write unit as wholes
TABLE.update(
    macx_workspace_bytes=(_Z, _OS + (_I,)),
    macx_read_fwd=(_I, _UNIT + (_V, _V, _V, _V, _Z, _V, _V, _V)),
    macx_read_fwd_l=(_I, _UNIT + (_V, _V, _V, _V, _V, _Z, _V, _V, _V)),      # (+ kb_lengths behind knowledgeBase)
    macx_read_bwd=(_I, _UNIT + (_V, _V, _Z, _V, _Z, _V, _P(MacxParamGrads), _V, _V, _V, _V)),
    macx_write_fwd=(_I, _UNIT + (_V, _V, _V, _V, _Z, _V, _V)),
    macx_write_bwd=(_I, _UNIT + (_V, _Z, _V, _Z, _V, _P(MacxParamGrads), _V, _V, _V, _V)))
# ---- embedding lookup on its own
TABLE.update(
    macx_embed_lookup=(_I, (_V, _V, _I, _I, _I, _F, _U, _U, _V, _V)),
    macx_embed_lookup_bwd=(_I, (_V, _V, _I, _I, _I, _I, _F, _U, _U, _V, _V)))
# ---- the ops.py primitives as single kernels
TABLE.update(
    macx_op_act=(_I, (_I, _V, _V, _Z, _I, _V, _V)),
    macx_op_act_bwd=(_I, (_I, _V, _V, _V, _Z, _I, _V, _V, _V)),
    macx_op_binary=(_I, (_I, _I, _V, _V, _Z, _I, _I, _F, _V, _V)),
    macx_op_reduce=(_I, (_I, _V, _Z, _I, _I, _V, _V, _V)),
    macx_op_softmax=(_I, (_V, _V, _I, _Z, _I, _V, _V)),
    macx_op_softmax_bwd=(_I, (_V, _V, _Z, _I, _V, _V)),
    macx_op_dropout=(_I, (_V, _Z, _U, _U, _U, _F, _U, _V, _V)),
    macx_op_dropout_w=(_I, (_V, _Z, _U, _U, _U, _F, _U, _V, _V, _V)))         # (the word in front of `out`)
# ---- (the header's tail)
TABLE.update(
    macx_strerror=(C.c_char_p, (_I,)),
    macx_abi_version=(_I, ()))

EXPORTS = tuple(TABLE)

_lib = None


class MacxError(RuntimeError):
    def __init__(self, code, where):
        self.code = code
        msg = lib().macx_strerror(code).decode() if _lib is not None else str(code)
        super().__init__("%s failed: %s (code %d)" % (where, msg, code))


class HandoffTimeout(RuntimeError):
    """A run's in-launch hand-off wait gave up (macx_run_status returned MACX_EWAIT): the run's final memory and gradients are
    NaN.  `bits`: the status word (HANDOFF_BITS), `first_step`: the step of the first give-up.  The status is sticky: clear it
    with the cell's / captured step's reset_status() once the error is handled."""

    def __init__(self, bits, first_step, where="MAC cell run"):
        self.bits, self.first_step = int(bits), int(first_step)
        what = [t for b, t in sorted(HANDOFF_BITS.items()) if self.bits & b] or ["unknown bits"]
        super().__init__("%s: in-launch hand-off timeout (status 0x%x: %s; first at step %d); the run's results are NaN"
                         % (where, self.bits, "; ".join(what), self.first_step))


def lib():
    """Load libmacx.so, rebuilding it first when the digest of csrc/ + include/ differs from the one it was built from
    (a sha256 comparison; a no-op when nothing changed).  Where hipcc is absent a library whose digest matches is loaded
    as it is; a stale one raises.  Raises if the library cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.build(force=bool(os.environ.get("MACX_REBUILD")))
    L = C.CDLL(path)
    missing = [n for n in EXPORTS if not hasattr(L, n)]
    if missing:
        raise ImportError("libmacx.so lacks symbols: %s" % missing)
    if L.macx_abi_version() != ABI_VERSION:
        raise ImportError("libmacx.so ABI %d != binding ABI %d" % (L.macx_abi_version(), ABI_VERSION))
    for n, (restype, argtypes) in TABLE.items():
        f = getattr(L, n)
        f.restype, f.argtypes = restype, list(argtypes)
    _lib = L
    return L


def ptr(t):
    """a tensor's device address as a ctypes argument; None -> NULL"""
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def stream_of(where):
    """torch's CURRENT stream on a tensor's device (or on a device) as a ctypes argument -- read it where the call is made"""
    return C.c_void_p(torch.cuda.current_stream(getattr(where, "device", where)).cuda_stream)


def check(code, where):
    if code != 0:
        raise MacxError(code, where)


PACK_TRANSPOSE, PACK_F32MFMA, PACK_BF16X3, PACK_KMAJOR = 1, 0 << 1, 1 << 1, 2 << 1


def kb_pack_flags():
    """macx_pack_weight flags for a weight handed to macx_kb_project (an fp32-operand entry point: native f32 MFMA in mode 0,
    the split-bf16 kernel otherwise) under the GEMM mode in force."""
    return PACK_BF16X3 if lib().macx_gemm_mode(-1) else PACK_F32MFMA
