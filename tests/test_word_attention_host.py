"""CPU: what tests/test_gpu_word_attention.py rests on (cases, data, reference, bounds: word_attention_cases.py).

  * pin: the plain fp64 restatement every device figure is taken against equals the oracle's control unit (mo.Ops.expMask and the
    attention and summary of MACCellOracle.control), values and every gradient, 1e-12, on five rows, one with a question of length 0
    and one of a length above S;
  * fair: an fp32 evaluation of the same formulas in another summation order (plain np.sum over d and over S, steps summed last) stays
    within HALF of every bound on every row; the worst ratio per output goes to the file MACX_WORD_ATTENTION_LOG names;
  * sharp: the kernels' loops restated in numpy stay within every bound as they are, and each of six planted defects exceeds a bound on
    every row where its path is live;
  * live inputs: every live word carries weight, padded words have an exactly zero reference gradient, the data property d_b's constant
    rests on, and every word inside a question's length has a non-zero reference gradient in every row of the cell table;
  * paths: every row takes the path it names under the restated loop rules, the issue's rows are all there, and the rules' C++ text
    still reads as restated;
  * the workspace size call equals the restated layout for every row."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import mac_oracle as mo
import state_grads_ref as sr
import word_attention_cases as wa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mac-network_amd", "csrc")

_REF = {}          # one row's data, reference and bounds at a time


def ref_of(r):
    if _REF.get("id") != r.id:
        data = wa.make_data(r)
        t = wa.terms(data)
        _REF.clear()
        _REF.update(id=r.id, data=data, ref=wa.reference(data), terms=t, bounds=wa.bounds(data, t))
    return _REF


def outputs_of(r):
    return wa.OUTPUTS if r.bwd else wa.OUTPUTS_FWD


# ---- pin ------------------------------------------------------------------------------------------------------------------
W_NAME = "MACnetwork/MACCell/control/inter2logits/linearLayerlogits/weights/weight"
B_NAME = "MACnetwork/MACCell/control/inter2logits/linearLayerlogits/biases/bias"


@pytest.mark.parametrize("rid, lengths", [("B3-S4-d128", None), ("B3-S65-d256", None), ("B2-S129-d576", None), ("B3-S33-d68", None),
                                          ("B3-S65-d256", (65, 0, 72))])
def test_reference_is_the_oracles_control_unit(rid, lengths):
    r = wa.BY_ID[rid]
    data = wa.make_data(r, lengths=lengths)
    mine = wa.reference(data)
    dt = torch.float64
    cfg = mo.flag_file_config("args", netLength=1, memDim=r.d, ctrlDim=r.d, attDim=r.d)
    prm = {W_NAME: data.w.to(dt).clone().requires_grad_(True), B_NAME: torch.tensor(data.bias, dtype=dt, requires_grad=True)}
    cc, words = data.cc[0].to(dt).requires_grad_(True), data.words.to(dt).requires_grad_(True)
    vs = mo.VarStore(params=prm, dtype=dt)
    cell = mo.MACCellOracle(cfg, vs, torch.zeros(r.B, r.d, dtype=dt), words, words, data.lengths, torch.zeros(r.B, 1, r.d, dtype=dt),
                            1.0, 1.0, 1.0, r.B, False)
    cell.attentions = {"question": []}                                       # zero_state's list, without its state variables
    with vs.scope("MACnetwork"), vs.scope("MACCell"):
        control, cont = cell.control(cc, words, words, data.lengths, None)
    assert cont is cc and set(prm) == {W_NAME, B_NAME}                       # nothing created: the unit read the two variables named
    att = cell.attentions["question"][-1]
    (control * data.dc[0].to(dt)).sum().backward()
    close = lambda a, b: float((a.reshape(b.shape) - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(mine["att"], att.detach()) and close(mine["control"], control.detach())
    assert close(mine["d_cc"], cc.grad) and close(mine["d_words"], words.grad) and close(mine["d_w"], prm[W_NAME].grad)
    assert close(mine["d_b"], prm[B_NAME].grad)
    assert float(words.grad.abs().max()) > 1e-3
    if lengths:
        assert float((att[1].detach() - 1.0 / r.S).abs().max()) < 1e-15 and float(words.grad[1].abs().amax(-1).min()) > 0     # length 0: uniform, every word reached
        assert float(att[2].detach().min()) > 0                                                                               # a length above S: all live
    # the bounds' own fp64 intermediates are this reference's
    t = wa.terms(data)
    assert close(torch.from_numpy(t["att"]), mine["att"])
    d_words = np.einsum("zbs,zbk->bsk", t["att"], t["dc"]) + np.einsum("zbs,zbk->bsk", t["dl"], t["ccw"])
    assert close(torch.from_numpy(d_words), mine["d_words"])


# ---- fair -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", wa.ROWS + wa.CELL_ROWS, ids=lambda r: r.id)
def test_fp32_in_another_order_is_within_half_of_every_bound(row):
    c = ref_of(row)
    res = wa.ratios(wa.eval_fp32(c["data"]), c["ref"], c["bounds"], outputs_of(row))
    wa.log(wa.line(row, "fp32", res))
    bad = ["%s %.3f > %.1f: %s" % (k, v[0], wa.FAIR, v[1]) for k, v in res.items() if not v[0] <= wa.FAIR]
    assert not bad, "\n".join(bad)


# ---- sharp ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", wa.ROWS + wa.CELL_ROWS, ids=lambda r: r.id)
def test_restated_loops_are_within_every_bound(row):
    c = ref_of(row)
    res = wa.ratios(wa.kernel_restatement(c["data"], recurrent=row.recurrent, bwd=row.bwd), c["ref"], c["bounds"], outputs_of(row))
    wa.log(wa.line(row, "loops", res))
    assert all(v[0] <= 1.0 for v in res.values()), res


@pytest.mark.parametrize("name", sorted(wa.DEFECTS))
def test_a_planted_defect_exceeds_a_bound(name):
    rows = [r for r in wa.ROWS + wa.CELL_ROWS if wa.defect_is_live(name, r)]
    assert len(rows) >= 2, name
    kept = []
    for r in rows:
        c = ref_of(r)
        res = wa.ratios(wa.kernel_restatement(c["data"], defect=name, recurrent=r.recurrent, bwd=r.bwd), c["ref"], c["bounds"], outputs_of(r))
        worst = max(res, key=lambda k: res[k][0])
        print("defect %s %-22s %s %.1f at %s" % (name, r.id, worst, res[worst][0], res[worst][1]))
        if not res[worst][0] > 1.0:
            kept.append((r.id, res))
    assert not kept, (wa.DEFECTS[name], kept)


def test_defects_are_live_where_the_table_says():
    live = {n: [r.id for r in wa.ROWS + wa.CELL_ROWS if wa.defect_is_live(n, r)] for n in wa.DEFECTS}
    assert len(live["a"]) >= 25 and "B3-S33-d128" in live["a"] and "B3-S32-d128" not in live["a"]
    assert "B1-S1-d64" not in live["b"] and len(live["b"]) == len(wa.ROWS) + len(wa.CELL_ROWS) - 1
    assert "B3-S65-d256" in live["c"] and "B3-S64-d256" not in live["c"] and "B3-S65-d260" not in live["c"]
    assert set(live["d"]) == {r.id for r in wa.CELL_ROWS if r.p >= 5 and not r.recurrent} and len(live["d"]) >= 6
    assert set(live["f"]) == {r.id for r in wa.CELL_ROWS if r.flags == "args1"} and len(live["f"]) == 2


# ---- live inputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", wa.ROWS, ids=lambda r: r.id)
def test_inputs_are_live(row):
    c = ref_of(row)
    t, ref = c["terms"], c["ref"]
    for b, n in enumerate(row.lengths):
        assert float((t["att"][0, b, :n] * n).min()) >= 0.05, (row.id, b)
        assert float(ref["att"][0, b, n:].abs().sum()) == 0.0
        if n < row.S:
            assert float(ref["d_words"][b, n:].abs().max()) == 0.0                         # exactly zero
        assert float(c["bounds"]["d_words"][b, n:].max(initial=0.0)) == 0.0
        if n > 1:
            assert float(ref["d_words"][b, :n].abs().amax(-1).min()) > 0
    # the data property d_b's constant rests on (word_attention_cases: bounds)
    att_da, dl = wa.db_condition(t)
    assert att_da <= 2.0 * dl, (att_da, dl)
    for b, n in enumerate(row.lengths):                                                    # a one-word question: dl exactly zero
        if n == 1:
            assert float(np.abs(t["dl"][:, b]).max()) == 0.0 and float(t["att"][0, b, 0]) == 1.0


@pytest.mark.parametrize("row", wa.CELL_ROWS, ids=lambda r: r.id)
def test_cell_rows_reach_every_live_word(macx, row):
    """the reference gradient of every word inside its question's length is non-zero, of every padded word exactly zero; g_att is live
    at every step"""
    cfg, vq, words, lengths, kb = wa.cell_inputs(row)
    assert tuple(lengths.tolist()) == row.lengths and row.lengths[0] == row.S and cfg.netLength == row.p
    assert bool(cfg.controlFeedPrev) == row.recurrent
    ref = wa.cell_reference(macx, row)
    g = ref["inputs"][1].grad
    for b, n in enumerate(row.lengths):
        assert float(g[b, :n].abs().amax(-1).min()) > 0, (row.id, b)
        assert n == row.S or float(g[b, n:].abs().max()) == 0.0
    assert len(ref["cell"].attentions["question"]) == row.p
    att = torch.stack(ref["cell"].attentions["question"]).detach()
    assert float((att.sum(-1) - 1).abs().max()) < 1e-12 and att.shape == (row.p, row.B, row.S)


@pytest.mark.parametrize("row", wa.CELL_ROWS, ids=lambda r: r.id)
def test_cell_rows_are_fair_to_the_finer_metrics(macx, row):
    """the draw each cell row runs on: the reference keeps every entry of ctrlLogits_w's gradient above 2^-8 of the largest, and the fp32
    oracle stays within half of GRAD_TOL per word, per question and per column (word_attention_cases.cell_fairness); it is the first
    such draw (checked where that takes a few draws)"""
    import test_gpu_state_grads as sg
    f = wa.cell_fairness(macx, row)
    wa.log("%-24s fp32 oracle: d_words per word %.3f d_vecQuestions per question %.3f ctrlLogits_w per column %.3f of GRAD_TOL; smallest entry "
           "%.1e of the largest" % (row.id, f["d_words"] / sg.GRAD_TOL, f["d_vecQuestions"] / sg.GRAD_TOL, f["ctrlLogits_w"] / sg.GRAD_TOL, f["floor"]))
    assert wa.cell_is_fair(f, sg.GRAD_TOL), f
    if row.draw <= 6:
        assert wa.first_fair_draw(macx, row, sg.GRAD_TOL) == row.draw


# ---- paths ----------------------------------------------------------------------------------------------------------------
def test_tables_hold_the_issue_rows():
    have = [(r.B, r.S, r.d, r.bwd) for r in wa.ROWS]
    want = [(1, 1, 64), (3, 4, 128), (3, 5, 128), (3, 31, 128), (3, 32, 128), (3, 33, 128), (3, 63, 256), (3, 64, 256), (3, 65, 256),
            (2, 65, 64), (2, 96, 320), (3, 127, 128), (3, 128, 128), (3, 129, 128), (2, 129, 576), (2, 255, 128), (2, 256, 128),
            (2, 33, 1024), (2, 256, 1024), (5, 65, 512)]
    assert have == [w + (True,) for w in want] + [(3, 33, 68, False), (3, 65, 260, False)]
    cells = [(r.flags, r.B, r.S, r.p, r.d, r.N) for r in wa.CELL_ROWS]
    assert cells == [("args", 3, 33, 4, 128, 9), ("args", 2, 64, 8, 128, 9), ("args", 2, 65, 5, 128, 9), ("args", 2, 65, 9, 128, 9),
                     ("args", 2, 129, 32, 128, 9), ("args", 2, 256, 7, 128, 9), ("args", 2, 65, 5, 512, 20), ("args1", 2, 65, 3, 128, 9),
                     ("args1", 2, 130, 5, 128, 9), ("args3", 2, 65, 5, 128, 9), ("args4", 2, 129, 3, 128, 9)]
    for r in wa.ROWS:
        assert r.lengths[0] == r.S and all(n in (1, r.S - 1, 32, 33, 64, 65) and n <= r.S for n in r.lengths[1:]), r.id
    named = {n for r in wa.ROWS for n in r.lengths[1:]}
    assert named >= {1, 32, 33, 64, 65}
    assert [(r.B, r.S, r.d) for r in wa.PADDING_ROWS] == [(3, 65, 256), (2, 129, 128)]


@pytest.mark.parametrize("row", wa.ROWS + wa.CELL_ROWS, ids=lambda r: r.id)
def test_row_takes_the_path_it_names(row):
    rt = wa.route(row.S, row.d, 1 if row.recurrent else row.Z)           # recurrent control: nz = 1 per launch
    assert row.expect, row.id
    for k, v in row.expect.items():
        assert rt[k] == v, (row.id, k, rt[k], v)


def test_the_edges_the_tables_were_chosen_for():
    routes = {r.id: wa.route(r.S, r.d) for r in wa.ROWS}
    assert {(rt["trips"], rt["reread"]) for rt in routes.values()} >= {(1, 0), (1, 1), (1, 27), (1, 28), (2, 0), (2, 1), (2, 7), (3, 7),
                                                                      (4, 0), (4, 1), (5, 7), (8, 0), (8, 1)}
    assert {(rt["passes"], rt["last_pass"]) for rt in routes.values()} >= {(1, 1), (1, 63), (1, 64), (2, 1), (2, 32), (2, 63), (2, 64),
                                                                          (3, 1), (4, 63), (4, 64)}
    assert {rt["k256"] for rt in routes.values()} == {1, 2, 3, 4} and {rt["k512"] for rt in routes.values()} == {1, 2}
    assert {rt["slabs"] for rt in routes.values()} >= {1, 2, 4, 5, 8, 9, 16, None}
    assert {rt["lanes_last"] for rt in routes.values()} >= {1, 16, 17, 32, 64}
    # a second pass together with a second Racc slot; every slot; a last pass of one word with more than two steps
    cells = {r.id: (wa.route(r.S, r.d, r.p), r) for r in wa.CELL_ROWS}
    assert any(rt["passes"] >= 2 and rt["racc"] >= 2 and not r.recurrent for rt, r in cells.values())
    assert any(rt["racc"] == wa.CB_MAXZ // 4 and rt["passes"] == 3 and rt["last_pass"] == 1 for rt, r in cells.values())
    assert sum(1 for rt, r in cells.values() if rt["last_pass"] == 1 and r.p > 2) >= 5
    assert any(r.recurrent and rt["passes"] >= 3 for rt, r in cells.values())
    assert wa.route(33, 128)["trips"] == 2 and wa.route(32, 128)["trips"] == 1 and wa.route(256, 128)["trips"] == 8


def test_the_rules_read_as_restated():
    """the C++ text behind route(): the constants, the batch loop with its clamp and drop, the width loops, the slab pass and Racc"""
    flat = lambda s: re.sub(r"\s+", " ", s)
    small = flat(open(os.path.join(CSRC, "macx_small.hip.h")).read())
    small = small[small.index("struct CtrlP {"): small.index("struct KbAttP {")]                 # the three word-attention kernels
    api = flat(open(os.path.join(CSRC, "macx_api.hip")).read())
    assert "constexpr int C_MAXS = %d;" % wa.C_MAXS in small and "constexpr int CA_U = %d;" % wa.CA_U in small
    assert "constexpr int CB_MAXZ = %d;" % wa.CB_MAXZ in small
    assert small.count("for (int s0 = wave; s0 < p.S; s0 += 4 * CA_U) {") == 2
    assert small.count("(size_t)min(s0 + 4 * u, p.S - 1) * p.d + k);") == 2
    assert small.count("const int s = s0 + 4 * u;") == 2 and small.count("if (lane == 0 && s < p.S)") == 2
    assert small.count("for (int k = lane * 4; k < p.d; k += 256) {") == 2
    assert "for (int k = tid * 2; k < p.d; k += 512) {" in small
    assert "__shared__ float s_logit[C_MAXS];" in small and "__shared__ float s_da[C_MAXS];" in small
    assert "__shared__ float s_words[%d][%d];" % (wa.SLAB, wa.SLAB) in small
    assert "for (int sb = 0; sb < p.S; sb += %d) {" % wa.SLAB in small and "const int sn = min(%d, p.S - sb);" % wa.SLAB in small
    assert "const int b = blockIdx.x, c0 = blockIdx.y * %d;" % wa.SLAB in small
    assert "float Racc[CB_MAXZ / 4];" in small and small.count("const int z = grp + 4 * i;") == 2
    assert "for (int s = grp; s < sn; s += 4) {" in small
    assert "*dst = p.acc_words ? *dst + v : v;" in small and "*dst = p.acc_words ? *dst + t : t;" in small
    # one launcher per direction: every launch of the three kernels in the library is one of these three lines
    assert api.count("hipLaunchKernelGGL(control_bwd_apply_kernel, dim3(B, d / %d), dim3(256), 0, st, c);" % wa.SLAB) == 1
    assert api.count("hipLaunchKernelGGL(control_bwd_dl_kernel, dim3(B, nz), dim3(256), 0, st, c);") == 1
    assert api.count("hipLaunchKernelGGL(control_attend_kernel, dim3(B, nz), dim3(256), 0, st, c);") == 1
    assert [api.count(k) for k in ("control_bwd_apply_kernel,", "control_bwd_dl_kernel,", "control_attend_kernel,")] == [1, 1, 1]
    assert "c.B = B; c.S = S; c.d = d; c.nz = nz;" in api
    # ... which the cell calls with nz = p where the control is not recurrent, and step by step where it is
    assert "CKI(control_attend(B, s->S, d, p, saved + L.cc," in api and "return control_attend(B, S, d, 1, cc_i," in api
    assert "CKI(control_attend_bwd(B, S, d, p, DC + Bd," in api and "CKI(control_attend_bwd(B, S, d, 1, DC + (size_t)(i + 1) * Bd," in api
    assert "return control_attend(s->B, s->S, s->d, 1, cc," in api and "CKI(control_attend_bwd(B, S, d, 1, d_control," in api
    assert "s->S > C_MAXS || s->N > K_MAXN || s->p > CB_MAXZ" in api
    assert "if (s->B < 1 || s->S < 1 || s->S > C_MAXS || s->d < 4 || s->d % 4 != 0) return MACX_EINVAL;" in api
    assert "if (s->B < 1 || s->S < 1 || s->S > C_MAXS || s->d < 64 || s->d % 64 != 0) return MACX_EINVAL;" in api
    assert "c.dwords = dwords; c.acc_words = acc_words;" in api
    assert "ws + W.ctrl_dl, dcc_i, GI->words, 1," in api and "ws + W.ctrl_dl, ws + W.dcc, GI->words, 0," in api


# ---- the workspace size ---------------------------------------------------------------------------------------------------
def test_workspace_size_equals_the_restated_layout(macx):
    L = macx._lib.lib()
    for r in wa.ROWS + wa.CELL_ROWS:
        sh = macx._lib.MacxShapes(B=r.B, S=r.S, N=1, d=r.d, p=1, b0=0)
        want = wa.al4(r.B * r.S) + wa.al4(r.B * r.d) + wa.al4(r.B)
        assert L.macx_control_attend_bwd_ws_floats(C.byref(sh)) == want == wa.ws_floats(r.B, r.S, r.d), r.id
    assert wa.ws_floats(3, 65, 256) == 196 + 768 + 4 and wa.ws_floats(5, 65, 512) == 328 + 2560 + 8
