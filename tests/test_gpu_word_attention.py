"""-m gpu: the word attention of the control unit -- control_attend_kernel, control_bwd_dl_kernel, control_bwd_apply_kernel -- at its batch,
slab and step edges.

Cases, data, reference and bounds: word_attention_cases.py (the path every row takes is in its table and is held to the kernels' loop
rules on the CPU by test_word_attention_host.py, which also shows the bounds fair -- fp32 in another order within half of each -- and
sharp -- six planted defects each exceed one):
  * 2a, the exports on their own (macx_control_attend / macx_control_attend_bwd, 22 rows, two of them forward only because the backward
    refuses d % 64): every element of att, control, d_cc, d_words, d_w and d_b within its bound against the plain fp64 restatement; att
    and d_words of the padded words exactly zero; every output and the workspace between sentinel bands that stay intact; a second
    forward + backward gives the same bits;
  * padding content (U(-100, 100) past each length) changes no bit of any output; a question of length 0 attends uniformly (1 / S within
    one ulp) and its gradient reaches every word; a length above S leaves every word live;
  * S = 257, d % 4, d % 64, a short workspace, B = 0 and S = 0 are refused on the host, before any launch;
  * 2b, the multi-step launches through macx.MACCell in training mode (grids (B, p), nz = p, the accumulating recurrent form), the loss on
    the final state, every att_question map and the controls history, against the fp64 oracle: states and histories < FWD_TOL, every
    att_question map <= 2e-6, every gradient per tensor < GRAD_TOL, and d_words PER (QUESTION, WORD), d_vecQuestions per question and
    ctrlLogits_w per column < GRAD_TOL as well; a second run gives the same bits.
`-s` (and any failure) prints every figure with the worst question, word (its position modulo 32 and 64, its pass) and column; observed:
profiles/word_attention_errors.txt.
"""
import ctypes as C

import pytest
import torch

from abi_kit import Guarded, bits_equal, ptr
from helpers import rel_err
import state_grads_ref as sr
import test_gpu_state_grads as sg
import word_attention_cases as wa

pytestmark = pytest.mark.gpu

EINVAL, ESMALL = -1, -4


# ---- 2a: the exports ------------------------------------------------------------------------------------------------------
def run_exports(macx, dev, r, data):
    """forward (+ backward where the row has one) on guarded outputs -> {output: host tensor}, "ws"; asserts the bands"""
    L = macx._lib.lib()
    B, S, d = r.B, r.S, r.d
    sh = macx._lib.MacxShapes(B=B, S=S, N=1, d=d, p=1, b0=0)
    cc, dc, words, w = [t.to(dev).contiguous() for t in (data.cc[0], data.dc[0], data.words, data.w)]
    bias, lengths = torch.tensor([data.bias], device=dev), data.lengths.to(dev)
    n_ws = L.macx_control_attend_bwd_ws_floats(C.byref(sh))
    assert n_ws == wa.ws_floats(B, S, d)
    sizes = dict(att=B * S, control=B * d)
    if r.bwd:
        sizes.update(d_cc=B * d, d_words=B * S * d, d_w=d, d_b=1, ws=n_ws)
    buf = {k: Guarded(n, dev) for k, n in sizes.items()}
    macx._lib.check(L.macx_control_attend(C.byref(sh), ptr(cc), ptr(words), ptr(lengths), ptr(w), ptr(bias), ptr(buf["att"].view),
                                          ptr(buf["control"].view), None), "macx_control_attend")
    if r.bwd:
        macx._lib.check(L.macx_control_attend_bwd(C.byref(sh), ptr(dc), ptr(cc), ptr(buf["att"].view), ptr(words), ptr(w), ptr(buf["ws"].view), n_ws,
                                                  ptr(buf["d_cc"].view), ptr(buf["d_words"].view), ptr(buf["d_w"].view), ptr(buf["d_b"].view), None),
                        "macx_control_attend_bwd")
    else:
        one = torch.zeros(max(n_ws, B * S * d), device=dev)
        assert L.macx_control_attend_bwd(C.byref(sh), ptr(dc), ptr(cc), ptr(buf["att"].view), ptr(words), ptr(w), ptr(one), n_ws, ptr(one), ptr(one),
                                         ptr(one), ptr(one), None) == EINVAL                     # d % 64
    torch.cuda.synchronize()
    broken = [k for k, g in buf.items() if not g.intact()]
    assert not broken, "sentinel bands overwritten around %s (%s)" % (broken, r.id)
    shapes = dict(att=(B, S), control=(B, d), d_cc=(B, d), d_words=(B, S, d), d_w=(d,), d_b=(), ws=(n_ws,))
    return {k: g.view.clone().cpu().view(shapes[k]) for k, g in buf.items()}


def check_against_bounds(r, data, got, what="hip"):
    ref = wa.reference(data)
    outs = wa.OUTPUTS if r.bwd else wa.OUTPUTS_FWD
    res = wa.ratios(got, ref, wa.bounds(data), outs)
    wa.log(wa.line(r, what, res))
    for k, (q, where) in res.items():
        print("    %-8s %.3f of its bound at %s" % (k, q, where))
    bad = ["%s %.3f of its bound at %s" % (k, q, where) for k, (q, where) in res.items() if not q <= 1.0]
    assert not bad, "\n".join([r.reaches, str(wa.route(r.S, r.d))] + bad)
    # padded words: exactly zero attention and exactly zero gradient
    for b, n in enumerate(data.lengths.tolist()):
        if 0 < n < r.S:
            assert float(got["att"][b, n:].abs().max()) == 0.0, (r.id, b)
            if r.bwd:
                assert float(got["d_words"][b, n:].abs().max()) == 0.0, (r.id, b)
    return ref


@pytest.mark.parametrize("row", wa.ROWS, ids=lambda r: r.id)
def test_exports_at_the_batch_slab_and_width_edges(macx, dev, row):
    data = wa.make_data(row)
    first = run_exports(macx, dev, row, data)
    second = run_exports(macx, dev, row, data)
    assert all(bool(torch.isfinite(v).all()) for k, v in first.items() if k != "ws")
    check_against_bounds(row, data, first)
    differs = [k for k in first if not bits_equal(first[k], second[k])]
    assert not differs, "a second forward + backward differs in %s" % differs


@pytest.mark.parametrize("row", wa.PADDING_ROWS, ids=lambda r: r.id)
def test_padding_content_does_not_matter(macx, dev, row):
    """the words past each length filled with U(-100, 100): every output bit for bit what the same call gives with them zeroed (their
    logits round to -1e30, att = 0, fmaf(0, x, r) = r)"""
    data = wa.make_data(row)
    filled, zeroed = wa.fill_padding(data), wa.zero_padding(data)
    pad = [filled.words[b, n:] for b, n in enumerate(row.lengths) if n < row.S]
    assert pad and all(float(x.abs().max()) > 90 and bool(torch.isfinite(x).all()) for x in pad)
    a, b = run_exports(macx, dev, row, filled), run_exports(macx, dev, row, zeroed)
    differs = [k for k in wa.OUTPUTS if not bits_equal(a[k], b[k])]
    assert not differs, "padding content reaches %s" % differs
    assert torch.equal(a["ws"], b["ws"])                                        # (the dl scratch may differ in the sign of a zero)
    check_against_bounds(row, zeroed, a, "padding")


@pytest.mark.parametrize("row", wa.PADDING_ROWS, ids=lambda r: r.id)
def test_length_zero_and_a_length_above_S(macx, dev, row):
    """length 0: expMask makes every logit -1e30, so the attention is uniform and the gradient reaches every word, as in the fp64
    reference; length S + 7: every word is live"""
    S = row.S
    lengths = (S, 0, S + 7) if row.B == 3 else (0, S + 7)
    zero, above = lengths.index(0), lengths.index(S + 7)
    data = wa.make_data(row, lengths=lengths)
    got = run_exports(macx, dev, row, data)
    ref = check_against_bounds(row, data, got, "lengths")
    att = got["att"][zero].double()
    assert float((att - 1.0 / S).abs().max()) <= 2.0 ** -23 / S and bool((got["att"][zero] == got["att"][zero, 0]).all())
    assert float(got["d_words"][zero].abs().amax(-1).min()) > 0 and float(ref["d_words"][zero].abs().amax(-1).min()) > 0
    assert float(got["att"][above].min()) > 0 and float(got["d_words"][above].abs().amax(-1).min()) > 0


def test_refusals_come_before_any_launch(macx, dev):
    L = macx._lib.lib()
    big = lambda: torch.full((257 * 64 * 2 + 64,), 7.0, device=dev)
    cc, words, w, bias, att, ctl, dc, ws, dcc, dwords, dw, db = [big() for _ in range(12)]
    lengths = torch.ones(4, dtype=torch.int32, device=dev)
    outs = (att, ctl, ws, dcc, dwords, dw, db)

    def fwd(B, S, d):
        sh = macx._lib.MacxShapes(B=B, S=S, N=1, d=d, p=1, b0=0)
        return L.macx_control_attend(C.byref(sh), ptr(cc), ptr(words), ptr(lengths), ptr(w), ptr(bias), ptr(att), ptr(ctl), None)

    def bwd(B, S, d, short=0):
        sh = macx._lib.MacxShapes(B=B, S=S, N=1, d=d, p=1, b0=0)
        n = L.macx_control_attend_bwd_ws_floats(C.byref(sh))
        return L.macx_control_attend_bwd(C.byref(sh), ptr(dc), ptr(cc), ptr(att), ptr(words), ptr(w), ptr(ws), n - short, ptr(dcc), ptr(dwords),
                                         ptr(dw), ptr(db), None)

    assert fwd(2, 257, 64) == EINVAL and bwd(2, 257, 64) == EINVAL                  # S above C_MAXS
    assert fwd(2, 5, 66) == EINVAL                                                  # d % 4
    assert bwd(2, 5, 68) == EINVAL                                                  # d % 64
    assert bwd(2, 5, 64, short=1) == ESMALL
    assert fwd(0, 5, 64) == EINVAL and bwd(0, 5, 64) == EINVAL                      # B < 1
    assert fwd(2, 0, 64) == EINVAL and bwd(2, 0, 64) == EINVAL                      # S < 1: a softmax over nothing
    assert fwd(-1, 5, 64) == EINVAL and bwd(2, -3, 64) == EINVAL
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs), "a refused call wrote"
    assert fwd(2, 5, 64) == 0 and bwd(2, 5, 64) == 0                                # and the same buffers are accepted at a legal shape
    torch.cuda.synchronize()
    assert (macx._lib.MACX_EINVAL, macx._lib.MACX_ESMALL) == (EINVAL, ESMALL)


# ---- 2b: the multi-step launches, through the cell ------------------------------------------------------------------------
def run_cell(macx, dev, r, Gs):
    cfg, vq, words, lengths, kb = wa.cell_inputs(r)
    cell, params, inputs = sg._build(macx, dev, cfg, vq, words, lengths, kb)
    assert type(cell).__name__ == "MACCell"
    state = cell.run()
    sr.aux_loss(cell, state, Gs, lambda G: G.to(dev)).backward()
    torch.cuda.synchronize()
    if hasattr(cell, "status"):
        assert cell.status() == (0, -1)
    return cfg, cell, state, params, inputs


@pytest.mark.parametrize("row", wa.CELL_ROWS, ids=lambda r: r.id)
def test_multi_step_launches_through_the_cell(macx, dev, row):
    B, S, p = row.B, row.S, row.p
    Gs = sr.incoming(wa.cell_targets(p), B, S, row.N, row.d, p)
    cfg, cell, state, params, inputs = run_cell(macx, dev, row, Gs)
    ref = wa.cell_reference(macx, row, params.to_reference_dict())
    assert all(torch.equal(ref["Gs"][k], Gs[k]) for k in Gs)
    fwd = {"memory": rel_err(state.memory, ref["memory"]), "control": rel_err(state.control, ref["control"]),
           "controls": rel_err(cell.controls, ref["cell"].controls), "memories": rel_err(cell.memories, ref["cell"].memories)}
    att = max(float((cell.attentions["question"][i].detach().cpu().double() - ref["cell"].attentions["question"][i].detach()).abs().max())
              for i in range(p))
    errs = sg._grad_errors(macx, cfg, p, params, inputs, ref)
    rows = wa.per_row_err(inputs[1].grad, ref["inputs"][1].grad)                                    # [B, S]
    b, s = divmod(int(rows.argmax()), S)
    vq_rows = wa.per_row_err(inputs[0].grad, ref["inputs"][0].grad)
    (wname, _), = macx.params.reference_names(cfg, p)["ctrlLogits_w"]
    assert wname == wa.CTRL_W
    w_cols = wa.per_row_err(params.ctrlLogits_w.grad.reshape(-1, 1), ref["params"][wname].grad.reshape(-1, 1))
    worst = max(errs, key=errs.get)
    wa.log("%-24s fwd %.2f att %.2f grad %.3f (%s) d_words per word %.3f d_vecQuestions per question %.3f ctrlLogits_w per column %.3f"
           % (row.id, max(fwd.values()) / sg.FWD_TOL, att / 2e-6, errs[worst] / sg.GRAD_TOL, worst,
              float(rows.max()) / sg.GRAD_TOL, float(vq_rows.max()) / sg.GRAD_TOL, float(w_cols.max()) / sg.GRAD_TOL))
    print("    worst word: question %d (length %d) %s over %d steps; worst column of ctrlLogits_w %d"
          % (b, row.lengths[b], wa.word_where(s), p, int(w_cols.argmax())))
    bad = {k: v for k, v in fwd.items() if not v < sg.FWD_TOL}
    bad.update({k: v for k, v in errs.items() if not v < sg.GRAD_TOL})
    if not att <= 2e-6:
        bad["att_question"] = att
    if not float(rows.max()) < sg.GRAD_TOL:
        bad["d_words question %d %s" % (b, wa.word_where(s))] = float(rows.max())
    if not float(vq_rows.max()) < sg.GRAD_TOL:
        bad["d_vecQuestions question %d" % int(vq_rows.argmax())] = float(vq_rows.max())
    if not float(w_cols.max()) < sg.GRAD_TOL:
        bad["ctrlLogits_w column %d" % int(w_cols.argmax())] = float(w_cols.max())
    assert not bad, "\n".join([row.reaches, str(bad)])
    for q, n in enumerate(row.lengths):                                                          # padded words: exactly zero
        assert n == S or float(inputs[1].grad[q, n:].abs().max()) == 0.0, q
    # a second run: the same bits
    _, cell2, state2, params2, inputs2 = run_cell(macx, dev, row, Gs)
    assert bits_equal(state.memory.detach(), state2.memory.detach()) and bits_equal(cell.controls.detach(), cell2.controls.detach())
    assert all(bits_equal(cell.attentions["question"][i].detach(), cell2.attentions["question"][i].detach()) for i in range(p))
    assert all(bits_equal(a.grad, c.grad) for a, c in zip(inputs, inputs2)), "input gradients differ between two runs"
    differs = [f for f in params.fields if not bits_equal(getattr(params, f).grad, getattr(params2, f).grad)]
    assert not differs, differs
