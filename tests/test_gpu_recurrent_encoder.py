"""-m gpu: macx.RecurrentQuestionEncoder (macx_rnn_encoder_forward_w / _backward_w) -- encType RNN | GRU | LSTM in one direction
or two -- against tests/rnn_ref.py in fp64 with identical dropout masks, under the tolerances tests/test_gpu_encoder.py holds the
bidirectional LSTM to on the same arithmetic (outputs 1e-5 relative, every parameter gradient 2e-4 with a floor of 1e-7, exact
zeros past a question's end); bit equality with macx.QuestionEncoder for (LSTM, two directions); the raw ABI's refusals; and the
whole tower captured with such an encoder.

Shapes: B = 17 runs a second 16-question block with one live row; h = 128 / 256 are the K loop's clamped and exactly-full
trips, h = 512 its second trip and the largest LDS tile; E = 300 is the padded embedding; S = 1 and a zero-length question are
the recurrence's edges."""
import ctypes as C

import pytest
import torch

import rnn_ref
from abi_kit import Guarded, bits_equal, guarded_allocations, assert_guards_intact, ptr
from helpers import rel_err
from oracle import dropout_hash as dh
from oracle import mac_oracle as mo
from test_gpu_encoder import make_questions

pytestmark = pytest.mark.gpu

PAIRS = [(cell, bi) for cell in ("RNN", "GRU", "LSTM") for bi in (False, True)]
SEED = 9


def config(cell, bi, E, h, **over):
    enc = 2 * h if bi else h
    return mo.flag_file_config("args", encType=cell, encBi=bi, ctrlDim=enc, memDim=enc, attDim=enc, encDim=enc, wrdEmbDim=E, **over)


def make_encoder(macx, dev, cfg, V):
    enc = macx.RecurrentQuestionEncoder(cfg, vocab=V, generator=torch.Generator().manual_seed(3)).to(dev)
    gb = torch.Generator().manual_seed(7)
    with torch.no_grad():                                  # (zero biases would leave their terms untested)
        for f in enc.FIELDS:
            if f.endswith("bias"):
                getattr(enc, f).add_((torch.rand(getattr(enc, f).shape, generator=gb) - 0.5).to(dev))
    return enc


def run_case(macx, dev, cell, bi, B, S, V, E, h, train, b0=0, min_len=1, word=None, **over):
    cfg = config(cell, bi, E, h, **over)
    enc = make_encoder(macx, dev, cfg, V)
    w = enc.dirs * h
    q, lengths = make_questions(B, S, V, seed=11, min_len=min_len)       # question 0 full, question 1 of min_len
    wt = None if word is None else torch.tensor([word - (1 << 32) if word >= (1 << 31) else word], dtype=torch.int32, device=dev)
    with guarded_allocations() as seen:
        words, vecQ = enc(q.to(dev), lengths.to(dev), train=train, seed=SEED, b0=b0, **({} if wt is None else {"mask_word": wt}))
        g = torch.Generator().manual_seed(5)
        dW, dQ = torch.randn(B, S, w, generator=g) / B, torch.randn(B, w, generator=g) / B
        ((words * dW.to(dev)).sum() + (vecQ * dQ.to(dev)).sum()).backward()
        torch.cuda.synchronize()
    assert_guards_intact(seen, "saved / ws of %s" % cell)                # nothing written outside `saved` and `ws`
    dt = torch.float64
    prm = {k: v.cpu().to(dt).requires_grad_(True) for k, v in enc.to_reference_dict().items()}
    ki, kq = (enc.keep_in, enc.keep_q) if train else (1.0, 1.0)
    masks = None
    if train:
        masks = [torch.from_numpy(dh.mask_for(SEED, 11, 0, ki, (B, S, E), b0=b0, word=word or 0)).to(dt),
                 torch.from_numpy(dh.mask_for(SEED, 12, 0, kq, (B, w), b0=b0, word=word or 0)).to(dt)]
    rw, rq = rnn_ref.question_encoder(cfg, mo.VarStore(params=prm, dtype=dt), q, lengths, V, keep_input=ki, keep_question=kq, masks=masks)
    ((rw * dW.to(dt)).sum() + (rq * dQ.to(dt)).sum()).backward()
    return enc, words, vecQ, rw, rq, prm, lengths


def check_case(enc, words, vecQ, rw, rq, prm, lengths):
    B, S = words.shape[:2]
    errs = {"words": rel_err(words, rw), "vecQ": rel_err(vecQ, rq)}
    grads = {f: rel_err(getattr(enc, f).grad, prm[enc.REF_NAMES[f]].grad, floor=1e-7) for f in enc.FIELDS if getattr(enc, f).grad is not None}
    print(errs, grads)
    assert errs["words"] < 1e-5 and errs["vecQ"] < 1e-5, errs
    for b in range(B):      # dynamic_rnn: zero output past the question's end
        assert int(lengths[b]) == S or float(words[b, int(lengths[b]):].detach().abs().max()) == 0.0
    for f, e in grads.items():
        assert e < 2e-4, (f, e)
    assert set(grads) == set(enc.FIELDS) - ({"emb"} if not enc.emb.requires_grad else set())


@pytest.mark.parametrize("B,S,V,E,h,train", [(3, 5, 11, 20, 128, False), (17, 7, 13, 300, 128, True), (2, 9, 30, 64, 256, True)])
@pytest.mark.parametrize("cell,bi", PAIRS)
def test_matches_the_fp64_restatement(macx, dev, cell, bi, B, S, V, E, h, train):
    check_case(*run_case(macx, dev, cell, bi, B, S, V, E, h, train, b0=2))


@pytest.mark.parametrize("cell", ["LSTM", "GRU"])
def test_one_direction_at_the_parser_defaults_width(macx, dev, cell):
    check_case(*run_case(macx, dev, cell, False, 2, 3, 9, 24, 512, True, b0=2))


@pytest.mark.parametrize("cell,bi", PAIRS)
def test_a_single_position(macx, dev, cell, bi):
    check_case(*run_case(macx, dev, cell, bi, 2, 1, 4, 16, 128, False, b0=2))


@pytest.mark.parametrize("cell,bi", PAIRS)
def test_a_zero_length_question(macx, dev, cell, bi):
    enc, words, vecQ, rw, rq, prm, lengths = run_case(macx, dev, cell, bi, 3, 4, 9, 20, 128, True, b0=2, min_len=0)
    assert lengths.tolist()[:2] == [4, 0]
    assert float(words[1].abs().max()) == 0.0 and float(vecQ[1].abs().max()) == 0.0           # the zero state, copied through
    check_case(enc, words, vecQ, rw, rq, prm, lengths)


def test_bidirectional_lstm_returns_the_existing_encoders_bits(macx, dev):
    B, S, V, E, h = 5, 7, 13, 20, 128
    cfg = config("LSTM", True, E, h)
    new = make_encoder(macx, dev, cfg, V)
    old = macx.QuestionEncoder(cfg, vocab=V).to(dev)
    assert type(old) is macx.QuestionEncoder and old.FIELDS == new.FIELDS
    old.load_reference_dict(new.to_reference_dict())
    q, lengths = make_questions(B, S, V, seed=11)
    word = torch.tensor([0x1234ABC], dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(5)
    dW, dQ = torch.randn(B, S, 2 * h, generator=g).to(dev), torch.randn(B, 2 * h, generator=g).to(dev)
    res = []
    for enc in (old, new):
        words, vecQ = enc(q.to(dev), lengths.to(dev), train=True, seed=SEED, b0=2, mask_word=word)
        torch.autograd.backward([words, vecQ], [dW, dQ])
        torch.cuda.synchronize()
        res.append([words.detach(), vecQ.detach()] + [getattr(enc, f).grad for f in enc.FIELDS])
    assert len(res[0]) == 7
    for i, (a, b) in enumerate(zip(*res)):
        assert torch.equal(a, b) and bits_equal(a, b), i


@pytest.mark.parametrize("cell,bi", [("GRU", True), ("RNN", False), ("LSTM", False)])
def test_determinism_shards_and_fixed_embeddings(macx, dev, cell, bi):
    a = run_case(macx, dev, cell, bi, 6, 5, 10, 24, 128, True, wrdEmbFixed=True)
    b = run_case(macx, dev, cell, bi, 6, 5, 10, 24, 128, True, wrdEmbFixed=True)
    assert a[0].emb.grad is None and a[0].fw_kernel.grad is not None                         # a fixed embedding gets no gradient
    assert bits_equal(a[1], b[1]) and bits_equal(a[2], b[2])                                  # two runs, the same bits
    for f in a[0].FIELDS[1:]:
        assert bits_equal(getattr(a[0], f).grad, getattr(b[0], f).grad), f
    # b0: a data-parallel shard computes exactly the rows the full batch would (dropout keyed on the global question)
    enc = a[0]
    q, lengths = make_questions(6, 5, 10, seed=2)
    with torch.no_grad():
        w_full, v_full = enc(q.to(dev), lengths.to(dev), train=True, seed=4)
        w_sh, v_sh = enc(q[4:].to(dev), lengths[4:].to(dev), train=True, seed=4, b0=4)
    assert bits_equal(w_full[4:], w_sh) and bits_equal(v_full[4:], v_sh)


@pytest.mark.parametrize("cell,bi", [("GRU", False), ("RNN", True)])
def test_under_a_mask_word(macx, dev, cell, bi):
    word = 0x9E3779B9
    with_word = run_case(macx, dev, cell, bi, 3, 5, 11, 20, 128, True, b0=2, word=word)
    check_case(*with_word)                                                                    # rnn_ref under keep_mask(..., word=w)
    plain = run_case(macx, dev, cell, bi, 3, 5, 11, 20, 128, True, b0=2)
    assert not bits_equal(with_word[2], plain[2]) and not bits_equal(with_word[1], plain[1])  # ... which are not word 0's masks
    zero = run_case(macx, dev, cell, bi, 3, 5, 11, 20, 128, True, b0=2, word=0)
    assert bits_equal(zero[1], plain[1]) and bits_equal(zero[2], plain[2])


def test_raw_abi_refuses_before_it_launches(macx, dev):
    """cell / dirs out of range, h = 640, a NULL candidate kernel for the GRU, a short `saved`: the code, and nothing written"""
    L, lib = macx._lib.lib(), macx._lib
    B, S, V, E, h = 2, 3, 5, 8, 128
    q, lengths = make_questions(B, S, V, seed=1)
    q, lengths = q.to(dev), lengths.to(dev)
    good = dict(B=B, S=S, V=V, E=E, h=h, b0=0, cell=lib.RNN_CELL["GRU"], dirs=1)
    n_saved = L.macx_rnn_encoder_saved_floats(C.byref(lib.MacxRnnShapes(**good)))
    n_ws = L.macx_rnn_encoder_ws_floats(C.byref(lib.MacxRnnShapes(**good)))
    assert n_saved > 0 and n_ws > 0
    t = {f: torch.randn(s, device=dev) * 0.1 for f, s in (("emb", (V, E)), ("fw_kernel", (E + h, 2 * h)), ("fw_bias", (2 * h,)),
                                                           ("fw_candidate_kernel", (E + h, h)), ("fw_candidate_bias", (h,)))}
    d_words, d_vec = torch.randn(B, S, h, device=dev), torch.randn(B, h, device=dev)
    cases = [(dict(good, cell=3), None, 0, lib.MACX_EINVAL), (dict(good, cell=-1), None, 0, lib.MACX_EINVAL),
             (dict(good, dirs=3), None, 0, lib.MACX_EINVAL), (dict(good, dirs=0), None, 0, lib.MACX_EINVAL),
             (dict(good, h=640), None, 0, lib.MACX_EUNSUPPORTED), (dict(good, h=96), None, 0, lib.MACX_EINVAL),
             (good, "fw_candidate_kernel", 0, lib.MACX_EINVAL), (good, "fw_bias", 0, lib.MACX_EINVAL), (good, None, 4, lib.MACX_ESMALL)]
    for shapes, null, short, code in cases:
        sh = lib.MacxRnnShapes(**shapes)
        sized = (L.macx_rnn_encoder_saved_floats(C.byref(sh)), L.macx_rnn_encoder_ws_floats(C.byref(sh)))
        assert sized == ((n_saved, n_ws) if shapes is good else (0, 0)), shapes
        ps = lib.MacxRnnParams(**{f: (0 if f == null else v.data_ptr()) for f, v in t.items()})
        words, vecQ, saved = Guarded(B * S * h, dev), Guarded(B * h, dev), Guarded(n_saved, dev)
        rc = L.macx_rnn_encoder_forward_w(C.byref(sh), 1.0, 1.0, 1, C.byref(ps), ptr(q), ptr(lengths), ptr(words.view), ptr(vecQ.view),
                                          ptr(saved.view), n_saved - short, None, None)
        torch.cuda.synchronize()
        assert rc == code, (shapes, null, short, rc)
        assert words.untouched() and vecQ.untouched() and saved.untouched(), (shapes, null, short)
        grads = {f: Guarded(v.numel(), dev) for f, v in t.items()}
        gs = lib.MacxRnnGrads(**{f: g.view.data_ptr() for f, g in grads.items()})
        ws = Guarded(n_ws, dev)
        rc = L.macx_rnn_encoder_backward_w(C.byref(sh), 1.0, 1.0, 1, C.byref(ps), ptr(q), ptr(lengths), ptr(saved.view), n_saved - short,
                                           ptr(ws.view), n_ws, ptr(d_words), ptr(d_vec), C.byref(gs), None, None)
        torch.cuda.synchronize()
        assert rc == code, (shapes, null, short, rc)
        assert ws.untouched() and all(g.untouched() for g in grads.values()), (shapes, null, short)
    # a NULL gradient pointer the cell needs, and a short ws
    sh = lib.MacxRnnShapes(**good)
    ps = lib.MacxRnnParams(**{f: v.data_ptr() for f, v in t.items()})
    saved, ws = Guarded(n_saved, dev), Guarded(n_ws, dev)
    grads = {f: Guarded(v.numel(), dev) for f, v in t.items()}
    for null, short, code in (("fw_candidate_bias", 0, lib.MACX_EINVAL), (None, 4, lib.MACX_ESMALL)):
        gs = lib.MacxRnnGrads(**{f: (0 if f == null else g.view.data_ptr()) for f, g in grads.items()})
        rc = L.macx_rnn_encoder_backward_w(C.byref(sh), 1.0, 1.0, 1, C.byref(ps), ptr(q), ptr(lengths), ptr(saved.view), n_saved, ptr(ws.view),
                                           n_ws - short, ptr(d_words), ptr(d_vec), C.byref(gs), None, None)
        torch.cuda.synchronize()
        assert rc == code and ws.untouched() and all(g.untouched() for g in grads.values()), (null, short, rc)
    # ... and the accepted call writes inside its buffers only (pointers the GRU in one direction does not use stay NULL)
    words, vecQ = Guarded(B * S * h, dev), Guarded(B * h, dev)
    rc = L.macx_rnn_encoder_forward_w(C.byref(sh), 1.0, 1.0, 1, C.byref(ps), ptr(q), ptr(lengths), ptr(words.view), ptr(vecQ.view),
                                      ptr(saved.view), n_saved, None, None)
    gs = lib.MacxRnnGrads(**{f: g.view.data_ptr() for f, g in grads.items()})
    rc2 = L.macx_rnn_encoder_backward_w(C.byref(sh), 1.0, 1.0, 1, C.byref(ps), ptr(q), ptr(lengths), ptr(saved.view), n_saved, ptr(ws.view), n_ws,
                                        ptr(d_words), ptr(d_vec), C.byref(gs), None, None)
    torch.cuda.synchronize()
    assert (rc, rc2) == (0, 0)
    for g in [words, vecQ, saved, ws] + list(grads.values()):
        assert g.intact()
    assert all(bool(torch.isfinite(g.view).all()) for g in [words, vecQ] + list(grads.values()))


# ---------------------------------------------------------------------------------------------------------------------------
# the tower: the `args` flag file's option set with a GRU in two directions, and with --encBi off + LSTM
# ---------------------------------------------------------------------------------------------------------------------------
from test_gpu_feature_store import A, B, CIN, D, E, H, P, S, V, W, make_store, questions as tower_questions  # noqa: E402

TOWERS = [dict(encType="GRU", encBi=True), dict(encType="LSTM", encBi=False)]


def recurrent_tower(macx, dev, over):
    """test_gpu_feature_store.make_net's tower (the shapes of test_full_tower_ids_to_logits_gradients) with the encoder's options"""
    cfg = macx.configs.flag_file_config("args", netLength=P, memDim=D, ctrlDim=D, attDim=D, encDim=D, wrdEmbDim=E, outClassifierDims=[32],
                                        answerWordsNum=A, **over)
    cfg.stemDim = 128
    return macx.MACNet(cfg, vocab=V, H=H, W=W, imageInDim=CIN, answerWordsNum=A, generator=torch.Generator().manual_seed(4),
                       encoder="recurrent").to(dev)


def tower_inputs(dev, seed):
    g = torch.Generator().manual_seed(seed)
    q, lengths, ans = tower_questions(dev, seed=seed)
    return torch.relu(torch.randn(B, H * W, CIN, generator=g)).to(dev), q, lengths, ans


@pytest.mark.parametrize("over", TOWERS, ids=["gru_bi", "lstm_uni"])
def test_captured_forward_replays_the_eager_tower(macx, dev, over):
    net = recurrent_tower(macx, dev, over)
    assert type(net.enc) is macx.RecurrentQuestionEncoder
    fwd = macx.CapturedTowerForward(net, B, S, H=H, W=W, imageInDim=CIN)
    assert fwd.captured, "the capture's self-check failed in this process: %r" % (fwd.verify_report,)
    for seed in (1, 2):
        images, q, lengths, _ = tower_inputs(dev, seed)
        with torch.no_grad():
            ref = net(images, q, lengths, train=False).clone()
        got = fwd(images, q, lengths)
        torch.cuda.synchronize()
        assert bits_equal(ref, got), seed
    fwd.check()


def eager_step(macx, dev, ref, rbucket, ropt, batch, it, seed):
    images, q, lengths, ans = batch
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    w = macx.graph.mix32(it) & 0xFFFFFFFF
    word.fill_(w - (1 << 32) if w >= (1 << 31) else w)
    for t in ref.tensors():
        t.grad = None
    logits = ref(images, q, lengths, train=True, seed=seed, check_ids=False, mask_word=word)
    loss, pred = ref.loss_and_pred(logits, ans)
    rbucket.begin_step(B, B)
    loss.backward()
    rbucket.allreduce_(B, B)
    norm = ropt.step(flat_grad=rbucket.flat)
    torch.cuda.synchronize()
    return loss.detach(), logits.detach(), pred, norm


@pytest.mark.parametrize("over", TOWERS, ids=["gru_bi", "lstm_uni"])
def test_captured_train_step_replays_the_eager_step(macx, dev, over):
    net, ref = recurrent_tower(macx, dev, over), recurrent_tower(macx, dev, over)
    bucket, rbucket = macx.dp.TowerBuckets(net, fused_gather=True), macx.dp.TowerBuckets(ref)
    opt, ropt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-3), macx.optim.FlatAdamEMA(rbucket.tensors(), lr=1e-3)
    step = macx.CapturedTowerTrainStep(net, opt, bucket, B, S, H=H, W=W, imageInDim=CIN, seed=1234)
    assert step.captured, "the capture's self-check failed in this process: %r" % (step.verify_report,)
    assert bits_equal(opt.flat, ropt.flat)
    losses = []
    for it in range(2):                                    # fresh mask words: replay(iteration=it)
        batch = tower_inputs(dev, 20 + it)
        step.load(*batch)
        step.replay(iteration=it)
        loss, logits, pred, norm = eager_step(macx, dev, ref, rbucket, ropt, batch, it, 1234)
        pairs = {"loss": (step.loss, loss), "logits": (step.logits, logits), "pred": (step.pred, pred), "norm": (step.norm, norm),
                 "flat gradient": (bucket.flat, rbucket.flat), "m": (opt.m, ropt.m), "v": (opt.v, ropt.v), "flat parameters": (opt.flat, ropt.flat)}
        for what, (a, b) in pairs.items():
            assert bits_equal(a.reshape(-1), b.reshape(-1)), (it, what)
        losses.append(float(loss))
    assert all(torch.isfinite(torch.tensor(losses))) and float(step.norm) > 0
    step.check()


def test_captured_train_step_on_a_question_store(macx, dev):
    """once with questions=: the GRU tower trains by question id as its twin does through load()"""
    from test_gpu_question_store import assert_same_step, make_questions as make_question_store, sliced
    feats, qs = make_store(macx, dev), make_question_store(macx, dev)
    steps = []
    for questions in (qs, None):
        net = recurrent_tower(macx, dev, TOWERS[0])
        bucket = macx.dp.TowerBuckets(net, fused_gather=True)
        opt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-3)
        steps.append(macx.CapturedTowerTrainStep(net, opt, bucket, B, S, seed=1234, features=feats, weights=True, totals=True,
                                                 questions=questions))
        assert steps[-1].captured, "the capture's self-check failed in this process: %r" % (steps[-1].verify_report,)
    step, twin = steps
    for it, ids in enumerate(([7, 0, 7], [1, 2, 3])):
        assert step.load_ids(torch.tensor(ids, device=dev)) == B
        step.replay(iteration=it)
        w = sliced(dev, ids)
        assert twin.load(None, w["questions"], w["lengths"], w["answers"], image_ids=w["rows"], weights=w["weights"]) == B
        twin.replay(iteration=it)
        assert_same_step(step, twin, ids)
    assert qs.check() is qs
