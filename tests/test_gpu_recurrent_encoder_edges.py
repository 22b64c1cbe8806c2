"""-m gpu: the recurrent question encoder at its block, width and length edges -- rnn_step_kernel<MODE> / rnn_step_bwd_kernel<MODE>
(macx_rnn.hip.h), the two LSTM step kernels with their direction count, and the host sequence rnn_forward / rnn_backward that serves
all six (cell, directions) pairs -- through macx.RecurrentQuestionEncoder (macx.QuestionEncoder for the old bidirectional LSTM path)
against rnn_ref in fp64.  tests/recurrent_encoder_cases.py has the table, the data and the metrics; tests/test_recurrent_encoder_cases_host.py
shows on the CPU that the metrics are fair and sharp and that every row runs the edge it names.

  * every row of the table, forward and backward: words per (question, position, direction), vecQ per (question, direction), every
    kernel gradient per column and per row of its input and recurrent rows and of each gate's columns, every bias gradient per gate,
    the embedding gradient per token; exact zeros past a question's end, for an empty question and for a token nothing holds; `saved`
    and `ws` between guard bands;
  * two runs give the same bits; a shuffled batch gives every question the bits it had; the backward pass is linear in the cotangents
    to the bit under x 2^+-16; one cotangent at a time, and garbage in d_words past a question's end; lengths above S and below 0 under
    check_ids=False behave as S and 0, bit for bit.

`-s` prints every figure with the place of the worst entry; MACX_RECURRENT_ENCODER_LOG=<file> appends them (with the fp32 restatement's
figure of the same row beside) the way profiles/recurrent_encoder_errors.txt was recorded."""
import os

import pytest
import torch

import recurrent_encoder_cases as rc
from abi_kit import assert_guards_intact, bits_equal, guarded_allocations

pytestmark = pytest.mark.gpu

_WARM = set()
_WORST = {}            # (pair, group) -> [device value / tolerance, fp32 value / tolerance]


@pytest.fixture(scope="module", autouse=True)
def summary():
    yield
    if _WORST:
        rc.log("worst value / tolerance per pair and metric: device (fp32 rnn_ref on the CPU)")
        for pair in sorted({p for p, _ in _WORST}):
            rc.log("%-7s " % ("%sx%d" % pair) + "  ".join("%s %.4f (%s)" % (g, _WORST[pair, g][0], "%.4f" % _WORST[pair, g][1] if _WORST[pair, g][1] else "-")
                                                        for g in rc.GROUPS if (pair, g) in _WORST))
    _WORST.clear()
    rc._REFS.clear()


def build(macx, dev, c):
    new = rc.make_encoder(macx, c, dev)
    if not c.old_path:
        return new
    old = macx.QuestionEncoder(rc.config(c), vocab=c.V).to(dev)
    assert type(old) is macx.QuestionEncoder and old.FIELDS == new.FIELDS
    old.load_reference_dict(new.to_reference_dict())
    return old


def forward(enc, c, dev, q, lengths, check_ids=True):
    return enc(q.to(dev), lengths.to(dev), train=c.train, seed=rc.SEED, b0=rc.B0, check_ids=check_ids)


def gradients(enc, outs, cots, dev):
    """{field: gradient} of sum (out cot) over the (output, cotangent) pairs given; the graph is kept for another call"""
    g = torch.autograd.grad(list(outs), [getattr(enc, f) for f in enc.FIELDS], [t.to(dev) for t in cots], retain_graph=True)
    torch.cuda.synchronize()
    return dict(zip(enc.FIELDS, g))


def run(macx, dev, c, data=None, check_ids=True, d_words=True, d_vecQ=True, scale=1.0):
    """one forward and backward of the row inside guard bands -> what rc.reference returns, on the device"""
    warm_up(macx, dev, c)
    data = data or rc.make_data(c)
    enc = build(macx, dev, c)
    with guarded_allocations() as seen:
        words, vecQ = forward(enc, c, dev, data.q, data.lengths, check_ids)
        pairs = ([(words, data.d_words * scale)] if d_words else []) + ([(vecQ, data.d_vecQ * scale)] if d_vecQ else [])
        grads = gradients(enc, *zip(*pairs), dev)
    assert_guards_intact(seen, "saved / ws of %s" % c.id)
    assert len(seen) >= 2, len(seen)                                       # `saved` and `ws`
    return dict(words=words.detach(), vecQ=vecQ.detach(), grads=grads)


def warm_up(macx, dev, c):
    """a row wider than h = 128 runs behind an h = 128 run of its pair in this process: the backward kernels raise their LDS attribute
    from a smaller request, the way a process that meets the widths in the table's order does"""
    pair = (c.cell, c.dirs)
    if c.h > 128 and pair not in _WARM:
        w = rc.WARM_UP[pair]
        _WARM.add(pair)
        run(macx, dev, w)
    _WARM.add(pair)


def hold(macx, c, got, ref, what="device", keep=True):
    errs = rc.errors(c, got, ref)
    rc.log(rc.line(c, what, errs))
    e32 = {}
    if os.environ.get("MACX_RECURRENT_ENCODER_LOG") and keep:
        e32 = rc.worst_by_group(rc.errors(c, rc.reference(macx, c, dtype=torch.float32), ref))
        rc.log("%-44s %-10s " % ("", "fp32") + "  ".join("%s %.4f" % (g, e32[g][0]) for g in rc.GROUPS if g in e32))
    for g, (v, name, where) in rc.worst_by_group(errs).items():
        print("    %-18s %.4f of its tolerance: %s, %s" % (g, v, name, where))
        if keep:
            w = _WORST.setdefault(((c.cell, c.dirs), g), [0.0, 0.0])
            w[0], w[1] = max(w[0], v), max(w[1], e32[g][0] if e32 else 0.0)
    bad = rc.failures(errs)
    assert not bad, (c.id, what, bad)
    assert set(got["grads"]) == set(ref["grads"])


def same_bits(a, b, what):
    assert bits_equal(a["words"], b["words"]), (what, "words")
    assert bits_equal(a["vecQ"], b["vecQ"]), (what, "vecQ")
    for f in a["grads"]:
        assert bits_equal(a["grads"][f], b["grads"][f]), (what, f)


@pytest.mark.parametrize("cid", [c.id for c in rc.CASES])
def test_row_against_fp64(macx, dev, cid):
    c = rc.BY_ID[cid]
    print("\n%s: %s" % (c.id, c.reaches))
    hold(macx, c, run(macx, dev, c), rc.cached_reference(macx, c))


@pytest.mark.parametrize("cid", rc.DETERMINISM_IDS)
def test_a_second_run_gives_the_same_bits(macx, dev, cid):
    c = rc.BY_ID[cid]
    same_bits(run(macx, dev, c), run(macx, dev, c), c.id)


@pytest.mark.parametrize("c", rc.PERMUTATION_CASES, ids=lambda c: c.id)
def test_a_shuffled_batch_gives_every_question_its_bits(macx, dev, c):
    """evaluation (keep = 1: no mask keyed on a question's place): the same batch size, so the same launches; a row's products depend
    on nothing else in its tile"""
    assert not c.train
    data, enc = rc.make_data(c), build(macx, dev, c)
    perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(21))
    assert not torch.equal(perm, torch.arange(c.B)) and int((perm // 16 != torch.arange(c.B) // 16).sum()) > c.B // 2       # across blocks
    with torch.no_grad():
        words, vecQ = forward(enc, c, dev, data.q, data.lengths)
        words_p, vecQ_p = forward(enc, c, dev, data.q[perm], data.lengths[perm])
    torch.cuda.synchronize()
    for i, b in enumerate(perm.tolist()):
        assert bits_equal(words_p[i], words[b]) and bits_equal(vecQ_p[i], vecQ[b]), (c.id, "question %d at place %d" % (b, i))


@pytest.mark.parametrize("c", rc.HOMOGENEITY_CASES, ids=lambda c: c.id)
def test_backward_is_linear_in_the_cotangents_to_the_bit(macx, dev, c):
    """d_words and d_vecQ x 2^k: every gradient is the base run's x 2^k, bit for bit (test_recurrent_encoder_cases_host shows that no
    entry can underflow at k = -16)"""
    data, enc = rc.make_data(c), build(macx, dev, c)
    with guarded_allocations() as seen:
        words, vecQ = forward(enc, c, dev, data.q, data.lengths)
        base = gradients(enc, (words, vecQ), (data.d_words, data.d_vecQ), dev)
        for k in (16, -16):
            f = 2.0 ** k
            got = gradients(enc, (words, vecQ), (data.d_words * f, data.d_vecQ * f), dev)
            for name in enc.FIELDS:
                assert float(base[name].abs().max()) > 0 and bits_equal(got[name], base[name] * f), (c.id, k, name)
    assert_guards_intact(seen, c.id)
    hold(macx, c, dict(words=words.detach(), vecQ=vecQ.detach(), grads=base), rc.reference(macx, c), keep=False)


def fill_padding(d_words, lengths, lim=100.0, seed=5):
    """d_words with U(-lim, lim) at every position past a question's end"""
    g = torch.Generator().manual_seed(seed)
    out = d_words.clone()
    S = out.shape[1]
    for b, n in enumerate(lengths.tolist()):
        out[b, n:] = (torch.rand(S - n, out.shape[2], generator=g) * 2 - 1) * lim
    return out


@pytest.mark.parametrize("c", rc.COTANGENT_CASES, ids=lambda c: c.id)
def test_one_cotangent_at_a_time(macx, dev, c):
    """d_vecQ alone, d_words alone, both: three backward calls on one `saved`, each against the fp64 reference of its own loss; what
    d_words holds past a question's end reaches no gradient"""
    data, enc = rc.make_data(c), build(macx, dev, c)
    assert int((data.lengths < c.S).sum()) >= 2
    with guarded_allocations() as seen:
        words, vecQ = forward(enc, c, dev, data.q, data.lengths)
        outs = dict(words=words.detach(), vecQ=vecQ.detach())
        only_q = gradients(enc, (vecQ,), (data.d_vecQ,), dev)
        only_w = gradients(enc, (words,), (data.d_words,), dev)
        both = gradients(enc, (words, vecQ), (data.d_words, data.d_vecQ), dev)
        dirty = fill_padding(data.d_words, data.lengths)
        assert not torch.equal(dirty, data.d_words)
        dirty_w = gradients(enc, (words,), (dirty,), dev)
        dirty_both = gradients(enc, (words, vecQ), (dirty, data.d_vecQ), dev)
    assert_guards_intact(seen, c.id)
    hold(macx, c, dict(outs, grads=only_q), rc.reference(macx, c, d_words=False), "d_vecQ", keep=False)
    hold(macx, c, dict(outs, grads=only_w), rc.reference(macx, c, d_vecQ=False), "d_words", keep=False)
    hold(macx, c, dict(outs, grads=both), rc.reference(macx, c), "both", keep=False)
    for f in enc.FIELDS:
        assert bits_equal(dirty_w[f], only_w[f]) and bits_equal(dirty_both[f], both[f]), (c.id, f)
        assert not bits_equal(only_w[f], both[f]) and not bits_equal(only_q[f], both[f]), (c.id, f)


@pytest.mark.parametrize("c", rc.CLAMP_CASES, ids=lambda c: c.id)
def test_lengths_outside_the_padded_question_are_clamped(macx, dev, c):
    """check_ids=False, as the bench loop and the captured steps call it: a length of S + 3 and one of -2 give the outputs and gradients
    of S and 0, bit for bit, and nothing is written outside `saved` and `ws`"""
    data = rc.make_data(c)
    assert data.lengths.tolist()[:2] == [c.S, 0]
    wild = data.lengths.clone()
    wild[0], wild[1] = c.S + 3, -2
    base = run(macx, dev, c, data=data, check_ids=False)
    got = run(macx, dev, c, data=data._replace(lengths=wild), check_ids=False)
    same_bits(got, base, c.id)
    hold(macx, c, got, rc.reference(macx, c), "clamped", keep=False)
    with pytest.raises(ValueError, match="question length outside"):                         # ... which check_ids=True refuses
        forward(build(macx, dev, c), c, dev, data.q, wild)
