"""-m gpu: evaluation records resident in device memory on the tower -- macx.EvalRecords filed from eager runs, and inside
CapturedTowerForward(records=rec)'s graph.  Every comparison is an equality of bits: the expected tables are the cloned
state tensors and logits of eager runs, filed by tests/records_ref.py (slots in ascending order, .astype(float16) for fp16 tables).

The tower is narrow: d 128 for the eager runs and 256 under capture (the fused question encoder, which the captured classes require,
starts at 128 units per direction: encDim = ctrlDim = 256), S 6, B 6, 9 answers, vocabulary 12, 5 images of 4 x 4 (N 16; args, p 2) or 4 x 5 (N 20; args3, p 3: the
option set with self-attention); the store holds 40 questions of 5 words (one padded column) with image rows and kb_lengths."""
import numpy as np
import pytest
import torch

import records_ref
from abi_kit import bits_equal

pytestmark = pytest.mark.gpu

S, S_TAB, B, A, V, E, IMAGES, CIN, QN = 6, 5, 6, 9, 12, 20, 5, 128, 40
D_EAGER, D_CAPTURED = 128, 256
TOWERS = {"args": ("args", 2, 4, 4, ("kb", "question")), "args3": ("args3", 3, 4, 5, ("kb", "question", "self"))}
SEGMENTS = {"kb": "att_kb", "question": "att_question", "self": "att_self"}


def make_net(macx, dev, flags, p, H, W, d):
    cfg = macx.configs.flag_file_config(flags, netLength=p, memDim=d, ctrlDim=d, attDim=d, encDim=d, wrdEmbDim=E, outClassifierDims=[32],
                                        answerWordsNum=A)
    cfg.stemDim = 128
    return macx.MACNet(cfg, vocab=V, H=H, W=W, imageInDim=CIN, answerWordsNum=A, generator=torch.Generator().manual_seed(4)).to(dev)


def make_features(macx, dev, H, W):
    g = torch.Generator().manual_seed(6)
    return macx.FeatureStore(IMAGES, H, W, CIN, dtype=torch.float16, device=dev).write(0, torch.relu(torch.randn(IMAGES, CIN, H, W, generator=g))).check()


def host_columns(N):
    g = torch.Generator().manual_seed(11)
    lengths = torch.randint(1, S_TAB + 1, (QN,), generator=g, dtype=torch.int32)
    q = torch.randint(1, V + 1, (QN, S_TAB), generator=g, dtype=torch.int32) * (torch.arange(S_TAB)[None] < lengths[:, None]).to(torch.int32)
    return dict(questions=q, lengths=lengths, answers=torch.randint(0, A, (QN,), generator=g, dtype=torch.int32),
                image_rows=torch.randint(0, IMAGES, (QN,), generator=g, dtype=torch.int32),
                kb_lengths=torch.randint(1, N + 1, (QN,), generator=g, dtype=torch.int32))


def tower(macx, dev, name, d):
    flags, p, H, W, maps = TOWERS[name]
    return (make_net(macx, dev, flags, p, H, W, d), make_features(macx, dev, H, W), macx.QuestionStore(device=dev, **host_columns(H * W)),
            p, H * W, maps)


def eager_run(net, feats, qs, ids, maps):
    """one eager forward of the batch `ids` names (the gather's slot rules: a dead slot runs slot 0's question): the logits and the
    run's stacked maps, cloned, as numpy; and the cell"""
    batch = qs.gather(ids, S=S)
    with torch.no_grad():
        logits = net(feats, batch.questions, batch.lengths, image_ids=batch.image_ids, kb_lengths=batch.kb_lengths, check_ids=False)
    cell = net.last_cell
    out = {m: cell.state_tensor(SEGMENTS[m]).detach().clone().cpu().numpy() for m in maps}
    out["logits"] = logits.detach().clone().cpu().numpy()[None]
    return out, cell, logits


def nan_tables(rec):
    return {k: np.full(tuple(t.shape), np.nan, dtype=np.float16 if t.dtype == torch.float16 else np.float32) for k, t in rec.tables.items()}


def shown(k, rows):
    """what read() shows of a table: row i of "self" is its first i + 1 entries, zeros behind them (the run's buffer holds what it held)"""
    return np.tril(rows) if k == "self" else rows


def entries(k, rows):
    """the entries of [rows, steps, n] that belong to the map, flat"""
    return rows[:, np.tril(np.ones(rows.shape[1:], dtype=bool))] if k == "self" else rows.reshape(-1)


def captured(obj):
    assert obj.captured is True, "the capture's self-check failed in this process: %r" % (obj.verify_report,)
    return obj


@pytest.mark.parametrize("name", list(TOWERS))
def test_eager_file_run_files_the_runs_maps_by_id(macx, dev, name):
    net, feats, qs, p, N, maps = tower(macx, dev, name, D_EAGER)
    recs = [macx.EvalRecords(qs, p=p, N=N, S=S, answers=A, maps=maps, dtype=dt) for dt in (torch.float32, torch.float16)]
    assert recs[0].nbytes == QN * (p * (N + S + (p if "self" in maps else 0)) + A) * 4
    ids = torch.tensor([7, QN - 1, 7, -1, 0, QN - 1], dtype=torch.int32, device=dev)      # two ids twice, a dead slot
    run, cell, logits = eager_run(net, feats, qs, ids, maps)
    for rec in recs:
        assert rec.file_run(ids, cell, logits) is rec
        want = {k: records_ref.scatter(t, run[k], ids.cpu().numpy()) for k, t in nan_tables(rec).items()}
        got = rec.read()
        for k in want:
            assert got[k].dtype == want[k].dtype and bits_equal(got[k], shown(k, want[k])), (name, k, rec.dtype)
        filed = sorted({7, QN - 1, 0})
        assert all(np.isfinite(entries(k, got[k][filed])).all() for k in got)
        assert all(np.isnan(entries(k, np.delete(got[k], filed, axis=0))).all() for k in got)      # never filed: NaN
        assert got["logits"].dtype == np.float32                                           # whatever the maps' dtype
        some = rec.read([QN - 1, 3])
        assert all(bits_equal(some[k], got[k][[QN - 1, 3]]) for k in got)
    # file() with the tensors themselves is the same call; a second batch overwrites only what it names
    rec = recs[0]
    before = rec.read()
    ids2 = torch.tensor([3, 7, 12, 12, 12, 5], device=dev)                                  # (int64: converted)
    run2, cell2, logits2 = eager_run(net, feats, qs, ids2.to(torch.int32), maps)
    given = {("self_att" if m == "self" else m): cell2.state_tensor(SEGMENTS[m]) for m in maps}
    rec.file(ids2, logits=logits2, **given)
    got = rec.read()
    for k in got:
        assert bits_equal(got[k], shown(k, records_ref.scatter(before[k], run2[k], ids2.cpu().numpy()))), k
    assert rec.clear() is rec and all(np.isnan(entries(k, v)).all() for k, v in rec.read().items())
    assert qs.check() is qs


@pytest.mark.parametrize("name,dtype", [("args", torch.float16), ("args3", torch.float32)])
def test_an_epoch_of_replays_files_every_questions_maps(macx, dev, name, dtype):
    net, feats, qs, p, N, maps = tower(macx, dev, name, D_CAPTURED)
    cols = host_columns(N)
    rec = macx.EvalRecords(qs, p=p, N=N, S=S, answers=A, maps=maps, logits=True, dtype=dtype)
    table = qs.predictions()
    fwd = captured(macx.CapturedTowerForward(net, B, S, features=feats, questions=qs, score=True, predictions=table, kb_lengths=True,
                                             records=rec))
    assert all(bool(torch.isnan(t).all()) for t in rec.tables.values()) and bool((table == -1).all())      # the self-check's rows are gone
    perm = torch.randperm(QN, generator=torch.Generator().manual_seed(2)).to(torch.int32)
    never, twice = int(perm[37]), int(perm[3])
    perm[37] = twice                                     # one question in the first and in the last batch; another one never named
    # the eager epoch: what every batch's run held, filed in the batches' order
    want, preds = nan_tables(rec), {}
    batches = [perm[k:k + B] for k in range(0, QN, B)]
    assert [len(b) for b in batches] == [6] * 6 + [4]                                     # the last batch is short: two dead slots
    for ids in batches:
        full = torch.cat([ids, torch.full((B - len(ids),), -1, dtype=torch.int32)])
        run, _, logits = eager_run(net, feats, qs, full.to(dev), maps)
        want = {k: records_ref.scatter(want[k], run[k], full.numpy()) for k in want}
        for b, q in enumerate(ids.tolist()):
            preds[q] = int(logits[b].argmax())
    # the captured epoch
    order = macx.EpochOrder(qs, B, order=perm)
    sizes = []
    for _ in range(order.steps):
        sizes.append(fwd.next_batch(order))
        fwd.replay()
    assert sizes == [6] * 6 + [4] and qs.check() is qs
    got = rec.read()
    for k in want:
        assert bits_equal(got[k], shown(k, want[k])), (name, k)
    filed = sorted(set(perm.tolist()))
    assert never not in filed and len(filed) == QN - 1
    assert all(np.isnan(entries(k, got[k][[never]])).all() for k in got) and all(np.isfinite(entries(k, got[k][filed])).all() for k in got)
    # the filed logits name the filed predictions
    index, prob = rec.topk(1)
    assert index[filed, 0].cpu().tolist() == table[filed].cpu().tolist() == [preds[q] for q in filed]
    assert int(table[never]) == -1 and bool(torch.isnan(prob[never]).all())
    # padded columns are exact zeros: behind a question's length, behind its knowledge base's size
    for q in filed:
        assert not got["question"][q][:, int(cols["lengths"][q]):].astype(np.float32).any(), q
        assert got["question"][q][:, :int(cols["lengths"][q])].astype(np.float32).sum() > 0
        assert not got["kb"][q][:, int(cols["kb_lengths"][q]):].astype(np.float32).any(), q
    # instances(): one record per question, rows cut at the question's own sizes
    out = rec.instances([{"index": q} for q in filed[:3]], filed[:3], predictions=table)
    for q, record in zip(filed[:3], out):
        assert record["index"] == q and record["prediction"] == preds[q]
        assert [len(row) for row in record["attentions"]["question"]] == [int(cols["lengths"][q])] * p
        assert [len(row) for row in record["attentions"]["kb"]] == [int(cols["kb_lengths"][q])] * p
        assert record["attentions"]["kb"][p - 1] == got["kb"][q][p - 1, :int(cols["kb_lengths"][q])].astype(np.float64).tolist()
        if "self" in maps:
            assert [len(row) for row in record["attentions"]["self"]] == list(range(1, p + 1))
    # an id outside the store files nothing and still trips the store's check
    rec.clear()
    fwd.question_ids.copy_(torch.tensor([filed[0], filed[1], QN + 3, filed[2], -1, -1]))
    fwd.replay()
    poisoned = rec.read()
    for k in poisoned:
        rows = [q for q in range(QN) if not np.isnan(entries(k, poisoned[k][[q]])).all()]
        assert rows == filed[:3], k
        assert np.isfinite(entries(k, poisoned[k][filed[:3]])).all()
    with pytest.raises(ValueError, match="outside"):
        qs.check()


def test_without_records_the_launches_are_those_of_before(macx, dev):
    """the library calls of one forward: a class built with records=None makes none to macx_records_scatter, and records=rec adds
    exactly one, at the end"""
    net, feats, qs, p, N, maps = tower(macx, dev, "args", D_CAPTURED)
    rec = macx.EvalRecords(qs, p=p, N=N, S=S, answers=A, maps=maps)
    kw = dict(features=feats, questions=qs, score=True, kb_lengths=True, verify=False)
    plain = macx.CapturedTowerForward(net, B, S, predictions=qs.predictions(), **kw)
    filing = macx.CapturedTowerForward(net, B, S, predictions=qs.predictions(), records=rec, **kw)
    assert plain.records is None and filing.records is rec and plain.captured and filing.captured
    L, calls = macx._lib.lib(), []

    def wrap(name, fn):
        def call(*args):
            calls.append(name)
            return fn(*args)
        return call
    real = {n: getattr(L, n) for n in macx._lib.EXPORTS}
    try:
        for n, fn in real.items():
            setattr(L, n, wrap(n, fn))
        plain._eager()
        before, calls = calls, []
        filing._eager()
    finally:
        for n, fn in real.items():
            setattr(L, n, fn)
    torch.cuda.synchronize(dev)
    launches = lambda names: [n for n in names if not n.endswith("_floats") and n not in ("macx_saved_segment", "macx_check", "macx_cell_route")]
    assert "macx_records_scatter" not in before and "macx_preds_scatter" in before
    assert launches(calls) == launches(before) + ["macx_records_scatter"]
