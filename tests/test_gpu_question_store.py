"""-m gpu: questions resident in device memory on the tower.  macx.QuestionStore's eager gather against indexing on the host, and the
captured classes built with questions=: every comparison is an equality of bits with a twin class built WITHOUT questions= that is
given the same batch through load() -- host-sliced questions, lengths, answers, weights and image rows.

The tower is tests/test_gpu_feature_store.py's (B 3, H 4, W 3, C 128, d 256, p 2, S 6, 7 answers, vocabulary 12, 5 images); the store
holds 8 questions of 5 words (one padded column), their answers, image rows and weights."""
import pytest
import torch

from abi_kit import bits_equal
from test_gpu_feature_store import A, B, S, V, make_net, make_store

pytestmark = pytest.mark.gpu

QN, S_TAB = 8, 5
ROWS = [4, 1, 4, 0, 2, 3, 1, 4]                     # the image of each question: ids [0, 1, 2] look at rows [4, 1, 4]
PERM = [5, 2, 7, 0, 1, 6, 4, 3]


def host_columns():
    g = torch.Generator().manual_seed(11)
    lengths = torch.tensor([5, 2, 4, 1, 3, 5, 2, 4], dtype=torch.int32)
    q = torch.randint(1, V + 1, (QN, S_TAB), generator=g, dtype=torch.int32) * (torch.arange(S_TAB)[None] < lengths[:, None]).to(torch.int32)
    return dict(questions=q, lengths=lengths, answers=torch.randint(0, A, (QN,), generator=g, dtype=torch.int32),
                image_rows=torch.tensor(ROWS, dtype=torch.int32), weights=torch.tensor([1.0, 0.5, 2.0, 1.0, 0.25, 1.0, 1.5, 1.0]))


def make_questions(macx, dev):
    return macx.QuestionStore(device=dev, **host_columns())


def sliced(dev, ids):
    """the batch `ids` names, sliced on the host and padded to S columns: what load() takes"""
    c, ids = host_columns(), torch.as_tensor(ids).long()
    q = torch.cat([c["questions"], torch.zeros(QN, S - S_TAB, dtype=torch.int32)], 1)
    return {k: v.to(dev) for k, v in dict(questions=q[ids], lengths=c["lengths"][ids], answers=c["answers"][ids], rows=c["image_rows"][ids],
                                          weights=c["weights"][ids]).items()}


def captured(obj):
    assert obj.captured, "the capture's self-check failed in this process: %r" % (obj.verify_report,)
    return obj


def test_eager_gather_is_indexing_and_feeds_the_net(macx, dev):
    net, feats, qs = make_net(macx, dev), make_store(macx, dev), make_questions(macx, dev)
    assert (qs.count, qs.S, qs.max_word <= V, qs.max_answer < A) == (QN, S_TAB, True, True) and qs.nbytes == QN * S_TAB * 4 + 4 * QN * 4
    for ids in ([7, 0, 7], [1, 2, 3], [6]):
        want = sliced(dev, ids)
        got = qs.gather(torch.tensor(ids, device=dev), S=S)
        assert got.kb_lengths is None and got.image_index is None
        for a, b in ((got.questions, want["questions"]), (got.lengths, want["lengths"]), (got.answers, want["answers"]),
                     (got.image_ids, want["rows"]), (got.weights, want["weights"])):
            assert bits_equal(a, b), ids
        narrow = qs.gather(torch.tensor(ids, dtype=torch.int32, device=dev))                 # S defaults to the store's
        assert bits_equal(narrow.questions, want["questions"][:, :S_TAB])
        if len(ids) == B:
            with torch.no_grad():
                a = net(feats, got.questions, got.lengths, image_ids=got.image_ids)
                b = net(feats, want["questions"], want["lengths"], image_ids=want["rows"])
            assert bits_equal(a, b)
    grouped = qs.gather(torch.tensor([0, 1, 2, -1], device=dev), S=S, images=3)
    assert grouped.image_ids.tolist() == [4, 1, 4] and grouped.image_index.tolist() == [0, 1, 0, 0] and grouped.weights.tolist() == [1.0, 0.5, 2.0, 0.0]
    assert qs.check() is qs
    qs.gather(torch.tensor([0, QN], device=dev))
    with pytest.raises(ValueError, match="outside"):
        qs.check()
    table = qs.predictions()
    qs.scatter_predictions(table, torch.tensor([3, 4, 5], dtype=torch.int32, device=dev), torch.tensor([6, -1, 2], dtype=torch.int32, device=dev))
    assert table.tolist() == [-1, -1, 5, -1, -1, -1, 3, -1]


def test_forward_class_follows_ids(macx, dev):
    net, feats, qs = make_net(macx, dev), make_store(macx, dev), make_questions(macx, dev)
    table = qs.predictions()
    fwd = captured(macx.CapturedTowerForward(net, B, S, features=feats, questions=qs, predictions=table))
    twin = captured(macx.CapturedTowerForward(net, B, S, features=feats))
    assert fwd.question_ids.tolist() == [-1] * B and fwd.question_ids.dtype == torch.int32 and int(qs.bad) == 0
    assert bool((table == -1).all())                                        # the self-check's predictions are gone

    def reference(ids):
        w = sliced(dev, ids)
        return twin(None, w["questions"], w["lengths"], image_ids=w["rows"]).clone(), twin.pred.clone()
    for ids in ([7, 0, 7], [1, 2, 3]):
        assert fwd.load_ids(torch.tensor(ids, device=dev)) == B
        logits, pred = reference(ids)
        assert bits_equal(fwd.replay(), logits) and torch.equal(fwd.pred, pred)
    fwd.question_ids.copy_(torch.tensor([5, 5, 6]))                         # one graph follows ids written between replays
    logits, pred556 = reference([5, 5, 6])
    assert bits_equal(fwd.replay(), logits)
    # the table: every batch's predictions placed by id, the other entries as they were
    want = torch.full((QN,), -1, dtype=torch.int32)
    for ids in ([7, 0, 7], [1, 2, 3], [5, 5, 6]):
        want[torch.tensor(ids)] = reference(ids)[1].cpu()
    assert table.cpu().tolist() == want.tolist() and want[4] == -1
    with pytest.raises(ValueError, match="load_ids"):
        w = sliced(dev, [0, 1, 2])
        fwd.load(None, w["questions"], w["lengths"], image_ids=w["rows"])
    with pytest.raises(IndexError, match=r"outside \[0, 8\)"):
        fwd.load_ids(torch.tensor([0, QN, 1], device=dev))
    with pytest.raises(ValueError, match="got 2"):                          # no weights: full batches only
        fwd.load_ids(torch.tensor([0, 1], device=dev))
    assert qs.check() is qs


def train_pair(macx, dev, **kw):
    """(step built with questions=, its twin without, the store) on two nets of the same parameters"""
    feats, qs = make_store(macx, dev), make_questions(macx, dev)
    out = []
    for questions in (qs, None):
        net = make_net(macx, dev, **({"stemDropout": 1.0} if "images" in kw else {}))
        bucket = macx.dp.TowerBuckets(net, fused_gather=True)
        opt = macx.optim.FlatAdamEMA(bucket.tensors(), lr=1e-3)
        out.append(captured(macx.CapturedTowerTrainStep(net, opt, bucket, B, S, seed=1234, features=feats, weights=True, totals=True,
                                                        questions=questions, **kw)))
    assert bits_equal(out[0].opt.flat, out[1].opt.flat)
    return out[0], out[1], qs


def written(step):
    return {"loss": step.loss, "logits": step.logits, "pred": step.pred, "norm": step.norm, "flat gradient": step.bucket.flat,
            "flat parameters": step.opt.flat, "totals": step.totals.tensor}


def assert_same_step(step, twin, what):
    torch.cuda.synchronize()
    a, b = written(step), written(twin)
    for name in a:
        assert bits_equal(a[name].reshape(-1), b[name].reshape(-1)), (what, name)


def test_training_class_trains_as_the_load_route(macx, dev):
    step, twin, qs = train_pair(macx, dev)
    assert step.question_ids.tolist() == [-1] * B and int(qs.bad) == 0 and step.totals.read()["weight"] == 0
    for it, ids in enumerate(([7, 0, 7], [1, 2, 3])):
        assert step.load_ids(torch.tensor(ids, device=dev)) == B
        step.replay(iteration=it)
        w = sliced(dev, ids)
        assert twin.load(None, w["questions"], w["lengths"], w["answers"], image_ids=w["rows"], weights=w["weights"]) == B
        twin.replay(iteration=it)
        assert_same_step(step, twin, ids)
    # a short batch: the same bits whatever stale id sat in the dead slot, and the bits of the twin's short load()
    state, tstate, results = step._state(), twin._state(), []
    w = sliced(dev, [5, 1])
    for stale in (3, 0, 7):
        step._restore(state)
        step.totals.reset()
        step.question_ids.fill_(stale)
        assert step.load_ids(torch.tensor([5, 1], device=dev)) == 2 and step.n == 2
        assert step.question_ids.tolist() == [5, 1, -1]
        step.replay(iteration=7)
        assert step.weights.tolist() == [1.0, 0.5, 0.0] and step.pred[2].item() == -1
        results.append({k: v.clone() for k, v in written(step).items()})
    for other in results[1:]:
        assert all(bits_equal(results[0][k][:2] if k in ("logits", "pred") else results[0][k], other[k][:2] if k in ("logits", "pred") else other[k])
                   for k in other)
    twin._restore(tstate)
    twin.totals.reset()
    assert twin.load(None, w["questions"], w["lengths"], w["answers"], image_ids=w["rows"], weights=w["weights"]) == 2
    twin.replay(iteration=7)
    assert_same_step(step, twin, "short batch")
    assert not bits_equal(step.opt.flat, state[0][0])                       # (the step trained)
    assert qs.check() is qs


def test_shared_images_are_grouped_on_the_device(macx, dev):
    """ids whose rows are [4, 1, 4]: the twin is loaded with the two distinct rows and the index the host would build"""
    ids = [0, 1, 2]
    w = sliced(dev, ids)
    assert w["rows"].tolist() == [4, 1, 4]
    rows, index = torch.tensor([4, 1], device=dev), torch.tensor([0, 1, 0], dtype=torch.int32, device=dev)
    net, feats, qs = make_net(macx, dev), make_store(macx, dev), make_questions(macx, dev)
    fwd = captured(macx.CapturedTowerForward(net, B, S, features=feats, images=2, questions=qs))
    twin = captured(macx.CapturedTowerForward(net, B, S, features=feats, images=2))
    fwd.load_ids(torch.tensor(ids, device=dev))
    assert bits_equal(fwd.replay(), twin(None, w["questions"], w["lengths"], image_ids=rows, image_index=index))
    assert fwd.image_ids.tolist() == [4, 1] and fwd.image_index.tolist() == [0, 1, 0]
    fwd.load_ids(torch.tensor([6, 6, 1], device=dev))                      # one distinct row: the second image slot copies the first
    w1 = sliced(dev, [6, 6, 1])
    assert bits_equal(fwd.replay(), twin(None, w1["questions"], w1["lengths"], image_ids=torch.tensor([1, 1], device=dev),
                                         image_index=torch.zeros(B, dtype=torch.int32, device=dev)))
    assert fwd.image_ids.tolist() == [1, 1] and fwd.image_index.tolist() == [0, 0, 0] and qs.check() is qs
    step, ttwin, tqs = train_pair(macx, dev, images=2)
    for it in range(2):
        step.load_ids(torch.tensor(ids, device=dev))
        step.replay(iteration=it)
        ttwin.load(None, w["questions"], w["lengths"], w["answers"], image_ids=rows, image_index=index, weights=w["weights"])
        ttwin.replay(iteration=it)
        assert_same_step(step, ttwin, it)
    assert tqs.check() is tqs


def test_an_epoch_is_a_loop_of_replays(macx, dev):
    net, feats, qs = make_net(macx, dev), make_store(macx, dev), make_questions(macx, dev)
    table = qs.predictions()
    fwd = captured(macx.CapturedTowerForward(net, B, S, features=feats, questions=qs, score=True, predictions=table))
    twin = captured(macx.CapturedTowerForward(net, B, S, features=feats, score=True))
    order = macx.EpochOrder(qs, B, order=torch.tensor(PERM))
    assert order.steps == 3 and fwd.totals.read()["weight"] == 0
    want, sizes = torch.full((QN,), -1, dtype=torch.int32), []
    for k in range(order.steps):
        ids = PERM[k * B:(k + 1) * B]
        n = fwd.next_batch(order)
        sizes.append(n)
        assert fwd.question_ids.tolist() == ids + [-1] * (B - n)
        logits = fwd.replay()
        w = sliced(dev, ids)
        ref = twin(None, w["questions"], w["lengths"], image_ids=w["rows"], answers=w["answers"], weights=w["weights"])
        assert tuple(logits.shape) == (n, A) and bits_equal(logits, ref) and bits_equal(fwd.loss, twin.loss)
        assert torch.equal(fwd.pred, twin.pred)
        want[torch.tensor(ids)] = twin.pred[:n].cpu()
    assert sizes == [3, 3, 2]
    assert bits_equal(fwd.totals.tensor, twin.totals.tensor) and fwd.totals.read()["weight"] == pytest.approx(8.25)
    assert table.cpu().tolist() == want.tolist() and bool((want >= 0).all())
    with pytest.raises(IndexError, match="exhausted"):
        fwd.next_batch(order)
    assert qs.check() is qs
    order.rewind()                                                          # a second epoch in the store's own order
    assert fwd.next_batch(order) == B and fwd.question_ids.tolist() == [0, 1, 2]


def test_an_id_outside_the_store_poisons_its_question(macx, dev):
    net, feats, qs = make_net(macx, dev), make_store(macx, dev), make_questions(macx, dev)
    fwd = captured(macx.CapturedTowerForward(net, B, S, features=feats, questions=qs, score=True))
    fwd.load_ids(torch.tensor([3, 5, 2], device=dev))
    clean = fwd.replay().clone()
    assert bool(torch.isfinite(clean).all()) and bool(torch.isfinite(fwd.loss)) and qs.check() is qs
    fwd.totals.reset()
    fwd.question_ids.copy_(torch.tensor([3, QN, 2]))
    logits = fwd.replay()
    assert bool(torch.isnan(logits[1]).all()) and bool(torch.isnan(fwd.loss))
    assert bits_equal(logits[[0, 2]], clean[[0, 2]])                        # the other questions are exact
    assert fwd.totals.read()["loss"] != fwd.totals.read()["loss"]           # NaN totals: the epoch's score cannot hide it
    with pytest.raises(ValueError, match="outside"):
        qs.check()
