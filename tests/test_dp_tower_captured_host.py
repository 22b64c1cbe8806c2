"""The host side of macx.CapturedDPTowerTrainStep -- the whole tower's data-parallel step replayed between its collectives -- and of
the bucket mode it stands on, TowerBuckets(exchange=False): the export, the signature, what the constructor refuses and in which
words, and a phase-1 hook that never starts a collective.  No GPU: the refusals are raised before anything is allocated."""
import inspect
import types

import pytest
import torch

from test_tower_graph_host import small_net

ARGS = dict(B=2, S=7, H=5, W=5, imageInDim=128, global_batch=5, b0=0)


def test_the_class_is_exported_and_is_a_tower_exchange_step(macx):
    cls = macx.CapturedDPTowerTrainStep
    assert cls is macx.graph.CapturedDPTowerTrainStep
    assert issubclass(cls, macx.dp.TowerExchangeStep)
    assert cls.__bases__ == (macx.graph._Captured, macx.graph._TowerInputs, macx.graph._MaskWord, macx.dp.TowerExchangeStep)
    assert not issubclass(cls, macx.CapturedTowerTrainStep)
    # the parts are this class's own, the sequence and its collectives are TowerExchangeStep's, untouched
    assert cls.exchange_step is macx.dp.TowerExchangeStep.exchange_step and cls.factor is macx.dp.TowerExchangeStep.factor
    for part in ("run_part_q", "run_part_a", "run_part_b"):
        assert getattr(cls, part) is not getattr(macx.dp.TowerExchangeStep, part)
    assert callable(cls.load_dead) and callable(cls.step)


def test_signature_and_defaults(macx):
    sig = inspect.signature(macx.CapturedDPTowerTrainStep.__init__).parameters
    assert list(sig)[1:9] == ["net", "opt", "bucket", "B", "S", "H", "W", "imageInDim"]
    want = dict(H=14, W=14, imageInDim=1024, global_batch=None, b0=0, group=None, seed=0, warmup=2, capture=True, verify=True, check_every=0,
                images=None, kb_lengths=False, image_lengths=False, att_loss=None, aux_loss=None, weights=False, totals=None, features=None,
                questions=None)
    assert {k: sig[k].default for k in want} == want
    assert inspect.signature(macx.CapturedDPTowerTrainStep.step).parameters["iteration"].default is None
    # the one-process class is what it was
    assert "global_batch" not in inspect.signature(macx.CapturedTowerTrainStep.__init__).parameters
    sig = inspect.signature(macx.dp.TowerBuckets.__init__).parameters
    assert list(sig)[1:] == ["net", "group", "fused_gather", "exchange"] and sig["exchange"].default is True
    assert list(inspect.signature(macx.dp.TowerBuckets.gather_).parameters)[1:] == ["shard_size", "global_size"]


@pytest.mark.parametrize("kw, words", [(dict(att_loss=dict(on="kb", kind="entropy")), "no att_loss.*normalised by p \\* B"),
                                       (dict(aux_loss=lambda cell, state: state.memory.sum()), "no aux_loss.*normalised by p \\* B"),
                                       (dict(questions=object()), "no questions= store.*in front of")])
def test_out_of_scope_arguments_are_refused_by_name(macx, kw, words):
    """before the device is asked for: the message names the reason on any box"""
    with pytest.raises(ValueError, match=words):
        macx.CapturedDPTowerTrainStep(small_net(macx), None, None, **ARGS, **kw)


def test_construction_needs_the_device_as_the_one_process_step_does(macx):
    net = small_net(macx)
    with pytest.raises(RuntimeError, match="HIP device") as mine:
        macx.CapturedDPTowerTrainStep(net, None, None, **ARGS)
    with pytest.raises(RuntimeError, match="HIP device") as theirs:
        macx.CapturedTowerTrainStep(net, None, None, 2, 7, H=5, W=5, imageInDim=128)
    assert str(mine.value).replace("CapturedDPTowerTrainStep", "CapturedTowerTrainStep") == str(theirs.value)
    generic = small_net(macx, encBi=False)
    with pytest.raises(macx.UnsupportedOptions, match="net.enc"):
        macx.CapturedDPTowerTrainStep(generic, None, None, **ARGS)
    with pytest.raises(ValueError, match=r"\[4, 6\) of a global batch of 5"):
        macx.CapturedDPTowerTrainStep(net, None, None, **dict(ARGS, b0=4))
    with pytest.raises(ValueError, match="totals= belongs to the weighted answer loss"):
        macx.CapturedDPTowerTrainStep(net, None, None, totals=True, **ARGS)


def test_bucket_and_optimizer_are_checked(macx, monkeypatch):
    """(the checks sit behind the device's: here the device check is stood in for, and every refusal is raised before an allocation)"""
    monkeypatch.setattr(macx.graph, "_require_hip", lambda dev, who, what: dev)
    net, other = small_net(macx), small_net(macx)

    def fused(**kw):                              # (the spare tables of fused_gather=True are device memory: flagged after construction)
        bucket = macx.dp.TowerBuckets(net, **kw)
        bucket.fused_gather = True
        return bucket
    exchanging = fused()
    assert exchanging.exchange is True
    own = types.SimpleNamespace(params=exchanging.tensors(), flat=torch.zeros(exchanging.flat.numel()))
    with pytest.raises(ValueError, match="exchange=False.*inside part A"):
        macx.CapturedDPTowerTrainStep(net, own, exchanging, **ARGS)
    with pytest.raises(ValueError, match="fused_gather=True"):
        macx.CapturedDPTowerTrainStep(net, own, macx.dp.TowerBuckets(net, exchange=False), **ARGS)
    bucket = fused(exchange=False)
    assert bucket.exchange is False
    with pytest.raises(ValueError, match="another net"):
        macx.CapturedDPTowerTrainStep(other, own, bucket, **ARGS)
    foreign = types.SimpleNamespace(params=list(net.tensors()), flat=torch.zeros(bucket.flat.numel()))       # the net's order, not the bucket's
    assert any(a is not b for a, b in zip(foreign.params, bucket.tensors()))
    with pytest.raises(ValueError, match="built over bucket.tensors"):
        macx.CapturedDPTowerTrainStep(net, foreign, bucket, **ARGS)
    short = types.SimpleNamespace(params=bucket.tensors(), flat=torch.zeros(bucket.flat.numel() - 4))
    with pytest.raises(ValueError, match="built over bucket.tensors"):
        macx.CapturedDPTowerTrainStep(net, short, bucket, **ARGS)


def test_a_bucket_that_does_not_exchange_starts_no_collective_from_the_hook(macx, monkeypatch):
    calls = []
    monkeypatch.setattr(macx.dp, "_world", lambda group: 2)                    # a faked world above 1
    monkeypatch.setattr(macx.dp.dist, "all_reduce", lambda *a, **kw: calls.append("all_reduce"))
    net = small_net(macx)
    bucket = macx.dp.TowerBuckets(net, exchange=False)
    assert bucket._active() and net.cell.after_backward_phase1 == bucket._phase1
    for t in bucket.tensors():
        t.grad = torch.ones_like(t)
    bucket.begin_step(2, 5)
    bucket._phase1(bucket.flat[bucket.cell_lo:bucket.cell_hi])               # the buffer the cell's backward pass hands its hook
    assert calls == [] and not bucket._early_started
    # ... and gather_ is the rest of allreduce_ without one: gather, flat *= shard / global, .grad published as views of flat
    flat = bucket.gather_(2, 5)
    assert calls == [] and flat is bucket.flat
    for i, t in enumerate(bucket.tensors()):
        assert t.grad.data_ptr() == flat.data_ptr() + 4 * bucket.offsets[i]
        assert torch.equal(t.grad, torch.full_like(t, 2.0 / 5.0))
    # the default bucket is what it was: the same hook call starts the early exchange, and gather_ is not its method
    net2 = small_net(macx)
    exchanging = macx.dp.TowerBuckets(net2)
    monkeypatch.setattr(exchanging, "_start_early", lambda: calls.append("early"))
    for t in exchanging.tensors():
        t.grad = torch.ones_like(t)
    exchanging.begin_step(2, 5)
    exchanging._phase1(exchanging.flat[exchanging.cell_lo:exchanging.cell_hi])
    assert calls == ["early"]
    with pytest.raises(RuntimeError, match="exchange=False"):
        exchanging.gather_(2, 5)


def test_nothing_was_added_to_the_library(macx):
    """(restates the pin of test_dp_tower_graph_host.py: the step replays existing launches, so a stray export fails HERE, by name)"""
    assert len(macx._lib.EXPORTS) == 109, "CapturedDPTowerTrainStep adds no kernel and no export: %d" % len(macx._lib.EXPORTS)
    assert macx._lib.ABI_VERSION == 5 and macx._lib.lib().macx_abi_version() == 5
