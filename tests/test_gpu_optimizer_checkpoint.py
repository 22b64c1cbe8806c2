"""-m gpu: a checkpoint training continues from bit for bit -- checkpoint.save_npz(path, net, optimizer=opt) /
load_npz(path, net, optimizer=opt) on the small tower of tests/test_gpu_tower_graph.py, with eager steps (net, loss_and_pred, bucket,
opt.step) whose inputs and dropout seed are fixed per iteration.  Every comparison is an equality of bits."""
import numpy as np
import pytest
import torch

from abi_kit import bits_equal
from test_gpu_tower_graph import B, inputs, make_net

pytestmark = pytest.mark.gpu

SCALARS = ("step", "lr", "beta1", "beta2", "eps", "clip_norm", "ema_decay")


def trainer(macx, dev, seed, **opt_kw):
    net = make_net(macx, dev, seed=seed)
    bucket = macx.dp.TowerBuckets(net, fused_gather=True)
    return net, bucket, macx.optim.FlatAdamEMA(bucket.tensors(), **dict(dict(lr=1e-3), **opt_kw))


def train(net, bucket, opt, iterations):
    for it in iterations:
        images, q, lengths, answers = inputs(net.tensors()[0].device, 100 + it)
        for t in bucket.tensors():
            t.grad = None
        logits = net(images, q, lengths, train=True, seed=1000 + it, check_ids=False)
        loss, _ = net.loss_and_pred(logits, answers)
        bucket.begin_step(B, B)
        loss.backward()
        bucket.allreduce_(B, B)
        opt.step(flat_grad=bucket.flat)
    torch.cuda.synchronize()
    return loss.detach()


def state(opt):
    return dict(params=opt.flat, m=opt.m, v=opt.v, ema=opt.ema)


@pytest.fixture(scope="module")
def saved(macx, dev, tmp_path_factory):
    """two steps, the checkpoint, two more steps: (path, keys, the trainer, clones of its state X after step 4)"""
    path = str(tmp_path_factory.mktemp("ckpt") / "resume.npz")
    net, bucket, opt = trainer(macx, dev, seed=0)
    train(net, bucket, opt, (0, 1))
    keys = macx.checkpoint.save_npz(path, net, optimizer=opt)
    loss = train(net, bucket, opt, (2, 3))
    return path, keys, (net, bucket, opt), dict({k: v.clone() for k, v in state(opt).items()}, loss=loss.clone(), t=opt.t)


def test_training_continues_bit_for_bit(macx, dev, saved):
    path, _, _, X = saved
    net2, bucket2, opt2 = trainer(macx, dev, seed=9, lr=5e-2, beta1=0.5, clip_norm=1.0)      # other weights, other hyper-parameters
    assert not bits_equal(opt2.flat, X["params"])
    where = [p.data_ptr() for p in net2.tensors()]
    flat_at = opt2.flat.data_ptr()
    assert macx.checkpoint.load_npz(path, net2, optimizer=opt2) == []
    assert (opt2.t, opt2.lr, opt2.beta1, opt2.clip_norm) == (2, 1e-3, 0.9, 8.0)
    # in place: every parameter is the view of opt2.flat it was
    assert [p.data_ptr() for p in net2.tensors()] == where and opt2.flat.data_ptr() == flat_at
    for i, p in enumerate(opt2.params):
        assert p.data_ptr() == flat_at + 4 * opt2.offsets[i] and bits_equal(p.data, opt2.layout.view(opt2.flat, i))
    loss = train(net2, bucket2, opt2, (2, 3))
    assert opt2.t == X["t"] == 4 and bits_equal(loss, X["loss"])
    for name, t in state(opt2).items():
        assert bits_equal(t, X[name]), name


def test_the_file_holds_slots_and_scalars_under_reference_names(macx, dev, saved):
    path, keys, (net, _, opt), _ = saved
    with np.load(path) as z:
        files = set(z.files)
        assert files == set(keys)
        weights = set(macx.checkpoint.reference_state_dict(net))
        owned = sorted(k for k in weights if k[:-2] + "/Adam:0" in files)
        assert set(owned) == weights                                        # (this net has no tensor outside the optimizer)
        for k in owned:
            for suffix in ("/Adam:0", "/Adam_1:0", "/ExponentialMovingAverage:0"):
                assert k[:-2] + suffix in files and z[k[:-2] + suffix].shape == z[k].shape, (k, suffix)
        assert {"macx/optimizer/" + s for s in SCALARS} <= files and "macx/optimizer/guard" not in files
        assert int(z["macx/optimizer/step"]) == 2 and float(z["macx/optimizer/lr"]) == 1e-3
        assert files == weights | {k[:-2] + s for k in owned for s in ("/Adam:0", "/Adam_1:0", "/ExponentialMovingAverage:0")} \
            | {"macx/optimizer/" + s for s in SCALARS}


def test_a_file_with_slots_loads_as_plain_weights(macx, dev, saved):
    path, _, _, _ = saved
    net3 = make_net(macx, dev, seed=4)
    assert macx.checkpoint.load_npz(path, net3) == []
    with np.load(path) as z:
        for k, v in macx.checkpoint.reference_state_dict(net3).items():
            assert bits_equal(v.numpy(), z[k]), k
    net4 = make_net(macx, dev, seed=5)                                      # ... and its shadows, as before
    macx.checkpoint.load_npz(path, net4, use_ema=True)
    with np.load(path) as z:
        k = "macModel/" + next(iter(net4.cell.to_reference_dict())) + ":0"
        assert bits_equal(macx.checkpoint.reference_state_dict(net4)[k].numpy(), z[k[:-2] + "/ExponentialMovingAverage:0"])


def test_a_file_without_optimizer_state_is_a_key_error(macx, dev, saved, tmp_path):
    _, _, (net, _, opt), _ = saved
    bare = str(tmp_path / "weights.npz")
    macx.checkpoint.save_npz(bare, net)
    net2, _, opt2 = trainer(macx, dev, seed=9)
    before = [t.clone() for t in (opt2.flat, opt2.m, opt2.v, opt2.ema)]
    with pytest.raises(KeyError, match="optimizer"):
        macx.checkpoint.load_npz(bare, net2, optimizer=opt2)
    assert all(bits_equal(a, b) for a, b in zip(before, (opt2.flat, opt2.m, opt2.v, opt2.ema))) and opt2.t == 0     # nothing was changed
    with pytest.raises(ValueError, match="ema_tensors"):
        macx.checkpoint.save_npz(bare, net, ema_tensors=opt.ema_state(), optimizer=opt)
    other, _, _ = trainer(macx, dev, seed=3)
    with pytest.raises(ValueError, match="does not own"):                   # an optimizer over another net's tensors
        macx.checkpoint.save_npz(bare, other, optimizer=opt)


def test_guard_words_round_trip(macx, dev, tmp_path):
    path = str(tmp_path / "guarded.npz")
    net, bucket, opt = trainer(macx, dev, seed=0, guard=True)
    nan = torch.full_like(opt.flat, float("nan"))
    opt.step(flat_grad=nan)                                                 # attempt 1: skipped
    train(net, bucket, opt, (0,))                                           # attempt 2: applied
    opt.step(flat_grad=nan)                                                 # attempt 3: skipped
    assert opt.guard_counts() == (1, 2, 1, 3) and opt.t == 3
    keys = macx.checkpoint.save_npz(path, net, optimizer=opt)
    assert "macx/optimizer/guard" in keys
    with np.load(path) as z:
        assert z["macx/optimizer/guard"].tolist() == [1, 2, 1, 3]
    net2, _, opt2 = trainer(macx, dev, seed=9, guard=True)
    macx.checkpoint.load_npz(path, net2, optimizer=opt2)
    assert opt2.guard_counts() == (1, 2, 1, 3) and opt2.t == 3
    assert all(bits_equal(a, b) for a, b in zip((opt.flat, opt.m, opt.v, opt.ema), (opt2.flat, opt2.m, opt2.v, opt2.ema)))
    net3, _, opt3 = trainer(macx, dev, seed=2)                              # an unguarded optimizer takes the file and ignores the words
    macx.checkpoint.load_npz(path, net3, optimizer=opt3)
    assert opt3.guard is None and opt3.t == 3 and bits_equal(opt3.m, opt.m)
    # ... while a guarded optimizer needs them
    bare = str(tmp_path / "unguarded.npz")
    macx.checkpoint.save_npz(bare, net3, optimizer=opt3)
    with pytest.raises(KeyError, match="guard"):
        macx.checkpoint.load_npz(bare, net2, optimizer=opt2)
