"""The host side of the attention loss (macx_att_loss, macx.losses, att_loss= / aux_loss= on the captured training steps): the fp64
reference the GPU tests compare with is held to autograd of its own loss, and every refusal that is raised before anything asks
for the device -- with the never-constructed instances tests/test_lengths_paths_host.py uses.  No GPU."""
import inspect

import pytest
import torch

import att_loss_ref as ar
from test_lengths_paths_host import bare, tower_inputs

B, S, N, P = 6, 7, 25, 3
TRAIN_CLASSES = ("CapturedTrainStep", "CapturedDPTrainStep", "CapturedTowerTrainStep")


@pytest.mark.parametrize("kind", ["ce", "entropy"])
@pytest.mark.parametrize("per_step", [False, True])
def test_reference_gradient_is_autograd_of_its_loss(kind, per_step):
    p, b, n = 3, 5, 17
    lengths = torch.tensor([17, 1, 9, 0, 30])                            # 0 and 30: the clamp to [1, n]
    att, target = ar.draw(p, b, n, lengths, seed=3, nan=True)
    g = torch.Generator().manual_seed(4)
    sw, rw = 0.5 + torch.rand(p, generator=g), 0.5 + torch.rand(b, generator=g)
    rw[2] = 0.0
    kw = dict(target=(target if per_step else target[0]) if kind == "ce" else None, lengths=lengths, step_weights=sw, row_weights=rw,
              kind=kind, eps=1e-8, scale=0.37)
    a = att.to(torch.float64).requires_grad_(True)
    rows = ar.rows(a, **kw)
    assert bool(torch.isfinite(rows).all())                              # the NaN behind the lengths reached nothing
    rows.sum().backward()
    closed = ar.d_att(att, **kw)
    assert bool(torch.isfinite(a.grad).all()) and bool(torch.isfinite(closed).all())
    assert float((a.grad - closed).abs().max()) <= 1e-12 * max(1.0, float(closed.abs().max()))
    dead = ~ar.live_mask(lengths, b, n)
    assert int(dead.sum()) == (0 + 16 + 8 + 16 + 0)
    for t in (a.grad, closed):
        assert bool((t[:, dead] == 0).all()) and bool((t[:, 2] == 0).all())           # masked cells and the unsupervised question: exactly 0
    rows = rows.detach()
    assert float(rows[:, 2].abs().max()) == 0.0 and float(rows[:, 0].abs().min()) > 0
    assert bool((ar.abs_term_sums(att, **kw) >= rows.abs()).all())


def test_export_is_bound_and_keywords_default_to_off(macx):
    assert "macx_att_loss" in macx._lib.EXPORTS and macx._lib.ABI_VERSION == 5
    order = list(macx._lib.TABLE)
    assert order.index("macx_att_loss") == order.index("macx_answer_loss") + 1            # the header's position
    assert macx._lib.ATT_LOSS_KINDS == {"ce": 0, "entropy": 1}
    for name in TRAIN_CLASSES:
        sig = inspect.signature(getattr(macx, name).__init__).parameters
        assert sig["att_loss"].default is None and sig["aux_loss"].default is None, name
        load = inspect.signature(getattr(macx, name).load).parameters
        assert all(load[k].default is None for k in ("att_target", "att_row_weights", "att_step_weights")), name
    assert hasattr(macx.MACCell, "state_tensor") and hasattr(macx.cell.PaddedMACCell, "state_tensor")


def test_attention_loss_has_no_cpu_path(macx):
    att, target = ar.draw(2, 3, 5, None, seed=1, nan=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        macx.losses.attention_loss(att, target)
    with pytest.raises(RuntimeError, match="no CPU path"):
        macx.losses.attention_loss(att, kind="entropy")
    # what is refused before the device is asked for
    with pytest.raises(ValueError, match="eps"):
        macx.losses.attention_loss(att, target, eps=0.0)
    with pytest.raises(ValueError, match="eps"):
        macx.losses.attention_loss(att, target, eps=float("inf"))
    with pytest.raises(ValueError, match="kind"):
        macx.losses.attention_loss(att, target, kind="kl")


@pytest.mark.parametrize("name", TRAIN_CLASSES)
@pytest.mark.parametrize("spec,error,match", [
    (3, TypeError, "dict"),
    ({"on": "self"}, ValueError, "aux_loss"),
    ({"kind": "kl"}, ValueError, "kind"),
    ({"eps": 0.0}, ValueError, "eps"),
    ({"eps": -1e-8}, ValueError, "eps"),
    ({"weight": float("nan")}, ValueError, "scale|weight"),
    ({"lam": 0.1}, ValueError, "lam"),
    ({"kind": "entropy", "per_step_target": True}, ValueError, "per_step_target"),
])
def test_att_loss_dict_is_validated_before_the_device(macx, name, spec, error, match):
    cls = getattr(macx, name)
    with pytest.raises(error, match=match):
        if name == "CapturedTowerTrainStep":
            from test_tower_graph_host import small_net
            cls(small_net(macx), None, None, B, S, H=5, W=5, imageInDim=128, att_loss=spec)
        elif name == "CapturedDPTrainStep":
            cls(None, None, None, B, S, N, global_batch=2 * B, att_loss=spec)
        else:
            cls(None, None, B, S, N, att_loss=spec)


def test_dp_step_refuses_aux_loss_and_names_att_loss(macx):
    with pytest.raises(TypeError, match="att_loss="):
        macx.CapturedDPTrainStep(None, None, None, B, S, N, global_batch=2 * B, aux_loss=lambda cell, state: state.memory.sum())


def _cell_args(name):
    x = [torch.zeros(B, 128), torch.zeros(B, S, 128), torch.full((B,), S, dtype=torch.int32), torch.zeros(B, N, 128)]
    return x, ({} if name == "CapturedForward" else {"d_memory": torch.zeros(B, 128)})


def _call_load(macx, name, attrs, **kw):
    if name.startswith("CapturedTower"):
        images, q, lengths = tower_inputs()
        x = (images, q, lengths) + ((torch.zeros(B, dtype=torch.int32),) if name == "CapturedTowerTrainStep" else ())
        return bare(macx, name, B=B, S=S, G=None, N=N, **attrs).load(*x, **kw)
    x, train = _cell_args(name)
    return bare(macx, name, **dict(train, **attrs)).load(*x, **dict(train, **kw))


@pytest.mark.parametrize("name", TRAIN_CLASSES)
def test_load_takes_att_target_exactly_when_built_for_ce(macx, name):
    target, rw, sw = torch.zeros(B, N), torch.ones(B), torch.ones(P)
    spec = dict(on="kb", kind="ce")
    # built without att_loss: every one of the three is refused
    with pytest.raises(TypeError, match="no att_target"):
        _call_load(macx, name, {}, att_target=target)
    with pytest.raises(TypeError, match="no att_row_weights"):
        _call_load(macx, name, {}, att_row_weights=rw)
    with pytest.raises(TypeError, match="no att_step_weights"):
        _call_load(macx, name, {}, att_step_weights=sw)
    # built for ce: the target is required
    built = dict(att_loss=spec, att_target=target.clone(), att_row_weights=rw.clone(), att_step_weights=sw.clone())
    with pytest.raises(TypeError, match="needs att_target"):
        _call_load(macx, name, built)
    # built for entropy: there is no target to load
    entropy = dict(att_loss=dict(on="kb", kind="entropy"), att_row_weights=rw.clone(), att_step_weights=sw.clone())
    with pytest.raises(TypeError, match="no att_target"):
        _call_load(macx, name, entropy, att_target=target)
    # shapes and dtypes
    for kw in (dict(att_target=torch.zeros(B, N + 1)), dict(att_target=torch.zeros(P, B, N)), dict(att_target=torch.zeros(B, N, dtype=torch.int32)),
               dict(att_target=target, att_row_weights=torch.ones(B + 1)), dict(att_target=target, att_step_weights=torch.ones(P, 1))):
        with pytest.raises(ValueError, match="att_"):
            _call_load(macx, name, built, **kw)


def test_forward_classes_take_none_of_it(macx):
    with pytest.raises(TypeError, match="no att_target"):
        _call_load(macx, "CapturedForward", {}, att_target=torch.zeros(B, N))
    assert "att_target" not in inspect.signature(macx.CapturedTowerForward.load).parameters
