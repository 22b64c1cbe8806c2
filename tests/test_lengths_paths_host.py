"""The host side of knowledge-base sizes on the captured paths and of sizes per shared image (macx_kb_gather_l / macx_kb_gather_bwd_l,
macx_read_fwd_l, `image_lengths=` on stem.kb_gather / MACNetCore / MACNet, `kb_lengths=` / `image_lengths=` / `images=` on the
captured classes): the exports, the keywords that default to the behaviour of before, and the refusals, which are raised before
anything asks for the device.  No GPU."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from test_tower_graph_host import small_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, G, N = 6, 7, 3, 25
NEW = ("macx_kb_gather_l", "macx_kb_gather_bwd_l", "macx_read_fwd_l")
CELL_CLASSES = ("CapturedForward", "CapturedTrainStep", "CapturedDPTrainStep")
TOWER_CLASSES = ("CapturedTowerForward", "CapturedTowerTrainStep")


def tower_inputs():
    return torch.zeros(G, N, 128), torch.ones(B, S, dtype=torch.int32), torch.full((B,), S, dtype=torch.int32)


INDEX = torch.tensor([1, 1, 0, 2, 0, 1], dtype=torch.int32)
SIZES = torch.tensor([25, 1, 9], dtype=torch.int32)


def test_new_symbols_are_declared_and_exported_with_signatures(macx):
    L = macx._lib.lib()
    header = open(os.path.join(ROOT, "include", "macx.h")).read()
    declared = set(re.findall(r"\b(macx_[a-z_0-9]+)\s*\(", header))
    for n in NEW:
        assert n in declared and n in macx._lib.EXPORTS and hasattr(L, n), n
        assert getattr(L, n).restype is C.c_int, n
    # the plain gather plus the lengths behind the index (and, forward, the per-question lengths in front of the stream)
    plain = list(L.macx_kb_gather.argtypes)
    assert list(L.macx_kb_gather_l.argtypes) == plain[:2] + [C.c_void_p] + plain[2:-1] + [C.c_void_p, plain[-1]]
    assert list(L.macx_kb_gather_bwd_l.argtypes) == plain[:2] + [C.c_void_p] + plain[2:]
    # macx_read_fwd plus kb_lengths behind the knowledge base
    plain = list(L.macx_read_fwd.argtypes)
    assert list(L.macx_read_fwd_l.argtypes) == plain[:5] + [C.c_void_p] + plain[5:]
    assert macx._lib.ABI_VERSION == 5 and L.macx_abi_version() == 5


def test_new_keywords_default_to_off(macx):
    for cls in (macx.MACNetCore, macx.MACNet):
        assert inspect.signature(cls.forward).parameters["image_lengths"].default is None, cls
    assert inspect.signature(macx.stem.kb_gather).parameters["image_lengths"].default is None
    for name in CELL_CLASSES + TOWER_CLASSES:
        assert inspect.signature(getattr(macx, name).__init__).parameters["kb_lengths"].default is False, name
        assert inspect.signature(getattr(macx, name).load).parameters["kb_lengths"].default is None, name
    for name in TOWER_CLASSES:
        assert inspect.signature(getattr(macx, name).__init__).parameters["image_lengths"].default is False, name
        assert inspect.signature(getattr(macx, name).load).parameters["image_lengths"].default is None, name
    assert inspect.signature(macx.CapturedTowerTrainStep.__init__).parameters["images"].default is None
    assert inspect.signature(macx.CapturedTowerTrainStep.load).parameters["image_index"].default is None


def test_image_lengths_need_image_index_and_exclude_kb_lengths(macx):
    net = small_net(macx)
    images, q, lengths = tower_inputs()
    core = lambda **kw: macx.MACNetCore.forward(net, images, torch.zeros(B, 256), torch.zeros(B, S, 256), lengths, **kw)
    for call in (lambda **kw: net(images, q, lengths, **kw), core):
        with pytest.raises(ValueError, match="image_index"):
            call(image_lengths=SIZES)
        with pytest.raises(ValueError, match="kb_lengths"):
            call(image_index=INDEX, image_lengths=SIZES, kb_lengths=torch.full((B,), 5, dtype=torch.int32))
        # valid arguments pass the validation: what stops them here is the missing device
        with pytest.raises(RuntimeError, match="no CPU path|HIP device"):
            call(image_index=INDEX, image_lengths=SIZES)


@pytest.mark.parametrize("bad", ["too short", "per question", "two axes", "float", "bool", "list"])
def test_image_lengths_shape_and_dtype_are_refused_on_the_host(macx, bad):
    net = small_net(macx)
    images, q, lengths = tower_inputs()
    sizes = {"too short": torch.ones(G - 1, dtype=torch.int32), "per question": torch.ones(B, dtype=torch.int32),
             "two axes": torch.ones(G, 1, dtype=torch.int64), "float": torch.ones(G), "bool": torch.ones(G, dtype=torch.bool),
             "list": [25, 1, 9]}[bad]
    with pytest.raises(ValueError, match="image_lengths"):
        net(images, q, lengths, image_index=INDEX, image_lengths=sizes)
    with pytest.raises(ValueError, match="image_lengths"):
        macx.MACNetCore.forward(net, images, torch.zeros(B, 256), torch.zeros(B, S, 256), lengths, image_index=INDEX, image_lengths=sizes)


@pytest.mark.parametrize("sizes", [[25, 0, 9], [25, 1, 26]])
def test_image_lengths_range_is_checked_on_the_host(macx, sizes):
    net = small_net(macx)
    images, q, lengths = tower_inputs()
    with pytest.raises(ValueError, match=r"image_lengths must lie in \[1, 25\]"):
        net(images, q, lengths, image_index=INDEX, image_lengths=torch.tensor(sizes))
    with pytest.raises(ValueError, match=r"image_lengths must lie in \[1, 25\]"):
        macx.MACNetCore.forward(net, images, torch.zeros(B, 256), torch.zeros(B, S, 256), lengths, image_index=INDEX,
                                image_lengths=torch.tensor(sizes), check_kb_lengths=True)
    with pytest.raises(RuntimeError, match="no CPU path|HIP device"):        # unchecked: on to the device (the kernel clamps)
        net(images, q, lengths, image_index=INDEX, image_lengths=torch.tensor(sizes), check_ids=False)


def bare(macx, name, **attrs):
    """an instance that was never constructed (construction needs the device): load() refuses its arguments before it touches a tensor"""
    obj = object.__new__(getattr(macx, name))
    for k, v in attrs.items():
        setattr(obj, k, v)
    return obj


@pytest.mark.parametrize("name", CELL_CLASSES)
def test_cell_load_takes_kb_lengths_exactly_when_built_with_them(macx, name):
    x = [torch.zeros(B, 128), torch.zeros(B, S, 128), torch.full((B,), S, dtype=torch.int32), torch.zeros(B, N, 128)]
    train = {} if name == "CapturedForward" else {"d_memory": torch.zeros(B, 128)}
    with pytest.raises(TypeError, match="no kb_lengths"):
        bare(macx, name, **train).load(*x, kb_lengths=torch.ones(B, dtype=torch.int32), **train)
    with pytest.raises(TypeError, match="needs kb_lengths"):
        bare(macx, name, kb_lengths=torch.ones(B, dtype=torch.int32), **train).load(*x, **train)
    built = bare(macx, name, kb_lengths=torch.ones(B, dtype=torch.int32), knowledgeBase=x[3], **train)
    for bad in (torch.ones(B - 1, dtype=torch.int32), torch.ones(B), torch.ones(B, dtype=torch.bool)):
        with pytest.raises(ValueError, match="kb_lengths"):
            built.load(*x, kb_lengths=bad, **train)
    for bad in ([1, 1, 0, 1, 1, 1], [1, 1, N + 1, 1, 1, 1]):                 # check_ids: the range, on the host
        with pytest.raises(ValueError, match=r"kb_lengths must lie in \[1, 25\]"):
            built.load(*x, kb_lengths=torch.tensor(bad), **train)


@pytest.mark.parametrize("name", TOWER_CLASSES)
def test_tower_load_takes_lengths_exactly_when_built_with_them(macx, name):
    images, q, lengths = tower_inputs()
    x = (images, q, lengths) + ((torch.zeros(B, dtype=torch.int32),) if name == "CapturedTowerTrainStep" else ())
    kbl, iml = torch.ones(B, dtype=torch.int32), torch.ones(G, dtype=torch.int32)
    geometry = dict(B=B, S=S, G=G, N=N)
    with pytest.raises(TypeError, match="no kb_lengths"):
        bare(macx, name, **geometry).load(*x, image_index=INDEX, kb_lengths=kbl)
    with pytest.raises(TypeError, match="no image_lengths"):
        bare(macx, name, **geometry).load(*x, image_index=INDEX, image_lengths=iml)
    with pytest.raises(TypeError, match="needs kb_lengths"):
        bare(macx, name, kb_lengths=kbl, **geometry).load(*x, image_index=INDEX)
    with pytest.raises(TypeError, match="needs image_lengths"):
        bare(macx, name, image_lengths=iml, **geometry).load(*x, image_index=INDEX)
    with pytest.raises(ValueError, match="image_lengths"):                     # one size per IMAGE
        bare(macx, name, image_lengths=iml, **geometry).load(*x, image_index=INDEX, image_lengths=kbl)
    with pytest.raises(ValueError, match=r"image_lengths must lie in \[1, 25\]"):
        bare(macx, name, image_lengths=iml, **geometry).load(*x, image_index=INDEX, image_lengths=torch.tensor([1, 26, 1]))
    with pytest.raises(ValueError, match=r"kb_lengths must lie in \[1, 25\]"):
        bare(macx, name, kb_lengths=kbl, **geometry).load(*x, image_index=INDEX, kb_lengths=torch.tensor([1, 1, 1, 0, 1, 1]))


def test_tower_constructors_refuse_before_the_device(macx):
    net = small_net(macx)
    assert net.stem.keep < 1.0                                      # the flag file's stemDropout
    with pytest.raises(ValueError, match="stemDropout"):            # the eager path's refusal, at construction
        macx.CapturedTowerTrainStep(net, None, None, B, S, H=5, W=5, imageInDim=128, images=G)
    for make in (lambda **kw: macx.CapturedTowerForward(net, B, S, H=5, W=5, imageInDim=128, **kw),
                 lambda **kw: macx.CapturedTowerTrainStep(net, None, None, B, S, H=5, W=5, imageInDim=128, **kw)):
        with pytest.raises(ValueError, match="images=G"):
            make(image_lengths=True)
    keeps = small_net(macx, stemDropout=1.0)
    with pytest.raises(ValueError, match="kb_lengths"):
        macx.CapturedTowerTrainStep(keeps, None, None, B, S, H=5, W=5, imageInDim=128, images=G, image_lengths=True, kb_lengths=True)
    with pytest.raises(RuntimeError, match="HIP device"):           # a stem that keeps everything: on to the device
        macx.CapturedTowerTrainStep(keeps, None, None, B, S, H=5, W=5, imageInDim=128, images=G, image_lengths=True)
