"""The host side of questions that share images (macx_kb_gather / macx_kb_gather_bwd, `image_index=` on MACNetCore / MACNet, `images=`
on CapturedTowerForward): the exports, the keywords that default to the behaviour of before, and the refusals, which are raised before
anything asks for the device.  No GPU."""
import ctypes as C
import inspect

import pytest
import torch

from test_tower_graph_host import small_net

B, S = 6, 7


def tower_inputs(G=3):
    images = torch.zeros(G, 25, 128)
    q = torch.ones(B, S, dtype=torch.int32)
    lengths = torch.full((B,), S, dtype=torch.int32)
    return images, q, lengths


def test_gather_symbols_are_exported_with_signatures(macx):
    L = macx._lib.lib()
    sig = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    for n in ("macx_kb_gather", "macx_kb_gather_bwd"):
        assert n in macx._lib.EXPORTS
        f = getattr(L, n)
        assert list(f.argtypes) == sig and f.restype is C.c_int, n
    assert macx._lib.ABI_VERSION == 5 and L.macx_abi_version() == 5


def test_new_keywords_default_to_the_old_behaviour(macx):
    for cls in (macx.MACNetCore, macx.MACNet):
        assert inspect.signature(cls.forward).parameters["image_index"].default is None, cls
        assert inspect.signature(cls.forward).parameters["check_index"].default is False, cls
    assert inspect.signature(macx.CapturedTowerForward.__init__).parameters["images"].default is None
    for f in (macx.CapturedTowerForward.load, macx.CapturedTowerForward.__call__):
        assert inspect.signature(f).parameters["image_index"].default is None, f


@pytest.mark.parametrize("bad", ["too short", "two axes", "float", "bool"])
def test_image_index_shape_and_dtype_are_refused_on_the_host(macx, bad):
    net = small_net(macx)
    images, q, lengths = tower_inputs()
    index = {"too short": torch.zeros(B - 1, dtype=torch.int32), "two axes": torch.zeros(B, 1, dtype=torch.int64),
             "float": torch.zeros(B), "bool": torch.zeros(B, dtype=torch.bool)}[bad]
    with pytest.raises(ValueError, match="image_index"):
        net(images, q, lengths, image_index=index)
    with pytest.raises(ValueError, match="image_index"):            # the core on the encoder's outputs
        macx.MACNetCore.forward(net, images, torch.zeros(B, 256), torch.zeros(B, S, 256), lengths, image_index=index)


def test_training_with_a_dropping_stem_is_refused_on_the_host(macx):
    index = torch.tensor([1, 1, 0, 2, 0, 1], dtype=torch.int32)
    images, q, lengths = tower_inputs()
    net = small_net(macx)
    assert net.stem.keep < 1.0                                      # the flag file's stemDropout
    with pytest.raises(ValueError, match="stemDropout"):
        net(images, q, lengths, train=True, seed=1, image_index=index)
    with pytest.raises(ValueError, match="stemDropout"):
        macx.MACNetCore.forward(net, images, torch.zeros(B, 256), torch.zeros(B, S, 256), lengths, train=True, seed=1, image_index=index)
    # evaluation, and training with a stem that keeps everything, pass the validation: what stops them here is the missing device
    for net, train in ((net, False), (small_net(macx, stemDropout=1.0), True)):
        with pytest.raises(RuntimeError, match="no CPU path|HIP device"):
            net(images, q, lengths, train=train, seed=1, image_index=index)


def test_the_opt_in_range_check_runs_on_the_host(macx):
    net = small_net(macx)
    images, q, lengths = tower_inputs(G=3)
    for index in ([1, 1, 0, 3, 0, 1], [1, -1, 0, 2, 0, 1]):
        with pytest.raises(IndexError, match="image_index"):
            net(images, q, lengths, image_index=torch.tensor(index), check_index=True)
    with pytest.raises(RuntimeError, match="no CPU path|HIP device"):   # in range: on to the device
        net(images, q, lengths, image_index=torch.tensor([1, 1, 0, 2, 0, 1]), check_index=True)


def test_without_image_index_a_cpu_call_still_has_no_cpu_path(macx):
    net = small_net(macx)
    images, q, lengths = tower_inputs(G=B)
    with pytest.raises(RuntimeError, match="no CPU path|HIP device"):
        net(images, q, lengths)
    with pytest.raises(RuntimeError, match="no CPU path|HIP device"):
        macx.MACNetCore.forward(net, images, torch.zeros(B, 256), torch.zeros(B, S, 256), lengths)
    with pytest.raises(RuntimeError, match="HIP device"):
        macx.CapturedTowerForward(net, B, S, H=5, W=5, imageInDim=128, images=3)
