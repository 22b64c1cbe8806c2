"""The host side of the guarded optimizer step (macx_adam_ema_step_g / _pg, optim.FlatAdamEMA(guard=True)): the exports against the
header, every MACX_EINVAL of the two calls (returned before any HIP call, so without a device and on addresses that are never
dereferenced), and the constructor's refusal, raised before the device is asked.  No GPU."""
import ctypes as C
import math

import pytest
import torch

from abi_kit import ptr
from test_abi_host import header_prototypes, prototype_mismatches

NEW = ("macx_adam_ema_step_g", "macx_adam_ema_step_pg")
A16 = 0x10000           # addresses that are never dereferenced: every call below is refused before anything is launched

# a legal call, then one argument at a time made illegal
G_NAMES = ("n", "params", "grads", "m", "v", "ema", "lr", "beta1", "beta2", "eps", "step", "clip_norm", "ema_decay", "skip_above", "guard",
           "ws", "norm_out")
G_OK = dict(zip(G_NAMES, (1000, A16, 2 * A16, 3 * A16, 4 * A16, 5 * A16, 1e-3, 0.9, 0.999, 1e-8, 1, 8.0, 0.999, 0.0, 6 * A16, 7 * A16, 8 * A16)))
PG_NAMES = ("n", "params", "grads", "m", "v", "ema", "lr_t_dev", "beta1", "beta2", "eps", "clip_norm", "ema_decay", "skip_above", "guard",
            "ws", "norm_out")
PG_OK = dict(zip(PG_NAMES, (1000, A16, 2 * A16, 3 * A16, 4 * A16, 5 * A16, 9 * A16, 0.9, 0.999, 1e-8, 8.0, 0.999, 0.0, 6 * A16, 7 * A16, 8 * A16)))
# what the guard adds ...
GUARD_BAD = [("guard", 0), ("guard", 6 * A16 + 1), ("guard", 6 * A16 + 2), ("skip_above", -1.0), ("skip_above", math.nan), ("skip_above", -math.inf)]
# ... and what the unguarded namesakes already refuse
PLAIN_BAD = [("params", 0), ("grads", 0), ("m", 0), ("v", 0), ("ws", 0), ("ema", 0), ("n", 0)]
G_BAD = GUARD_BAD + PLAIN_BAD + [("step", 0), ("step", -3)]
PG_BAD = GUARD_BAD + PLAIN_BAD + [("lr_t_dev", 0)]


def test_exports_are_in_the_table_in_the_headers_place(macx):
    protos = header_prototypes()
    for n in NEW:
        assert n in macx._lib.EXPORTS and n in macx._lib.TABLE and n in protos, n
    assert prototype_mismatches({n: macx._lib.TABLE[n] for n in NEW}) == []
    # the namesake's arguments with skip_above (float) and guard (pointer) in front of ws
    for new, old in zip(NEW, ("macx_adam_ema_step", "macx_adam_ema_step_p")):
        ret, args = protos[old]
        assert protos[new] == (ret, args[:-3] + ["float", "pointer"] + args[-3:]), new
        o, n = macx._lib.TABLE[old][1], macx._lib.TABLE[new][1]
        assert n == o[:-3] + (C.c_float, C.c_void_p) + o[-3:], new
    assert len(G_NAMES) + 1 == len(protos[NEW[0]][1]) and len(PG_NAMES) + 1 == len(protos[NEW[1]][1])      # (+ the stream)
    order = list(macx._lib.EXPORTS)
    at = order.index("macx_adam_ema_step_p")
    assert tuple(order[at + 1:at + 3]) == NEW                             # directly behind macx_adam_ema_step_p, as in the header
    L = macx._lib.lib()
    for n in NEW:
        assert list(getattr(L, n).argtypes) == list(macx._lib.TABLE[n][1]) and getattr(L, n).restype is C.c_int
    assert macx._lib.ABI_VERSION == 5 and L.macx_abi_version() == 5       # new exports only, no struct


def test_the_legal_calls_differ_from_the_refused_ones_in_one_argument(macx):
    """(the legal calls themselves would launch: they run in tests/test_gpu_guarded_step.py.  Here: the unguarded namesakes refuse
    what PLAIN_BAD lists, so those rows test the checks the guarded calls share with them.)"""
    L = macx._lib.lib()
    for name, value in PLAIN_BAD + [("step", 0)]:
        a = dict(G_OK, **{name: value})
        assert L.macx_adam_ema_step(*[a[k] for k in G_NAMES if k not in ("skip_above", "guard")], None) == macx._lib.MACX_EINVAL, name
    for name, value in PLAIN_BAD + [("lr_t_dev", 0)]:
        a = dict(PG_OK, **{name: value})
        assert L.macx_adam_ema_step_p(*[a[k] for k in PG_NAMES if k not in ("skip_above", "guard")], None) == macx._lib.MACX_EINVAL, name


@pytest.mark.parametrize("name,value", G_BAD)
def test_step_g_refuses_before_any_launch(macx, name, value):
    a = dict(G_OK, **{name: value})
    assert macx._lib.lib().macx_adam_ema_step_g(*[a[k] for k in G_NAMES], None) == macx._lib.MACX_EINVAL


@pytest.mark.parametrize("name,value", PG_BAD)
def test_step_pg_refuses_before_any_launch(macx, name, value):
    a = dict(PG_OK, **{name: value})
    assert macx._lib.lib().macx_adam_ema_step_pg(*[a[k] for k in PG_NAMES], None) == macx._lib.MACX_EINVAL


def test_a_guard_at_an_odd_host_address_is_refused(macx):
    """the same refusal on real memory (abi_kit.ptr of a host tensor): bytes 1.. of a 32-byte buffer are no uint32 words"""
    buf = torch.zeros(32, dtype=torch.uint8)
    for off in (1, 2, 3):
        a = dict(G_OK, guard=ptr(buf[off:]))
        assert macx._lib.lib().macx_adam_ema_step_g(*[a[k] for k in G_NAMES], None) == macx._lib.MACX_EINVAL
    assert not buf.any()


def test_skip_above_needs_the_guard(macx):
    """raised before the parameters are looked at, let alone a device: an empty parameter list gets this far"""
    with pytest.raises(ValueError, match="guard=True"):
        macx.optim.FlatAdamEMA([], skip_above=1.0)
    with pytest.raises(ValueError, match="guard=True"):
        macx.optim.FlatAdamEMA([torch.zeros(3)], skip_above=1.0, guard=False)
    for bad in (-1.0, math.nan):
        with pytest.raises(ValueError, match="skip_above"):
            macx.optim.FlatAdamEMA([torch.zeros(3)], guard=True, skip_above=bad)
    with pytest.raises(RuntimeError, match="HIP device"):                 # (a legal pairing goes on to ask for device parameters)
        macx.optim.FlatAdamEMA([torch.zeros(3)], guard=True, skip_above=1.0)
