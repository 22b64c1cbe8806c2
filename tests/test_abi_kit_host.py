"""CPU: what tests/abi_kit.py promises -- exactly the properties on which the per-file copies it replaced disagreed."""
import numpy as np
import pytest
import torch

import abi_kit


def _from_bits(words, dtype):
    return torch.tensor(words, dtype={torch.float32: torch.int32, torch.float16: torch.int16}[dtype]).view(dtype)


# (dtype, quiet NaN, the same NaN with another payload)
NANS = [(torch.float32, 0x7FC00000, 0x7FC00001), (torch.float16, 0x7E00, 0x7E01)]


@pytest.mark.parametrize("dtype,nan,other", NANS, ids=["fp32", "fp16"])
@pytest.mark.parametrize("as_numpy", [False, True], ids=["torch", "numpy"])
def test_bits_equal(dtype, nan, other, as_numpy):
    conv = (lambda t: t.numpy()) if as_numpy else (lambda t: t)
    eq = lambda a, b: abi_kit.bits_equal(conv(a), conv(b))
    t = torch.arange(12, dtype=torch.float32).sub(5.5).to(dtype).view(3, 4)
    assert eq(t, t.clone())
    strided = t.t()                                                     # a non-contiguous view against its contiguous copy
    assert not strided.is_contiguous() and eq(strided, strided.contiguous())
    assert eq(_from_bits([nan, 0], dtype), _from_bits([nan, 0], dtype))
    assert not eq(_from_bits([nan, 0], dtype), _from_bits([other, 0], dtype))
    zero = torch.zeros(4, dtype=dtype)
    assert torch.equal(zero, -zero) and not eq(zero, -zero)
    assert not eq(zero, zero.view(2, 2))
    ints = zero.view(torch.int32 if dtype is torch.float32 else torch.int16)
    assert not eq(zero, ints) and eq(ints, ints.clone())


def test_bits_equal_refuses_a_tensor_against_an_array():
    t = torch.ones(3)
    assert not abi_kit.bits_equal(t, t.numpy()) and not abi_kit.bits_equal(t.numpy(), t)


def test_bits_widths():
    for dtype, want in ((torch.float32, torch.int32), (torch.float16, torch.int16), (torch.bfloat16, torch.int16), (torch.uint8, torch.uint8)):
        t = torch.ones(2, 3, dtype=dtype, requires_grad=dtype.is_floating_point).t()
        b = abi_kit.bits(t)
        assert b.dtype is want and b.shape == t.shape and b.is_contiguous() and not b.requires_grad and b.device.type == "cpu"
    assert abi_kit.bits(torch.tensor([1.0, -0.0])).tolist() == [0x3F800000, -0x80000000]


@pytest.mark.parametrize("kw", [{}, {"before": 0}, {"fill": -7, "dtype": torch.int32}, {"fill": float("nan")}, {"fill": -0.0}],
                         ids=["default", "before0", "int32", "nan", "minus0"])
def test_guarded(kw):
    n = 10

    def fresh():
        g = abi_kit.Guarded(n, "cpu", **kw)
        assert g.view.numel() == n and g.view.data_ptr() % 16 == 0 and g.view.dtype is kw.get("dtype", torch.float32)
        assert g.buf.numel() == kw.get("before", abi_kit.GUARD) + n + abi_kit.GUARD
        assert g.intact() and g.untouched()
        return g

    g = fresh()
    g.view[3] = 1
    assert g.intact() and not g.untouched()
    first = g.view.data_ptr() - g.buf.data_ptr()
    assert first == kw.get("before", abi_kit.GUARD) * g.buf.element_size()
    if kw.get("before", abi_kit.GUARD):
        g = fresh()
        g.buf[g.before - 1] = 1                                         # the one element just in front of the view
        assert not g.intact() and not g.untouched()
    g = fresh()
    g.buf[g.before + n] = 1                                             # the one just behind it
    assert not g.intact() and not g.untouched()
    g = fresh()
    g.buf[-1] = 0                                                       # +0.0 is not the fill, whatever the fill (-0.0 included)
    assert not g.intact()
    assert fresh().np(2, 5).shape == (2, 5) and isinstance(fresh().np(2, 5), np.ndarray)


def test_guard_constants():
    assert abi_kit.GUARD % 4 == 0 and abi_kit.ALLOC_GUARD % 4 == 0                          # 16-byte alignment of the inner view
    assert abs(abi_kit.SENT) > 1e11 and abi_kit.SENT != abi_kit.ALLOC_SENTINEL


def test_ptr():
    t = torch.zeros(8)
    assert abi_kit.ptr(None) is None
    assert abi_kit.ptr(t).value == t.data_ptr() and abi_kit.ptr(t[3:]).value == t.data_ptr() + 12
