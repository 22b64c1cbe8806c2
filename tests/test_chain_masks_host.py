"""The scalar identities behind the chain kernels' select-free forms (macx_common.hip.h: lane_mask, mask_f, bit_mask), checked bit
for bit against the selects they replace over a float grid with NaN (quiet, either sign, with payload), +-0, +-inf, denormals and
the extremes.  numpy restates the device expressions on 32-bit words; no GPU.

    mask for select          as_float(as_uint(t) & m)            ==  c ? t : 0.f          m = c ? ~0 : 0
    the other question       as_float(as_uint(t) ^ (as_uint(t) & m))  ==  c ? 0.f : t     (stage B0, two-question kernel)
    keep factor              as_float(sbfe(bits, e, 1) & as_uint(inv))  ==  bit e ? inv : 0.f
    dropped value            mask(g * inv, sbfe(bits, e, 1))     ==  bit e ? g * inv : 0.f
    no dropout               mask(g * 1.0f, ~0)                  ==  g                    (chain_fwd's logits pass multiplies always)
    sums                     acc + masked                        ==  acc + select         (same addend bits, same addition)
A multiply by 0 / 1 in place of the mask is NOT the select (NaN * 0, inf * 0): asserted too, as the reason for the masks.
ELU and its derivative keep their selects: the sign-bit form returns a positive NaN's own payload where the select returns
exp(NaN) - 1 -- not bit-identical for every input, so it was not adopted; nothing to check here.
"""
import numpy as np
import pytest


def _grid():
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFD00001,
                        0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF,
                        0x3F800000, 0xBF800000, 0x3F7FFFFF, 0x3F800001, 0x33800000, 0xB3800000], dtype=np.uint32)
    rng = np.random.default_rng(17)
    rand = rng.integers(0, 2 ** 32, size=4096, dtype=np.uint64).astype(np.uint32)
    rand = rand[(rand & 0x7F800000) != 0x7F800000]          # random words: finite values only (the NaNs above are quiet ones)
    return np.concatenate([special, rand])


GRID = _grid()
F = lambda u: u.view(np.float32)        # noqa: E731
U = lambda f: f.view(np.uint32)         # noqa: E731


def _sbfe1(bits, e):
    """v_bfe_i32 bits, e, 1: bit e spread over the word"""
    return np.where((bits >> np.uint32(e)) & np.uint32(1), np.uint32(0xFFFFFFFF), np.uint32(0)).astype(np.uint32)


def _select(c, t_bits):
    return np.where(c, t_bits, np.uint32(0)).astype(np.uint32)      # 0.f is the all-zero word


@pytest.mark.parametrize("c", [False, True])
def test_mask_is_the_select(c):
    m = np.uint32(0xFFFFFFFF if c else 0)
    assert np.array_equal(GRID & m, _select(c, GRID))
    # ... and the two-question form's other half: t ^ (t & m) is t where the mask is zero, +0.0 where it is set
    assert np.array_equal(GRID ^ (GRID & m), _select(not c, GRID))


def test_a_multiply_is_not_the_select():
    with np.errstate(invalid="ignore"):
        prod = U(F(GRID) * np.float32(0.0))
    differs = prod != 0
    assert differs.any() and np.isnan(F(GRID[differs])).any() and np.isinf(F(GRID[differs])).any()


@pytest.mark.parametrize("inv", [1.0, 1.0 / 0.85, 1.0 / 0.5])
def test_keep_factor(inv):
    invb = U(np.array([inv], dtype=np.float32))[0]
    bits = np.arange(256, dtype=np.uint32)
    for e in range(8):
        want = np.where((bits >> e) & 1, invb, np.uint32(0)).astype(np.uint32)
        assert np.array_equal(_sbfe1(bits, e) & invb, want)
    # bits above the byte do not matter to bit e (the stand-in for missing keep bytes ORs 0xFF into whatever was read)
    junk = (bits | np.uint32(0xABCD0000))
    assert np.array_equal(_sbfe1(junk, 3), _sbfe1(bits, 3))


@pytest.mark.parametrize("inv", [1.0 / 0.85, 1.0 / 0.5])
def test_dropped_value(inv):
    inv = np.float32(inv)
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = U(F(GRID) * inv)
    for bit in (0, 1):
        bits = np.full(GRID.shape, bit << 5, dtype=np.uint32)
        assert np.array_equal(scaled & _sbfe1(bits, 5), _select(bit == 1, scaled))


def test_no_dropout_multiplies_by_one():
    """chain_fwd's logits pass: without read dropout every keep bit is set and the factor is 1.0f -- the value's own bits, denormals
    included (the kernels run with fp32 denormals on); a quiet NaN keeps its payload"""
    with np.errstate(invalid="ignore"):
        one = U(F(GRID) * np.float32(1.0))
    assert np.array_equal(one & np.uint32(0xFFFFFFFF), GRID)


@pytest.mark.parametrize("c", [False, True])
def test_sums_take_the_same_addend(c):
    acc = F(GRID[::-1].copy())
    m = np.uint32(0xFFFFFFFF if c else 0)
    with np.errstate(invalid="ignore", over="ignore"):
        a = U(acc + F(GRID & m))
        b = U(acc + F(_select(c, GRID)))
    assert np.array_equal(a, b)
