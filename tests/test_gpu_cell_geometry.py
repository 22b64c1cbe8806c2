"""-m gpu: the fused cell against the fp64 oracle at the widths, tile edges and questions-per-tile counts that the kernel dispatch
instantiates differently and no other test launches: d = 384 (chain<384>, the 128-wide S_b contraction, kw = jw = 1 above 128
columns), 512 < d < 1024 (the per-product H2 route at 640 / 768 / 896), the ragged last tile and the row-count boundaries of the 16-,
32- and 64-row d = 512 chain kernels, their keep = 1 backward, and 64-row backward tiles that touch 3, 4 or 5 questions.

The checks are test_gpu_cell's own (final state, dKB / dwords / dvecQ and every parameter gradient to FWD_TOL / GRAD_TOL; attentions
and histories where the forward test is named), re-used as test_gpu_limits.py does.  Each case prints the largest forward and
gradient error it saw and the route the library planned for it (macx_cell_route; `pytest -s`).

Observed on an MI355X (256 CUs), default kernel family: flag file, B S N d p, largest forward error (bound 2e-5), largest gradient
error (bound 2e-4), route ("fill a/b": filler workgroups of chain_fwd / of chain_bwd for dKB; tests/route_cases.py holds this column as
data and tests/test_route_host.py asserts it on the library's plan for 256 compute units).  A kernel trace of the
d = 384, M = 8232 and 640 / 768 / 896 cases shows chain_fwd/bwd_kernel<384, 0, .., 64> + sb_h2_kernel + wgrad_h2_kernel<1, 1>,
chain_fwd/bwd_kernel<512, 4, .., 64> + chain_dkb_rest_kernel<512, 4> + sb_h2w_kernel + wgrad_h2_kernel<2, 2>, and kb_gemm_h2_kernel
per product with no chain kernel.  Intermediate products (bound 1e-6): 1.6e-7 / 1.7e-7 / 1.3e-7 (X / H1 / I2) at d = 384,
1.9e-7 / 2.0e-7 / 2.0e-7 at M = 8232.
  args   3 7   49 384 2 train  3.27e-07  7.12e-06  chain<384>, 64-row x 3 (ragged), S_b deferred 128x128 kw=jw=1 fill 0/0
  args1  2 5  100 384 3 train  5.62e-07  4.77e-06  chain<384>, 64-row x 4 (ragged), S_b deferred 128x128 kw=jw=1 fill 0/0
  args4  3 6   20 384 2 eval   2.77e-07  4.69e-06  chain<384>, 64-row x 1 (ragged), S_b per step kw=jw=1 fill 0/0
  args   2 5  209 384 2 train  3.82e-07  3.87e-06  chain<384>, 64-row x 7 (ragged), S_b deferred 128x128 kw=jw=1 fill 0/0
  args   3 6   49 320 2 train  5.23e-07  6.11e-06  chain<384>, 64-row x 3 (ragged), S_b deferred 128x128 kw=jw=1 fill 0/0
  args   2 5   49 640 2 train  6.46e-07  8.64e-06  per-product kw=jw=1
  args3  2 5   33 768 2 train  1.04e-06  4.77e-06  per-product kw=jw=2
  args   1 4   16 896 1 eval   6.37e-07  1.91e-05  per-product kw=jw=1
  args  21 5  196 512 2 train  7.12e-07  2.37e-06  chain<512>, 32-row x 129 (ragged), S_b deferred 128x256 kw=jw=2 fill 127/0
  args  42 5  196 512 2 train  8.71e-07  3.51e-06  chain<512>, 64-row x 129 (ragged), S_b deferred 128x256 kw=jw=2 fill 127/127
  args  16 4  256 512 1 train  7.60e-07  2.12e-06  chain<512>, 16-row x 256, S_b deferred 128x256 kw=jw=2 fill 64/0
  args  32 4  256 512 1 train  7.19e-07  3.30e-06  chain<512>, 32-row x 256, S_b deferred 128x256 kw=jw=2 fill 0/0
  args  17 4  241 512 1 train  6.72e-07  2.97e-06  chain<512>, 32-row x 129 (ragged), S_b deferred 128x256 kw=jw=2 fill 127/0
  args  33 4  249 512 1 eval   8.31e-07  3.72e-06  chain<512>, 64-row x 129 (ragged), S_b deferred 128x256 kw=jw=2 fill 127/0
  args   3 9  196 512 2 eval   9.08e-07  7.28e-06  chain<512>, 16-row x 37 (ragged), S_b deferred 128x256 kw=jw=2 fill 64/0
  args1  5 7   49 512 3 eval   5.67e-07  3.45e-06  chain<512>, 16-row x 16 (ragged), S_b deferred 128x256 kw=jw=2 fill 64/0
  args   9 5   17 256 2 train  4.02e-07  1.60e-06  chain<256>, 64-row x 3 (ragged), S_b per step kw=jw=2 fill 0/0
  args   9 5   16 256 2 train  4.15e-07  4.81e-06  chain<256>, 64-row x 3 (ragged), S_b per step kw=jw=2 fill 0/0
  args   9 5   31 256 3 train  4.57e-07  1.13e-06  chain<256>, 64-row x 5 (ragged), S_b per step kw=jw=2 fill 0/0
  args   9 5   32 256 3 train  4.83e-07  1.60e-06  chain<256>, 64-row x 5 (ragged), S_b deferred 128x256 kw=jw=2 fill 0/0
  args1  7 5   21 128 2 eval   2.60e-07  2.09e-06  chain<128>, 64-row x 3 (ragged), S_b per step kw=jw=1 fill 0/0
  args   5 4   15 256 2 train  3.25e-07  6.78e-06  per-product kw=jw=2
"""
import ctypes as C

import pytest
import torch

from abi_kit import ptr
import helpers
import route_cases as rc
import test_gpu_cell as cellmod
from helpers import make_case
from test_gpu_cell import FWD_TOL, GRAD_TOL, build_cell

pytestmark = pytest.mark.gpu


def _route(macx, name, B, S, N, d, p):
    """the library's own route plan for this case on the current device (macx_cell_route, ncu = 0: exactly what the launches follow;
    the dropout moves no field that is printed).  What it says on 256 compute units is asserted in tests/test_route_host.py."""
    dk, dlog = rc.padded(d)
    return rc.route(macx, *rc.frozen(macx, name, (B, S, N, dk, p, dlog), None), ncu=0)


@pytest.fixture
def observed(monkeypatch):
    """test_gpu_cell's parity tests, observed: every rel_err they compute and every cell they build is kept for the caller.
    For the printed record only: which figure is the forward one rests on the ORDER of the calls in test_gpu_cell (the final memory
    first); what passes or fails is decided there, on its own tolerances, whatever this fixture sees."""
    seen = {"errs": [], "cells": []}
    plain_build = cellmod.build_cell

    def rel_err(a, b, floor=1e-6):
        e = helpers.rel_err(a, b, floor=floor)
        seen["errs"].append(e)
        return e

    def build(*a, **kw):
        out = plain_build(*a, **kw)
        seen["cells"].append(out[0])
        return out

    monkeypatch.setattr(cellmod, "rel_err", rel_err)
    monkeypatch.setattr(cellmod, "build_cell", build)
    return seen


def _parity(macx, dev, observed, name, B, S, N, d, p, train):
    """every gradient against the oracle; returns the cell.  The first error the shared test computes is the final memory's."""
    try:
        cellmod.test_backward_matches_oracle_autograd(macx, dev, name, B, S, N, d, p, train)
    finally:
        e = observed["errs"]
        if e:
            print("\nGEOMETRY %s B=%d S=%d N=%d d=%d p=%d train=%d: fwd %.2e (tol %.0e) grad %.2e (tol %.0e) | %s"
                  % (name, B, S, N, d, p, train, e[0], FWD_TOL, max(e[1:] or [0.0]), GRAD_TOL, rc.describe(_route(macx, name, B, S, N, d, p))))
    cell = observed["cells"][-1]
    assert cell.status() == (0, -1)
    return cell


WIDTH_384 = [
    ("args", 3, 7, 49, 384, 2, True),          # chain<384> forward and backward, one 64-row tile per 1.3 questions, S_b on the 128-wide kernel
    ("args1", 2, 5, 100, 384, 3, True),        # recurrent control: dc inside the loop at the narrow wgrad tiles (kw = jw = 1 at 384)
    ("args4", 3, 6, 20, 384, 2, False),        # write gate, evaluation: the keep = 1 backward, N < 32 (S_b once per step)
    ("args", 2, 5, 209, 384, 2, True),         # a question's knowledge base crosses a row tile (209 = 3 x 64 + 17)
    ("args", 3, 6, 49, 320, 2, True),          # 320 -> 384 through PaddedMACCell: dropout indices at the logical width
]


@pytest.mark.parametrize("name,B,S,N,d,p,train", WIDTH_384)
def test_width_384_matches_the_oracle(macx, dev, observed, name, B, S, N, d, p, train):
    _parity(macx, dev, observed, name, B, S, N, d, p, train)


@pytest.mark.parametrize("name,B,S,N,d,p,train", [WIDTH_384[0], WIDTH_384[2]])
def test_width_384_forward_stepwise(macx, dev, name, B, S, N, d, p, train):
    """attentions (question, kb, gate), histories and the state of every step at d = 384"""
    cellmod.test_forward_stepwise_matches_oracle(macx, dev, name, B, S, N, d, p, train)


@pytest.mark.parametrize("name,B,S,N,d,p,train", [
    ("args", 2, 5, 49, 640, 2, True),          # per-product route (use_chain is false above 512), kw = jw = 1 at five 128-column blocks
    ("args3", 2, 5, 33, 768, 2, True),         # kw = jw = 2 at 768, self-attention over the histories
    ("args", 1, 4, 16, 896, 1, False),         # one question, one step, evaluation: kw = jw = 1 at seven blocks
])
def test_widths_between_512_and_1024_match_the_oracle(macx, dev, observed, name, B, S, N, d, p, train):
    _parity(macx, dev, observed, name, B, S, N, d, p, train)


@pytest.mark.parametrize("name,B,S,N,d,p,train", [
    ("args", 21, 5, 196, 512, 2, True),        # M = 4116 = 128 x 32 + 20: ragged last 32-row tile
    ("args", 42, 5, 196, 512, 2, True),        # M = 8232 = 128 x 64 + 40: ragged last 64-row tile, 129 tiles: forward and dKB fillers both active
    ("args", 16, 4, 256, 512, 1, True),        # M = 4096: the last row count of the 16-row geometry (256 tiles)
    ("args", 32, 4, 256, 512, 1, True),        # M = 8192: the last row count of the 32-row geometry (256 tiles)
    ("args", 17, 4, 241, 512, 1, True),        # M = 4097: the first of the 32-row geometry, one row in the last tile
    ("args", 33, 4, 249, 512, 1, False),       # M = 8217: just past 8192, 64-row tiles, 25 rows in the last one, keep = 1
    ("args", 3, 9, 196, 512, 2, False),        # the keep = 1 backward (bits_or = 0xFF, no keep bytes) on 16-row tiles
    ("args1", 5, 7, 49, 512, 3, False),        # ... with recurrent control
])
def test_d512_tile_geometry_matches_the_oracle(macx, dev, observed, name, B, S, N, d, p, train):
    """(the hand-off status of every case is asserted clean in _parity: (0, -1) through cell.status())"""
    _parity(macx, dev, observed, name, B, S, N, d, p, train)


@pytest.mark.parametrize("name,B,S,N,d,p,train", [
    ("args", 9, 5, 17, 256, 2, True),          # a 64-row tile touches 5 questions (rows 64..127 = questions 3..7): the division path of stage B0
    ("args", 9, 5, 16, 256, 2, True),          # 4 questions per tile, aligned
    ("args", 9, 5, 31, 256, 3, True),          # 4 questions (nq > 3) with chain_sums off
    ("args", 9, 5, 32, 256, 3, True),          # 3 questions: the first N with chain_sums and the deferred S_b
    ("args1", 7, 5, 21, 128, 2, False),        # 4 questions per tile at the narrowest width, recurrent control, the keep = 1 backward
    ("args", 5, 4, 15, 256, 2, True),          # N = 15: the last N off the chain kernels (they take N >= 16)
])
def test_questions_per_tile_match_the_oracle(macx, dev, observed, name, B, S, N, d, p, train):
    _parity(macx, dev, observed, name, B, S, N, d, p, train)


@pytest.mark.parametrize("row", rc.GEOMETRY, ids=["%s-B%d-N%d-d%d-p%d" % (r[0], r[1], r[3], r[4], r[5]) for r in rc.GEOMETRY])
def test_route_for_the_current_device_is_the_route_for_its_compute_units(macx, dev, row):
    """ncu = 0 (what every launch plans with) asks the device: the same plan as naming its compute units.  Nothing is launched."""
    name, B, S, N, d, p = row[:6]
    dk, dlog = rc.padded(d)
    opts, sh = rc.frozen(macx, name, (B, S, N, dk, p, dlog), None)
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    for dp in (None, rc.dropout(macx, 0.9, 0.85, 0.8)):
        assert rc.route(macx, opts, sh, drop=dp, ncu=0) == rc.route(macx, opts, sh, drop=dp, ncu=ncu)
    assert ncu > 0


@pytest.mark.parametrize("B,S,N,d", [(3, 7, 49, 384), (42, 5, 196, 512)])
def test_chain_kernel_intermediate_products(macx, dev, B, S, N, d):
    """X, H1 and I2 of step 0 (macx_saved_activation), each against the fp64 product of the operand the kernel multiplied (the kept
    X for H1, the kept H1 for I2), so that a failure names the stage: error per unit of the row's largest sum |a w| + |b| below
    1e-6, the bound of test_gpu_h2.py::test_chain_kernel_products_on_wide_dynamic_range, on N(0,1)-scale inputs.  H1 =
    elu((X * y) W1a + X W1b + b1) with y = projY(memory 0) in fp64 from the run's own initial memory; ELU is 1-Lipschitz, so the
    pre-activation's scale bounds it."""
    L = macx._lib.lib()
    p = 1
    cfg, vq, words, lengths, kb = make_case("args", B, S, N, d, p)
    params = macx.MACCellParams(cfg, p, generator=torch.Generator().manual_seed(2)).to(dev)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for f in ("projX_b", "projY_b", "memKbProj_b", "memKbProj2_b"):
            getattr(params, f).copy_((torch.rand(d, generator=g) - 0.5) * 0.2)
    vqd, wd, kbd, ld = vq.to(dev), words.to(dev), kb.to(dev), lengths.to(dev)
    cell = macx.MACCell(vqd, wd, wd, ld, kbd, 1.0, 1.0, 1.0, B, True, config=cfg, params=params, seed=1, gemm="h2")
    run = macx.cell._Run(cell, True)
    run.begin()
    run.step(0)
    outs = []
    for which in (1, 2, 3):
        o = torch.empty(B * N, d, device=dev)
        macx._lib.check(L.macx_saved_activation(C.byref(run.opts), C.byref(run.shapes), which, 0, ptr(run.saved), run.saved_floats, ptr(o),
                                                run.stream), "macx_saved_activation")
        outs.append(o)
    mem0 = run.segment("memories", (p + 1, B, d))[0].clone()
    torch.cuda.synchronize()
    assert run.status() == (0, -1)
    X, H1, I2 = [o.cpu().double() for o in outs]
    w = lambda f: getattr(params, f).detach().cpu().double()
    y = mem0.cpu().double() @ w("projY_W") + w("projY_b")                    # [B, d]; keep = 1: no mask on the memory
    yr = y.repeat_interleave(N, dim=0)                                       # [B * N, d]
    W1a, W1b = w("memKbProj_W")[:d], w("memKbProj_W")[d:]
    A0 = kb.double().reshape(-1, d)
    pre1 = (X * yr) @ W1a + X @ W1b + w("memKbProj_b")
    stages = [("X", X, A0 @ w("projX_W") + w("projX_b"), A0.abs() @ w("projX_W").abs() + w("projX_b").abs()),
              ("H1", H1, torch.nn.functional.elu(pre1), (X * yr).abs() @ W1a.abs() + X.abs() @ W1b.abs() + w("memKbProj_b").abs()),
              ("I2", I2, H1 @ w("memKbProj2_W") + w("memKbProj2_b"), H1.abs() @ w("memKbProj2_W").abs() + w("memKbProj2_b").abs())]
    rows = _route(macx, "args", B, S, N, d, p)["tile_rows"]
    for name, got, ref, mag in stages:
        scale = mag.amax(dim=1, keepdim=True) + 1e-300
        e = ((got - ref).abs() / scale).amax(dim=1)
        r = int(e.argmax())
        print("\nGEOMETRY products d=%d M=%d %s: max %.2e mean %.2e, worst row %d (tile %d of %d, %d-row tiles)"
              % (d, B * N, name, float(e.max()), float(e.mean()), r, r // rows, (B * N + rows - 1) // rows, rows))
        assert float(e.max()) < 1e-6, "%s: %.3e at row %d = tile %d of %d (%d-row tiles)" % (
            name, float(e.max()), r, r // rows, (B * N + rows - 1) // rows, rows)


@pytest.mark.parametrize("name,B,S,N,d,p", [("args", 3, 7, 49, 384, 2), ("args", 42, 5, 196, 512, 2)])
def test_second_run_is_bit_identical(macx, dev, name, B, S, N, d, p):
    """no floating-point atomics anywhere: final memory, the projX and memKbProj weight gradients and dKB of a second run on the same
    inputs, parameters and masks are the first run's bits"""
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    dmem = torch.randn(B, d, generator=torch.Generator().manual_seed(9)) / B
    runs = []
    for _ in range(2):
        cell, params, (vqd, wd, kbd) = build_cell(macx, dev, cfg, vq, words, lengths, kb, True, seed=5, requires_grad=True)
        state = cell.run()
        (state.memory * dmem.to(dev)).sum().backward()
        torch.cuda.synchronize()
        assert cell.status() == (0, -1)
        runs.append((state.memory.detach().clone(), params.projX_W.grad.clone(), params.memKbProj_W.grad.clone(), kbd.grad.clone()))
    assert bool(torch.isfinite(runs[0][0]).all())
    for what, a, b in zip(("memory", "projX_W.grad", "memKbProj_W.grad", "knowledgeBase.grad"), *runs):
        assert torch.equal(a, b), what
