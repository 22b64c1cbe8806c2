"""-m gpu: a run reports whether its in-launch hand-offs completed (include/macx.h macx_run_status; MACCell.status / .check; the
captured steps' check_every).  d = 512 shapes at which the filler workgroups of chain_fwd run (tests/test_gpu_knobs.py).  No test
here makes a wait time out: the sticky status is exercised by WRITING the word, the give-up branch by macx_handoff_selftest, which
runs the kernels' wait routine on words of its own with a budget of 0 polls."""
import ctypes as C

import pytest
import torch

import abi_kit
from helpers import make_case
from test_gpu_cell import build_cell

pytestmark = pytest.mark.gpu

SHAPES = [("args", 5, 5, 49, 512, 4), ("args", 8, 7, 196, 512, 3)]


def _train_run(macx, dev, name, B, S, N, d, p):
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    cell, params, leaves = build_cell(macx, dev, cfg, vq, words, lengths, kb, True, seed=11, requires_grad=True, tune={"pre_fill": 1})
    state = cell.run()
    gm = torch.randn(B, d, generator=torch.Generator().manual_seed(3)).to(dev)
    (state.memory * gm).sum().backward()
    torch.cuda.synchronize()
    return cell, state, params, leaves


def _abi_status(macx, run):
    bits, first = C.c_uint32(99), C.c_int32(99)
    stream = abi_kit.stream(run.saved.device)
    rc = run.L.macx_run_status(C.byref(run.opts), C.byref(run.shapes), run.keep, abi_kit.ptr(run.saved),
                               C.c_size_t(run.saved_floats), stream, C.byref(bits), C.byref(first))
    return rc, bits.value, first.value


def _status_words(macx, run):
    off, cnt = C.c_size_t(0), C.c_size_t(0)
    assert run.L.macx_saved_segment(C.byref(run.opts), C.byref(run.shapes), run.keep, macx._lib.SEG["status"], C.byref(off), C.byref(cnt)) == 0
    return run.saved.view(torch.int32)[off.value: off.value + cnt.value]


@pytest.mark.parametrize("name,B,S,N,d,p", SHAPES)
def test_clean_run_reports_ok(macx, dev, name, B, S, N, d, p):
    cell, state, params, (vqd, wd, kbd) = _train_run(macx, dev, name, B, S, N, d, p)
    assert cell.status() == (0, -1)
    cell.check()
    assert _abi_status(macx, cell._run) == (macx._lib.MACX_OK, 0, -1)
    assert int(cell._run.saved.view(torch.int32)[-576 + 63]) == 0
    assert bool(torch.isfinite(state.memory).all()) and bool(torch.isfinite(kbd.grad).all())
    assert int(_status_words(macx, cell._run).abs().sum()) == 0


@pytest.mark.parametrize("name,B,S,N,d,p", SHAPES)
def test_status_is_sticky_until_reset(macx, dev, name, B, S, N, d, p):
    cell, state, params, _ = _train_run(macx, dev, name, B, S, N, d, p)
    run = cell._run
    mem = state.memory.detach().clone()
    words = _status_words(macx, run)
    words[0] = 1                      # an injection, not a provoked timeout
    words[1] = 3                      # 1 + step
    with pytest.raises(macx.HandoffTimeout) as e:
        cell.check()
    assert (e.value.bits, e.value.first_step) == (1, 2)
    assert _abi_status(macx, run) == (macx._lib.MACX_EWAIT, 1, 2)
    run.forward()                     # macx_cell_begin + every step again, on the same buffer: the counters are zeroed, the status is not
    torch.cuda.synchronize()
    assert int(run.saved.view(torch.int32)[-576 + 63]) == 0
    assert cell.status() == (1, 2)
    assert torch.equal(cell._memories_all[p], mem)
    cell.reset_status()
    assert cell.status() == (0, -1)
    assert _abi_status(macx, run) == (macx._lib.MACX_OK, 0, -1)
    cell.check()


def test_captured_step_checks_every_k_replays(macx, dev):
    name, B, S, N, d, p = SHAPES[0]
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    params = macx.MACCellParams(cfg, p, generator=torch.Generator().manual_seed(5)).to(dev)
    step = macx.CapturedTrainStep(cfg, params, B, S, N, seed=7, check_every=1)
    assert step.captured
    g = torch.Generator().manual_seed(9)
    step.load(vq.to(dev), words.to(dev), lengths.to(dev), kb.to(dev), torch.randn(B, d, generator=g).to(dev))
    step.set_mask_word(0x1234567)
    for _ in range(3):
        step.replay()                 # check_every = 1: each of them ends in a check
    torch.cuda.synchronize()
    want = [t.grad.clone() for t in step._leaves()]
    want_mem = step.memory.clone()
    run = step.cell._run
    assert not run.status_reset_pending
    _status_words(macx, run)[0] = 2
    with pytest.raises(macx.HandoffTimeout):
        step.replay()
    with pytest.raises(macx.HandoffTimeout):      # sticky across replays
        step.replay()
    step.reset_status()
    step.replay()
    torch.cuda.synchronize()
    assert step.status() == (0, -1)
    assert torch.equal(step.memory, want_mem)
    for t, w in zip(step._leaves(), want):
        assert torch.equal(t.grad, w)
    # check_every = 0 (the default): replay() adds nothing, check() still tells
    step.check_every = 0
    _status_words(macx, run)[0] = 1
    step.replay()
    torch.cuda.synchronize()
    with pytest.raises(macx.HandoffTimeout):
        step.check()
    step.reset_status()
    step.check()


def test_captured_forward_has_the_interface(macx, dev):
    name, B, S, N, d, p = SHAPES[0]
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    params = macx.MACCellParams(cfg, p, generator=torch.Generator().manual_seed(5)).to(dev)
    fwd = macx.CapturedForward(cfg, params, B, S, N, check_every=2)
    fwd(vq.to(dev), words.to(dev), lengths.to(dev), kb.to(dev))
    fwd.replay()
    assert fwd.status() == (0, -1)
    _status_words(macx, fwd.cell._run)[0] = 1
    fwd.replay()                      # replay 3 of check_every = 2: not checked
    with pytest.raises(macx.HandoffTimeout):
        fwd.replay()                  # replay 4: checked
    fwd.reset_status()
    fwd.check()


def test_wait_routine_selftest(macx, dev):
    L = macx._lib.lib()
    out = (C.c_uint32 * 8)(*([99] * 8))
    stream = abi_kit.stream(dev)
    assert L.macx_handoff_selftest(stream, out) == macx._lib.MACX_OK
    arrived, gave_up = list(out)[:4], list(out)[4:]
    assert arrived == [1, 0, 0, 0]            # arrived, status 0, no step, nobody told to poison
    assert gave_up == [0, 2, 7, 1]            # budget 0: gave up at once, bit set, 1 + step 6 recorded, all 256 threads told to poison


def test_generic_path_has_nothing_to_report(macx, dev):
    from oracle import mac_oracle as mo
    Bq, S, N, d, p = 3, 5, 14, 128, 2
    dcfg = mo.default_config(netLength=p, memDim=d, ctrlDim=d, attDim=d)
    vq, words, lengths, kb = macx.configs.synthetic_inputs(Bq, S, N, d, seed=3)
    vs = mo.VarStore(generator=torch.Generator().manual_seed(1))
    mo.mac_network(dcfg, vs, vq, words, words, lengths, kb)
    gp = macx.GenericParams(device=dev).load_reference_dict(vs.params)
    cell = macx.MACCell(vq.to(dev), words.to(dev), words.to(dev), lengths.to(dev), kb.to(dev), 1.0, 1.0, 1.0, Bq, False,
                        config=dcfg, params=gp)
    assert isinstance(cell, macx.GenericMACCell)
    with torch.no_grad():
        cell.run()
    assert cell.status() == (0, -1)
    assert cell.check() is None
