"""-m gpu: losses on the fused cell's attention maps and step states (macx_cell_backward_x / macx_state_grads).

The reference is oracle.mac_oracle.mac_network at fp64 with autograd, on the same parameters, inputs and hash_mask_fn masks; the
loss is written once for both sides (tests/state_grads_ref.aux_loss).  Tolerances are tests/test_gpu_cell.py's (FWD_TOL, GRAD_TOL),
per tensor, relative to the tensor's largest reference entry.  tests/test_state_grads_host.py shows that the single-output
reference gradients are far above rel_err's floor.

1  one test per single output (d_memory = d_control = None): every input gradient and every parameter gradient
2  every map of every step + both histories + the final state at once, on the shapes that select the backward pass's routes
3  exactness: NULL struct / struct of NULLs == macx_cell_backward; zero gradients == none; per-step loop == run(); phases 1 + 2 == one call
4  kb_lengths: what the incoming att_kb gradient holds in the padded cells does not reach any gradient
5  d_att_self / d_att_gate for a cell without the option: MACX_EINVAL
6  the generic path agrees (a loss on att_kb against the oracle)
7  MACNet: CE + 0.1 * attention loss through net.last_cell == the modules composed by hand, != CE alone
"""
import ctypes as C

import pytest
import torch

from oracle import mac_oracle as mo
from helpers import make_case, rel_err
import abi_kit
import state_grads_ref as sr

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5     # tests/test_gpu_cell.py
GRAD_TOL = 2e-4


def _build(macx, dev, cfg, vq, words, lengths, kb, seed=5, gemm=None, kb_lengths=None, gen_seed=5, train=True):
    """tests/test_gpu_cell.py::build_cell with gemm= and kb_lengths= (non-zero biases, inputs that take gradients)"""
    p = cfg.netLength
    params = macx.MACCellParams(cfg, p, generator=torch.Generator().manual_seed(gen_seed)).to(dev)
    g = torch.Generator().manual_seed(gen_seed + 1)
    with torch.no_grad():
        for f in params.fields:
            t = getattr(params, f)
            if f.endswith("_b"):
                t.copy_((torch.rand(t.shape, generator=g) - 0.5) * 0.2)
    vqd, wd, kbd = [t.to(dev).requires_grad_(True) for t in (vq, words, kb)]
    kw = {}
    if gemm is not None:
        kw["gemm"] = gemm
    if kb_lengths is not None:
        kw["kb_lengths"] = torch.as_tensor(kb_lengths, dtype=torch.int64).to(dev)
    cell = macx.MACCell(vecQuestions=vqd, questionWords=wd, questionCntxWords=wd, questionLengths=lengths.to(dev),
                        knowledgeBase=kbd, memoryDropout=cfg.memoryDropout, readDropout=cfg.readDropout,
                        writeDropout=cfg.writeDropout, batchSize=vq.shape[0], train=train, config=cfg, params=params,
                        seed=seed, **kw)
    return cell, params, (vqd, wd, kbd)


def _grad_errors(macx, cfg, p, params, inputs, ref):
    """{tensor: error} of every input gradient and every parameter gradient against the oracle's (a gradient the oracle does not
    have -- the loss does not reach that tensor -- is a zero)"""
    zero_if_none = lambda g, like: torch.zeros_like(like) if g is None else g
    errs = {}
    for n, got, want in zip(("vecQuestions", "words", "knowledgeBase"), inputs, ref["inputs"]):
        assert got.grad is not None, n
        errs[n] = rel_err(got.grad, zero_if_none(want.grad, want))
    names = macx.params.reference_names(cfg, p)
    for f in params.fields:
        gt = getattr(params, f).grad
        assert gt is not None, f
        for refname, idx in names[f]:
            rg = zero_if_none(ref["params"][refname].grad, ref["params"][refname])
            got = gt if idx is None else gt[idx]
            # d/d(logit bias) of a softmax is analytically zero: compare absolutely (tests/test_gpu_cell.py)
            floor = 5e-2 if refname.endswith("linearLayerlogits/biases/bias") else 1e-6
            errs[refname] = rel_err(got.reshape(rg.shape), rg, floor=floor)
    return errs


def _parity(macx, dev, name, B, S, N, d, p, targets, gemm=None, expect="MACCell", tag=""):
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    cell, params, inputs = _build(macx, dev, cfg, vq, words, lengths, kb, gemm=gemm)
    assert type(cell).__name__ == expect
    state = cell.run()
    tg = targets(cfg) if callable(targets) else targets
    Gs = sr.incoming(tg, B, S, N, d, p)
    sr.aux_loss(cell, state, Gs, lambda G: G.to(dev)).backward()
    torch.cuda.synchronize()
    ref = sr.oracle_aux(cfg, params.to_reference_dict(), vq, words, lengths, kb, Gs, train=True, seed=5)
    fwd = {"memory": rel_err(state.memory, ref["memory"]), "control": rel_err(state.control, ref["control"]),
           "controls": rel_err(cell.controls, ref["cell"].controls), "memories": rel_err(cell.memories, ref["cell"].memories)}
    errs = _grad_errors(macx, cfg, p, params, inputs, ref)
    worst = max(errs, key=errs.get)
    print("\nSTATEGRAD %s%s B%d S%d N%d d%d p%d %s: fwd %.2e grad %.2e (%s)"
          % (tag, name, B, S, N, d, p, gemm or "h2", max(fwd.values()), errs[worst], worst))
    bad = {k: v for k, v in fwd.items() if not v < FWD_TOL}
    bad.update({k: v for k, v in errs.items() if not v < GRAD_TOL})
    assert not bad, bad
    if hasattr(cell, "status"):
        assert cell.status() == (0, -1)
    return errs, ref


# ================================================= 1 ===============================================================================
@pytest.mark.parametrize("kind,idx,name", sr.SINGLE_CASES)
def test_single_output_loss_matches_oracle(macx, dev, kind, idx, name):
    sh = sr.SINGLE_SHAPE
    _, ref = _parity(macx, dev, name, sh["B"], sh["S"], sh["N"], sh["d"], sr.steps_of(name), [(kind, idx)],
                     tag="%s[%d] " % (kind, idx))
    for n, x in zip(("vecQuestions", "words", "knowledgeBase"), ref["inputs"]):       # not a comparison of zeros
        if n in sr.REACHED[kind]:
            assert float(x.grad.abs().max()) > 1e-4, n


# ================================================= 2 ===============================================================================
@pytest.mark.parametrize("name,B,S,N,d,p,gemm", [
    ("args", 3, 9, 49, 128, 3, None),            # H2 below the chain width
    ("args", 3, 9, 196, 512, 2, None),           # chain kernels, 16-row tiles
    ("args", 24, 7, 196, 512, 2, None),          # 32-row tiles, dy summed by the linear
    ("args1", 5, 7, 49, 512, 3, None),           # recurrent control, dc inside the loop
    ("args3", 3, 9, 49, 128, 4, None),           # self attention
    ("args4", 3, 9, 49, 128, 3, None),           # gate
    ("args", 2, 7, 30, 128, 18, None),           # more than 16 steps
    ("args", 2, 5, 20, 128, 1, None),            # a single step
    ("args1", 3, 9, 49, 128, 3, "native"),       # native f32 GEMM family
    ("args4", 3, 9, 49, 128, 3, "split"),        # split GEMM family
])
def test_everything_at_once_matches_oracle(macx, dev, name, B, S, N, d, p, gemm):
    _parity(macx, dev, name, B, S, N, d, p, lambda cfg: sr.all_targets(cfg, p), gemm=gemm, tag="all ")


def test_everything_at_once_padded_cell(macx, dev):
    """memDim = 136 runs 256 wide on zero-padded weights (PaddedMACCell); the states, the histories and the gate come back 136 wide
    by ordinary slicing, which carries the gradient"""
    B, S, N, d, p = 3, 9, 49, 136, 3
    _parity(macx, dev, "args4", B, S, N, d, p, lambda cfg: sr.all_targets(cfg, p), expect="PaddedMACCell", tag="all padded ")


# ================================================= 3 ===============================================================================
def _all_grads(grads, gi):
    return [grads[f] for f in sorted(grads)] + list(gi)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _zero_state_grads(run, dev):
    names = ["d_" + s for s in ("controls", "memories", "att_question", "att_kb")]
    if run.opts.write_self_att:
        names.append("d_att_self")
    if run.opts.write_gate:
        names.append("d_att_gate")
    shapes = run.state_grad_shapes()
    return {n: torch.zeros(shapes[n], device=dev) for n in names}


@pytest.mark.parametrize("name,B,S,N,d,p", [("args", 3, 9, 49, 128, 3), ("args", 3, 9, 196, 512, 2), ("args1", 3, 9, 49, 128, 3),
                                            ("args3", 3, 9, 49, 128, 4), ("args4", 3, 9, 49, 128, 3)])
def test_null_struct_and_zero_gradients_are_the_plain_backward(macx, dev, name, B, S, N, d, p):
    """macx_cell_backward_x through ctypes with a NULL struct and with a struct of NULLs: bit for bit macx_cell_backward.  Explicit
    all-zero gradients for every field: torch.equal to none at all."""
    L = macx._lib.lib()
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    cell, params, _ = _build(macx, dev, cfg, vq, words, lengths, kb)
    cell.run()
    run = cell._run
    g = torch.Generator().manual_seed(9)
    dmem, dctl = (torch.randn(B, d, generator=g) / B).to(dev), (torch.randn(B, d, generator=g) / B).to(dev)
    stream = abi_kit.stream(dev)

    def call(fn, *extra):
        args, grads, gi, flat, keep = run.backward_begin(dctl, dmem)
        assert args[-1] is None                                               # no state gradient: a NULL struct
        macx._lib.check(fn(*args[:-1], *extra, stream), "backward")
        torch.cuda.synchronize()
        return _all_grads(grads, gi)

    plain = call(L.macx_cell_backward)
    assert _same(call(L.macx_cell_backward_x, None), plain)
    nulls = macx._lib.MacxStateGrads()
    assert _same(call(L.macx_cell_backward_x, C.byref(nulls)), plain)
    assert _same(call(L.macx_cell_backward_phase_x, None, 0), plain)
    # the Python route: None and explicit zeros
    grads, gvq, gw, gkb = run.backward(dctl, dmem)
    torch.cuda.synchronize()
    assert _same(_all_grads(grads, (gvq, gw, gkb)), plain)
    grads, gvq, gw, gkb = run.backward(dctl, dmem, _zero_state_grads(run, dev))
    torch.cuda.synchronize()
    assert _same(_all_grads(grads, (gvq, gw, gkb)), plain)


@pytest.mark.parametrize("name,B,S,N,d,p", [("args", 3, 9, 49, 128, 3), ("args1", 3, 9, 196, 512, 2), ("args3", 3, 9, 49, 128, 4)])
def test_phases_with_struct_are_the_single_call(macx, dev, name, B, S, N, d, p):
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    cell, params, _ = _build(macx, dev, cfg, vq, words, lengths, kb)
    cell.run()
    run = cell._run
    L = macx._lib.lib()
    g = torch.Generator().manual_seed(4)
    dmem = (torch.randn(B, d, generator=g) / B).to(dev)
    sg = {k: torch.randn(v.shape, generator=g).to(dev) / B for k, v in _zero_state_grads(run, dev).items()}
    stream = abi_kit.stream(dev)
    args, grads, gi, flat, keep = run.backward_begin(None, dmem, sg)
    assert args[-1] is not None
    macx._lib.check(L.macx_cell_backward_x(*args, stream), "macx_cell_backward_x")
    torch.cuda.synchronize()
    one = _all_grads(grads, gi)
    args, grads, gi, flat, keep = run.backward_begin(None, dmem, sg)
    run.backward_phase(args, 1)
    run.backward_phase(args, 2)
    torch.cuda.synchronize()
    assert _same(_all_grads(grads, gi), one)
    # ... and the struct arrived: not the plain call's gradients
    args, grads, gi, flat, keep = run.backward_begin(None, dmem)
    macx._lib.check(L.macx_cell_backward_x(*args, stream), "macx_cell_backward_x")
    torch.cuda.synchronize()
    assert not _same(_all_grads(grads, gi), one)


@pytest.mark.parametrize("name,B,S,N,d,p", [("args", 3, 9, 49, 128, 3), ("args3", 3, 9, 49, 128, 4), ("args1", 3, 9, 196, 512, 2)])
def test_stepwise_loop_with_auxiliary_loss_is_run(macx, dev, name, B, S, N, d, p):
    """the loop of model.py:453-458 and then a loss on the maps and the histories: bit for bit run() + the same loss.  The entries
    the earlier steps published are replaced at the last step; one fetched before it is a constant."""
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    Gs = sr.incoming(sr.all_targets(cfg, p), B, S, N, d, p)
    results = []
    for mode in ("loop", "run"):
        cell, params, inputs = _build(macx, dev, cfg, vq, words, lengths, kb)
        if mode == "loop":
            state = cell.zero_state(B)
            for i in range(p):
                cell.iteration = i
                _, state = cell(cell.none, state)
                if i == 0 and p > 1:
                    early = cell.attentions["kb"][0]
                    assert not early.requires_grad                          # fetched before the last step: a constant
            assert len(cell.attentions["kb"]) == p and len(cell.attentions["question"]) == p
        else:
            state = cell.run()
        assert all(a.requires_grad for a in cell.attentions["kb"] + cell.attentions["question"])
        assert cell.controls.requires_grad and cell.memories.requires_grad and not cell.infos.requires_grad
        sr.aux_loss(cell, state, Gs, lambda G: G.to(dev)).backward()
        torch.cuda.synchronize()
        results.append([t.grad for t in inputs] + [t.grad for t in params.tensors()])
    assert _same(results[0], results[1])


def test_no_grad_publishes_constants(macx, dev):
    cfg, vq, words, lengths, kb = make_case("args", 2, 5, 20, 128, 2)
    cell, params, _ = _build(macx, dev, cfg, vq, words, lengths, kb)
    with torch.no_grad():
        cell.run()
    assert not cell.attentions["kb"][0].requires_grad and not cell.controls.requires_grad
    with pytest.raises(RuntimeError, match="does not require grad"):
        cell.attentions["kb"][0].sum().backward()


@pytest.mark.parametrize("train", [False, True])
def test_maps_follow_the_final_state_and_are_dropped_after_backward(macx, dev, train):
    """What decides is whether the run keeps its activations, as for the final state: train=False only sets every dropout to keep
    1.0 (an evaluation-mode cell whose inputs take gradients has always returned a differentiable final state, and now differentiable
    maps with it); nothing that takes a gradient -> constants.  Once backward() has run the cell publishes plain views again, so a
    kept cell does not keep the finished autograd graph alive."""
    cfg, vq, words, lengths, kb = make_case("args", 2, 5, 20, 128, 2)
    cell, params, inputs = _build(macx, dev, cfg, vq, words, lengths, kb, train=train)
    state = cell.run()
    assert state.memory.requires_grad and cell.attentions["kb"][0].requires_grad and cell.memories.requires_grad
    lists = {k: v for k, v in cell.attentions.items()}
    fetched = cell.attentions["kb"][1]
    (state.memory.sum() + fetched.sum() * 2).backward()
    torch.cuda.synchronize()
    assert inputs[2].grad is not None and bool(torch.isfinite(inputs[2].grad).all())
    assert all(cell.attentions[k] is lists[k] for k in lists)                     # the same lists, entries replaced
    assert len(cell.attentions["kb"]) == 2 and not cell.attentions["kb"][1].requires_grad and not cell.controls.requires_grad
    assert torch.equal(cell.attentions["kb"][1], fetched.detach())
    for t in params.tensors() + list(inputs):                                     # nothing takes a gradient: constants
        t.requires_grad_(False)
    frozen = macx.MACCell(vecQuestions=inputs[0], questionWords=inputs[1], questionCntxWords=inputs[1], questionLengths=lengths.to(dev),
                          knowledgeBase=inputs[2], memoryDropout=cfg.memoryDropout, readDropout=cfg.readDropout,
                          writeDropout=cfg.writeDropout, batchSize=2, train=train, config=cfg, params=params, seed=5)
    st = frozen.run()
    assert not st.memory.requires_grad and not frozen.attentions["kb"][0].requires_grad and not frozen.memories.requires_grad


def test_misaligned_final_gradient_with_history_gradients(macx, dev):
    """A d_memory / d_control that is not 16-byte aligned takes the backward pass's other start (fills and copies instead of the one
    init launch); with gradients for the histories that route copies them and adds the final state's gradient.  Bit for bit the
    aligned call's gradients."""
    name, B, S, N, d, p = "args", 3, 9, 49, 128, 3
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    cell, params, _ = _build(macx, dev, cfg, vq, words, lengths, kb)
    cell.run()
    run = cell._run
    g = torch.Generator().manual_seed(3)
    buf_m, buf_c = torch.randn(B * d + 4, generator=g).to(dev) / B, torch.randn(B * d + 4, generator=g).to(dev) / B
    sg = {k: torch.randn(run.state_grad_shapes()[k], generator=g).to(dev) / B for k in ("d_memories", "d_controls")}
    results = []
    for off in (0, 1):                                                            # 1 float = 4 bytes off a 16-byte boundary
        dm, dc = buf_m[off: off + B * d].view(B, d), buf_c[off: off + B * d].view(B, d)
        if off:
            dm.copy_(buf_m[:B * d].view(B, d).clone()); dc.copy_(buf_c[:B * d].view(B, d).clone())
            assert dm.data_ptr() % 16 == 4 and dm.is_contiguous()
        for state_grads in (sg, None, {"d_memories": sg["d_memories"]}):
            grads, gvq, gw, gkb = run.backward(dc, dm, state_grads)
            torch.cuda.synchronize()
            results.append(_all_grads(grads, (gvq, gw, gkb)))
    for aligned, shifted in zip(results[:3], results[3:]):
        assert _same(aligned, shifted)
    assert not _same(results[0], results[1]) and not _same(results[0], results[2])


# ================================================= 4 ===============================================================================
@pytest.mark.parametrize("name,B,S,N,d,p,kb_lengths", [("args", 3, 9, 49, 128, 2, [49, 1, 23]),
                                                       ("args", 3, 9, 196, 512, 2, [196, 1, 77])])     # 77: inside a 16-row tile
def test_kb_lengths_padded_cells_of_the_incoming_gradient(macx, dev, name, B, S, N, d, p, kb_lengths):
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    for b, n in enumerate(kb_lengths):
        kb[b, n:] = 0.0
    g = torch.Generator().manual_seed(12)
    G_junk = torch.randn(p, B, N, generator=g)
    G_zero = G_junk.clone()
    for b, n in enumerate(kb_lengths):
        G_junk[:, b, n:] = 1e3 * torch.randn(p, N - n, generator=g)
        G_zero[:, b, n:] = 0.0
    dmem = torch.randn(B, d, generator=g) / B
    results = []
    for G in (G_zero, G_junk):
        cell, params, inputs = _build(macx, dev, cfg, vq, words, lengths, kb, kb_lengths=kb_lengths)
        state = cell.run()
        loss = (state.memory * dmem.to(dev)).sum()
        for i in range(p):
            loss = loss + (cell.attentions["kb"][i] * G[i].to(dev)).sum()
        loss.backward()
        torch.cuda.synchronize()
        for b, n in enumerate(kb_lengths):
            assert bool((inputs[2].grad[b, n:] == 0).all()), "question %d: padded rows of knowledgeBase.grad are not 0" % b
        results.append([t.grad for t in inputs] + [t.grad for t in params.tensors()])
    assert all(bool(torch.isfinite(t).all()) for t in results[1])
    assert _same(results[0], results[1])


# ================================================= 5 ===============================================================================
def test_map_gradient_without_the_option_is_refused(macx, dev):
    L = macx._lib.lib()
    B, S, N, d, p = 2, 5, 20, 128, 2
    cfg, vq, words, lengths, kb = make_case("args", B, S, N, d, p)
    cell, params, _ = _build(macx, dev, cfg, vq, words, lengths, kb)
    cell.run()
    run = cell._run
    assert not run.opts.write_self_att and not run.opts.write_gate
    stream = abi_kit.stream(dev)
    junk = torch.zeros(p * B * d, device=dev)
    for field in ("d_att_self", "d_att_gate"):
        args, grads, gi, flat, keep = run.backward_begin(None, torch.ones(B, d, device=dev))
        for t in list(grads.values()) + list(gi):
            t.fill_(7.0)
        sg = macx._lib.MacxStateGrads()
        setattr(sg, field, junk.data_ptr())
        for fn, tail in ((L.macx_cell_backward_x, ()), (L.macx_cell_backward_phase_x, (1,))):
            assert fn(*args[:-1], C.byref(sg), *tail, stream) == macx._lib.MACX_EINVAL
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in list(grads.values()) + list(gi))       # nothing was launched
    with pytest.raises(KeyError):
        run.backward(None, None, {"d_infos": junk})
    with pytest.raises(ValueError, match="d_att_kb"):
        run.backward(None, None, {"d_att_kb": torch.zeros(p, B, N + 1, device=dev)})


# ================================================= 6 ===============================================================================
def test_generic_path_agrees(macx, dev):
    """an option set of the generic path (writeInputs = SUM with a gate): the same single-output loss on att_kb against the oracle"""
    from test_gpu_generic import make_cfg, oracle_params, run_generic, assert_grad
    B, S, N, d, p = 3, 7, 20, 128, 3
    cfg = make_cfg("write_sum", d, p)
    vq, words, lengths, kb = mo.synthetic_inputs(B, S, N, d, seed=11)
    params = oracle_params(cfg, vq, words, lengths, kb)
    Gs = sr.incoming([("att_kb", 1)], B, S, N, d, p)
    ref = sr.oracle_aux(cfg, params, vq, words, lengths, kb, Gs, train=True, seed=91, b0=1)
    cell, gp, inputs = run_generic(macx, dev, cfg, params, vq, words, lengths, kb, True, 91, 1, True)
    assert isinstance(cell, macx.GenericMACCell)
    state = cell.run()
    sr.aux_loss(cell, state, Gs, lambda G: G.to(dev)).backward()
    torch.cuda.synchronize()
    grads = gp.grads_by_name()
    for k, v in ref["params"].items():
        if v.grad is None:
            assert grads[k] is None or float(grads[k].abs().max()) == 0.0, k
            continue
        assert_grad(grads[k], v.grad, k, GRAD_TOL)
    for n, got, want in zip(("vecQuestions", "words", "knowledgeBase"), inputs, ref["inputs"]):
        assert want.grad is not None and float(want.grad.abs().max()) > 1e-4, n
        assert rel_err(got.grad, want.grad) < GRAD_TOL, n


# ================================================= 7 ===============================================================================
@pytest.mark.parametrize("stem", ["fused", "generic"])
def test_macnet_auxiliary_loss_through_last_cell(macx, dev, stem):
    """CE + 0.1 * sum_i (last_cell.attentions["kb"][i] * G_i).sum(): gradients into the stem, the encoder and the images are bit for bit
    those of encoder -> stem -> MACCell -> output unit composed by hand, and not those of CE alone.  The fused stem treats the image
    features as data (no gradient, with or without the loss); the generic stem (here: kernel sizes 3, 1) differentiates them."""
    B, H, W, Cin, d, p, S, A, V, E = 3, 4, 3, 128, 128, 2, 6, 7, 12, 20
    N = H * W
    cfg = mo.flag_file_config("args", netLength=p, memDim=d, ctrlDim=d, attDim=d, encDim=d, wrdEmbDim=E, outClassifierDims=[32],
                              answerWordsNum=A)
    cfg.stemDim = 128
    if stem == "generic":
        cfg.stemKernelSizes = [3, 1]
    net = macx.MACNet(cfg, vocab=V, H=H, W=W, imageInDim=Cin, answerWordsNum=A, generator=torch.Generator().manual_seed(4)).to(dev)
    assert isinstance(net.stem, macx.GenericStem) == (stem == "generic")
    g = torch.Generator().manual_seed(6)
    img0 = torch.relu(torch.randn(B, N, Cin, generator=g))
    lengths = torch.tensor([S, 2, 4], dtype=torch.int32)
    q = torch.randint(1, V + 1, (B, S), generator=g, dtype=torch.int32)
    q = (q * (torch.arange(S).unsqueeze(0) < lengths.unsqueeze(1)).to(torch.int32)).to(dev)
    lengths = lengths.to(dev)
    answers = torch.randint(0, A, (B,), generator=g).to(dev)
    G = torch.randn(p, B, N, generator=g).to(dev)
    tensors = [t for t in net.stem.tensors() + net.enc.tensors() if t.requires_grad]      # (the flag file may fix the embeddings)
    assert len(tensors) >= 6

    def grads_of(forward, lam):
        for t in net.tensors():
            t.grad = None
        img = img0.to(dev).requires_grad_(True)
        logits, cell = forward(img)
        loss, _ = net.loss_and_pred(logits, answers)
        if lam:
            loss = loss + lam * sum((cell.attentions["kb"][i] * G[i]).sum() for i in range(p))
        loss.backward()
        torch.cuda.synchronize()
        assert (img.grad is not None) == (stem == "generic")
        return [t.grad.clone() for t in tensors] + ([img.grad.clone()] if stem == "generic" else [])

    def whole(img):
        logits = net(img, q, lengths, train=True, seed=21)
        return logits, net.last_cell

    def by_hand(img):
        words, vecQ = net.enc(q, lengths, train=True, seed=21, b0=0, check_ids=True)
        kb = net.stem(img, train=True, seed=21, b0=0)
        cell = macx.MACCell(vecQuestions=vecQ, questionWords=words, questionCntxWords=words, questionLengths=lengths, knowledgeBase=kb,
                            memoryDropout=cfg.memoryDropout, readDropout=cfg.readDropout, writeDropout=cfg.writeDropout, batchSize=B,
                            train=True, config=cfg, params=net.cell, netLength=p, seed=21, b0=0)
        return net.out(cell.run().memory, vecQ, train=True, seed=21, b0=0), cell

    aux = grads_of(whole, 0.1)
    assert _same(aux, grads_of(by_hand, 0.1))
    ce = grads_of(whole, 0.0)
    assert not any(torch.equal(a, b) for a, b in zip(aux, ce))
