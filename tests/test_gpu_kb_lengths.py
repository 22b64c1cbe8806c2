"""-m gpu: per-question knowledge-base sizes (kb_lengths) from the attention kernel to the tower.

The reference is the fp64 oracle with ops.expMask in front of the read unit's softmax (tests/kb_lengths_ref.py, itself checked
against the unpatched oracle on the cut knowledge base by tests/test_kb_lengths_host.py).  Tolerances are those of
tests/test_gpu_cell.py (FWD_TOL 2e-5, GRAD_TOL 2e-4, attention 2e-6 absolute) and, for the kernel on its own, of
tests/test_gpu_units.py::test_kb_attend_unit_forward_and_backward (1e-5 of the largest reference entry).

T0  a zero row in a contraction over rows: macx_wgrad in families 0 and 2 on gradients of size 1e-6 with one all-zero row
T1  macx_kb_attend_fwd_l on its own: NaN in every padded logit and row, exact zeros, clamped lengths, NULL == macx_kb_attend_fwd
T2  kb_lengths = full(N) is bit for bit the cell without kb_lengths
T3  forward + every gradient against the masked oracle: H2 below and on the chain kernels, recurrent control, self attention, gate,
    more than 16 steps, the split and native families
T4  the same on PaddedMACCell (d = 200) and on the generic path (the reference's default option set)
T5  what the padded rows hold (zeros against 1e3 N(0,1)) does not reach the forward pass; gradients agree within GRAD_TOL
T6  MACNet.forward(kb_lengths=) is encoder -> stem -> MACCell(kb_lengths=) -> output unit, bit for bit; range, shape, device errors
"""
import pytest
import torch

from abi_kit import bits, ptr
from oracle import mac_oracle as mo
from helpers import make_case, oracle_run, rel_err, max_abs, default_gemm_mode
from kb_lengths_ref import masked_kb_attention

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-5     # tests/test_gpu_cell.py
GRAD_TOL = 2e-4
ATT_TOL = 2e-6


# ================================================= T0 ==============================================================================
@pytest.mark.parametrize("zero_in", ["G", "A"])
@pytest.mark.parametrize("M", [65, 257])
def test_t0_zero_row_in_a_contraction(macx, dev, M, zero_in):
    """C = A^T G with A ~ N(0,1), G ~ 1e-6 N(0,1) and one all-zero row in G (then in A): the H2 family (2) within
    1.5 x family 0's err / S + 2^-23, maximum and mean -- the bound of test_gpu_gemm_exports.py::test_wgrad_three_families.

    What it can and cannot show: macx_wgrad takes fp32 operands, and in family 2 it runs the split-bf16 kernel (wgrad_any), which
    has no per-row exponents -- so this passes with either zero-block exponent (before the change to h2_exponent, on an MI355X:
    family 2 err / S 1.57e-07 / 1.71e-07 / 7.3e-08 / 5.8e-08 against family 0's 9.0e-08 / 1.07e-07 / 5.0e-08 / 5.7e-08).  The
    contractions that do bring rows to a common exponent (wgrad_h2_kernel, sb_h2_kernel, sb_h2w_kernel) run on their own, zero
    rows included, in test_gpu_h2_contractions.py (macx_h2_wgrad / macx_h2_sb, every element against fp64 within a derived
    bound); T3 and T5 below run them through the cell, and those are the tests that fail with exponent 0 for a zero block
    (dWx wrong by 1.0 of its largest entry, dW2 by 0.15 .. 0.62, dW1 by 0.03 .. 0.22; the split and native families pass)."""
    L = macx._lib.lib()
    Kd, Jd = 128, 256
    g = torch.Generator().manual_seed(M * 17 + (zero_in == "A"))
    A = torch.randn(M, Kd, generator=g)
    G = torch.randn(M, Jd, generator=g) * 1e-6
    (G if zero_in == "G" else A)[M // 2] = 0.0
    ref = A.double().t() @ G.double()
    S = A.double().abs().t() @ G.double().abs()
    assert bool((S > 0).all())
    Ad, Gd = A.to(dev), G.to(dev)
    stats = {}
    try:
        for mode in (0, 2):
            L.macx_gemm_mode(mode)
            ns = L.macx_wgrad_splits(M, Kd, Jd)
            out = torch.empty(Kd, Jd, device=dev)
            ws = torch.empty(ns * Kd * Jd, device=dev)
            macx._lib.check(L.macx_wgrad(ptr(Ad), Kd, ptr(Gd), Jd, M, Kd, Jd, ptr(out), ptr(ws), None), "wgrad")
            torch.cuda.synchronize()
            e = (out.cpu().double() - ref).abs() / S
            stats[mode] = (float(e.max()), float(e.mean()))
    finally:
        L.macx_gemm_mode(default_gemm_mode())
    (m0, a0), (m2, a2) = stats[0], stats[2]
    print("\nKBLEN T0 M=%d zero row in %s: err/S max (mean) family 0 %.3e (%.3e) | family 2 %.3e (%.3e)" % (M, zero_in, m0, a0, m2, a2))
    assert m2 <= 1.5 * m0 + 2.0 ** -23, (m2, m0)
    assert a2 <= 1.5 * a0 + 2.0 ** -23, (a2, a0)


# ================================================= T1 ==============================================================================
@pytest.mark.parametrize("B,N,d,lengths", [
    (3, 49, 128, [49, 1, 23]),
    (2, 300, 256, [300, 1]),           # N > 256: rows past the prefetch window
    (2, 300, 256, [270, 257]),         # ... with the boundary inside the streamed tail
    (2, 300, 256, [0, 400]),           # out of range: clamped to [1, N]
    (1, 1, 128, [1]),
])
def test_t1_kb_attend_kernel_with_lengths(macx, dev, B, N, d, lengths):
    L = macx._lib.lib()
    g = torch.Generator().manual_seed(B * 1000 + N + lengths[0])
    logits = torch.randn(B, N, generator=g) * 3
    kb = torch.randn(B, N, d, generator=g)
    bias = torch.tensor([0.3])
    live = [min(max(v, 1), N) for v in lengths]
    att_ref = torch.zeros(B, N, dtype=torch.float64)
    info_ref = torch.zeros(B, d, dtype=torch.float64)
    for b, n in enumerate(live):
        att_ref[b, :n] = torch.softmax(logits[b, :n].double() + 0.3, dim=-1)
        info_ref[b] = (att_ref[b, :n].unsqueeze(-1) * kb[b, :n].double()).sum(0)
    lo_nan, kb_nan = logits.clone(), kb.clone()
    for b, n in enumerate(live):
        lo_nan[b, n:] = float("nan")
        kb_nan[b, n:] = float("nan")
    lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
    bi = bias.to(dev)
    rel = lambda a, r: float((a.cpu().double() - r).abs().max() / max(float(r.abs().max()), 1e-6))

    def run(lo, kbt, ln):
        lo, kbt = lo.to(dev), kbt.to(dev)
        att, info = torch.full((B, N), 7.0, device=dev), torch.full((B, d), 7.0, device=dev)
        if ln is False:
            macx._lib.check(L.macx_kb_attend_fwd(B, N, d, ptr(lo), ptr(bi), ptr(kbt), ptr(att), ptr(info), None), "fwd")
        else:
            macx._lib.check(L.macx_kb_attend_fwd_l(B, N, d, ptr(lo), ptr(bi), ptr(kbt), ptr(ln), ptr(att), ptr(info), None), "fwd_l")
        torch.cuda.synchronize()
        return att, info

    att, info = run(lo_nan, kb_nan, lens)
    assert torch.isfinite(att).all() and torch.isfinite(info).all()
    assert rel(att, att_ref) < 1e-5 and rel(info, info_ref) < 1e-5
    for b, n in enumerate(live):
        assert bool((bits(att[b, n:]) == 0).all()), "padded attention of question %d is not +0.0" % b
    # the padding's content is not an input: the clean tensors give the same bits
    att2, info2 = run(logits, kb, lens)
    assert torch.equal(bits(att), bits(att2)) and torch.equal(bits(info), bits(info2))
    # every length N, and no lengths at all (NULL), are macx_kb_attend_fwd bit for bit
    plain = run(logits, kb, False)
    for ln in (torch.full((B,), N, dtype=torch.int32, device=dev), None):
        full = run(logits, kb, ln)
        assert torch.equal(bits(full[0]), bits(plain[0])) and torch.equal(bits(full[1]), bits(plain[1]))
    assert L.macx_kb_attend_fwd_l(B, 1025, d, ptr(logits.to(dev)), ptr(bi), ptr(kb.to(dev)), ptr(lens), ptr(att), ptr(info), None) == macx._lib.MACX_EINVAL


# ================================================= cells ===========================================================================
def _build(macx, dev, cfg, vq, words, lengths, kb, train, kb_lengths, seed=5, gemm=None, gen_seed=5):
    """tests/test_gpu_cell.py::build_cell with kb_lengths= and gemm= (non-zero biases, inputs that take gradients)"""
    p = cfg.netLength
    params = macx.MACCellParams(cfg, p, generator=torch.Generator().manual_seed(gen_seed)).to(dev)
    g = torch.Generator().manual_seed(gen_seed + 1)
    with torch.no_grad():
        for f in params.fields:
            t = getattr(params, f)
            if f.endswith("_b"):
                t.copy_((torch.rand(t.shape, generator=g) - 0.5) * 0.2)
    vqd, wd, kbd = [t.to(dev).requires_grad_(True) for t in (vq, words, kb)]
    kw = {} if kb_lengths is None else {"kb_lengths": torch.as_tensor(kb_lengths, dtype=torch.int64).to(dev)}
    if gemm is not None:
        kw["gemm"] = gemm
    cell = macx.MACCell(vecQuestions=vqd, questionWords=wd, questionCntxWords=wd, questionLengths=lengths.to(dev),
                        knowledgeBase=kbd, memoryDropout=cfg.memoryDropout, readDropout=cfg.readDropout,
                        writeDropout=cfg.writeDropout, batchSize=vq.shape[0], train=train, config=cfg, params=params,
                        seed=seed, **kw)
    return cell, params, (vqd, wd, kbd)


def _seeds(B, d):
    g = torch.Generator().manual_seed(9)
    return torch.randn(B, d, generator=g) / B, torch.randn(B, d, generator=g) / B


def _run(cell, dmem, dctl, dev):
    state = cell.run()
    ((state.memory * dmem.to(dev)).sum() + (state.control * dctl.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    return state


def _zero_padding(kb, kb_lengths):
    kb = kb.clone()
    for b, n in enumerate(kb_lengths):
        kb[b, n:] = 0.0
    return kb


def _check_mask(cell, kbd, kb_lengths, p):
    """attention rows sum to 1 (1e-5), masked attention is exactly 0, padded knowledge-base rows get a gradient of exactly 0"""
    B = len(kb_lengths)
    for i in range(p):
        a = cell.attentions["kb"][i]
        assert float(a.min()) >= 0 and max_abs(a.sum(-1), torch.ones(B)) < 1e-5
        for b, n in enumerate(kb_lengths):
            assert bool((a[b, n:] == 0).all()), "step %d: question %d attends to its padding" % (i, b)
    for b, n in enumerate(kb_lengths):
        assert bool((kbd.grad[b, n:] == 0).all()), "question %d: padded rows of knowledgeBase.grad are not 0" % b


def _masked_parity(macx, dev, name, B, S, N, d, p, train, kb_lengths, gemm=None, expect=None):
    assert len(kb_lengths) == B and N in kb_lengths and 1 in kb_lengths and any(v % 16 for v in kb_lengths)
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    kb = _zero_padding(kb, kb_lengths)
    dmem, dctl = _seeds(B, d)
    cell, params, (vqd, wd, kbd) = _build(macx, dev, cfg, vq, words, lengths, kb, train, kb_lengths, gemm=gemm)
    if expect is not None:
        assert type(cell).__name__ == expect
    state = _run(cell, dmem, dctl, dev)
    with masked_kb_attention(kb_lengths, N):
        ref = oracle_run(cfg, params.to_reference_dict(), vq, words, lengths, kb, train=train, seed=5, need_grad=True,
                         d_memory=dmem, d_control=dctl)
    rc = ref["cell"]
    errs = {"memory": rel_err(state.memory, ref["memory"]), "control": rel_err(state.control, ref["control"]),
            "memories": rel_err(cell.memories, rc.memories), "infos": rel_err(cell.infos, rc.infos)}
    att = max(max(max_abs(cell.attentions[k][i], rc.attentions[k][i]) for i in range(p)) for k in ("kb", "question"))
    rvq, rwords, rkb = ref["inputs"]
    gerrs = {"vecQuestions": rel_err(vqd.grad, rvq.grad), "words": rel_err(wd.grad, rwords.grad),
             "knowledgeBase": rel_err(kbd.grad, rkb.grad)}
    names = macx.params.reference_names(cfg, p)
    for f in params.fields:
        gt = getattr(params, f).grad
        assert gt is not None, f
        for refname, idx in names[f]:
            rg = ref["params"][refname].grad
            got = gt if idx is None else gt[idx]
            floor = 5e-2 if refname.endswith("linearLayerlogits/biases/bias") else 1e-6      # analytically zero: absolute
            gerrs[refname] = rel_err(got.reshape(rg.shape), rg, floor=floor)
    print("\nKBLEN parity %s B%d S%d N%d d%d p%d %s lengths %s: fwd %.2e att %.2e grad %.2e (%s)"
          % (name, B, S, N, d, p, gemm or "h2", kb_lengths, max(errs.values()), att, max(gerrs.values()), max(gerrs, key=gerrs.get)))
    bad = {k: v for k, v in errs.items() if not v < FWD_TOL}
    bad.update({k: v for k, v in gerrs.items() if not v < GRAD_TOL})
    assert not bad, bad
    assert att < ATT_TOL
    _check_mask(cell, kbd, kb_lengths, p)
    return cell


# ================================================= T2 ==============================================================================
@pytest.mark.parametrize("name,B,S,N,d,p", [("args", 3, 9, 49, 128, 2), ("args", 3, 9, 196, 512, 2)])
def test_t2_full_lengths_are_the_cell_without_lengths(macx, dev, name, B, S, N, d, p):
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    dmem, dctl = _seeds(B, d)
    runs = []
    for kl in (None, [N] * B):
        cell, params, inputs = _build(macx, dev, cfg, vq, words, lengths, kb, True, kl)
        runs.append((cell, _run(cell, dmem, dctl, dev), params, inputs))
    (c0, s0, p0, i0), (c1, s1, p1, i1) = runs
    assert torch.equal(bits(s0.memory), bits(s1.memory)) and torch.equal(bits(s0.control), bits(s1.control))
    for k in ("kb", "question"):
        for a, b in zip(c0.attentions[k], c1.attentions[k]):
            assert torch.equal(bits(a), bits(b)), k
    for a, b in zip(i0, i1):
        assert torch.equal(bits(a.grad), bits(b.grad))
    for f in p0.fields:
        assert torch.equal(bits(getattr(p0, f).grad), bits(getattr(p1, f).grad)), f


# ================================================= T3 ==============================================================================
@pytest.mark.parametrize("name,B,S,N,d,p,kb_lengths,gemm", [
    ("args", 3, 9, 49, 128, 3, [49, 1, 23], None),               # H2 below the chain width
    ("args", 3, 9, 196, 512, 2, [196, 1, 77], None),             # chain kernels, 16-row tiles, a boundary inside a tile, deferred S_b
    ("args1", 5, 7, 49, 512, 3, [49, 1, 23, 37, 16], None),      # recurrent control
    ("args3", 3, 9, 49, 128, 4, [23, 49, 1], None),              # self attention (not masked: its name is "selfAttention")
    ("args4", 3, 9, 49, 128, 3, [1, 30, 49], None),              # write gate
    ("args", 2, 7, 30, 128, 18, [30, 1], None),                  # more than 16 steps
    ("args", 3, 9, 49, 128, 3, [49, 1, 23], "split"),
    ("args", 3, 9, 49, 128, 3, [49, 1, 23], "native"),
])
def test_t3_masked_cell_matches_masked_oracle(macx, dev, name, B, S, N, d, p, kb_lengths, gemm):
    cell = _masked_parity(macx, dev, name, B, S, N, d, p, True, kb_lengths, gemm=gemm)
    assert cell.status() == (0, -1)


# ================================================= T4 ==============================================================================
def test_t4_padded_width_cell(macx, dev):
    """memDim = 200 runs 256 wide on zero-padded weights (PaddedMACCell): kb_lengths passes through"""
    _masked_parity(macx, dev, "args", 3, 9, 49, 200, 2, True, [49, 1, 23], expect="PaddedMACCell")


def test_t4_generic_path(macx, dev):
    """the reference's default option set ("defaults" of tests/test_gpu_generic.py): the plan's read-unit softmax takes the lengths"""
    from test_gpu_generic import make_cfg, oracle_params, assert_grad
    B, S, N, d, p = 3, 7, 20, 128, 3
    kb_lengths = [20, 1, 7]
    cfg = make_cfg("defaults", d, p)
    vq, words, lengths, kb = mo.synthetic_inputs(B, S, N, d, seed=11)
    kb = _zero_padding(kb, kb_lengths)
    params = oracle_params(cfg, vq, words, lengths, kb)
    g = torch.Generator().manual_seed(3)
    dM, dC = torch.randn(B, d, generator=g), torch.randn(B, d, generator=g)
    with masked_kb_attention(kb_lengths, N):
        ref = oracle_run(cfg, params, vq, words, lengths, kb, train=True, seed=91, b0=1, need_grad=True, d_memory=dM, d_control=dC)
    gp = macx.GenericParams(device=dev).load_reference_dict(params)
    vqd, wd, kbd = [t.to(dev).requires_grad_(True) for t in (vq, words, kb)]
    cell = macx.MACCell(vecQuestions=vqd, questionWords=wd, questionCntxWords=wd, questionLengths=lengths.to(dev),
                        knowledgeBase=kbd, memoryDropout=cfg.memoryDropout, readDropout=cfg.readDropout,
                        writeDropout=cfg.writeDropout, batchSize=B, train=True, config=cfg, params=gp, seed=91, b0=1,
                        kb_lengths=torch.tensor(kb_lengths, device=dev))
    assert isinstance(cell, macx.GenericMACCell)
    state = cell.run()
    ((state.memory * dM.to(dev)).sum() + (state.control * dC.to(dev)).sum()).backward()
    torch.cuda.synchronize()
    rc = ref["cell"]
    assert rel_err(state.memory, ref["memory"]) < FWD_TOL and rel_err(state.control, ref["control"]) < FWD_TOL
    assert rel_err(cell.memories, rc.memories) < FWD_TOL and rel_err(cell.infos, rc.infos) < FWD_TOL
    for kind in ("kb", "question"):
        for a, b in zip(cell.attentions[kind], rc.attentions[kind]):
            assert max_abs(a, b) < ATT_TOL
    grads = gp.grads_by_name()
    for k, v in ref["params"].items():
        if v.grad is None:
            assert grads[k] is None or float(grads[k].abs().max()) == 0.0, k
            continue
        assert_grad(grads[k], v.grad, k, GRAD_TOL)
    for name, got, want in zip(("vecQuestions", "words", "knowledgeBase"), (vqd, wd, kbd), ref["inputs"]):
        if want.grad is not None:
            assert rel_err(got.grad, want.grad) < GRAD_TOL, name
    _check_mask(cell, kbd, kb_lengths, p)


# ================================================= T5 ==============================================================================
@pytest.mark.parametrize("name,B,S,N,d,p,kb_lengths", [("args", 3, 9, 49, 128, 2, [49, 1, 23]), ("args", 3, 9, 196, 512, 2, [196, 1, 77])])
def test_t5_padding_content_does_not_matter(macx, dev, name, B, S, N, d, p, kb_lengths):
    cfg, vq, words, lengths, kb = make_case(name, B, S, N, d, p)
    junk = kb.clone()
    g = torch.Generator().manual_seed(12)
    for b, n in enumerate(kb_lengths):
        junk[b, n:] = 1e3 * torch.randn(N - n, d, generator=g)
    dmem, dctl = _seeds(B, d)
    runs = []
    for k in (_zero_padding(kb, kb_lengths), junk):
        cell, params, inputs = _build(macx, dev, cfg, vq, words, lengths, k, True, kb_lengths)
        runs.append((cell, _run(cell, dmem, dctl, dev), params, inputs))
    (c0, s0, p0, i0), (c1, s1, p1, i1) = runs
    assert torch.equal(bits(s0.memory), bits(s1.memory)) and torch.equal(bits(s0.control), bits(s1.control))
    for k in ("kb", "question"):
        for a, b in zip(c0.attentions[k], c1.attentions[k]):
            assert torch.equal(bits(a), bits(b)), k
    errs = {"input %d" % j: rel_err(b.grad, a.grad) for j, (a, b) in enumerate(zip(i0, i1))}
    for f in p0.fields:
        floor = 5e-2 if f in ("kbLogits_b", "ctrlLogits_b", "selfLogits_b") else 1e-6      # softmax logit biases: analytically zero
        errs[f] = rel_err(getattr(p1, f).grad, getattr(p0, f).grad, floor=floor)
    print("\nKBLEN T5 %s N%d d%d: largest gradient difference %.2e (%s)" % (name, N, d, max(errs.values()), max(errs, key=errs.get)))
    bad = {k: v for k, v in errs.items() if not v < GRAD_TOL}
    assert not bad, bad
    _check_mask(c1, i1[2], kb_lengths, p)


# ================================================= T6 ==============================================================================
def _tower(macx, dev):
    B, H, W, Cin, d, p, S, A, V, E = 3, 4, 3, 128, 128, 2, 6, 7, 12, 20
    cfg = mo.flag_file_config("args", netLength=p, memDim=d, ctrlDim=d, attDim=d, encDim=d, wrdEmbDim=E, outClassifierDims=[32],
                              answerWordsNum=A)
    cfg.stemDim = 128
    net = macx.MACNet(cfg, vocab=V, H=H, W=W, imageInDim=Cin, answerWordsNum=A, generator=torch.Generator().manual_seed(4)).to(dev)
    g = torch.Generator().manual_seed(6)
    img = torch.relu(torch.randn(B, H * W, Cin, generator=g)).to(dev)
    lengths = torch.tensor([S, 2, 4], dtype=torch.int32)
    q = torch.randint(1, V + 1, (B, S), generator=g, dtype=torch.int32)
    q = q * (torch.arange(S).unsqueeze(0) < lengths.unsqueeze(1)).to(torch.int32)
    return net, cfg, img, q.to(dev), lengths.to(dev), (B, H * W, d, p)


def test_t6_tower_passes_kb_lengths_to_the_cell(macx, dev):
    net, cfg, img, q, lengths, (B, N, d, p) = _tower(macx, dev)
    kl = torch.tensor([N, 1, 7], device=dev)
    with torch.no_grad():
        logits = net(img, q, lengths, train=True, seed=21, kb_lengths=kl)
        masked_cell = net.last_cell
        plain = net(img, q, lengths, train=True, seed=21)
        words, vecQ = net.enc(q, lengths, train=True, seed=21, b0=0, check_ids=True)
        kb = net.stem(img, train=True, seed=21, b0=0)
        cell = macx.MACCell(vecQuestions=vecQ, questionWords=words, questionCntxWords=words, questionLengths=lengths, knowledgeBase=kb,
                            memoryDropout=cfg.memoryDropout, readDropout=cfg.readDropout, writeDropout=cfg.writeDropout, batchSize=B,
                            train=True, config=cfg, params=net.cell, netLength=p, seed=21, b0=0, kb_lengths=kl)
        by_hand = net.out(cell.run().memory, vecQ, train=True, seed=21, b0=0)
    torch.cuda.synchronize()
    assert torch.equal(bits(logits), bits(by_hand))
    assert not torch.equal(bits(logits), bits(plain))                     # the lengths arrived
    assert torch.equal(bits(logits[0]), bits(plain[0]))                   # ... and question 0, all of whose cells are live, is unchanged
    for a in masked_cell.attentions["kb"]:
        assert bool((a[1, 1:] == 0).all()) and bool((a[2, 7:] == 0).all())


def test_t6_errors(macx, dev):
    net, cfg, img, q, lengths, (B, N, d, p) = _tower(macx, dev)
    for bad in ([N + 1, 1, 7], [N, 0, 7]):
        with pytest.raises(ValueError, match="kb_lengths"):
            net(img, q, lengths, train=False, kb_lengths=torch.tensor(bad, device=dev))
    with torch.no_grad():                                                   # unchecked: clamped by the kernel, no error
        net(img, q, lengths, train=False, check_ids=False, kb_lengths=torch.tensor([N + 1, 0, 7], device=dev))
    cfg2, vq, words, ql, kb = make_case("args", 3, 5, 20, 128, 1)
    args = lambda: dict(vecQuestions=vq.to(dev), questionWords=words.to(dev), questionCntxWords=words.to(dev), questionLengths=ql.to(dev),
                        knowledgeBase=kb.to(dev), memoryDropout=1.0, readDropout=1.0, writeDropout=1.0, batchSize=3, train=False, config=cfg2)
    with pytest.raises(ValueError, match="kb_lengths"):
        macx.MACCell(**args(), kb_lengths=torch.tensor([20, 1, 7, 3], device=dev))
    with pytest.raises(ValueError, match="kb_lengths"):
        macx.MACCell(**args(), kb_lengths=torch.tensor([[20, 1, 7]], device=dev))
    with pytest.raises(RuntimeError, match="no CPU path"):
        macx.MACCell(**args(), kb_lengths=torch.tensor([20, 1, 7]))
