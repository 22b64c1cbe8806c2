"""-m gpu: the fused stem (macx.Stem) at its tile edges, in all three kernel families, forward AND backward, against mo.stem_cnn in fp64.

Cases, data and metrics: stem_geometry_cases.py (the route every case takes is in its table and is held to the launch rules on the CPU by
test_stem_geometry_host.py, which also shows that fp32 arithmetic on the same data uses at most a third of every bound):
  * per-image route: N = 2 ... 1024 on 16-, 32-, 64-, 112- and 208-row workgroups with one to 32 row blocks per image, ragged last tiles
    of one row, single-row images (six all-halo taps: exactly zero kernel gradients), kernel gradients in 1 ... 16 slabs with the cut
    inside an image, on 128 x 128 and 128 x 256 tiles; in the H2 family a last slab that starts AT row M (32 x 9 x 9) and one that starts
    204 rows PAST it (21 x 14 x 14): wgrad_split_kernel<WgFp16x2>'s producer and consumer loops make no pass (nloop = 0 / -3: one barrier on each
    side, every load clamped to row M - 1), the accumulators are stored as the exact zeros slab_reduce adds;
  * kb_conv_chain_kernel (H2 family, 64 rows of the flattened [B N] axis): M = 2, 63, 64, 65, image boundaries inside a tile, ragged last
    tiles; with Cout = 256 layer 1 leaves the chain while backward-data stays; E_MUL_DACT without keep bits (keep = 1).
Each case runs in families 2, 1 and 0, in training (keep < 1, hashed masks, b0 = 1) and at keep = 1, both with a backward pass.
kb: largest error PER IMAGE over that image's largest reference entry (1e-5; 2e-5 where a layer is 512 wide); kernel gradients: PER TAP
over that tap's largest reference entry (2e-4; a tap whose reference is exactly zero admits exactly zero); bias gradients: whole
tensor (2e-4).  A second forward and backward gives the same bits; the family in force afterwards is the session's default.
`-s` (and any failure) prints every figure and where the worst one sits; observed: profiles/stem_geometry_errors.txt."""
import pytest
import torch

import stem_geometry_cases as sg
from helpers import default_gemm_mode

pytestmark = pytest.mark.gpu

_REF = {}          # one case's fp64 references at a time, shared by its three families: {(case id, train): {...}}


def reference(macx, case):
    if _REF.get("id") != case.id:
        _REF.clear()
        cfg, stem, img, dout = sg.make_case(macx, case)
        _REF.update(id=case.id, data=(cfg, stem, img, dout))
        for train in sg.MODES:
            _REF[train] = sg.oracle(case, cfg, stem, img, dout, train, torch.float64)
    return _REF


def run_gpu(stem, imgd, doutd, train):
    for p in stem.parameters():
        p.grad = None
    kb = stem(imgd, train=train, seed=sg.SEED, b0=sg.B0)
    (kb * doutd).sum().backward()
    torch.cuda.synchronize()
    out = {"kb": kb.detach().clone()}
    for f in stem.FIELDS:
        out[f] = getattr(stem, f).grad.detach().clone()
    return out


@pytest.mark.parametrize("family", [2, 1, 0], ids=lambda f: sg.FAMILIES[f])
@pytest.mark.parametrize("case", sg.CASES, ids=lambda c: c.id)
def test_stem_geometry(macx, dev, case, family):
    L = macx._lib.lib()
    ref = reference(macx, case)
    cfg, host, img, dout = ref["data"]
    stem = macx.Stem(cfg, H=case.H, W=case.W, inDim=case.Cin, generator=torch.Generator().manual_seed(1))
    stem.load_state_dict(host.state_dict())
    stem = stem.to(dev)
    imgd, doutd = img.to(dev), dout.to(dev)
    runs = {}
    try:
        assert L.macx_gemm_mode(family) == family
        for train in sg.MODES:
            runs[train] = (run_gpu(stem, imgd, doutd, train), run_gpu(stem, imgd, doutd, train))
    finally:
        L.macx_gemm_mode(default_gemm_mode())
    assert L.macx_gemm_mode(-1) == default_gemm_mode()
    tol = sg.tolerances(case)
    bad = []
    for train in sg.MODES:
        first, second = runs[train]
        for k in sg.METRICS:
            assert torch.isfinite(first[k]).all(), (k, train)
            if not torch.equal(first[k], second[k]):
                bad.append("%s differs between two runs (%s)" % (k, "train" if train else "keep1"))
        e = sg.errors(case, first, ref[train])
        sg.log(sg.line(case, family, train, e))
        print("    " + e["where"])
        for k in sg.METRICS:
            if not e[k] < tol[k]:
                bad.append("%s %.3e >= %.1e (%s): %s" % (k, e[k], tol[k], "train" if train else "keep1", e["where"]))
    assert not bad, "\n".join([case.reaches, str(sg.route(case, family))] + bad)
