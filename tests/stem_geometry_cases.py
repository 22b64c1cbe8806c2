"""The fused stem (macx.Stem: two 3 x 3 SAME convolutions as implicit GEMMs) at its tile edges: case table, data, metrics.

Shared by tests/test_gpu_stem_geometry.py (the kernels, three families) and tests/test_stem_geometry_host.py (CPU: the table's claims
against a restatement of the launch rules, the inputs' fairness under the finer metrics, the magic division's refusal bound).

Routes (mac-network_amd/csrc/macx_api.hip, macx_gemm.hip.h, macx_gemm3h.hip.h, macx_wgrad6.hip.h), restated below in Python:
  * forward of layer 0 / layer 1 and backward-data are three GEMM launches [B N, 9 cin] x [9 cin, nout] with (cin, nout) =
    (Cin, Cmid), (Cmid, Cout), (Cout, Cmid).  In the H2 family a launch with nout == 512 and cin % 256 == 0 runs on
    kb_conv_chain_kernel (64 rows of the FLATTENED [B N] axis per workgroup); every other launch, and every launch of families 1 / 0,
    tiles each image by rt x 16 rows, rt = pick_rt(N, B, nout / 128).
  * the two kernel gradients reduce over the M = B N rows in conv_splits(9 cin / 128 * nout / 128, M) slabs of rows_per_split rows (H2:
    rounded up to 32, else to 2); slab_reduce sums ALL slabs, so a slab that starts at or past M has to hold exact zeros.
    Families 2 / 1 use 128 x 256 output tiles (JW = 2) when nout % 256 == 0, else 128 x 128.

pick_rt gives 13 x 16 rows only to a launch of at least 200 such workgroups (B nout / 128 ceil(N / 208) >= 200) and otherwise falls to
32-row tiles (16 for N <= 16), so at the small batches of this table an image of N > 32 pixels is ALWAYS cut into several row tiles:
N = 1024 is 32 of them.  The three `tall` cases are batches just large enough to keep the 4-, 7- and 13-tile kernels with two row blocks per image.
"""
import collections
import math
import os

import torch

from oracle import dropout_hash as dh
from oracle import mac_oracle as mo
import gradient_scale_cases as gsc

FAMILIES = {2: "h2", 1: "split", 0: "native"}
SEED = 5                      # dropout seed (sites 9 / 10, b0 = 1), as test_gpu_stem.run_case
B0 = 1
GRAD_TOL = 2e-4               # every gradient (test_gpu_stem.py)
K_MAXN = 1024                 # macx_small.hip.h
CC_ROWS = 64                  # rows of the flattened [B N] axis per workgroup of kb_conv_chain_kernel


def fwd_tol(c):
    """the stem tests' own forward bounds: 1e-5, and 2e-5 where a layer is 512 wide (test_gpu_stem.test_stem_clevr_shape)"""
    return 2e-5 if max(c.Cmid, c.Cout) >= 512 else gsc.STEM_FWD_TOL


# ---------------------------------------------------------------------------------------------------------------------------
# the launch rules, restated
# ---------------------------------------------------------------------------------------------------------------------------
def pick_rt(N, B, ncb):
    """kb_gemm_pick_rt (macx_gemm.hip.h): row tiles of 16 per workgroup"""
    cand = (13, 7, 4, 2, 1)
    k = 4 if N <= 16 else 3 if N <= 32 else 2 if N <= 64 else 1 if N <= 112 else 0
    blocks = lambda rt: B * ncb * ((N + rt * 16 - 1) // (rt * 16))
    while k < 3 and blocks(cand[k]) < 200:
        k += 1
    return cand[k]


def row_blocks(N, rt):
    """[(first row, rows)] of the workgroups of one image (kb_gemm3h_kernel: the 16-row tiles dealt evenly to ceil(N / (16 rt)) blocks)"""
    nrb = (N + rt * 16 - 1) // (rt * 16)
    ntiles = (N + 15) // 16
    tbase, textra = divmod(ntiles, nrb)
    out = []
    for rbi in range(nrb):
        nt = tbase + (1 if rbi < textra else 0)
        row0 = (rbi * tbase + min(rbi, textra)) * 16
        out.append((row0, min(N, row0 + nt * 16) - row0))
    return out


def conv_splits(tiles, M):
    """conv_splits (macx_api.hip): slabs of a kernel gradient"""
    best, beff = 1, 0.0
    for ns in range(1, 17):
        if (M + ns - 1) // ns < 256:
            break
        blocks = tiles * ns
        eff = blocks / (((blocks + 255) // 256) * 256)
        if eff > beff + 0.02:
            beff, best = eff, ns
    return best


def rows_per_split(M, ns, family):
    r = (M + ns - 1) // ns
    return (r + 31) & ~31 if family == 2 else (r + 1) & ~1


def on_chain(family, cin, nout):
    """kb_gemm3h_launch: the H2 family's launches on kb_conv_chain_kernel"""
    return family == 2 and nout == 512 and cin % 256 == 0


def launches(c):
    """[(name, cin, nout)] of the three GEMM launches of a forward + backward pass"""
    return [("fwd0", c.Cin, c.Cmid), ("fwd1", c.Cmid, c.Cout), ("bwd_data", c.Cout, c.Cmid)]


def route(c, family):
    """what the library does with case c in a family: {launch: "chain" | rt}, {"wgrad0" | "wgrad1": (slabs, rows per slab, empty slabs, JW)}"""
    r = {}
    for name, cin, nout in launches(c):
        r[name] = "chain" if on_chain(family, cin, nout) else pick_rt(c.N, c.B, nout // 128)
    for name, cin, nout in (("wgrad0", c.Cin, c.Cmid), ("wgrad1", c.Cmid, c.Cout)):
        ns = conv_splits(9 * cin // 128 * (nout // 128), c.M)
        rows = rows_per_split(c.M, ns, family)
        empty = sum(1 for s in range(ns) if s * rows >= c.M)
        r[name] = (ns, rows, empty, 1 if family == 0 else 2 if nout % 256 == 0 else 1)
    return r


# ---------------------------------------------------------------------------------------------------------------------------
# the magic division of the CONV kernel-gradient kernels (conv_wgrad: magic_n = ceil(2^32 / N), img = __umulhi(m, magic_n))
# ---------------------------------------------------------------------------------------------------------------------------
def magic(n):
    return ((1 << 32) + n - 1) // n


def magic_excess(n):
    """e = magic n - 2^32 (0 <= e < n): (m magic) >> 32 == m // n for every m with m e < 2^32"""
    return magic(n) * n - (1 << 32)


def refused_rows(n):
    """stem_check refuses B with (B n - 1) e >= 2^32: the smallest flattened row index that is NOT served (None: every row is, e = 0)"""
    e = magic_excess(n)
    return None if e == 0 else -(-(1 << 32) // e)           # ceil(2^32 / e)


def first_wrong_row(n):
    """the smallest m with (m magic(n)) >> 32 != m // n, found exactly (None: there is none, e = 0).
    With m = q n + r, r < n:  m magic = q (2^32 + e) + r magic, and r magic < 2^32, so the shifted product is q + ((q e + r magic) >> 32):
    wrong iff q e + r magic >= 2^32.  The smallest q for remainder r is ceil((2^32 - r magic) / e); the minimum over r of q n + r."""
    e, mg = magic_excess(n), magic(n)
    if e == 0:
        return None
    return min(max(0, -(-((1 << 32) - r * mg) // e)) * n + r for r in range(n))


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
class Case(collections.namedtuple("Case", "id B H W Cin Cmid Cout reaches expect")):
    """expect: {family: {launch: "chain" | rt, "wgrad0" / "wgrad1": (slabs, rows per slab, empty slabs, JW)}} -- written out by hand
    where the case was chosen for it (test_stem_geometry_host.py holds every entry to route()); families without an entry: no claim."""
    N = property(lambda c: c.H * c.W)
    M = property(lambda c: c.B * c.H * c.W)


def _case(B, H, W, ch=(128, 128, 128), reaches="", expect=None, tag=""):
    cid = "%dx%dx%d-%d-%d-%d%s" % ((B, H, W) + tuple(ch) + (tag,))
    return Case(cid, B, H, W, ch[0], ch[1], ch[2], reaches, expect or {})


def _all(fwd0, fwd1, bwd, w0, w1, w0_other=None, w1_other=None):
    """the same tile heights in all three families (none of the launches qualifies for the chain); kernel gradients: H2, then 1 / 0"""
    e = {}
    for f in (2, 1, 0):
        a, b = (w0, w1) if f == 2 else (w0_other or w0, w1_other or w1)
        if f == 0:
            a, b = a[:3] + (1,), b[:3] + (1,)
        e[f] = dict(fwd0=fwd0, fwd1=fwd1, bwd_data=bwd, wgrad0=a, wgrad1=b)
    return e


def _one(M, jw=1):
    """one slab (M < 2 x 256 rows, or no better filling): rows per slab = M rounded up, per family"""
    return (1, (M + 31) & ~31, 0, jw), (1, (M + 1) & ~1, 0, jw)


def _per_image():
    C3 = (128, 256, 384)      # layer 0's gradient on 128 x 256 tiles (JW = 2), layer 1's on 128 x 128 (384 % 256 != 0)
    out = []

    def add(B, H, W, rt, reaches, ch=(128, 128, 128), w=None, tag=""):
        M = B * H * W
        if w is None:
            jw0, jw1 = (2 if ch[1] % 256 == 0 else 1), (2 if ch[2] % 256 == 0 else 1)
            (a2, a1), (b2, b1) = _one(M, jw0), _one(M, jw1)
            w = (a2, b2, a1, b1)
        rt = rt if isinstance(rt, tuple) else (rt, rt, rt)
        out.append(_case(B, H, W, ch, reaches, _all(rt[0], rt[1], rt[2], w[0], w[1], w[2], w[3]), tag))

    add(1, 1, 2, 1, "smallest admitted grid (W >= 2); tap rows dy = -1 / +1 read halo only: six exactly zero taps; one 16-row tile")
    add(2, 3, 3, 1, "one 16-row tile, 9 of its rows live")
    add(3, 1, 17, 2, "N = 17: past the 16-row tile, one 32-row tile; single-row image")
    add(2, 3, 11, 2, "N = 33: pick_rt's class N <= 64 (4 x 16) falls to 32-row tiles at this batch: a second tile of ONE row")
    add(2, 5, 13, 2, "N = 65: class N <= 112 (7 x 16) falls to 32-row tiles: three tiles, the last of one row")
    add(5, 1, 113, 2, "N = 113: class N > 112 (13 x 16) falls to 32-row tiles, four per image; single-row image 113 wide; M = 565: two slabs "
                      "of 288 (H2) / 284 rows, the cut inside the third image",
        w=((2, 288, 0, 1), (2, 288, 0, 1), (2, 284, 0, 1), (2, 284, 0, 1)))
    add(2, 13, 16, 2, "N = 208 = 13 x 16: seven 32-row blocks of 2,2,2,2,2,2,1 tiles, no ragged row; JW = 2 and JW = 1", ch=C3)
    add(2, 11, 19, 2, "N = 209: 14 tiles in seven blocks, the last row alone in its 16-row tile; JW = 2 and JW = 1", ch=C3)
    add(1, 15, 15, 2, "N = 225: eight 32-row blocks (15 tiles), one live row in the last tile; JW = 2 and JW = 1", ch=C3)
    add(1, 8, 32, 2, "N = 256 (the 8 x 32 NLVR grid): eight full 32-row blocks; one slab of exactly 256 rows")
    add(1, 32, 32, 2, "N = K_MAXN = 1024: 32 blocks per image, halo rows up to 33; four slabs of exactly 256 rows",
        w=((4, 256, 0, 1), (4, 256, 0, 1), (4, 256, 0, 1), (4, 256, 0, 1)))
    add(32, 9, 9, 2, "M = 2592: ten slabs; H2 rounds 260 rows up to 288, so the tenth slab starts AT row 2592 = M (nchunk = 0)",
        w=((10, 288, 1, 1), (10, 288, 1, 1), (10, 260, 0, 1), (10, 260, 0, 1)))
    add(21, 14, 14, 2, "M = 4116: sixteen slabs; H2 rounds 258 rows up to 288, so the sixteenth starts at 4320 > M "
                       "(m_end - m_begin = -204, nchunk = -6, nloop = -3)",
        w=((16, 288, 1, 1), (16, 288, 1, 1), (16, 258, 0, 1), (16, 258, 0, 1)))
    # beyond the issue's table: batches just large enough (200 workgroups) that pick_rt KEEPS a taller tile for layer 0's forward and
    # backward-data (nout = 512 with cin = 128: off the chain in every family); the kernel deals an image's 16-row tiles evenly to
    # its row blocks.  Layer 1 (nout = 128) stays on 32-row tiles.
    T = (128, 512, 128)
    add(25, 5, 13, (4, 2, 4), "N = 65 on 4 x 16 rows: blocks of 3 + 2 tiles, one live row in the last", ch=T, tag="-tall",
        w=((6, 288, 0, 2), (6, 288, 0, 1), (6, 272, 0, 2), (6, 272, 0, 1)))
    add(25, 1, 113, (7, 2, 7), "N = 113 on 7 x 16 rows: blocks of 4 + 4 tiles, one live row in the last; single-row image", ch=T, tag="-tall",
        w=((7, 416, 0, 2), (7, 416, 0, 1), (7, 404, 0, 2), (7, 404, 0, 1)))
    add(25, 11, 19, (13, 2, 13), "N = 209 on 13 x 16 rows: blocks of 7 + 7 tiles (rows 0-111, 112-208), one live row in the last", ch=T,
        tag="-tall", w=((7, 768, 0, 2), (7, 768, 0, 1), (7, 748, 0, 2), (7, 748, 0, 1)))
    return out


def _chain():
    out = []

    def add(B, H, W, rt, reaches, ch=(256, 512, 512)):
        M = B * H * W
        (a2, a1), (b2, b1) = _one(M, 2), _one(M, 2 if ch[2] % 256 == 0 else 1)
        e = _all(rt, rt, rt, a2, b2, a1, b1)
        e[2].update(fwd0="chain", bwd_data="chain")
        if ch[2] == 512:
            e[2].update(fwd1="chain")
        out.append(_case(B, H, W, ch, reaches, e))

    add(1, 1, 2, 1, "M = 2: every loader row of the 64-row tile but two clamps to M - 1")
    add(1, 7, 9, 2, "M = 63: one row short of a tile")
    add(1, 8, 8, 2, "M = 64: exactly one tile")
    add(1, 5, 13, 2, "M = 65: one row into a second tile")
    add(1, 5, 13, 2, "M = 65 with Cout = 256: layer 1 leaves the chain (nout = 256), backward-data (nout = Cmid = 512) stays on it",
        ch=(256, 512, 256))
    add(3, 5, 5, 2, "M = 75, N = 25: two image boundaries inside the first tile, the tile boundary (row 64) inside the third image")
    add(1, 15, 15, 2, "M = 225: four tiles within one image, the last of 33 rows")
    add(2, 11, 19, 2, "M = 418: image boundary at row 209 inside the fourth tile, ragged last tile of 34 rows")
    return out


PER_IMAGE = _per_image()
CHAIN = _chain()
CASES = PER_IMAGE + CHAIN
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
MODES = (True, False)         # training (keep < 1, hashed masks) | keep = 1 -- both with a backward pass


# ---------------------------------------------------------------------------------------------------------------------------
# data and the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def make_case(macx, c):
    """(cfg, stem on the host, images [B, N, Cin], cotangent [B, N, Cout]): test_gpu_stem.run_case's data from host generators --
    the `args` flag file (ELU), biases uniform in +-0.5, images relu(randn), cotangent randn / B"""
    cfg = mo.flag_file_config("args", memDim=c.Cout, ctrlDim=c.Cout, attDim=c.Cout)
    cfg.stemDim = c.Cmid
    stem = macx.Stem(cfg, H=c.H, W=c.W, inDim=c.Cin, generator=torch.Generator().manual_seed(1))
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        stem.bias0.copy_(torch.rand(c.Cmid, generator=g) - 0.5)
        stem.bias1.copy_(torch.rand(c.Cout, generator=g) - 0.5)
    img = torch.relu(torch.randn(c.B, c.N, c.Cin, generator=g))
    dout = torch.randn(c.B, c.N, c.Cout, generator=g) / c.B
    return cfg, stem, img, dout


def oracle(c, cfg, stem, img, dout, train, dtype):
    """{"kb", "kernel0", "bias0", "kernel1", "bias1"}: mo.stem_cnn and its gradients in `dtype`, the masks of (SEED, sites 9 / 10, B0)"""
    prm = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in stem.to_reference_dict().items()}
    vs = mo.VarStore(params=prm, dtype=dtype)
    keep = stem.keep if train else 1.0
    masks = None
    if train:
        masks = [torch.from_numpy(dh.mask_for(SEED, 9, 0, keep, (c.B, c.N, c.Cin), b0=B0)).to(dtype),
                 torch.from_numpy(dh.mask_for(SEED, 10, 0, keep, (c.B, c.N, c.Cmid), b0=B0)).to(dtype)]
    out = mo.stem_cnn(cfg, vs, img.to(dtype), c.H, c.W, keep=keep, masks=masks)
    (out * dout.to(dtype)).sum().backward()
    res = {"kb": out.detach()}
    for f, name in stem.REF_NAMES.items():
        res[f] = prm[name].grad
    return res


# ---------------------------------------------------------------------------------------------------------------------------
# metrics
# ---------------------------------------------------------------------------------------------------------------------------
def _ratio(err, scale):
    """err / scale per group; a group whose reference is exactly zero admits exactly zero (0) and nothing else (inf)"""
    out = err / scale.clamp_min(1e-300)
    out = torch.where(scale > 0, out, torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return out


def per_image_err(got, ref):
    """[B] largest |got - ref| of each image over that image's largest |ref|, and the worst (image, pixel) of the batch"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    d = (got - ref).abs()
    B = ref.shape[0]
    e = _ratio(d.reshape(B, -1).amax(dim=1), ref.abs().reshape(B, -1).amax(dim=1))
    b = int(e.argmax())
    n = int(d[b].amax(dim=1).argmax())
    return e, (b, n)


def per_tap_err(got, ref):
    """[9] largest error of each tap's [Cin][Cout] block over that block's largest |ref| (kernels are [3, 3, Cin, Cout])"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    d = (got - ref).abs().reshape(9, -1).amax(dim=1)
    return _ratio(d, ref.abs().reshape(9, -1).amax(dim=1))


def whole_err(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    return float(_ratio((got - ref).abs().max(), ref.abs().max()))


def errors(c, got, ref):
    """{"kb", "kernel0", "kernel1", "bias0", "bias1"}: the figure each metric bounds, and "where": the worst pixel and taps, described"""
    e_img, (b, n) = per_image_err(got["kb"], ref["kb"])
    t0, t1 = per_tap_err(got["kernel0"], ref["kernel0"]), per_tap_err(got["kernel1"], ref["kernel1"])
    y, x = divmod(n, c.W)
    m = b * c.N + n
    border = y in (0, c.H - 1) or x in (0, c.W - 1)
    tap = lambda t: "(%d,%d)" % (int(t.argmax()) // 3 - 1, int(t.argmax()) % 3 - 1)
    rt = pick_rt(c.N, c.B, c.Cout // 128)
    blk = next(i for i, (r0, rows) in enumerate(row_blocks(c.N, rt)) if r0 <= n < r0 + rows)
    where = ("kb worst: image %d pixel (y %d, x %d)%s, flattened row %d (mod %d: %d), row block %d of %d-row tiles in its image; "
             "worst tap (dy,dx) kernel0 %s kernel1 %s" % (b, y, x, " BORDER" if border else "", m, CC_ROWS, m % CC_ROWS, blk, rt * 16,
                                                          tap(t0), tap(t1)))
    return dict(kb=float(e_img.max()), kernel0=float(t0.max()), kernel1=float(t1.max()), bias0=whole_err(got["bias0"], ref["bias0"]),
                bias1=whole_err(got["bias1"], ref["bias1"]), where=where)


def tolerances(c):
    return dict(kb=fwd_tol(c), kernel0=GRAD_TOL, kernel1=GRAD_TOL, bias0=GRAD_TOL, bias1=GRAD_TOL)


METRICS = ("kb", "kernel0", "kernel1", "bias0", "bias1")


def line(c, family, train, e):
    return "%-26s %-6s %-5s " % (c.id, FAMILIES.get(family, family), "train" if train else "keep1") + \
        " ".join("%s %.2e" % (k, e[k]) for k in METRICS)


def log(text):
    """append to the file MACX_STEM_GEOMETRY_LOG names (how profiles/stem_geometry_errors.txt is recorded); always printed (-s)"""
    print(text)
    path = os.environ.get("MACX_STEM_GEOMETRY_LOG")
    if path:
        with open(path, "a") as fh:
            fh.write(text + "\n")
