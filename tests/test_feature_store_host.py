"""The host side of image features resident in device memory (macx_features_pack / macx_features_gather, macx.FeatureStore,
`image_ids=` on MACNetCore / MACNet, `features=` on CapturedTowerForward / CapturedTowerTrainStep): the exports against the header,
every MACX_EINVAL of the two calls (returned before any HIP call, so without a device), the refusals by exception type and message,
and from_h5's chunk walk.  No GPU."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from test_abi_host import header_prototypes, prototype_mismatches
from test_lengths_paths_host import bare
from test_tower_graph_host import small_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H5 = os.path.join(ROOT, "tests", "golden", "h5", "features_like_reference.h5")
NEW = ("macx_features_pack", "macx_features_gather")
B, S = 6, 7
A16 = 0x10000           # addresses that are never dereferenced: every call below is refused before anything is launched


def test_exports_are_in_the_table_with_the_headers_prototypes(macx):
    protos = header_prototypes()
    for n in NEW:
        assert n in macx._lib.TABLE and n in protos, n
    assert prototype_mismatches({n: macx._lib.TABLE[n] for n in NEW}) == []
    assert protos["macx_features_pack"] == ("int", ["pointer", "int", "int", "int", "int", "pointer", "int", "size_t", "size_t",
                                                    "pointer", "pointer"])
    assert protos["macx_features_gather"] == ("int", ["pointer", "int", "size_t", "pointer", "int", "int", "int", "pointer", "pointer"])
    L = macx._lib.lib()
    for n in NEW:
        assert list(getattr(L, n).argtypes) == list(macx._lib.TABLE[n][1]) and getattr(L, n).restype is C.c_int
    assert macx._lib.ABI_VERSION == 5 and L.macx_abi_version() == 5                 # no struct changed
    assert macx._lib.FEATURES_DTYPE == {torch.float32: 0, torch.float16: 1}


# (src, layout, n, C, HW, table, dtype, row0, rows, overflow): a legal call, then one argument at a time made illegal
PACK_OK = dict(src=A16, layout=0, n=2, C=8, HW=9, table=2 * A16, dtype=1, row0=1, rows=4, overflow=3 * A16)
PACK_BAD = [("src", 0), ("table", 0), ("n", 0), ("n", -1), ("C", 0), ("HW", 0), ("HW", -3), ("rows", 0), ("C", 7), ("row0", -1),
            ("row0", 3), ("rows", 2), ("rows", 1 << 31), ("dtype", 2), ("dtype", -1), ("layout", 2), ("layout", -1), ("src", A16 + 4),
            ("table", 2 * A16 + 8), ("table", 2 * A16 + 2), ("overflow", 3 * A16 + 2)]
GATHER_OK = dict(table=A16, dtype=1, rows=4, ids=2 * A16, G=3, C=8, HW=9, out=3 * A16)
GATHER_BAD = [("table", 0), ("ids", 0), ("out", 0), ("G", 0), ("G", -2), ("C", 0), ("HW", 0), ("rows", 0), ("rows", -1), ("C", 6),
              ("rows", 1 << 31), ("dtype", 2), ("dtype", -1), ("table", A16 + 8), ("out", 3 * A16 + 4), ("ids", 2 * A16 + 2)]


def pack(L, a):
    return L.macx_features_pack(a["src"], a["layout"], a["n"], a["C"], a["HW"], a["table"], a["dtype"], a["row0"], a["rows"],
                                a["overflow"], None)


def gather(L, a):
    return L.macx_features_gather(a["table"], a["dtype"], a["rows"], a["ids"], a["G"], a["C"], a["HW"], a["out"], None)


@pytest.mark.parametrize("name,value", PACK_BAD)
def test_pack_refuses_before_any_launch(macx, name, value):
    assert pack(macx._lib.lib(), dict(PACK_OK, **{name: value})) == macx._lib.MACX_EINVAL


@pytest.mark.parametrize("name,value", GATHER_BAD)
def test_gather_refuses_before_any_launch(macx, name, value):
    assert gather(macx._lib.lib(), dict(GATHER_OK, **{name: value})) == macx._lib.MACX_EINVAL


def test_einval_cases_hold_for_both_dtypes_and_layouts(macx):
    """the argument checks do not depend on which kernel the call would launch"""
    L = macx._lib.lib()
    for dtype in (0, 1):
        for layout in (0, 1):
            assert pack(L, dict(PACK_OK, dtype=dtype, layout=layout, C=3, HW=3)) == macx._lib.MACX_EINVAL       # C*HW % 4
            assert pack(L, dict(PACK_OK, dtype=dtype, layout=layout, row0=2, n=3)) == macx._lib.MACX_EINVAL     # row0 + n > rows
        assert gather(L, dict(GATHER_OK, dtype=dtype, C=3, HW=3)) == macx._lib.MACX_EINVAL


# ---- FeatureStore ------------------------------------------------------------------------------------------------------------------
def cpu_store(macx, rows=5, H=5, W=5, C_=128, dtype=torch.float16):
    """a store on the host: construction, attributes and every refusal work without a device; write / gather do not"""
    return macx.FeatureStore(rows, H, W, C_, dtype=dtype, device="cpu")


def test_store_attributes(macx):
    s = cpu_store(macx)
    assert (s.rows, s.H, s.W, s.C, s.dtype) == (5, 5, 5, 128, torch.float16)
    assert s.nbytes == 5 * 25 * 128 * 2 and cpu_store(macx, dtype=torch.float32).nbytes == 5 * 25 * 128 * 4
    assert tuple(s.table.shape) == (5, 25, 128) and s.table.dtype == torch.float16 and not s.table.any()     # zero-initialised
    assert tuple(s.overflow.shape) == (1,) and s.overflow.dtype == torch.int32 and int(s.overflow) == 0
    assert macx.features.FeatureStore is macx.FeatureStore
    assert inspect.signature(macx.FeatureStore.from_h5).parameters["chunk_rows"].default == 256


def test_store_constructor_refusals(macx):
    with pytest.raises(TypeError, match="float16 or torch.float32"):
        macx.FeatureStore(4, 5, 5, 128, dtype=torch.bfloat16, device="cpu")
    for rows in (0, -1, 1 << 31):
        with pytest.raises(ValueError, match="rows"):
            macx.FeatureStore(rows, 5, 5, 128, device="cpu")
    with pytest.raises(ValueError, match="multiple of 4"):
        macx.FeatureStore(4, 3, 3, 3, device="cpu")
    with pytest.raises(ValueError, match="positive"):
        macx.FeatureStore(4, 0, 3, 4, device="cpu")


def test_write_refusals_and_no_cpu_path(macx):
    s = cpu_store(macx)
    with pytest.raises(TypeError, match="float32"):
        s.write(0, torch.zeros(1, 128, 5, 5, dtype=torch.float16))
    with pytest.raises(TypeError, match="float32"):
        s.write(0, [[1.0]])
    for shape in ((1, 128, 5, 4), (25, 128), (1, 24, 128), (1, 5, 128, 5)):
        with pytest.raises(ValueError, match="a chunk is"):
            s.write(0, torch.zeros(shape))
    for row0, n in ((-1, 1), (5, 1), (3, 3)):
        with pytest.raises(IndexError, match="outside the table"):
            s.write(row0, torch.zeros(n, 128, 5, 5))
    for chunk in (torch.zeros(2, 128, 5, 5), torch.zeros(2, 25, 128), np.zeros((2, 128, 5, 5), np.float32)):
        with pytest.raises(RuntimeError, match="HIP device"):             # a legal chunk: on to the device, and there is none
            s.write(1, chunk)


def test_check_reads_the_overflow_word(macx):
    s = cpu_store(macx)
    assert s.check() is s
    s.overflow.fill_(1)
    with pytest.raises(ValueError, match="float16"):
        s.check()
    f = cpu_store(macx, dtype=torch.float32)
    f.overflow.fill_(1)
    with pytest.raises(ValueError, match="float32"):
        f.check()


def test_gather_refusals_and_no_cpu_path(macx):
    s = cpu_store(macx)
    for bad in (torch.zeros(2, 2, dtype=torch.int32), [0, 1]):
        with pytest.raises(ValueError, match="image_ids must be a"):
            s.gather(bad)
    for bad in (torch.zeros(3), torch.zeros(3, dtype=torch.bool)):
        with pytest.raises(ValueError, match="integer dtype"):
            s.gather(bad)
    with pytest.raises(RuntimeError, match="HIP device"):
        s.gather(torch.tensor([0, 4, 4]))
    assert not hasattr(s.gather, "apply")                                # a plain call, not an autograd node


# ---- from_h5's chunk walk ----------------------------------------------------------------------------------------------------------
def test_from_h5_walks_the_dataset_in_chunks(macx, monkeypatch):
    seen = []

    def record(self, row0, chunk):
        seen.append((self, int(row0), torch.as_tensor(chunk).clone()))
        return self
    monkeypatch.setattr(macx.FeatureStore, "write", record)
    store = macx.FeatureStore.from_h5(H5, dtype=torch.float16, device="cpu", chunk_rows=3)
    assert (store.rows, store.C, store.H, store.W) == (7, 8, 3, 3) and store.dtype == torch.float16
    assert [(r, c.shape[0]) for _, r, c in seen] == [(0, 3), (3, 3), (6, 1)]
    assert all(s is store for s, _, _ in seen)
    with macx.h5.File(H5) as f:
        want = torch.from_numpy(np.asarray(f["features"]).copy())
    got = torch.cat([c for _, _, c in seen])
    assert got.dtype == torch.float32 and torch.equal(got, want)           # file layout [n, C, H, W], untouched
    # rows=: a prefix of the dataset; a chunk size that divides it leaves no short chunk
    del seen[:]
    store = macx.FeatureStore.from_h5(H5, dtype=torch.float32, device="cpu", chunk_rows=2, rows=4)
    assert store.rows == 4 and [(r, c.shape[0]) for _, r, c in seen] == [(0, 2), (2, 2)]
    assert torch.equal(torch.cat([c for _, _, c in seen]), want[:4])
    for rows in (0, 8):
        with pytest.raises(ValueError, match="rows"):
            macx.FeatureStore.from_h5(H5, device="cpu", rows=rows)
    with pytest.raises(ValueError, match="chunk_rows"):
        macx.FeatureStore.from_h5(H5, device="cpu", chunk_rows=0)


def test_from_h5_checks_the_overflow_word_at_the_end(macx, monkeypatch):
    def poisoned(self, row0, chunk):
        self.overflow.fill_(1)
        return self
    monkeypatch.setattr(macx.FeatureStore, "write", poisoned)
    with pytest.raises(ValueError, match="float16"):
        macx.FeatureStore.from_h5(H5, device="cpu", chunk_rows=3)


# ---- the tower ---------------------------------------------------------------------------------------------------------------------
def tower_inputs():
    return torch.ones(B, S, dtype=torch.int32), torch.full((B,), S, dtype=torch.int32)


def test_new_keywords_default_to_off(macx):
    for cls in (macx.MACNetCore, macx.MACNet):
        assert inspect.signature(cls.forward).parameters["image_ids"].default is None, cls
    for cls in (macx.CapturedTowerForward, macx.CapturedTowerTrainStep):
        assert inspect.signature(cls.__init__).parameters["features"].default is None, cls
        assert inspect.signature(cls.load).parameters["image_ids"].default is None, cls
        assert cls.features is None and cls.image_ids is None
    assert inspect.signature(macx.CapturedTowerForward.__call__).parameters["image_ids"].default is None


def test_forward_refusals(macx):
    net = small_net(macx)
    q, lengths = tower_inputs()
    store, ids = cpu_store(macx), torch.tensor([0, 4, 4, 1, 2, 3])
    core = lambda images, **kw: macx.MACNetCore.forward(net, images, torch.zeros(B, 256), torch.zeros(B, S, 256), lengths, **kw)
    for call in (lambda images, **kw: net(images, q, lengths, **kw), core):
        with pytest.raises(TypeError, match="image_ids= .* is required"):
            call(store)
        with pytest.raises(TypeError, match="image_ids name rows of a macx.FeatureStore"):
            call(torch.zeros(B, 25, 128), image_ids=ids)
        with pytest.raises(ValueError, match="the stem takes"):
            call(cpu_store(macx, H=5, W=5, C_=64), image_ids=ids)
        with pytest.raises(ValueError, match=r"image_ids must be a \[6\]"):
            call(store, image_ids=ids[:5])                                  # one image per question: [B]
        with pytest.raises(ValueError, match="integer dtype"):
            call(store, image_ids=ids.float())
        for bad in ([0, 5, 4, 1, 2, 3], [0, 4, -1, 1, 2, 3]):
            with pytest.raises(IndexError, match=r"image_ids outside \[0, 5\)"):
                call(store, image_ids=torch.tensor(bad), check_index=True)
        with pytest.raises(RuntimeError, match="no CPU path|HIP device"):   # valid: on to the device
            call(store, image_ids=ids, check_index=True)
        # with image_index the ids are per image: any count, and the index is validated as before
        with pytest.raises(ValueError, match="image_index"):
            call(store, image_ids=ids[:3], image_index=torch.zeros(B - 1, dtype=torch.int32))
        with pytest.raises(RuntimeError, match="no CPU path|HIP device"):
            call(store, image_ids=ids[:3], image_index=torch.tensor([0, 1, 2, 2, 1, 0]))
    with pytest.raises(IndexError, match="image_ids outside"):            # MACNet: check_ids (the default) covers the rows too
        net(store, q, lengths, image_ids=torch.tensor([0, 5, 4, 1, 2, 3]))
    with pytest.raises(RuntimeError, match="no CPU path|HIP device"):
        net(store, q, lengths, image_ids=torch.tensor([0, 5, 4, 1, 2, 3]), check_ids=False)


@pytest.mark.parametrize("name", ["CapturedTowerForward", "CapturedTowerTrainStep"])
def test_load_takes_image_ids_exactly_when_built_with_features(macx, name):
    q, lengths = tower_inputs()
    tail = (torch.zeros(B, dtype=torch.int32),) if name == "CapturedTowerTrainStep" else ()
    store, ids = cpu_store(macx), torch.tensor([0, 4, 4, 1, 2, 3])
    plain = bare(macx, name, B=B, S=S, N=25)
    with pytest.raises(ValueError, match="without features="):
        plain.load(torch.zeros(B, 25, 128), q, lengths, *tail, image_ids=ids)
    built = bare(macx, name, B=B, S=S, N=25, features=store, image_ids=torch.zeros(B, dtype=torch.int32))
    with pytest.raises(ValueError, match="captured with features="):
        built.load(torch.zeros(B, 25, 128), q, lengths, *tail)
    with pytest.raises(ValueError, match="captured with features="):
        built.load(torch.zeros(B, 25, 128), q, lengths, *tail, image_ids=ids)
    with pytest.raises(ValueError, match="captured with features="):
        built.load(None, q, lengths, *tail)
    with pytest.raises(ValueError, match="image_ids must have the leading size 6"):
        built.load(None, q, lengths, *tail, image_ids=ids[:4])
    with pytest.raises(ValueError, match="integer dtype"):
        built.load(None, q, lengths, *tail, image_ids=ids.float())
    with pytest.raises(IndexError, match=r"image_ids outside \[0, 5\)"):
        built.load(None, q, lengths, *tail, image_ids=torch.tensor([0, 4, 5, 1, 2, 3]))
    # shared images: the ids are per image
    shared = bare(macx, name, B=B, S=S, N=25, G=3, features=store, image_ids=torch.zeros(3, dtype=torch.int32),
                  image_index=torch.zeros(B, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"image_ids must be a \[3\]"):
        shared.load(None, q, lengths, *tail, image_ids=ids, image_index=torch.zeros(B, dtype=torch.int32))


def test_constructors_refuse_before_the_device(macx):
    net = small_net(macx, stemDropout=1.0)
    for make in (lambda **kw: macx.CapturedTowerForward(net, B, S, **kw),
                 lambda **kw: macx.CapturedTowerTrainStep(net, None, None, B, S, **kw)):
        with pytest.raises(RuntimeError, match="HIP device"):              # the device comes first, as for every captured class
            make(features=cpu_store(macx))
