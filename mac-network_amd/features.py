"""Image features resident in device memory: `FeatureStore` holds a whole feature set as one [rows, H*W, C] table (NHWC rows, what
the stem reads) in fp16 or fp32, filled once from the feature file (macx_features_pack), and a batch names its images by row id
(macx_features_gather, read when the kernel runs: a captured graph follows ids rewritten between replays).

    store = FeatureStore.from_h5("train.h5", dtype=torch.float16, device="cuda:0")     # 70 000 x 196 x 1024: 28.1 GB
    logits = net(store, questions, lengths, image_ids=ids)                              # ids: [B] integer device tensor

Values beyond fp16's range are refused (`check()` raises), not rescaled.  With several processes each rank holds its own store."""
import numpy as np
import torch

from . import _lib, generic, h5

INT_DTYPES = (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)


class FeatureStore:
    """A zero-initialised [rows, H*W, C] table on `device` and a 1-element overflow word.  The table is zeroed so that a captured
    class's self-check, which draws ids before the caller has written every row, never reads uninitialised bits.
    Attributes: rows, H, W, C, dtype, device, nbytes (the table's), table, overflow."""

    def __init__(self, rows, H, W, C, dtype=torch.float16, device="cuda"):
        rows, H, W, C = int(rows), int(H), int(W), int(C)
        if dtype not in _lib.FEATURES_DTYPE:
            raise TypeError("FeatureStore dtype must be torch.float16 or torch.float32, not %s" % (dtype,))
        if rows < 1 or rows >= 1 << 31:
            raise ValueError("FeatureStore rows must lie in [1, 2^31), got %d" % rows)
        if H < 1 or W < 1 or C < 1 or (H * W * C) % 4:
            raise ValueError("FeatureStore: H, W, C must be positive and H*W*C a multiple of 4 (16-byte quads), got (%d, %d, %d)"
                             % (H, W, C))
        self.rows, self.H, self.W, self.C, self.dtype = rows, H, W, C, dtype
        self.device = torch.device(device)
        self.table = torch.zeros(rows, H * W, C, dtype=dtype, device=self.device)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=self.device)

    @property
    def nbytes(self):
        return self.table.numel() * self.table.element_size()

    @property
    def hwc(self):
        return (self.H, self.W, self.C)

    def __repr__(self):
        return "<macx.FeatureStore %d x %d x %d x %d %s on %s, %.1f MB>" % (self.rows, self.H, self.W, self.C,
                                                                            str(self.dtype).replace("torch.", ""), self.device,
                                                                            self.nbytes / 1e6)

    def write(self, row0, chunk):
        """Rows row0 .. row0 + n - 1 <- chunk: [n, C, H, W] (the feature file's layout) or [n, H*W, C], fp32, on the host (uploaded
        first) or on the store's device.  A [n, H, W, C] chunk is the second layout reshaped.  Stream-ordered; nothing is checked
        on the host about the values: see check()."""
        row0 = int(row0)
        if isinstance(chunk, np.ndarray):
            chunk = torch.from_numpy(np.ascontiguousarray(chunk))
        if not torch.is_tensor(chunk) or chunk.dtype != torch.float32:
            raise TypeError("FeatureStore.write takes a float32 tensor or array, got %s"
                            % (chunk.dtype if torch.is_tensor(chunk) else type(chunk).__name__))
        H, W, C = self.hwc
        shape = tuple(chunk.shape)
        if len(shape) == 4 and shape[1:] == (C, H, W):
            layout = 0
        elif (len(shape) == 3 and shape[1:] == (H * W, C)) or (len(shape) == 4 and shape[1:] == (H, W, C)):
            layout = 1
        else:
            raise ValueError("FeatureStore.write: a chunk is [n, %d, %d, %d] (file layout) or [n, %d, %d]; got %s"
                             % (C, H, W, H * W, C, shape))
        n = shape[0]
        if n < 1 or row0 < 0 or row0 + n > self.rows:
            raise IndexError("FeatureStore.write: rows %d .. %d outside the table's [0, %d)" % (row0, row0 + n - 1, self.rows))
        generic._require_device(self.table, "the feature table")
        chunk = chunk.to(self.device).contiguous()
        _lib.check(_lib.lib().macx_features_pack(_lib.ptr(chunk), layout, n, C, H * W, _lib.ptr(self.table),
                                                 _lib.FEATURES_DTYPE[self.dtype], row0, self.rows, _lib.ptr(self.overflow),
                                                 _lib.stream_of(self.table)), "macx_features_pack")
        return self

    def check(self):
        """Reads the overflow word (one synchronisation): ValueError if any value written so far was NaN, infinite or beyond the
        table dtype's range."""
        if int(self.overflow.item()):
            raise ValueError("FeatureStore: a feature value is NaN, infinite or beyond the range of %s%s; such features are refused, "
                             "not rescaled" % (self.dtype, " (65504: a float32 store holds them)" if self.dtype == torch.float16 else ""))
        return self

    @classmethod
    def from_h5(cls, path, dataset="features", dtype=torch.float16, device="cuda", chunk_rows=256, rows=None):
        """The store of `path`'s [n, C, H, W] dataset (rows=None: all n; else its first `rows`), read through macx.h5 and packed
        in chunks of chunk_rows rows (the last may be shorter), then check()."""
        chunk_rows = int(chunk_rows)
        if chunk_rows < 1:
            raise ValueError("chunk_rows must be at least 1, got %d" % chunk_rows)
        with h5.File(path) as f:
            ds = f[dataset]
            if ds.ndim != 4:
                raise ValueError("%s: dataset %r is %s, not [n, C, H, W]" % (path, dataset, ds.shape))
            n, C, H, W = ds.shape
            rows = n if rows is None else int(rows)
            if rows < 1 or rows > n:
                raise ValueError("%s: rows = %d, the dataset has %d" % (path, rows, n))
            store = cls(rows, H, W, C, dtype=dtype, device=device)
            for r in range(0, rows, chunk_rows):
                store.write(r, torch.from_numpy(np.array(ds[r:min(r + chunk_rows, rows)], dtype=np.float32)))      # (a writable copy)
        return store.check()

    def check_ids(self, ids, count=None, host_check=False, what="image_ids"):
        """The validation of an id vector ([count] integer tensor), done before anything asks for the device.  host_check: also
        0 <= ids < rows on the host (synchronises), IndexError."""
        if not torch.is_tensor(ids) or ids.dim() != 1 or (count is not None and ids.shape[0] != count):
            raise ValueError("%s must be a [%s] tensor, one table row per image; got %s"
                             % (what, "G" if count is None else count, tuple(ids.shape) if torch.is_tensor(ids) else type(ids).__name__))
        if ids.dtype not in INT_DTYPES:
            raise ValueError("%s must have an integer dtype, not %s" % (what, ids.dtype))
        if host_check and ids.numel():
            lo, hi = int(ids.min()), int(ids.max())
            if lo < 0 or hi >= self.rows:
                raise IndexError("%s outside [0, %d)" % (what, self.rows))
        return ids

    def gather_into(self, ids, out):
        """out [G, H*W, C] fp32 <- the rows `ids` ([G] int32, contiguous, on the device) names: the one launch, no allocation (what
        the captured graphs record)."""
        _lib.check(_lib.lib().macx_features_gather(_lib.ptr(self.table), _lib.FEATURES_DTYPE[self.dtype], self.rows, _lib.ptr(ids),
                                                   ids.shape[0], self.C, self.H * self.W, _lib.ptr(out), _lib.stream_of(out)),
                   "macx_features_gather")
        return out

    def gather(self, ids):
        """[G, H*W, C] fp32 = table[ids] for a [G] integer device tensor.  An id outside [0, rows) gives that image a NaN block.
        Not an autograd node: image features take no gradient."""
        self.check_ids(ids)
        generic._require_device(ids, "image_ids")
        generic._require_device(self.table, "the feature table")
        if ids.dtype != torch.int32 or not ids.is_contiguous():
            ids = ids.to(torch.int32).contiguous()
        out = torch.empty(ids.shape[0], self.H * self.W, self.C, dtype=torch.float32, device=self.device)
        return self.gather_into(ids, out)


def check_store_images(images, image_ids, stem, count, host_check=False):
    """The validation of model.MACNet(Core).forward's `images` / `image_ids` pair, done before anything asks for the device.
    A tensor `images` takes no image_ids (TypeError) and returns None.  A FeatureStore needs image_ids ([count] integer tensor;
    count None: any number, the images of a batch with image_index) and the stem's (H, W, C); returns image_ids, whose leading
    size is the batch's image count -- what the validation of image_index / image_lengths reads from `images` otherwise."""
    if not isinstance(images, FeatureStore):
        if image_ids is not None:
            raise TypeError("image_ids name rows of a macx.FeatureStore; `images` is a %s" % type(images).__name__)
        return None
    if image_ids is None:
        raise TypeError("images is a macx.FeatureStore: image_ids= (the table rows of this batch's images) is required")
    want = (stem.H, stem.W, stem.inDim)
    if images.hwc != want:
        raise ValueError("the FeatureStore holds (H, W, C) = %s images, the stem takes %s" % (images.hwc, want))
    return images.check_ids(image_ids, count, host_check=host_check)
