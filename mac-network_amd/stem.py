"""Image input unit ("stem", model.py:165-204): 2 x (dropout -> conv3x3 SAME -> +b -> act) over the
pre-extracted 14 x 14 x 1024 features, producing the cell's knowledge base [B, H*W, memDim].
Implicit-GEMM convolutions on the fp32-MFMA knowledge-base GEMM kernel behind libmacx.so.
SURVEY.md 8f row 1.

    stem = Stem(config, H=14, W=14, inDim=1024).to(device)
    kb = stem(images, train=True, seed=step)          # images [B, H*W, inDim] (NHWC), kb [B, H*W, memDim]

Every other stem the reference builds -- any --stemNumLayers, --stemKernelSize(s), --stemStrideSizes, --stemDim, --stemLinear,
--locationAware (L / PE) -- runs on GenericStem: one general implicit-GEMM convolution per layer (macx_conv2d_*, exact fp32
MFMA), dropout / activation / bias-gradient kernels of the generic path between them.  Stem(config, ...) returns a GenericStem
for those option sets; --stemBN and --stemGridRnn raise what the reference raises (KeyError / NameError).
"""
import ctypes as C

import torch

from . import _lib, generic, unit
from .options import UnsupportedOptions, _resolve_act, fresh_seed

REF_NAMES = {"kernel0": "stem/cnnLayercnn_0/kernels/kernel", "bias0": "stem/cnnLayercnn_0/biases/bias",
             "kernel1": "stem/cnnLayercnn_1/kernels/kernel", "bias1": "stem/cnnLayercnn_1/biases/bias"}


def _check_fused(config):
    g = lambda n, dflt: getattr(config, n, dflt)
    if g("stemLinear", False) or g("stemBN", False) or g("stemGridRnn", False) or g("locationAware", False):
        raise UnsupportedOptions("stem: only the default 2-layer 3x3 CNN has a fused HIP path")
    if g("stemNumLayers", 2) != 2 or g("stemKernelSize", 3) != 3 or g("stemKernelSizes", None) or g("stemStrideSizes", None):
        raise UnsupportedOptions("stem: the fused stem is stemNumLayers=2, stemKernelSize=3, stride 1 only")


class Stem(unit.FusedUnit):
    """Fused stem (the default 2-layer 3x3 CNN).  Constructing it for any other option set returns a GenericStem: the same
    interface on one general convolution per layer."""
    FIELDS, REF_NAMES, ABI = _lib.STEM_FIELDS, REF_NAMES, "stem"
    SHAPES, PARAMS, GRADS = _lib.MacxStemShapes, _lib.MacxStemParams, _lib.MacxStemGrads
    check_fused = staticmethod(_check_fused)
    SIZE_ERROR = "stem: channel counts must be multiples of 128"

    def __init__(self, config, H=14, W=14, inDim=1024, generator=None):
        super().__init__()
        g = lambda n, dflt: getattr(config, n, dflt)
        _check_fused(config)
        self.H, self.W, self.inDim = H, W, inDim
        self.midDim, self.outDim = g("stemDim", 512), g("memDim", 512)
        self.act = _resolve_act(config, "RELU")               # CNNLayer's default act (ops.py:423)
        self.keep = float(g("stemDropout", 0.82))
        shapes = {"kernel0": (3, 3, inDim, self.midDim), "bias0": (self.midDim,), "kernel1": (3, 3, self.midDim, self.outDim),
                  "bias1": (self.outDim,)}
        for f in self.FIELDS:
            sh = shapes[f]
            if f.startswith("bias"):
                t = torch.zeros(sh)
            else:   # xavier-uniform over conv fans (ops.py:30): fan_in = 9*in, fan_out = 9*out
                t = unit.xavier_uniform(sh, 9 * sh[2] + 9 * sh[3], generator)
            self.register_parameter(f, torch.nn.Parameter(t))
        self.out_hw = (H, W)

    def forward(self, images, train=False, seed=None, b0=0, mask_word=None):
        """images: [B, H*W, inDim] / [B, H, W, inDim] (NHWC, what the graph sees after model.py:68) or the feed-dict layout
        [B, inDim, H, W] (h5 features, extract_features.py), which is transposed on the device first.
        mask_word: None, or the run's mask word (1-element int32 device tensor, as MACCell's), XORed into both dropout keys when
        the kernels run."""
        unit.require_device(images, "the stem")
        if images.dim() == 4 and images.shape[1] == self.inDim and tuple(images.shape[2:]) == (self.H, self.W):
            images = k_nchw_to_nhwc(images.contiguous(), self.inDim, self.H * self.W)
        elif images.dim() == 4:
            images = images.reshape(images.shape[0], self.H * self.W, self.inDim)
        sh = self.SHAPES(B=images.shape[0], H=self.H, W=self.W, Cin=self.inDim, Cmid=self.midDim, Cout=self.outDim, b0=int(b0))
        return self._call(sh, (self.act, self.keep if train else 1.0), seed, train, mask_word, images)

    def _outputs(self, sh, inputs):
        kb = torch.empty(sh.B, self.H * self.W, self.outDim, dtype=torch.float32, device=inputs[0].device)
        return (kb,), (kb,)                                   # (the backward pass reads the knowledge base, not the images)

    def _backward(self, sh, X, d_outs):
        return (d_outs[0].contiguous(),), (), (None,)         # image features are inputs, not trained (extract_features.py)


# -------------------------------------------------------------------------------------------------------------------
# the generic stem: every stem MACnet.stem builds (model.py:165-204) on the general convolution of macx_conv2d_*
# -------------------------------------------------------------------------------------------------------------------
SITE_STEM0, SITE_STEM1 = 9, 10          # the fused stem's dropout sites (macx_common.hip.h): layer 0's input, the later layers'


def out_dim(n, stride):
    """TF SAME: ceil(n / stride)"""
    return -(-n // stride)


def same_pads(n, k, stride):
    """(before, after) padding of TF's SAME along one axis of length n: the odd row goes after"""
    tot = max((out_dim(n, stride) - 1) * stride + k - n, 0)
    return tot // 2, tot - tot // 2


def location_grid(locType, H, W, locationDim, bias):
    """ops.locationL / ops.locationPE (ops.py:440-498) with mod = CNCT: the [H, W, c] float64 grid concatenated to the images.
    L: [x, y] from tf.meshgrid ("xy": channel 0 varies along W); PE: [sin x, cos x, sin y, cos y] of x / 10000^(i / dim)."""
    x = torch.linspace(-bias, bias, W, dtype=torch.float64)
    y = torch.linspace(-bias, bias, H, dtype=torch.float64)
    if locType == "L":
        return torch.stack([x.expand(H, W), y[:, None].expand(H, W)], dim=-1)
    if locType == "PE":
        i = torch.arange(locationDim, dtype=torch.float64)[None, :]
        fx, fy = x[:, None] / torch.pow(10000.0, i / locationDim), y[:, None] / torch.pow(10000.0, i / locationDim)
        parts = [fx.sin()[None].expand(H, W, -1), fx.cos()[None].expand(H, W, -1),
                 fy.sin()[:, None].expand(H, W, -1), fy.cos()[:, None].expand(H, W, -1)]
        return torch.cat(parts, dim=-1)
    raise KeyError(locType)          # ops.locations[locType] (argparse admits L / PE only)


def stem_layers(config, inDim, outDim):
    """The layer plan of MACnet.stem for an option set, raising what the reference raises while it builds the graph.
    Returns (linear, loc, layers): loc = (locationType, channels) or None; layers = [(k, stride, in, out)] in graph order."""
    g = lambda n, dflt: getattr(config, n, dflt)
    if g("stemLinear", False):                    # model.py:176-177: ops.linear(images, inDim, outDim), nothing else is read
        return True, None, [(1, 1, inDim, outDim)]
    L = int(g("stemNumLayers", 2))
    dims = [inDim] + [int(g("stemDim", 512))] * (L - 1) + [outDim]
    loc = None
    if g("locationAware", False):                 # model.py:181-184, ops.addLocation(mod = "CNCT")
        t = g("locationType", "L")
        c = 2 if t == "L" else 4 * int(g("locationDim", 32))
        if t not in ("L", "PE"):
            raise KeyError(t)
        loc = (t, c)
        dims[0] = inDim + c
    n = len(dims) - 1                             # ops.CNNLayer (ops.py:425-438)
    ksizes = g("stemKernelSizes", None)
    ksizes = [int(g("stemKernelSize", 3))] * n if ksizes is None else list(ksizes)
    strides = g("stemStrideSizes", None)
    strides = [1] * n if strides is None else list(strides)
    layers = []
    for i in range(n):
        k, s = int(ksizes[i]), int(strides[i])    # a list shorter than the layer count: IndexError, as in the reference
        if g("stemBN", False):
            # ops.cnn reads batchNorm["center"] from the dict model.py:96 builds without that key (after creating the kernel)
            raise KeyError("center")
        if k < 1 or s < 1:
            raise ValueError("stem layer %d: kernel size %d / stride %d (conv2d needs both >= 1)" % (i, k, s))
        layers.append((k, s, dims[i], dims[i + 1]))
    if g("stemGridRnn", False):
        raise NameError("name 'H' is not defined")   # model.py:199 ops.multigridRNNLayer(features, H, W, outDim)
    return False, loc, layers


def _ceil4(n):
    return (n + 3) // 4 * 4


# the kernel calls of the generic stem (tests/test_stem_variants_host.py swaps exactly these, together with generic.k_dropout /
# k_act / k_act_bwd / k_reduce, for torch restatements)
def k_conv_fwd(x, w, b, stride):
    """x [B,H,W,Cin], w [k,k,Cin,Cout] (HWIO), b [Cout] -> [B,Ho,Wo,Cout] (macx_conv2d_fwd)"""
    B, H, W, Cin = x.shape
    k, Cout = w.shape[0], w.shape[3]
    sh = _lib.MacxConvShapes(B, H, W, Cin, Cout, k, stride)
    y = torch.empty(B, out_dim(H, stride), out_dim(W, stride), Cout, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().macx_conv2d_fwd(C.byref(sh), _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), _lib.stream_of(x)),
               "macx_conv2d_fwd")
    return y


def k_conv_bwd_data(dy, w, x_shape, stride):
    B, H, W, Cin = x_shape
    k, Cout = w.shape[0], w.shape[3]
    sh = _lib.MacxConvShapes(B, H, W, Cin, Cout, k, stride)
    dx = torch.empty(B, H, W, Cin, dtype=torch.float32, device=dy.device)
    _lib.check(_lib.lib().macx_conv2d_bwd_data(C.byref(sh), _lib.ptr(dy), _lib.ptr(w), _lib.ptr(dx), _lib.stream_of(dy)),
               "macx_conv2d_bwd_data")
    return dx


def k_conv_wgrad(x, dy, w_shape, stride):
    B, H, W, Cin = x.shape
    k, Cout = w_shape[0], w_shape[3]
    sh = _lib.MacxConvShapes(B, H, W, Cin, Cout, k, stride)
    L = _lib.lib()
    n_ws = L.macx_conv2d_ws_floats(C.byref(sh))
    ws = torch.empty(max(n_ws, 1), dtype=torch.float32, device=x.device)
    dw = torch.empty(tuple(w_shape), dtype=torch.float32, device=x.device)
    _lib.check(L.macx_conv2d_wgrad(C.byref(sh), _lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), _lib.ptr(ws), n_ws, _lib.stream_of(x)),
               "macx_conv2d_wgrad")
    return dw


def k_nchw_to_nhwc(src, C_, HW):
    out = torch.empty(src.shape[0], HW, C_, dtype=torch.float32, device=src.device)
    _lib.check(_lib.lib().macx_images_to_nhwc(src.data_ptr(), src.shape[0], C_, HW, out.data_ptr(), _lib.stream_of(src)),
               "macx_images_to_nhwc")
    return out


class _Conv(torch.autograd.Function):
    """tf.nn.conv2d(x, w, [1, s, s, 1], "SAME") + b (ops.cnn, ops.py:401-406): forward, backward-data, kernel gradient, and the
    bias gradient as a fixed-order column sum of dy"""

    @staticmethod
    def forward(ctx, x, w, b, stride):
        x, w, b = generic._dev(x, "stem input"), generic._dev(w, "kernel"), generic._dev(b, "bias")
        ctx.stride = stride
        ctx.save_for_backward(x, w)
        return k_conv_fwd(x, w, b, stride)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        Cout = g.shape[-1]
        dx = k_conv_bwd_data(g, w, tuple(x.shape), ctx.stride) if ctx.needs_input_grad[0] else None
        dw = k_conv_wgrad(x, g, tuple(w.shape), ctx.stride) if ctx.needs_input_grad[1] else None
        db = generic.k_reduce(generic.R_ROWS, g, g.numel() // Cout, 1, Cout) if ctx.needs_input_grad[2] else None
        return dx, dw, db, None


class GenericStem(torch.nn.Module):
    """MACnet.stem (model.py:165-204) for any option set the reference builds: ops.CNNLayer's layers (per-layer kernel sizes and
    strides, TF SAME padding, dropout(stemDropout) on every layer input, bias, CNNLayer's "RELU" after every layer), the
    location grid of --locationAware concatenated in front of layer 0, or --stemLinear's single dense layer.  Same interface
    as Stem; the knowledge base has out_hw = (Ho, Wo) cells per image (ceil(H / prod(strides)) ...).

    Variables (names, shapes, creation order) are the reference's: stem/cnnLayercnn_{i}/kernels/kernel [k,k,in,out] and
    .../biases/bias [out], or stem/linearLayer/weights/weight [in,out] and .../biases/bias.
    Dropout masks: layer 0's input (images plus location channels) on (SITE_STEM0, step 0), layer i >= 1's on (SITE_STEM1, step
    i - 1), flat index over the layer's logical [B, H_i, W_i, C_i] input from global question b0 -- the fused stem's masks when
    there are two layers."""

    def __init__(self, config, H=14, W=14, inDim=1024, generator=None):
        super().__init__()
        g = lambda n, dflt: getattr(config, n, dflt)
        self.H, self.W, self.inDim = H, W, inDim
        self.outDim = int(g("memDim", 512))
        self.linear, self.loc, self.layers = stem_layers(config, inDim, self.outDim)
        bad = [c for c in [inDim] + [cout for (_, _, _, cout) in self.layers] if c % 4]   # (layer 0's location channels: padded)
        if bad:
            raise UnsupportedOptions("stem: channel counts must be multiples of 4 (16-byte rows), got %d" % bad[0])
        self.act = _resolve_act(config, "RELU")       # CNNLayer's default act (ops.py:423)
        self.keep = float(g("stemDropout", 0.82))
        self.grid = None
        if self.loc is not None:
            self.grid = location_grid(self.loc[0], H, W, int(g("locationDim", 32)), float(g("locationBias", 1.0))).float()
        self.names = []
        hw = (H, W)
        for i, (k, s, cin, cout) in enumerate(self.layers):
            scope = "stem/linearLayer" if self.linear else "stem/cnnLayercnn_%d" % i
            shape = (cin, cout) if self.linear else (k, k, cin, cout)
            w = unit.xavier_uniform(shape, (cin + cout) * (1 if self.linear else k * k), generator)
            wname, bname = ("weights/weight", "biases/bias") if self.linear else ("kernels/kernel", "biases/bias")
            self.register_parameter("kernel%d" % i, torch.nn.Parameter(w))
            self.register_parameter("bias%d" % i, torch.nn.Parameter(torch.zeros(cout)))
            self.names += [("kernel%d" % i, scope + "/" + wname), ("bias%d" % i, scope + "/" + bname)]
            hw = (out_dim(hw[0], s), out_dim(hw[1], s))
        self.out_hw = hw

    @property
    def N(self):
        return self.out_hw[0] * self.out_hw[1]

    def tensors(self):
        return [getattr(self, f) for f, _ in self.names]

    def to_reference_dict(self):
        return {n: getattr(self, f).detach().clone() for f, n in self.names}

    @torch.no_grad()
    def load_reference_dict(self, ref):
        """Adopt {TF variable name: array} (names with or without 'macModel/' and ':0')."""
        src = {}
        for k, v in ref.items():
            k = k[len("macModel/"):] if k.startswith("macModel/") else k
            src[k[:-2] if k.endswith(":0") else k] = v
        for f, n in self.names:
            if n in src:
                p = getattr(self, f)
                v = torch.as_tensor(src[n])
                if tuple(v.shape) != tuple(p.shape):
                    raise ValueError("%s: shape %s, the stem wants %s" % (n, tuple(v.shape), tuple(p.shape)))
                p.copy_(v.to(p.dtype))
        return self

    def forward(self, images, train=False, seed=None, b0=0, mask_word=None):
        """images: [B, H*W, inDim] / [B, H, W, inDim] (NHWC) or the feed-dict layout [B, inDim, H, W].
        Returns the knowledge base [B, Ho*Wo, memDim]."""
        unit.refuse_mask_word(mask_word, "stem", "macx_stem_forward_w")
        generic._require_device(images, "images")
        H, W, B = self.H, self.W, images.shape[0]
        if images.dim() == 4 and images.shape[1] == self.inDim and tuple(images.shape[2:]) == (H, W):
            images = k_nchw_to_nhwc(images.contiguous(), self.inDim, H * W)
        x = images.reshape(B, H, W, self.inDim)
        b0 = int(b0)
        if self.linear:                               # ops.linear: no dropout, no activation
            w = getattr(self, "kernel0")
            y = _Conv.apply(x, w.reshape(1, 1, *w.shape), self.bias0, 1)
            return y.reshape(B, H * W, self.outDim)
        if self.grid is not None:
            grid = self.grid.to(x.device)
            x = torch.cat([x, grid[None].expand(B, H, W, grid.shape[-1])], dim=-1)
        keep = self.keep if train else 1.0
        seed = fresh_seed(seed, train) & 0xFFFFFFFF
        for i, (k, s, cin, cout) in enumerate(self.layers):
            if keep < 1.0:
                per_q = x.shape[1] * x.shape[2] * cin
                if (b0 + B) * per_q >= 1 << 32:
                    raise ValueError("stem dropout: (b0 + B) * H * W * C = %d reaches the 32-bit element index" % ((b0 + B) * per_q))
                site, step = (SITE_STEM0, 0) if i == 0 else (SITE_STEM1, i - 1)
                x = generic._Dropout.apply(x, seed, site, step, keep, b0 * per_q)
            w = getattr(self, "kernel%d" % i)
            if cin % 4:                               # location channels (1024 + 2): zero channels meet zero kernel rows
                pad = _ceil4(cin) - cin
                x = torch.nn.functional.pad(x, (0, pad))
                w = torch.nn.functional.pad(w, (0, 0, 0, pad))
            x = generic._Act.apply(_Conv.apply(x, w, getattr(self, "bias%d" % i), s), self.act, None)
        return x.reshape(B, self.N, self.outDim)


Stem.GENERIC = GenericStem

# -------------------------------------------------------------------------------------------------------------------
# questions that share images: the stem runs once per image, every question gets a copy of its image's block
# -------------------------------------------------------------------------------------------------------------------
def check_image_index(image_index, B, train, stem, images=None, host_check=False):
    """The validation of model.MACNet(Core).forward's image_index (a [B] integer tensor: question b looks at images[image_index[b]]),
    done before anything asks for the device.  Returns None for None.  host_check: also 0 <= index < G on the host (synchronises)."""
    if image_index is None:
        return None
    if not torch.is_tensor(image_index) or image_index.dim() != 1 or image_index.shape[0] != B:
        raise ValueError("image_index must be a [%d] tensor, one image number per question; got %s"
                         % (B, tuple(image_index.shape) if torch.is_tensor(image_index) else type(image_index).__name__))
    if image_index.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError("image_index must have an integer dtype, not %s" % image_index.dtype)
    keep = 1.0 if getattr(stem, "linear", False) else float(stem.keep)       # (--stemLinear has no dropout)
    if train and keep < 1.0:
        # model.py:165-204 feeds every question its own copy of the image and draws the stem's dropout mask per question
        raise ValueError("image_index with train=True needs stemDropout = 1.0 (this stem keeps %g): the reference draws the stem's "
                         "dropout mask per question, which one stem pass per image cannot reproduce" % keep)
    if host_check and images is not None and B > 0:
        G = images.shape[0]
        lo, hi = int(image_index.min()), int(image_index.max())
        if lo < 0 or hi >= G:
            raise IndexError("image_index outside [0, %d)" % G)
    return image_index


def check_image_lengths(image_lengths, image_index, kb_lengths, images=None, N=None, host_check=False):
    """The validation of model.MACNet(Core).forward's image_lengths (a [G] integer tensor: image g's knowledge base is the first
    image_lengths[g] of the stem's N cells), done before anything asks for the device.  Returns None for None.  host_check (with N):
    also 1 <= length <= N on the host (synchronises)."""
    if image_lengths is None:
        return None
    if image_index is None:
        raise ValueError("image_lengths are the sizes of shared images: they need image_index (one image per question: kb_lengths)")
    if kb_lengths is not None:
        raise ValueError("image_lengths and kb_lengths both given: with image_lengths the per-question sizes are made on the device "
                         "(image_lengths[image_index])")
    G = None if images is None else images.shape[0]
    if not torch.is_tensor(image_lengths) or image_lengths.dim() != 1 or (G is not None and image_lengths.shape[0] != G):
        raise ValueError("image_lengths must be a [%s] tensor, one size per image; got %s"
                         % ("G" if G is None else G, tuple(image_lengths.shape) if torch.is_tensor(image_lengths) else type(image_lengths).__name__))
    if image_lengths.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError("image_lengths must have an integer dtype, not %s" % image_lengths.dtype)
    if host_check and N is not None and image_lengths.numel():
        lo, hi = int(image_lengths.min()), int(image_lengths.max())
        if lo < 1 or hi > N:
            raise ValueError("image_lengths must lie in [1, %d] (the knowledge base's cells); got %d .. %d" % (N, lo, hi))
    return image_lengths


class _KBGather(torch.autograd.Function):
    """(kb, kb_lengths) = macx_kb_gather_l(kb_images, index, lengths); backward: the fixed-order sum of macx_kb_gather_bwd_l.
    lengths None (NULL; the plain macx_kb_gather / _bwd, which the library forwards to): kb[b] = kb_images[index[b]], kb_lengths None.
    Else question b's block is its image's first L rows and +0 behind them, kb_lengths[b] = L, L = clamp(lengths[index[b]], 1, N),
    and the backward pass writes zeros into every image's padded rows.
    index [B] and lengths [G]: int32 on the device, read when the kernels run."""

    @staticmethod
    def forward(ctx, kb_images, index, lengths):
        kb_images = generic._dev(kb_images, "the stem's output")
        generic._require_device(index, "image_index")
        if index.dtype != torch.int32 or not index.is_contiguous():
            index = index.to(torch.int32).contiguous()
        G, N, d = kb_images.shape
        B = index.shape[0]
        kb_lengths = None
        if lengths is not None:
            generic._require_device(lengths, "image_lengths")
            if lengths.dtype != torch.int32 or not lengths.is_contiguous():
                lengths = lengths.to(torch.int32).contiguous()
            if lengths.shape != (G,):
                raise ValueError("image_lengths must be [%d], one size per image" % G)
            kb_lengths = torch.empty(B, dtype=torch.int32, device=kb_images.device)
            ctx.mark_non_differentiable(kb_lengths)
        kb = torch.empty(B, N, d, dtype=torch.float32, device=kb_images.device)
        ptr = _lib.ptr
        _lib.check(_lib.lib().macx_kb_gather_l(ptr(kb_images), ptr(index), ptr(lengths), G, B, N, d, ptr(kb), ptr(kb_lengths),
                                               _lib.stream_of(kb)), "macx_kb_gather_l")
        ctx.index, ctx.lengths, ctx.G = index, lengths, G
        return kb, kb_lengths

    @staticmethod
    def backward(ctx, dkb, _):
        dkb = dkb.contiguous()
        B, N, d = dkb.shape
        out = torch.empty(ctx.G, N, d, dtype=torch.float32, device=dkb.device)
        ptr = _lib.ptr
        _lib.check(_lib.lib().macx_kb_gather_bwd_l(ptr(dkb), ptr(ctx.index), ptr(ctx.lengths), ctx.G, B, N, d, ptr(out),
                                                   _lib.stream_of(out)), "macx_kb_gather_bwd_l")
        return out, None, None


def kb_gather(kb_images, image_index, image_lengths=None):
    """[G, N, d] stem output -> the [B, N, d] knowledge base of B questions (differentiable in kb_images).
    image_lengths: None, or a [G] integer device tensor, the live cells of each image; then returns (kb, kb_lengths): the padded
    rows of kb are +0 whatever the stem's output holds there, kb_lengths [B] int32 is what the cell takes (made on the device)."""
    kb, kb_lengths = _KBGather.apply(kb_images, image_index, image_lengths)
    return kb if image_lengths is None else (kb, kb_lengths)
