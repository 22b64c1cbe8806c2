"""TEST INFRASTRUCTURE -- not part of the product path.

torch fp64 restatement of MACnet.stem (model.py:165-204) for every stem option the reference builds: --stemNumLayers,
--stemKernelSize / --stemKernelSizes, --stemStrideSizes, --stemDim, --stemLinear and --locationAware (ops.addLocation with
mod = "CNCT", ops.locationL / ops.locationPE, ops.py:440-560), over ops.CNNLayer / ops.cnn (ops.py:380-438) with TF's SAME
padding for any kernel size and stride.  Dropout takes explicit 0/1 masks, one per layer input, in layer order.

tests/test_stem_variants_reference.py pins it to the reference's own code; the product's GenericStem is checked against it.
"""
import math

import torch
import torch.nn.functional as F


def opt(cfg, name, dflt):
    return getattr(cfg, name, dflt)


def same_pads(n, k, s):
    """TF SAME along one axis: out = ceil(n / s); pad_total = max((out - 1) s + k - n, 0); the odd row after"""
    o = -(-n // s)
    tot = max((o - 1) * s + k - n, 0)
    return tot // 2, tot - tot // 2


def conv2d_same(x, w, s):
    """tf.nn.conv2d(x, w, [1, s, s, 1], "SAME"): x NHWC, w HWIO"""
    k = w.shape[0]
    pt, pb = same_pads(x.shape[1], k, s)
    pl, pr = same_pads(x.shape[2], k, s)
    xp = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xp, w.permute(3, 2, 0, 1), stride=s).permute(0, 2, 3, 1)


def location_grid(loc_type, h, w, dim, bias, dtype=torch.float64):
    """ops.locationL / ops.locationPE: [h, w, 2] or [h, w, 4 dim]"""
    xs = torch.linspace(-bias, bias, w, dtype=dtype)
    ys = torch.linspace(-bias, bias, h, dtype=dtype)
    if loc_type == "L":
        gx, gy = torch.meshgrid(xs, ys, indexing="xy")          # tf.meshgrid's default "xy": [h, w], gx varies along w
        return torch.stack([gx, gy], dim=-1)
    x, y = xs[:, None], ys[:, None]
    i = torch.arange(dim, dtype=dtype)[None, :]
    sx, cx = torch.sin(x / torch.pow(10000.0, i / dim)), torch.cos(x / torch.pow(10000.0, i / dim))
    sy, cy = torch.sin(y / torch.pow(10000.0, i / dim)), torch.cos(y / torch.pow(10000.0, i / dim))
    tile_x = lambda t: t[None].repeat(h, 1, 1)                 # noqa: E731
    tile_y = lambda t: t[:, None].repeat(1, w, 1)              # noqa: E731
    return torch.cat([tile_x(sx), tile_x(cx), tile_y(sy), tile_y(cy)], dim=-1)


def plan(cfg, in_dim, out_dim):
    """(linear, loc_channels, [(scope, kernel shape, stride)]) as MACnet.stem builds it; raises what the reference raises"""
    if opt(cfg, "stemLinear", False):
        return True, 0, [("stem/linearLayer", (in_dim, out_dim), 1)]
    L = opt(cfg, "stemNumLayers", 2)
    dims = [in_dim] + [opt(cfg, "stemDim", 512)] * (L - 1) + [out_dim]
    loc = 0
    if opt(cfg, "locationAware", False):
        loc = 2 if opt(cfg, "locationType", "L") == "L" else 4 * opt(cfg, "locationDim", 32)
        dims[0] = in_dim + loc
    n = len(dims) - 1
    ks = [opt(cfg, "stemKernelSize", 3)] * n if opt(cfg, "stemKernelSizes", None) is None else opt(cfg, "stemKernelSizes", None)
    st = [1] * n if opt(cfg, "stemStrideSizes", None) is None else opt(cfg, "stemStrideSizes", None)
    layers = []
    for i in range(n):
        k, s = ks[i], st[i]
        if opt(cfg, "stemBN", False):
            raise KeyError("center")
        layers.append(("stem/cnnLayercnn_%d" % i, (k, k, dims[i], dims[i + 1]), s))
    if opt(cfg, "stemGridRnn", False):
        raise NameError("name 'H' is not defined")
    return False, loc, layers


def variable_names(cfg, in_dim, out_dim):
    """[(name, shape)] in creation order"""
    linear, _, layers = plan(cfg, in_dim, out_dim)
    out = []
    for scope, shape, _ in layers:
        out += [(scope + ("/weights/weight" if linear else "/kernels/kernel"), shape), (scope + "/biases/bias", (shape[-1],))]
    return out


def xavier_limit(shape):
    rf = 1
    for s in shape[:-2]:
        rf *= s
    return math.sqrt(6.0 / (shape[-2] * rf + shape[-1] * rf))


def relu_of(cfg):
    r = opt(cfg, "relu", "STD")
    return (lambda x: torch.relu(x)) if r == "STD" else (lambda x: torch.where(x > 0, x, torch.expm1(torch.clamp(x, max=0))))


def stem(cfg, images, params, out_dim, keep=1.0, masks=None):
    """images [B, H, W, C] (fp64) -> [B, Ho*Wo, out_dim]; params {name: tensor}; masks: one 0/1 tensor per layer input"""
    B, H, W, C = images.shape
    linear, loc, layers = plan(cfg, C, out_dim)
    if linear:
        (scope, _, _), = layers
        y = images.reshape(-1, C) @ params[scope + "/weights/weight"] + params[scope + "/biases/bias"]
        return y.reshape(B, H * W, out_dim)
    x = images
    if loc:
        grid = location_grid(opt(cfg, "locationType", "L"), H, W, opt(cfg, "locationDim", 32), opt(cfg, "locationBias", 1.0),
                             images.dtype)
        x = torch.cat([x, grid[None].expand(B, H, W, loc)], dim=-1)
    act = relu_of(cfg)
    for i, (scope, _, s) in enumerate(layers):
        if masks is not None:
            x = x / keep * masks[i]
        x = act(conv2d_same(x, params[scope + "/kernels/kernel"], s) + params[scope + "/biases/bias"])
    return x.reshape(B, -1, out_dim)
