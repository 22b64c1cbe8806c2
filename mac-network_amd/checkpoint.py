"""Weights in and out under the reference's TF variable names (SURVEY.md 8b "parameters", 8f row 4 "ckpt formats").

Two carriers: the reference's own V2 checkpoint files (`load_tf_checkpoint` / `save_tf_checkpoint`, read and written by
tf_bundle.py without TensorFlow), and an .npz of the same name -> array mapping, which a maintainer can also dump in a
TF environment

    np.savez("macx_weights.npz", **{v.name: sess.run(v) for v in tf.global_variables()})      # main.py:185-193 restores them

Names are `macModel/<scope>/...:0` (model.py:774); EMA shadows (model.py:659-663, main.py:172-174 `emaSaver`) are
`<name>/ExponentialMovingAverage`.  `load_reference` accepts names with or without the `macModel/` prefix and the `:0`
suffix; `reference_state_dict` / `save_npz` emit the canonical form.

Optimizer state.  The reference's OWN slots are not imported from a TensorFlow checkpoint: its `saver` stores them under
`trainAddOptimizer/...` names that depend on graph construction order, so they cannot be matched to variables reliably (and
`save_tf_checkpoint` writes none).  This project's own state does travel, in the .npz carrier: `save_npz(path, net,
optimizer=opt)` adds, per variable the optimizer owns, `<name>/Adam:0` (m), `<name>/Adam_1:0` (v) and
`<name>/ExponentialMovingAverage:0` (opt.ema) -- names `load_reference` ignores, so the file still loads as plain weights -- and
under `macx/optimizer/` the scalars `step` (opt.t, which counts attempts: optim.FlatAdamEMA), `lr`, `beta1`, `beta2`, `eps`,
`clip_norm`, `ema_decay`, and `guard` (the four words) for a guarded optimizer.  `load_npz(path, net, optimizer=opt)` puts all of
it back in place: training continues bit for bit.
"""
import numpy as np
import torch

PREFIX = "macModel/"
EMA_SUFFIX = "/ExponentialMovingAverage"
OPT_PREFIX = "macx/optimizer/"
OPT_SCALARS = ("step", "lr", "beta1", "beta2", "eps", "clip_norm", "ema_decay")
# (flat buffer of the optimizer, suffix of its variables' slot names); ema only where the optimizer keeps one
OPT_SLOTS = (("m", "/Adam"), ("v", "/Adam_1"), ("ema", EMA_SUFFIX))


def _modules(net):
    mods = []
    for attr in ("enc", "stem", "cell", "out"):
        m = getattr(net, attr, None)
        if hasattr(m, "to_reference_dict"):          # (a GenericQuestionEncoder's own .enc is a width)
            mods.append(m)
    if not mods:          # a single component (MACCellParams, Stem, ...)
        mods = [net]
    return mods


def reference_state_dict(net):
    """{TF variable name: tensor (CPU)} for a MACNet / MACNetCore / single component."""
    out = {}
    for m in _modules(net):
        for k, v in m.to_reference_dict().items():
            out[PREFIX + k + ":0"] = v.detach().cpu()
    return out


def _normalise(d):
    out = {}
    for k, v in d.items():
        k = k[:-2] if k.endswith(":0") else k
        k = k[len(PREFIX):] if k.startswith(PREFIX) else k
        out[k] = v
    return out


@torch.no_grad()
def load_reference(net, d, use_ema=False, strict=True):
    """Copy weights named as in the reference into `net`.  use_ema: take the `/ExponentialMovingAverage` shadow of each
    variable when present (what the reference evaluates with, main.py:172-174).  strict: every variable of `net` must be
    present with the reference's shape; extra keys (optimizer slots, baseline variables) are ignored."""
    src = _normalise(d)
    if use_ema:
        for k in list(src):
            if k.endswith(EMA_SUFFIX):
                src[k[:-len(EMA_SUFFIX)]] = src[k]
    missing, bad = [], []
    lazy = [m for m in _modules(net) if getattr(m, "lazy_scopes", None)]
    for m in lazy:
        # a module whose variables only appear on first use (generic.GenericParams before the first forward pass) has nothing to
        # ask for yet: hand it every model variable stored under its scope, so that the first forward finds them instead of
        # drawing fresh ones
        scoped = {k: v for k, v in src.items() if k.startswith(tuple(m.lazy_scopes)) and not k.endswith(EMA_SUFFIX)
                  and "/Adam" not in k and "/ExponentialMovingAverage" not in k}
        have_now = set(m.to_reference_dict())
        new = {k: v for k, v in scoped.items() if k not in have_now}
        if new:
            m.load_reference_dict(new)
        if strict and not m.tensors():
            raise KeyError("no variable under %s in the source: the lazily built module would start from random weights"
                           % (m.lazy_scopes,))
    for m in _modules(net):
        want = m.to_reference_dict()
        for k, w in want.items():
            if k not in src:
                missing.append(k)
            elif tuple(np.shape(src[k])) != tuple(w.shape):
                bad.append((k, tuple(np.shape(src[k])), tuple(w.shape)))
    if bad:
        raise ValueError("shape mismatch (name, given, expected): %s" % bad[:5])
    if missing and strict:
        raise KeyError("missing variables: %s%s" % (missing[:5], " ..." if len(missing) > 5 else ""))
    for m in _modules(net):
        want = m.to_reference_dict()
        have = {k: (src[k] if k in src else want[k]) for k in want}
        m.load_reference_dict(have)
    return missing


def _slots(opt):
    return [(getattr(opt, attr), suffix) for attr, suffix in OPT_SLOTS if getattr(opt, attr) is not None]


def _owned(net, opt):
    """the optimizer's parameters matched to the net's tensors by identity -> the canonical names of the variables they make up.
    A slot follows its parameter through to_reference_dict / load_reference_dict (slices and reshapes), so the names are found
    the same way: ones in the optimizer's tensors, zeros in the others, and a variable is owned iff it comes out all ones."""
    mine = {id(t) for t in net.tensors()}
    stray = [i for i, p in enumerate(opt.params) if id(p) not in mine]
    if stray:
        raise ValueError("the optimizer holds %d tensor(s) the net does not own (first: parameter %d): it was built over another net"
                         % (len(stray), stray[0]))
    own = {id(p) for p in opt.params}
    live = [p.detach().clone() for p in net.tensors()]
    try:
        with torch.no_grad():
            for p in net.tensors():
                p.fill_(1.0 if id(p) in own else 0.0)
        marks = {k: v.numpy() for k, v in reference_state_dict(net).items()}
    finally:
        with torch.no_grad():
            for p, l in zip(net.tensors(), live):
                p.copy_(l)
    mixed = [k for k, v in marks.items() if (v == 1.0).any() and not (v == 1.0).all()]
    if mixed:
        raise ValueError("variables made of tensors inside and outside the optimizer: %s" % mixed[:5])
    return sorted(k for k, v in marks.items() if v.size and (v == 1.0).all())


def _optimizer_arrays(net, opt):
    """{key: array} of an optim.FlatAdamEMA's state: the slots of every owned variable, the scalars, the guard words"""
    owned = _owned(net, opt)
    arrs = {}
    live = opt.flat.clone()
    try:
        with torch.no_grad():
            for buf, suffix in _slots(opt):
                opt.flat.copy_(buf)                  # the parameters are views of opt.flat: they now show the slot
                named = reference_state_dict(net)
                for k in owned:
                    arrs[k[:-2] + suffix + ":0"] = named[k].numpy()
    finally:
        with torch.no_grad():
            opt.flat.copy_(live)
    arrs[OPT_PREFIX + "step"] = np.asarray(opt.t, dtype=np.int64)
    for name in OPT_SCALARS[1:]:
        arrs[OPT_PREFIX + name] = np.asarray(getattr(opt, name), dtype=np.float64)
    if getattr(opt, "guard", None) is not None:
        arrs[OPT_PREFIX + "guard"] = opt.guard.cpu().numpy().astype(np.uint32)
    return arrs


@torch.no_grad()
def _load_optimizer(net, opt, src, strict):
    """The reverse, IN PLACE: the slots travel through the parameters (views of opt.flat before and after) into their flat buffers;
    run it BEFORE the weights are loaded.  Everything is looked up first, so a KeyError leaves net and optimizer as they were."""
    owned = _owned(net, opt)
    keys = [k[:-2] + suffix + ":0" for _, suffix in _slots(opt) for k in owned]
    keys += [OPT_PREFIX + n for n in OPT_SCALARS] + ([OPT_PREFIX + "guard"] if getattr(opt, "guard", None) is not None else [])
    missing = [k for k in keys if k not in src]
    if missing and strict:
        raise KeyError("the file carries no optimizer state for: %s%s (written without optimizer=, or by another kind of optimizer)"
                       % (missing[:5], " ..." if len(missing) > 5 else ""))
    live = opt.flat.clone()
    for buf, suffix in _slots(opt):
        opt.flat.copy_(buf)                          # a variable the file lacks (strict=False) keeps the slot it has
        have = {k: src[k[:-2] + suffix + ":0"] for k in owned if k[:-2] + suffix + ":0" in src}
        for m in _modules(net):
            want = m.to_reference_dict()
            m.load_reference_dict({k: have.get(PREFIX + k + ":0", w) for k, w in want.items()})
        buf.copy_(opt.flat)
    opt.flat.copy_(live)
    if OPT_PREFIX + "step" in src:
        opt.t = int(src[OPT_PREFIX + "step"])
    for name in OPT_SCALARS[1:]:                     # (opt.lr_t is rewritten by the next advance())
        if OPT_PREFIX + name in src:
            setattr(opt, name, float(src[OPT_PREFIX + name]))
    if getattr(opt, "guard", None) is not None and OPT_PREFIX + "guard" in src:
        opt.guard.copy_(torch.from_numpy(np.asarray(src[OPT_PREFIX + "guard"]).astype(np.uint32).view(np.int32)))
    return missing


def save_npz(path, net, ema_tensors=None, optimizer=None):
    """Write the reference-named weights (and, when given, the EMA shadows in `net.tensors()` order) to an .npz.
    optimizer: an optim.FlatAdamEMA over tensors of `net` -- its m, v, EMA shadow, step count, hyper-parameters and guard words are
    written too (the module docstring has the keys), which makes the file a checkpoint `load_npz(..., optimizer=)` resumes from bit
    for bit.  The shadow then comes from the optimizer: ema_tensors= as well is a ValueError.  One synchronisation."""
    if optimizer is not None and ema_tensors is not None:
        raise ValueError("save_npz: optimizer= writes the EMA shadow from optimizer.ema; give ema_tensors= or optimizer=, not both")
    arrs = {k: v.numpy() for k, v in reference_state_dict(net).items()}
    if optimizer is not None:
        arrs.update(_optimizer_arrays(net, optimizer))
    if ema_tensors is not None:
        live = [p.detach().clone() for p in net.tensors()]
        try:
            with torch.no_grad():
                for p, e in zip(net.tensors(), ema_tensors):
                    p.copy_(e.reshape(p.shape))
            for k, v in reference_state_dict(net).items():
                arrs[k[:-2] + EMA_SUFFIX + ":0"] = v.numpy()
        finally:
            with torch.no_grad():
                for p, l in zip(net.tensors(), live):
                    p.copy_(l)
    np.savez(path, **arrs)
    return sorted(arrs)


def load_npz(path, net, use_ema=False, strict=True, optimizer=None):
    """optimizer: an optim.FlatAdamEMA over tensors of `net` -- its state is restored from a file written with
    save_npz(..., optimizer=): m, v and the EMA shadow are copied IN PLACE (every parameter stays the view of optimizer.flat it
    was, at the same address), t, the hyper-parameters and the guard words are set.  Under strict a file without that state is a
    KeyError and nothing is changed.  Without optimizer= such a file loads its weights as any other."""
    with np.load(path) as z:
        src = {k: z[k] for k in z.files}
    if optimizer is not None:
        _load_optimizer(net, optimizer, src, strict)
    return load_reference(net, src, use_ema=use_ema, strict=strict)


def load_tf_checkpoint(prefix, net, use_ema=False, strict=True, verify=True):
    """Restore `net` from a TensorFlow V2 checkpoint written by the reference's saver (main.py:236-262), e.g.
    prefix = "weights/clevrExperiment/weights25.ckpt".  Returns the list of missing variables (empty under strict)."""
    from . import tf_bundle
    return load_reference(net, tf_bundle.read_checkpoint(prefix, verify=verify), use_ema=use_ema, strict=strict)


def save_tf_checkpoint(prefix, net):
    """Write the reference-named weights as a V2 checkpoint the reference's `saver.restore` (main.py:185-193) can read
    for every variable it finds (variable names carry no ":0" in a checkpoint)."""
    from . import tf_bundle
    return tf_bundle.write_checkpoint(prefix, {k[:-2]: v.numpy() for k, v in reference_state_dict(net).items()})
