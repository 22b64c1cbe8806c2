"""TEST INFRASTRUCTURE: executes the reference's OWN code -- the upstream project's {config,ops,mac_cell,model}.py,
unmodified -- on the eager TF-1.x stand-in of tests/tf1_shim, and adapts its inputs/outputs so that
oracle/mac_oracle.py can be compared with it on identical parameters, inputs and dropout draws.

What comes from the reference here: the flag parser (config.parseArgs on the published flag files), every
line of MACCell (mac_cell.py:59-592), the ops.py primitives it calls, and MACnet.MACnetwork / outputOp /
classifier / addAnswerLossOp / addPredOp / stem (model.py:165-204, 428-489, 512-612), called as plain functions
on a stand-in `self` that carries only the attributes those methods read.
What does not: TensorFlow (replaced by the shim) -- and therefore TF's RNG stream; draws are injected.

Where the reference's code runs: MACX_REFERENCE_DIR names a checkout of the upstream project.  Without it, every call
below is REPLAYED from tests/golden/reference_exec/ -- what the reference's code returned (parsed flags, states, logits,
draws, variables, the exception it raised) for exactly these arguments, recorded by a live session with
MACX_RECORD_REFERENCE=1.  A replayed result is built like a live one: its variables and inputs are leaf tensors, and a
backward pass through its outputs must bring exactly the cotangents of the recorded session (checked) and receives the
gradients the reference's graph produced for them.  A call that was never recorded fails.
"""
import atexit
import builtins
import hashlib
import importlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

REF = os.environ.get("MACX_REFERENCE_DIR", "")
SHIM = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tf1_shim")
FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_exec")
RECORD = os.environ.get("MACX_RECORD_REFERENCE") == "1"

_mods = {}


# ---------------------------------------------------------------------------------------------------------------
# record / replay.  A result is stored as JSON with references: "rng" = the n-th draw of the stand-in's seeded generator
# (variables and dropout draws: regenerated, not stored), "t" = a stored array, "leaf" / "out" = where autograd connects.
# ---------------------------------------------------------------------------------------------------------------
_store = {}                                        # replay: records and arrays of tests/golden/reference_exec
_new = {"records": {}, "blobs": {}}                # record: this session's


def _digest(a):
    return hashlib.sha1(("%s%s" % (a.dtype, a.shape)).encode() + a.tobytes()).hexdigest()[:20]


def _canon(x):
    """JSON-able, value-based description of a call argument (tensors by content digest)"""
    if isinstance(x, torch.Tensor):
        return "T:" + _digest(x.detach().contiguous().numpy())
    if isinstance(x, dict):
        return {"d": [[str(k), _canon(v)] for k, v in sorted(x.items())]}
    if isinstance(x, (list, tuple)):
        return [_canon(v) for v in x]
    if isinstance(x, float):
        return repr(x)
    if isinstance(x, torch.dtype):
        return str(x)
    if hasattr(x, "__dict__"):                     # the parsed config
        return _canon(vars(x))
    return x


def _cfg_digest(cfg):
    return None if cfg is None else hashlib.sha1(json.dumps(_canon(cfg), sort_keys=True).encode()).hexdigest()[:20]


def _regenerate(rng):
    """the stand-in's generator draws of one run, as tests/tf1_shim computes them"""
    gen, dt, out = torch.Generator().manual_seed(rng["seed"]), getattr(torch, rng["dtype"]), []
    for kind, shape, scale in rng["log"]:
        if kind == "normal":
            out.append((torch.randn(shape, generator=gen, dtype=torch.float64) * scale).to(dt))
        else:
            u = torch.rand(shape, generator=gen, dtype=torch.float64)
            out.append((u if kind == "uniform" else (u * 2 - 1) * scale).to(dt))
    return out


def _encode(x, ctx):
    if isinstance(x, torch.Tensor):
        a = x.detach().contiguous().numpy()
        h = _digest(a)
        e = {"rng": ctx["rng"][h]} if h in ctx["rng"] else {"t": h}
        _new["blobs"].setdefault(h, a) if "t" in e else None
        if x.requires_grad and x.is_leaf:
            if all(t is not x for t in ctx["leaves"]):
                ctx["leaves"].append(x)
            e["leaf"] = [i for i, t in enumerate(ctx["leaves"]) if t is x][0]
        elif x.requires_grad:
            ctx["outs"].append(x)
            e["out"] = len(ctx["outs"]) - 1
        return e
    if isinstance(x, dict):
        return {"d": [[k, _encode(v, ctx)] for k, v in x.items()]}
    if isinstance(x, (list, tuple)):
        return {"l": [_encode(v, ctx) for v in x]}
    if isinstance(x, (bool, int, float, str)) or x is None:
        return {"v": x}
    if all(hasattr(x, a) for a in CELL_ATTRS):     # the reference's MACCell: the histories the tests read
        return {"cell": [[a, _encode(getattr(x, a), ctx)] for a in CELL_ATTRS]}
    raise TypeError("cannot record a %r in a reference result" % type(x))


CELL_ATTRS = ("controls", "memories", "infos", "attentions")


class _Node(torch.autograd.Function):
    """the recorded run as one autograd node: its leaves in, its differentiable outputs out"""

    @staticmethod
    def forward(ctx, backward, values, *leaves):
        ctx.backward = backward
        ctx.set_materialize_grads(False)
        return tuple(v.clone() for v in values)

    @staticmethod
    def backward(ctx, *grads):
        return (None, None) + tuple(ctx.backward(grads))


def _decode(rec, blobs, backward):
    """the result as the tests see it: fresh leaves, the differentiable outputs from one _Node"""
    drawn = _regenerate(rec["rng"]) if "rng" in rec else []
    value = lambda e: (drawn[e["rng"]] if "rng" in e else torch.from_numpy(blobs[e["t"]].copy()))    # noqa: E731
    leaves, outs = {}, {}

    def scan(e):
        if "leaf" in e:
            leaves[e["leaf"]] = value(e).requires_grad_(True)
        elif "out" in e:
            outs[e["out"]] = value(e)
        for v in [v for _, v in e.get("d", []) + e.get("cell", [])] + e.get("l", []):
            scan(v)

    scan(rec["result"])
    leaves = [leaves[i] for i in range(len(leaves))]
    outs = _Node.apply(backward, [outs[i] for i in range(len(outs))], *leaves) if outs else ()

    def build(e):
        if "leaf" in e or "out" in e:
            return leaves[e["leaf"]] if "leaf" in e else outs[e["out"]]
        if "rng" in e or "t" in e:
            return value(e)
        if "d" in e or "cell" in e:
            d = {k: build(v) for k, v in e.get("d", e.get("cell"))}
            return SimpleNamespace(**d) if "cell" in e else d
        return [build(v) for v in e["l"]] if "l" in e else e["v"]

    return build(rec["result"])


def _load_store():
    if not _store:
        _store.update(records={}, blobs={})
        for f in sorted(os.listdir(FIXTURES)) if os.path.isdir(FIXTURES) else []:
            with np.load(os.path.join(FIXTURES, f)) as z:
                for k in z.files:
                    if k == "records":
                        _store["records"].update(json.loads(bytes(z[k]).decode()))
                    else:
                        _store["blobs"][k] = z[k]
    return _store["records"], _store["blobs"]


def _recorded(fn):
    """live call (and, with MACX_RECORD_REFERENCE=1, its record) or the replay of the recorded one"""
    flags = fn.__name__ == "parse_flags"
    sets_answers = fn.__name__ in ("run_reference", "run_reference_training")      # they set cfg.answerWordsNum first thing

    def call(*args, **kw):
        key = hashlib.sha1(json.dumps([fn.__name__, _canon(args), _canon(kw)], sort_keys=True).encode()).hexdigest()
        cfg = None if flags else args[0]
        if available():
            rec = {}
            try:
                res = fn(*args, **kw)
            except Exception as e:              # noqa: BLE001 -- the reference's exception is part of its result
                rec["raise"] = [type(e).__module__, type(e).__name__, str(e)]
                raise
            finally:
                if RECORD:
                    rec["cfg_after"] = _cfg_digest(cfg)
                    _new["records"][key] = rec
            if not RECORD or flags:             # (parse_flags hands out the reference's own config object: its code reads that one)
                if RECORD:
                    rec["result"] = _encode(dict(vars(res)), {"rng": {}, "leaves": [], "outs": []})
                return res
            st = load()["tf"].state
            rec["rng"] = {"seed": st.seed, "dtype": str(st.dtype).split(".")[-1], "log": [list(ev) for ev in st.rng]}
            ctx = {"rng": {_digest(v.numpy()): i for i, v in reversed(list(enumerate(_regenerate(rec["rng"]))))}, "leaves": [], "outs": []}
            rec["result"] = _encode(res, ctx)

            def backward(grads):
                pairs = [(o, g) for o, g in zip(ctx["outs"], grads) if g is not None]
                got = torch.autograd.grad([o for o, _ in pairs], ctx["leaves"], [g for _, g in pairs], allow_unused=True, retain_graph=True)
                rec["backward"] = {k: [None if g is None else _encode(g.detach(), {"rng": {}})["t"] for g in v]
                                   for k, v in (("cot", grads), ("grads", got))}
                return got

            return _decode(rec, _new["blobs"], backward)
        recs, blobs = _load_store()
        rec = recs.get(key)
        if rec is None:
            raise AssertionError("%s: no recorded reference run for these arguments in %s (record them with "
                                 "MACX_REFERENCE_DIR=<upstream checkout> MACX_RECORD_REFERENCE=1)" % (fn.__name__, FIXTURES))
        if sets_answers:
            cfg.answerWordsNum = kw.get("answerWordsNum", 7)
        if _cfg_digest(cfg) != rec["cfg_after"]:
            raise AssertionError("%s: the config differs from the recorded run's after the call" % fn.__name__)
        if "raise" in rec:
            mod, name, msg = rec["raise"]
            if mod != "builtins":
                raise AssertionError("the recorded reference raised %s.%s, which a replay cannot raise" % (mod, name))
            raise getattr(builtins, name)(msg)

        def backward(grads):
            if "backward" not in rec:
                raise AssertionError("%s: the recorded session ran no backward pass through this result" % fn.__name__)
            for i, (g, c) in enumerate(zip(grads, rec["backward"]["cot"])):
                if (g is None) != (c is None) or (g is not None and not torch.equal(g.detach(), torch.from_numpy(blobs[c].copy()))):
                    raise AssertionError("%s: output %d receives another cotangent than in the recorded session" % (fn.__name__, i))
            return [None if g is None else torch.from_numpy(blobs[g].copy()) for g in rec["backward"]["grads"]]

        res = _decode(rec, blobs, backward)
        return SimpleNamespace(**res) if flags else res

    call.__name__, call.__doc__ = fn.__name__, fn.__doc__
    return call


def write_records(path=FIXTURES, shard_bytes=900 * 1024):
    """this session's records -> path/reference_exec_NN.npz (the records' JSON, 200 per file, then the arrays; each file small)"""
    os.makedirs(path, exist_ok=True)
    for f in os.listdir(path):
        os.remove(os.path.join(path, f))
    keys, shards = sorted(_new["records"]), []
    for i in range(0, len(keys), 200):
        part = json.dumps({k: _new["records"][k] for k in keys[i:i + 200]}, sort_keys=True, separators=(",", ":"))
        shards.append({"records": np.frombuffer(part.encode(), dtype=np.uint8)})
    size = shard_bytes
    for h in sorted(_new["blobs"]):
        a = _new["blobs"][h]
        if size + a.nbytes > shard_bytes:
            shards.append({})
            size = 0
        shards[-1][h], size = a, size + a.nbytes + 200
    for i, z in enumerate(shards):
        np.savez_compressed(os.path.join(path, "reference_exec_%02d.npz" % i), **z)


if RECORD:
    atexit.register(lambda: _new["records"] and write_records())



def available():
    """the reference's code can run here (MACX_REFERENCE_DIR); otherwise its results are replayed"""
    return bool(REF) and os.path.isfile(os.path.join(REF, "mac_cell.py"))


def load():
    """Import the reference modules against the shim (once)."""
    if _mods:
        return _mods
    for p in (REF, SHIM):
        if p not in sys.path:
            sys.path.insert(0, p)
    tf = importlib.import_module("tensorflow")
    if not hasattr(tf, "shim_reset"):
        raise RuntimeError("a real tensorflow shadowed the test shim")
    for name in ("config", "ops", "mac_cell", "model"):
        m = importlib.import_module(name)
        if not os.path.abspath(m.__file__).startswith(os.path.abspath(REF)):
            raise RuntimeError("module %s resolved to %s, not the reference" % (name, m.__file__))
        _mods[name] = m
    _mods["tf"] = tf
    return _mods


@_recorded
def parse_flags(flag_file, *extra):
    """The reference's own parser (config.py:95-428) over one of its published flag files
    (configs/args*.txt) plus extra command-line flags; returns the `config` singleton."""
    M = load()
    # argparse only fills in defaults for attributes the namespace does not have yet, and the reference parses into its
    # module-level singleton (config.py:428): start every parse from a fresh process's state
    M["config"].config.__dict__.clear()
    argv = sys.argv
    try:
        sys.argv = ["main.py"] + (["@" + os.path.join(REF, "configs", flag_file)] if flag_file else []) + [str(a) for a in extra]
        M["config"].parseArgs()
    finally:
        sys.argv = argv
    cfg = M["config"].config
    # the reference's parser declares --unsharedCells with type=bool (config.py:297): any string is True; leave as parsed
    return cfg


def dims_flags(d, p, hidden=None):
    f = ["--netLength", p, "--memDim", d, "--ctrlDim", d, "--attDim", d]
    if hidden is not None:
        f += ["--outClassifierDims", hidden]
    return f


CELL_FLAGS = [  # every flag the cell reads
    "netLength", "memDim", "ctrlDim", "attDim", "unsharedCells", "initCtrl", "initMem", "initKBwithQ", "addNullWord",
    "controlWholeQ", "controlContinuous", "controlContextual", "controlInWordsProj", "controlOutWordsProj",
    "controlInputUnshared", "controlInputAct", "controlFeedPrev", "controlFeedPrevAtt", "controlFeedInputs",
    "controlContAct", "controlConcatWords", "controlProj", "controlProjAct", "readProjInputs", "readProjShared",
    "readMemAttType", "readMemConcatKB", "readMemConcatProj", "readMemProj", "readMemAct", "readCtrl",
    "readCtrlAttType", "readCtrlConcatKB", "readCtrlConcatProj", "readCtrlConcatInter", "readCtrlAct", "readSmryKBProj",
    "writeInputs", "writeConcatMul", "writeInfoProj", "writeInfoAct", "writeSelfAtt", "writeSelfAttMod",
    "writeMergeCtrl", "writeMemProj", "writeMemAct", "writeGate", "writeGateShared", "writeGateBias",
    "memoryVariationalDropout", "memoryDropout", "readDropout", "writeDropout", "relu", "mulBias", "memoryBN",
    "bnDecay", "bnCenter", "bnScale", "outQuestion", "outQuestionMul", "outClassifierDims", "outputDropout",
]


def snapshot(cfg):
    """The parsed values of the cell's flags as a plain dict (what the oracle's config must equal)."""
    return {k: getattr(cfg, k) for k in CELL_FLAGS}


@_recorded
def run_reference(cfg, vecQ, questionWords, questionCntxWords, lengths, kb, train=False, keeps=(1.0, 1.0, 1.0),
                  output_keep=1.0, preset=None, seed=0, dtype=torch.float64, need_grad=False, answers=None,
                  with_output=True, answerWordsNum=7, draws=None):
    """MACnet.MACnetwork (+ output unit) exactly as model.py builds it.  `draws`: optional list of uniform tensors
    replayed in call order (otherwise the shim's generator draws and logs them).
    Returns dict(control, memory, cell, variables, draws, logits, loss, preds, inputs)."""
    M = load()
    tf, model = M["tf"], M["model"]
    tf.shim_reset(dtype=dtype, seed=seed, preset=preset, require_grad=need_grad)
    if draws is not None:
        q = list(draws)
        tf.state.uniform_hook = lambda shape: _pop(q, shape)
    cfg.answerWordsNum = answerWordsNum       # set at run time by preprocess.py:685-686
    ins = [tf.wrap(t.detach().to(dtype).clone()).requires_grad_(need_grad) for t in (vecQ, questionWords, questionCntxWords, kb)]
    vq_, qw_, cw_, kb_ = ins
    B = vecQ.shape[0]
    fake = SimpleNamespace(dropouts={"memory": keeps[0], "read": keeps[1], "write": keeps[2], "output": output_keep},
                           batchSize=B, train=train, batchNorm=None, answerLossList=[], correctNumList=[], answerAccList=[])
    control, memory = model.MACnet.MACnetwork(fake, kb_, vq_, qw_, cw_, tf.wrap(lengths.clone()))
    out = dict(control=control, memory=memory, cell=fake.macCell, inputs=dict(vecQ=vq_, questionWords=qw_,
                                                                               questionCntxWords=cw_, kb=kb_))
    if with_output:
        features, dim = model.MACnet.outputOp(fake, memory, vq_, None, None)
        logits = model.MACnet.classifier(fake, features, dim)
        out["logits"] = logits
        if answers is not None:
            loss, losses = model.MACnet.addAnswerLossOp(fake, logits, answers)
            preds, corrects, correctNum = model.MACnet.addPredOp(fake, logits, answers)
            out.update(loss=loss, losses=losses, preds=preds, correctNum=correctNum)
    out["variables"] = dict(tf.state.variables)
    out["draws"] = [u for _, u in tf.state.draws]
    return out


def _pop(q, shape):
    if not q:
        raise AssertionError("the reference drew more random tensors than were recorded")
    u = q.pop(0)
    if tuple(u.shape) != tuple(shape):
        raise AssertionError("draw shape %s, recorded %s" % (tuple(shape), tuple(u.shape)))
    return u


def replay_mask_fn(draws, keeps, output_keep=1.0):
    """mask_fn for oracle.mac_oracle: hands the oracle floor(keep + U) for the reference's draws, FIFO.
    The oracle asks for masks in graph order; so does the reference (both are op-for-op)."""
    from oracle import dropout_hash as dh
    q = list(draws)
    site_keep = {dh.SITE_MEM_VAR: keeps[0], dh.SITE_MEM: keeps[0], dh.SITE_READ_KB: keeps[1], dh.SITE_READ_MEM: keeps[1],
                 dh.SITE_READ_ATT: keeps[1], dh.SITE_WRITE_INFO: keeps[2]}

    def fn(site, step, shape):
        u = _pop(q, shape)
        return torch.floor(site_keep[site] + u)

    def rest(keep):
        """remaining draws as masks (classifier layers), in order"""
        out = [torch.floor(keep + u) for u in q]
        del q[:]
        return out

    fn.rest = rest
    fn.left = lambda: len(q)
    return fn


@_recorded
def run_reference_stem(cfg, images_nhwc, keep=1.0, seed=0, dtype=torch.float64, need_grad=False, draws=None, out_dim=None):
    """MACnet.stem (model.py:165-204) exactly as the reference builds it: ops.CNNLayer -> ops.cnn (ops.py:380-438).
    images_nhwc [B,H,W,C] (the graph's layout after model.py:67-68).  Returns dict(kb [B,H*W,outDim], variables, draws, images)."""
    M = load()
    tf, model = M["tf"], M["model"]
    tf.shim_reset(dtype=dtype, seed=seed, require_grad=need_grad)
    if draws is not None:
        q = list(draws)
        tf.state.uniform_hook = lambda shape: _pop(q, shape)
    B, H, W, C = images_nhwc.shape
    img = tf.wrap(images_nhwc.detach().to(dtype).clone()).requires_grad_(need_grad)
    fake = SimpleNamespace(dropouts={"stem": keep}, batchSize=B, H=H, W=W, batchNorm=None)
    kb = model.MACnet.stem(fake, img, C, out_dim if out_dim is not None else cfg.memDim)
    return dict(kb=kb, variables=dict(tf.state.variables), draws=[u for _, u in tf.state.draws], images=img)


@_recorded
def run_reference_encoder(cfg, questions, lengths, emb, keep_input=1.0, keep_question=1.0, seed=0, dtype=torch.float64,
                          need_grad=False, draws=None):
    """qEmbeddingsOp (model.py:207-219) + encoder (model.py:279-307 -> ops.RNNLayer / biRNNLayer, ops.py:859-950) as the
    reference builds them; the recurrent cell and tf.nn.bidirectional_dynamic_rnn are the shim's restatement of TF's.
    Returns dict(words [B,S,encDim], vecQ [B,encDim], variables, draws)."""
    M = load()
    tf, model = M["tf"], M["model"]
    tf.shim_reset(dtype=dtype, seed=seed, require_grad=need_grad)
    if draws is not None:
        q = list(draws)
        tf.state.uniform_hook = lambda shape: _pop(q, shape)
    fake = SimpleNamespace(dropouts={"encInput": keep_input, "question": keep_question, "stateInput": 1.0}, batchSize=questions.shape[0])
    qs, _ = model.MACnet.qEmbeddingsOp(fake, tf.wrap(questions.clone()), emb.detach().to(dtype).clone())
    proj = (cfg.encDim != cfg.ctrlDim) or cfg.encProj                                    # model.py:785-787, as MACnet.build calls it
    words, vecQ = model.MACnet.encoder(fake, qs, tf.wrap(lengths.clone()), proj, proj, cfg.ctrlDim)
    return dict(words=words, vecQ=vecQ, variables=dict(tf.state.variables), draws=[u for _, u in tf.state.draws])


@_recorded
def run_reference_training(cfg, vecQ, questionWords, questionCntxWords, lengths, kb, answers, steps, lr, preset=None, seed=0,
                           dtype=torch.float64, answerWordsNum=7):
    """`steps` training steps exactly as model.py strings them: MACnetwork -> outputOp -> classifier -> addAnswerLossOp
    (evaluation-mode dropout: the optimizer is what is under test), then MACnet.addOptimizerOp (once) and, per step,
    MACnet.computeGradients + MACnet.addTrainingOp (model.py:615-669) -- clip_by_global_norm, AdamOptimizer.apply_gradients
    and ExponentialMovingAverage.apply as that code calls them, on the shim's restatement of those three TF classes.
    Returns per step: the gradients the reference computed, the global norm, and the variables / Adam slots / EMA shadows
    afterwards (name -> tensor, names without ':0')."""
    M = load()
    tf, model = M["tf"], M["model"]
    tf.shim_reset(dtype=dtype, seed=seed, preset=preset, require_grad=True)
    cfg.answerWordsNum = answerWordsNum
    B = vecQ.shape[0]
    fake = SimpleNamespace(dropouts={"memory": 1.0, "read": 1.0, "write": 1.0, "output": 1.0}, batchSize=B, train=True,
                           batchNorm=None, answerLossList=[], correctNumList=[], answerAccList=[], lr=lr)
    optimizer = model.MACnet.addOptimizerOp(fake)                       # model.py:616-620
    ins = [tf.wrap(t.detach().to(dtype).clone()) for t in (vecQ, questionWords, questionCntxWords, kb)]
    vq_, qw_, cw_, kb_ = ins
    out = []
    for step in range(steps):
        with tf.variable_scope(tf.get_variable_scope(), reuse=(True if step > 0 else None)):
            control, memory = model.MACnet.MACnetwork(fake, kb_, vq_, qw_, cw_, tf.wrap(lengths.clone()))
            features, dim = model.MACnet.outputOp(fake, memory, vq_, None, None)
            logits = model.MACnet.classifier(fake, features, dim)
            loss, _ = model.MACnet.addAnswerLossOp(fake, logits, answers)
        gv = model.MACnet.computeGradients(fake, optimizer, loss, None)                      # model.py:626-637
        grads = {v.name[:-2]: (None if g is None else g.detach().clone()) for g, v in gv}
        _, norm = model.MACnet.addTrainingOp(fake, optimizer, gv)                            # model.py:643-669
        names = list(tf.state.variables)
        out.append(dict(loss=float(loss), norm=float(norm), grads=grads,
                        variables={k: tf.state.variables[k].detach().clone() for k in names},
                        m={k: optimizer.m[k + ":0"].clone() for k in names if k + ":0" in optimizer.m},
                        v={k: optimizer.v[k + ":0"].clone() for k in names if k + ":0" in optimizer.v},
                        ema={k: tf.state.ema[k].clone() for k in names if k in tf.state.ema}))
    return dict(steps=out, global_step=fake.globalStep.value, ema_names=sorted(fake.emaDict),
                initial={k: v.detach().clone() for k, v in tf.state.initial.items()})
