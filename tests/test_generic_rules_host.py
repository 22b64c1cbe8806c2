"""CPU: the rule layer of the generic option path (mac-network_amd/generic.py: bin_bwd, linear_fwd / linear_bwd, act_bwd, act_code,
ScopeNames) -- the formulas the eager autograd nodes (_Binary, _Act, _Linear) and the plan's executor (plan._Exec) both call.
Kernel calls are the torch stand-ins of tests/test_generic_host.py.  (a) each rule against the same expression differentiated by
torch in fp64, and no launch for a gradient nobody wants; (b) an eager node and a one-node plan segment give the same bits;
(c) one scope namer under the variable store and the plan's compiler; (d) one activation table.  tests/test_gpu_generic.py
repeats (b) on the device through `stacks_agree`."""
import collections
import itertools
from types import SimpleNamespace

import pytest
import torch

from test_generic_host import host_generic          # noqa: F401 -- fixture: generic.k_* swapped for torch restatements

U = 2.0 ** -24                                      # fp32 unit round-off
SPREADS = ("same", "mid", "channel", "row")
B_SHAPE = {"same": (2, 3, 8), "mid": (2, 8), "channel": (8,), "row": (6,)}       # b under a of [2, 3, 8]


def rand(shape, seed, dev=None):
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return t.to(dev) if dev is not None else t


def within(got, ref, terms, abs_sum):
    """|got - ref| <= (terms summed + 2) * 2^-24 * sum |terms| per element: a sum of n terms that each carry up to two roundings of
    their own (a product, a scale) and n - 1 roundings of the additions is off by at most (n + 1) u sum |terms| to first order; +2
    leaves one rounding for an operand that is itself a rounded function value (tanh, sigmoid, exp)."""
    assert got.shape == ref.shape
    err, bound = (got.double() - ref).abs(), (terms + 2) * U * abs_sum
    assert bool((err <= bound).all()), "error / bound = %.3g" % float((err / bound.clamp_min(1e-300)).max())


@pytest.fixture
def calls(host_generic, monkeypatch):
    """generic.k_* name -> times called (on top of the torch stand-ins)"""
    seen = collections.Counter()

    def counted(name, f):
        def call(*a, **kw):
            seen[name] += 1
            return f(*a, **kw)
        return call
    for name in [n for n in vars(host_generic) if n.startswith("k_")]:
        monkeypatch.setattr(host_generic, name, counted(name, getattr(host_generic, name)))
    return seen


# ---------------------------------------------------------------------------------------------------------------------
# (a) the rules against torch fp64
# ---------------------------------------------------------------------------------------------------------------------
def spread_over(b, spread):
    """b as it meets a of [2, 3, 8]"""
    return b.reshape({"same": (2, 3, 8), "mid": (2, 1, 8), "channel": (8,), "row": (2, 3, 1)}[spread])


def summed_over(t, spread):
    """the sum of a [2, 3, 8] tensor over the axes b is spread along, in b's shape; and how many terms meet in an element"""
    if spread == "same":
        return t, 1
    axes, n = {"mid": ((1,), 3), "channel": ((0, 1), 6), "row": ((2,), 8)}[spread]
    return t.sum(axes).reshape(B_SHAPE[spread]), n


@pytest.mark.parametrize("want", [(True, False), (False, True), (True, True)], ids=["a", "b", "ab"])
@pytest.mark.parametrize("scale", [1.0, -0.5])
@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("op", ["add", "mul"])
def test_bin_bwd_against_fp64(macx, calls, op, spread, scale, want):
    G = macx.generic
    opc, mode = macx.plan._OPC[op], macx.plan._SPREAD[spread]
    a, b, g = rand((2, 3, 8), 1), rand(B_SHAPE[spread], 2), rand((2, 3, 8), 3)
    assert G.mid_of(mode, a) == (3 if spread == "mid" else 1)
    da, db = G.bin_bwd(opc, mode, scale, g, a, b, G.mid_of(mode, a), 8, *want)
    ad, bd, gd = a.double().requires_grad_(True), b.double().requires_grad_(True), g.double()
    y = scale * (ad + spread_over(bd, spread) if op == "add" else ad * spread_over(bd, spread))
    ra, rb = torch.autograd.grad(y, (ad, bd), gd)
    with torch.no_grad():
        ta = (scale * gd * (spread_over(bd, spread) if op == "mul" else 1.0)).abs()
        tb, n = summed_over((scale * gd * (ad if op == "mul" else 1.0)).abs(), spread)
    if want[0]:
        within(da, ra, 1, ta)
    else:
        assert da is None
    if want[1]:
        within(db, rb, n, tb)
    else:
        assert db is None
    # mul: one product per wanted side; add: the scaled gradient once, and only when there is a scale; the spread's sum for b alone
    assert calls["k_binary"] == (want[0] + want[1] if op == "mul" else int(scale != 1.0))
    assert calls["k_reduce"] == int(want[1] and spread != "same")
    assert sum(calls.values()) == calls["k_binary"] + calls["k_reduce"]


def act_fp64(G, code, x, alpha):
    L = G._lib.ACT
    if code == G.ACT_PRELU:
        return torch.where(x > 0, x, alpha * x)
    return {L["NON"]: lambda v: v * 1.0, L["TANH"]: torch.tanh, L["SIGMOID"]: torch.sigmoid, L["ELU"]: torch.nn.functional.elu,
            L["RELU"]: torch.relu}[code](x)


def act_dx_terms(G, code, x, alpha, g):
    """the fp64 terms whose sum is dx, as the derivative is evaluated from the function value: g (1 - t^2), g (s - s^2), one
    product for the others"""
    L = G._lib.ACT
    if code == L["TANH"]:
        return [g, g * torch.tanh(x) ** 2]
    if code == L["SIGMOID"]:
        return [g * torch.sigmoid(x), g * torch.sigmoid(x) ** 2]
    if code == L["ELU"]:
        return [g * torch.where(x > 0, torch.ones_like(x), torch.exp(x))]
    if code == L["RELU"]:
        return [g * (x > 0)]
    if code == G.ACT_PRELU:
        return [g * torch.where(x > 0, torch.ones_like(x), alpha.expand_as(x))]
    return [g]


def act_codes(G):
    return sorted(G._lib.ACT.values()) + [G.ACT_PRELU]


@pytest.mark.parametrize("want_alpha", [False, True])
@pytest.mark.parametrize("which", range(6))
def test_act_bwd_against_fp64(macx, calls, which, want_alpha):
    G = macx.generic
    code = act_codes(G)[which]
    assert len(act_codes(G)) == 6
    x, g = rand((4, 8), 4), rand((4, 8), 5)
    alpha = 0.25 + 0.1 * rand((8,), 6) if code == G.ACT_PRELU else None
    dx, dal = G.act_bwd(code, x, alpha, g, want_alpha)
    xd, gd = x.double().requires_grad_(True), g.double()
    ald = alpha.double().requires_grad_(True) if alpha is not None else None
    ref = torch.autograd.grad(act_fp64(G, code, xd, ald), (xd,) if ald is None else (xd, ald), gd)
    with torch.no_grad():
        terms = act_dx_terms(G, code, xd, ald, gd)
        within(dx, ref[0], len(terms), sum(t.abs() for t in terms))
        if code == G.ACT_PRELU and want_alpha:
            within(dal, ref[1], 4, (gd * xd * (xd <= 0)).abs().sum(0))          # the slope's gradient: g x over the 4 rows
        else:
            assert dal is None
    assert calls["k_act_bwd"] == 1
    assert calls["k_reduce"] == int(code == G.ACT_PRELU and want_alpha)
    assert sum(calls.values()) == calls["k_act_bwd"] + calls["k_reduce"]


# every combination of wanted gradients: of x, W and b with a bias, of x and W without one
LINEAR_WANTS = [(True, w) for w in itertools.product([False, True], repeat=3)] + \
               [(False, w + (False,)) for w in itertools.product([False, True], repeat=2)]


@pytest.mark.parametrize("bias,want", LINEAR_WANTS,
                         ids=lambda v: ("bias" if v else "nobias") if isinstance(v, bool) else "".join("xWb"[i] for i in range(3) if v[i]) or "none")
@pytest.mark.parametrize("xshape", [(5, 16), (2, 3, 16)])
def test_linear_rules_against_fp64(macx, calls, xshape, bias, want):
    G = macx.generic
    x, W, b = rand(xshape, 7), rand((16, 8), 8), (rand((8,), 9) if bias else None)
    g = rand(xshape[:-1] + (8,), 10)
    y, big = G.linear_fwd(x, W, b)
    assert big == ((2, 3) if len(xshape) == 3 else None) and big == G.big_of(x)
    assert calls["k_matmul"] == 1
    calls.clear()
    dx, dW, db = G.linear_bwd(x, W, g, big, *want)
    xd, Wd, gd = x.double().requires_grad_(True), W.double().requires_grad_(True), g.double()
    bd = b.double().requires_grad_(True) if bias else None
    yd = xd @ Wd + (bd if bias else 0.0)
    ref = torch.autograd.grad(yd, (xd, Wd) + ((bd,) if bias else ()), gd)
    rows = x.numel() // 16
    with torch.no_grad():
        within(y, yd, 16 + bias, xd.abs() @ Wd.abs() + (bd.abs() if bias else 0.0))
        x2, g2 = xd.reshape(rows, 16), gd.reshape(rows, 8)
        for got, wanted, r, terms, abs_sum in ((dx, want[0], ref[0], 8, (g2.abs() @ Wd.abs().t()).reshape(xshape)),
                                               (dW, want[1], ref[1], rows, x2.abs().t() @ g2.abs()),
                                               (db, want[2], ref[2] if bias else None, rows, g2.abs().sum(0))):
            if wanted:
                within(got, r, terms, abs_sum)
            else:
                assert got is None
    assert (calls["k_matmul"], calls["k_wgrad"], calls["k_reduce"]) == tuple(int(w) for w in want)
    assert sum(calls.values()) == sum(want)


# ---------------------------------------------------------------------------------------------------------------------
# (b) the two stacks agree: an eager node == a one-node plan segment, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def stacks_agree(macx, kind, eager, inputs, g, **attr):
    """inputs: feed name -> tensor, or None for an operand the node does not have.  `eager(*leaves)` runs the autograd node of
    generic.py; the plan route is a one-node Segment (feeds only) through plan.run_segment with a plain _Exec.  Output and the
    gradient of every input under the upstream gradient `g`: torch.equal.  Returns (y, gradients) of the eager route."""
    P = macx.plan
    seg = P.Segment(kind)
    seg.results["y"] = seg.emit(kind, *[seg.feed(name) if t is not None else -1 for name, t in inputs.items()], **attr)
    out = []
    for route in ("eager", "plan"):
        leaves = {name: t.detach().clone().requires_grad_(True) for name, t in inputs.items() if t is not None}
        if route == "eager":
            y = eager(*[leaves.get(name) for name in inputs])
        else:
            y = P.run_segment(seg, P._Exec(0, 0, {}, False, 1, g.device), leaves, None)["y"]
        (y * g).sum().backward()          # (upstream gradient g; backward(g) would load torch's symbolic-shape machinery once)
        out.append((y.detach(), [t.grad for t in leaves.values()]))
    (ye, ge), (yp, gp) = out
    assert torch.equal(ye, yp), kind
    assert len(ge) == len(gp) == sum(t is not None for t in inputs.values())
    for name, a, b in zip([n for n, t in inputs.items() if t is not None], ge, gp):
        assert a.shape == b.shape and torch.equal(a, b), (kind, name)
    return ye, ge


def bin_agrees(macx, a, op, spread, scale, dev=None):
    G, P = macx.generic, macx.plan
    bshape = {"same": a.shape, "mid": (a.shape[0], a.shape[2]), "channel": a.shape[2:], "row": (a.shape[0] * a.shape[1],)}[spread]
    return stacks_agree(macx, "bin", lambda p, q: G._Binary.apply(p, q, P._OPC[op], P._SPREAD[spread], scale),
                        {"a": a, "b": rand(tuple(bshape), 12, dev)}, rand(a.shape, 13, dev), op=op, spread=spread, scale=scale)


def act_agrees(macx, x, code, dev=None):
    G = macx.generic
    alpha = (0.25 + 0.1 * rand(x.shape[-1:], 14)).to(x.device) if code == G.ACT_PRELU else None
    return stacks_agree(macx, "act", lambda v, al: G._Act.apply(v, code, al), {"x": x, "alpha": alpha}, rand(x.shape, 15, dev), code=code)


def linear_agrees(macx, x, n, bias, dev=None):
    G = macx.generic
    W, b = rand((x.shape[-1], n), 16, dev), (rand((n,), 17, dev) if bias else None)
    return stacks_agree(macx, "linear", G._Linear.apply, {"x": x, "W": W, "b": b}, rand(x.shape[:-1] + (n,), 18, dev), const=0.0)


@pytest.mark.parametrize("scale", [1.0, -0.5])
@pytest.mark.parametrize("spread", SPREADS)
@pytest.mark.parametrize("op", ["add", "mul"])
def test_binary_node_and_plan_segment_agree(macx, host_generic, op, spread, scale):
    bin_agrees(macx, rand((2, 3, 8), 11), op, spread, scale)


@pytest.mark.parametrize("which", range(6))
def test_act_node_and_plan_segment_agree(macx, host_generic, which):
    act_agrees(macx, rand((4, 8), 11), act_codes(host_generic)[which])


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("xshape", [(5, 16), (2, 3, 16)])
def test_linear_node_and_plan_segment_agree(macx, host_generic, xshape, bias):
    linear_agrees(macx, rand(xshape, 11), 8, bias)


def test_act_node_leaves_a_fixed_slope_alone(macx, calls):
    """a PReLU slope that wants no gradient: no row sum, on the eager node as in the plan"""
    G = macx.generic
    x, alpha = rand((4, 8), 11).requires_grad_(True), torch.full((8,), 0.25)
    G._Act.apply(x, G.ACT_PRELU, alpha).backward(rand((4, 8), 12))
    assert x.grad is not None and calls["k_act_bwd"] == 1 and calls["k_reduce"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# (c) one scope namer
# ---------------------------------------------------------------------------------------------------------------------
def test_default_name_scopes_count_up_and_reset(macx):
    names, got = macx.generic.ScopeNames(), []

    def prelu():
        with names("prelu", default=True):
            got.append(names.full("alpha"))
    with names("a"):
        prelu()
        prelu()
    with names("a"):
        prelu()
    assert got == ["a/prelu/alpha", "a/prelu_1/alpha", "a/prelu/alpha"]
    assert names.stack == []


# (scope, default-name?, children) | a variable's leaf name
NESTED = [("MACnetwork", False, [
    ("write", False, ["bias", ("prelu", True, ["alpha"]), ("prelu", True, ["alpha"]),
                      ("linearLayer", False, [("prelu", True, ["alpha"]), ("BatchNorm", True, ["beta"])]),
                      ("prelu", True, ["alpha"]), ("BatchNorm", True, ["beta"])]),
    ("write", False, [("prelu", True, ["alpha"]), ("prelu", False, ["alpha"]), ("prelu", True, ["alpha"])]),
    ("read", False, [("prelu", True, ["alpha"])])])]


def test_store_and_compiler_name_variables_alike(macx):
    G, P = macx.generic, macx.plan
    store = G.GenericParams()
    e = P._Emitter(SimpleNamespace(), P.CellPlan())
    e.begin(P.Segment("t"))

    def walk(tree, scope, variable):
        for item in tree:
            if isinstance(item, str):
                variable(item)
            else:
                with scope(item[0], default=item[1]):
                    walk(item[2], scope, variable)
    walk(NESTED, store.scope, lambda leaf: store.get(leaf, (4,), "zeros"))
    walk(NESTED, e.names, lambda leaf: e.variable(leaf, (4,), "zeros"))
    assert list(store.names) == list(e.plan.variables)
    assert list(store.names) == [
        "MACnetwork/write/bias", "MACnetwork/write/prelu/alpha", "MACnetwork/write/prelu_1/alpha",
        "MACnetwork/write/linearLayer/prelu/alpha", "MACnetwork/write/linearLayer/BatchNorm/beta", "MACnetwork/write/prelu_2/alpha",
        "MACnetwork/write/BatchNorm/beta", "MACnetwork/read/prelu/alpha"]
    # a complete path is taken as it stands, whatever scope is open
    with store.scope("MACnetwork"):
        v = store.ensure("elsewhere/bias", (4,), "zeros")
        assert store.ensure("MACnetwork/write/bias", (4,), "zeros") is store.get("write/bias", (4,), "zeros")
    assert list(store.names)[-1] == "elsewhere/bias" and store.ensure("elsewhere/bias", (4,), 1.0) is v
    with pytest.raises(ValueError):
        store.ensure("elsewhere/bias", (5,), "zeros")


# ---------------------------------------------------------------------------------------------------------------------
# (d) one activation table
# ---------------------------------------------------------------------------------------------------------------------
RAISES = {"LKY": AttributeError, "SELU": UnboundLocalError}


def test_activation_table(macx):
    G = macx.generic
    for name, code in G._lib.ACT.items():
        if name != "RELU":
            assert all(G.act_code(name, relu) == code for relu in ("STD", "ELU", "PRM", "LKY", "SELU")), name
    assert G.act_code("RELU", "STD") == G._lib.ACT["RELU"]
    assert G.act_code("RELU", "ELU") == G._lib.ACT["ELU"]
    assert G.act_code("RELU", "PRM") == G.ACT_PRELU and G.ACT_PRELU not in G._lib.ACT.values()
    with pytest.raises(AttributeError, match="reluAlpha"):
        G.act_code("RELU", "LKY")
    with pytest.raises(UnboundLocalError, match="'output' referenced before assignment"):
        G.act_code("RELU", "SELU")


@pytest.mark.parametrize("relu", ["STD", "ELU", "PRM", "LKY", "SELU"])
def test_both_stacks_read_the_activation_table(macx, host_generic, relu):
    G, P = macx.generic, macx.plan
    cfg = SimpleNamespace(relu=relu)
    store = G.GenericParams()
    ops = G._Ops(cfg, store)
    e = P._Emitter(cfg, P.CellPlan())
    seg = e.begin(P.Segment("t"))
    e.w[seg.feed("x")] = 8
    x = rand((4, 8), 11)
    if relu in RAISES:
        with pytest.raises(RAISES[relu]):
            ops.act("RELU", x)
        with pytest.raises(RAISES[relu]):
            e.activation("RELU", seg.feeds["x"])
        return
    code = G.act_code("RELU", relu)
    y = ops.act("RELU", x)
    e.activation("RELU", seg.feeds["x"])
    (node,) = seg.nodes
    assert node.op == "act" and node.attr["code"] == code and len(node.ins) == (2 if relu == "PRM" else 1)
    assert list(store.names) == list(e.plan.variables) == (["prelu/alpha"] if relu == "PRM" else [])
    alpha = store.get("prelu/alpha", (8,), 0.25) if relu == "PRM" else None
    assert torch.equal(y, host_generic.k_act(code, x, alpha))
    assert ops.act("NON", x) is x and e.activation("NON", seg.feeds["x"]) == seg.feeds["x"]
