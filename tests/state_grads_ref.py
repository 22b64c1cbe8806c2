"""Shared by tests/test_state_grads_host.py and tests/test_gpu_state_grads.py: losses on a cell's attention maps and step states,
written once for both sides.  The oracle's cell (oracle.mac_oracle) and the HIP cells expose the same interface -- attentions[kind][i],
controls / memories as [B, steps + 1, d] -- so ONE function builds the loss for either; only the cast of the seeded incoming
gradients differs (fp64 on the CPU for the oracle, fp32 on the device for the cell).

A target is (kind, index): ("att_kb", i) ("att_question", i) ("att_self", i) ("att_gate", i) -- step i's map; ("controls", j)
("memories", j) -- history entry j, [:, j]; ("controls", None) ("memories", None) -- the whole history; ("memory", None)
("control", None) -- the final state, what the cell has always differentiated."""
import torch

from oracle import mac_oracle as mo

# (kind, index, flag file) of the single-output tests, all at SINGLE_SHAPE.  The host test asserts that the oracle's gradients of
# each are non-zero, the GPU test compares every gradient of each with the oracle's.
SINGLE_SHAPE = dict(B=3, S=9, N=49, d=128)
SINGLE_CASES = [
    ("att_kb", 0, "args"), ("att_kb", 1, "args1"), ("att_kb", 0, "args3"), ("att_kb", 0, "args4"),
    ("att_question", 0, "args"), ("att_question", 1, "args1"), ("att_question", 0, "args3"), ("att_question", 0, "args4"),
    ("controls", 1, "args"), ("controls", 2, "args1"),
    ("memories", 1, "args"), ("memories", 1, "args1"), ("memories", 1, "args3"), ("memories", 1, "args4"),
    ("att_self", 1, "args3"),
    ("att_gate", 0, "args4"),
]
# inputs a single-output loss must reach (the issue's table); controls: the control unit reads the question only
REACHED = {"att_kb": ("vecQuestions", "words", "knowledgeBase"), "att_question": ("vecQuestions", "words"),
           "controls": ("vecQuestions", "words"), "memories": ("vecQuestions", "words", "knowledgeBase"),
           "att_self": ("vecQuestions", "words"), "att_gate": ("vecQuestions", "words")}


def steps_of(name):
    return 4 if name == "args3" else 3


def target_tensor(cell, state, kind, idx):
    if kind == "memory":
        return state.memory
    if kind == "control":
        return state.control
    if kind in ("controls", "memories"):
        t = getattr(cell, kind)
        return t if idx is None else t[:, idx]
    return cell.attentions[kind[len("att_"):]][idx]


def target_shape(kind, idx, B, S, N, d, p):
    if kind in ("memory", "control"):
        return (B, d)
    if kind in ("controls", "memories"):
        return (B, p + 1, d) if idx is None else (B, d)
    return {"att_kb": (B, N), "att_question": (B, S), "att_self": (B, idx + 1), "att_gate": (B, d)}[kind]


def incoming(targets, B, S, N, d, p, seed=9):
    """{target: G}: seeded N(0,1) incoming gradients, / B for states (as tests/test_gpu_cell.py scales d_memory / d_control)"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for kind, idx in targets:
        G = torch.randn(target_shape(kind, idx, B, S, N, d, p), generator=g)
        out[(kind, idx)] = G if kind.startswith("att_") else G / B
    return out


def all_targets(cfg, p, final=True):
    """every map of every step, both whole histories, and (final) the final state"""
    t = [("att_kb", i) for i in range(p)] + [("att_question", i) for i in range(p)]
    if cfg.writeSelfAtt:
        t += [("att_self", i) for i in range(p)]
    if cfg.writeGate:
        t += [("att_gate", i) for i in range(p)]
    t += [("controls", None), ("memories", None)]
    if final:
        t += [("memory", None), ("control", None)]
    return t


def aux_loss(cell, state, Gs, cast):
    """sum over the targets of (tensor * G).sum()"""
    loss = 0
    for (kind, idx), G in Gs.items():
        loss = loss + (target_tensor(cell, state, kind, idx) * cast(G)).sum()
    return loss


class _State:
    def __init__(self, control, memory):
        self.control, self.memory = control, memory


def oracle_aux(cfg, ref_params, vq, words, lengths, kb, Gs, train=True, seed=0, b0=0):
    """fp64 oracle forward + autograd of aux_loss, on the masks of (seed, b0) -- tests/helpers.oracle_run with the loss on the
    cell's own tensors.  Returns dict(memory, control, cell, params, inputs) with .grad filled where the loss reaches."""
    dt = torch.float64
    params = {k: v.detach().cpu().to(dt).clone().requires_grad_(True) for k, v in ref_params.items()}
    vs = mo.VarStore(params=params, dtype=dt)
    vq_, words_, kb_ = [t.detach().cpu().to(dt).clone().requires_grad_(True) for t in (vq, words, kb)]
    keeps = (cfg.memoryDropout, cfg.readDropout, cfg.writeDropout) if train else (1.0, 1.0, 1.0)
    mask_fn = mo.hash_mask_fn(seed, keeps, b0=b0) if train else None
    c, m, cell = mo.mac_network(cfg, vs, vq_, words_, words_, lengths.cpu(), kb_, train=train, mask_fn=mask_fn, keeps=keeps)
    aux_loss(cell, _State(c, m), Gs, lambda G: G.to(dt)).backward()
    return dict(control=c, memory=m, cell=cell, params=params, inputs=(vq_, words_, kb_))
