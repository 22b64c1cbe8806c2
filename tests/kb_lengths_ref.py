"""The oracle with per-question knowledge-base sizes, without editing oracle/: a context manager that puts ops.expMask
(ops.py:243-247) in front of the READ unit's softmax.

    with masked_kb_attention(kb_lengths, N):
        ... mo.mac_network(...) / helpers.oracle_run(...)

mac_oracle.Ops.inter2att is called twice per step at most: by the read unit with the default name "" on interactions of shape
[B, N, width] (mac_cell.py:266), and by the write unit's self attention with name "selfAttention" on [B, steps so far, d].  Only
the first is masked: name == "" and interactions.shape[-2] == N.  Masked logits get -1e30 added (the reference's `inf`), whose
softmax is an exact 0 in fp32 and fp64 alike, so question b sees its first kb_lengths[b] cells and nothing of the rest -- the same
arithmetic as the unpatched oracle on kb[b:b+1, :kb_lengths[b]] (tests/test_kb_lengths_host.py checks exactly that).  The
attribute is restored on exit, also when the body raises."""
import torch

from oracle import mac_oracle as mo


class masked_kb_attention:
    def __init__(self, kb_lengths, N):
        self.lengths = torch.as_tensor(kb_lengths).detach().cpu().to(torch.int64)
        self.N = int(N)

    def __enter__(self):
        self._orig = orig = mo.Ops.inter2att
        lengths, N = self.lengths, self.N

        def inter2att(ops, interactions, dim, dropout=1.0, mask=None, name=""):
            if name != "" or interactions.shape[-2] != N:
                return orig(ops, interactions, dim, dropout=dropout, mask=mask, name=name)
            with ops.vs.scope("inter2att" + name):
                logits = ops.inter2logits(interactions, dim, dropout=dropout, mask=mask)
                return torch.softmax(mo.Ops.expMask(logits, lengths), dim=-1)

        mo.Ops.inter2att = inter2att
        return self

    def __exit__(self, *exc):
        mo.Ops.inter2att = self._orig
        return False
