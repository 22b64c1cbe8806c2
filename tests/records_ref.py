"""macx_records_scatter's contract (include/macx.h) restated in numpy: a loop over the slots in ascending order, later slots
overwriting earlier ones, and .astype for the conversion.  Depends on numpy only."""
import numpy as np

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


def scatter(table, src, ids):
    """table [Q, steps, n] (float32 or float16; a copy is returned), src [steps, B, n] float32, ids [B] integers:
    table[ids[b], i, :] = src[i, b, :] converted to the table's dtype for every slot with 0 <= ids[b] < Q, in ascending slot order --
    so the highest slot that names an id is the one whose rows remain; every other slot writes nothing."""
    out = np.array(table, copy=True)
    Q, steps, n = out.shape
    assert src.dtype == np.float32 and src.shape == (steps, len(ids), n)
    with np.errstate(over="ignore"):                 # beyond 65504: an infinity, which is the contract
        for b, q in enumerate(int(v) for v in ids):
            if 0 <= q < Q:
                out[q] = src[:, b, :].astype(out.dtype)
    return out


def dead_kinds(Q):
    """the ids that must write nothing: the dead slot and everything else outside [0, Q)"""
    return [-1, Q, Q + 5, -2, INT_MIN, INT_MAX]


def ids_with_every_kind(B, Q, rng):
    """[B] int32 ids: random live ids; one id three times (slots 0, B // 2, B - 1: B >= 5) and another twice (the first and the last
    slot still free) in non-adjacent slots; and dead_kinds(Q) in random free slots.  A batch too small for all of it (B < 11) takes
    what fits in this order -- the triple, -1, Q, the pair, the rest -- and always keeps a live slot."""
    ids = rng.integers(0, Q, size=B).astype(np.int64)
    free = list(range(B))
    live = 0                                         # slots that are certain to be live
    if B >= 5:
        for s in (0, B // 2, B - 1):
            ids[s] = ids[0]
            free.remove(s)
        live = 3
    if len(free) >= 4 and free[-1] - free[0] >= 2:
        ids[free[0]] = ids[free[-1]] = (ids[0] + 1) % Q if B >= 5 else ids[free[0]]
        free = free[1:-1]
        live += 2
    free = [free[i] for i in rng.permutation(len(free))]
    for bad in dead_kinds(Q):
        if len(free) > (0 if live else 1):
            ids[free.pop()] = bad
    return ids.astype(np.int32)
