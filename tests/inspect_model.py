"""What bns_table_tally must return, in plain numpy: the keys of a khash table per taxon bin and per clade.  No GPU, no library.

Input: the khash arrays (flags 2 bits per slot, keys, vals) and the flat parent array given to load_taxonomy.  Present slots are those
whose flag pair is 0 (neither empty nor deleted); the key itself never decides (0 and ~0 are legal keys).  A present key's value t goes
to tally_bin(t): 0 for t == 0; t for t < n whose chain of parents reaches a node with parent 0 over keys of the parent map only; n for
anything else."""
import numpy as np

TAX_ABSENT = 0xFFFFFFFF


def present_mask(flags, n_buckets):
    idx = np.arange(n_buckets, dtype=np.int64)
    return ((np.asarray(flags, dtype=np.uint32)[idx >> 4] >> ((idx & 15) << 1).astype(np.uint32)) & 3) == 0


def chain_ok(parent):
    """ok[v]: v is a key of the parent map and so is every node up to one whose parent is 0 (NODE_CHAIN_OK)"""
    parent = np.asarray(parent, dtype=np.uint32).astype(np.int64)
    n = parent.size
    ok = parent == 0
    ok[0] = False
    valid = (parent != TAX_ABSENT) & (parent > 0) & (parent < n)
    valid[0] = False
    up = np.where(valid, parent, 0)
    for _ in range(n):                                     # (one level per round; a taxonomy is shallow)
        new = ok | (valid & ok[up])
        if np.array_equal(new, ok):
            break
        ok = new
    return ok


def tally_bins(vals, parent):
    """tally_bin of bns_tally.hpp restated, for an array of values"""
    n = len(parent)
    ok = chain_ok(parent)
    t = np.asarray(vals, dtype=np.uint32).astype(np.int64)
    inside = (t > 0) & (t < n)
    good = np.zeros(t.size, dtype=bool)
    good[inside] = ok[t[inside]]
    return np.where(t == 0, 0, np.where(good, t, n))


def clade_sums(direct, parent):
    """clade[v] = direct over v's subtree for the nodes whose chain reaches a root; bins 0 and n as they are, every other entry 0"""
    parent = np.asarray(parent, dtype=np.uint32).astype(np.int64)
    n = parent.size
    ok = chain_ok(parent)
    clade = np.zeros(n + 1, dtype=np.uint64)
    clade[0], clade[n] = direct[0], direct[n]
    for v in np.nonzero(np.asarray(direct[:n]))[0]:
        if v == 0 or not ok[v]:
            continue
        c, x = direct[v], int(v)
        while x != 0:
            clade[x] += c
            x = int(parent[x])
    return clade


def model(flags, keys, vals, parent):
    """-> (direct, clade), uint64 arrays of n + 1 entries"""
    n = len(parent)
    nb = len(keys)
    assert len(vals) == nb
    pres = present_mask(flags, nb) if nb else np.zeros(0, dtype=bool)
    bins = tally_bins(np.asarray(vals)[pres], parent)
    direct = np.bincount(bins, minlength=n + 1).astype(np.uint64)
    return direct, clade_sums(direct, parent)
