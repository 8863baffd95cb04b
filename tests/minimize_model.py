"""The model of taxonomic-depth minimizer selection ("Defined behaviour"; bns_build_minimize_*, `bonsai build -D`), in
numpy and plain Python.  A helper module, not a conftest.  Nothing here comes from the device: the k-mers of every position are
computed from the bases, F (k-mer -> LCA of all sequences that hold it) with the oracle's lca_map_add, the depths from the parent
array, and the windows by the rule as it is written down:

  depth(t)  nodes on the chain t -> root, root included; 0 for 0xFFFFFFFF, an id that is no node, a chain that reaches no root
  score(x)  (0xFFFFFFFF - depth(F[x])) << 32 | F[x], smaller is better
  window p  of a sequence of n bases (max(0, n - w + 1) of them) holds the k-mers starting at p .. p + w - c and selects, among the
            valid ones, the smallest (score, k-mer); none valid: nothing
  M         every selected k-mer -> F[k-mer]
"""
import collections

import numpy as np

ABSENT = 0xFFFFFFFF
_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _i
    _CODE[_ch | 0x20] = _i


def comb_of(k, gaps):
    return k + (sum(int(g) for g in gaps) if gaps is not None else 0)


def is_spaced(gaps):
    return gaps is not None and any(int(g) for g in gaps)


def position_kmers(seq, k, gaps=None, canon=True):
    """(kmers uint64, valid bool) for every start position 0 .. n - c of seq (bytes or uint8 array); empty when n < c.  A spaced
    seed samples bases at the cumulative offsets of gaps + 1 and is never canonicalised; only the sampled bases must be A/C/G/T, and
    a spaced k-mer equal to ~0 (the all-T 32-mer) is not valid.  Contiguous: canonical = min(forward, reverse complement)."""
    a = np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq, dtype=np.uint8)
    spaced = is_spaced(gaps)
    pos = np.concatenate([[0], np.cumsum(np.asarray(gaps if gaps is not None else [0] * (k - 1), dtype=np.int64) + 1)]).astype(np.int64)
    c = int(pos[-1]) + 1
    n = a.size - c + 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=bool)
    code = _CODE[a]
    fwd = np.zeros(n, dtype=np.uint64)
    rc = np.zeros(n, dtype=np.uint64)
    bad = np.zeros(n, dtype=bool)
    for i in range(k):
        ci = code[int(pos[i]):int(pos[i]) + n]
        bad |= ci > 3
        c2 = (ci & 3).astype(np.uint64)
        fwd |= c2 << np.uint64(2 * (k - 1 - i))
        rc |= (np.uint64(3) - c2) << np.uint64(2 * i)
    if spaced:
        return fwd, ~bad & (fwd != np.uint64(0xFFFFFFFFFFFFFFFF))
    return (np.minimum(fwd, rc) if canon else fwd), ~bad


def depths(parent):
    """{id: depth} for every node of the parent array bns_load_taxonomy takes (parent[root] == 0, ABSENT where the id is no node)
    whose chain reaches a root; walked iteratively, every chain once (memoised)."""
    parent = np.asarray(parent)
    n = parent.size
    d = {}
    for t in np.flatnonzero(parent != ABSENT).tolist():
        if t == 0:
            continue
        chain = []
        x = t
        base = None
        while True:
            if x in d:
                base = d[x] or None                      # (0: x's own chain reaches no root)
                break
            if x == 0 or x >= n or int(parent[x]) == ABSENT or len(chain) > n:
                base = None                              # left the taxonomy before a root: no depth for anything on the chain
                break
            chain.append(x)
            if int(parent[x]) == 0:
                base = 0
                break
            x = int(parent[x])
        if base is None:
            for y in chain:
                d[y] = 0
        else:
            for i, y in enumerate(reversed(chain)):
                d[y] = base + i + 1
    return d


def full_map(oracle, tax, seqs, taxids, k, gaps=None, canon=True):
    """F: the oracle's sequential update_lca_map of every unwindowed k-mer of every sequence, as a dict"""
    t = oracle.Table()
    g = list(gaps) if gaps is not None else None
    for s, tx in zip(seqs, taxids):
        oracle.lca_map_add(t, tax, k, s, tx, gaps=g, canon=canon)
    f, keys, vals = t.arrays()
    i = np.arange(t.n_buckets)
    m = ((f[i >> 4] >> ((i & 15) << 1)) & 3) == 0
    return dict(zip(keys[m].tolist(), vals[m].tolist()))


def score_of(F, depth, x):
    v = F[x]
    return ((0xFFFFFFFF - depth.get(v, 0)) << 32) | v


def window_minima(entries, ws):
    """entries: one (score, kmer) tuple or None (not valid) per position; yields, per window of ws positions, the smallest valid
    entry or None.  A monotonic deque: O(positions) whatever ws."""
    dq = collections.deque()                             # indices, their entries ascending
    for i, e in enumerate(entries):
        if e is not None:
            while dq and entries[dq[-1]] >= e:
                dq.pop()
            dq.append(i)
        if i >= ws - 1:
            while dq and dq[0] <= i - ws:
                dq.popleft()
            yield entries[dq[0]] if dq else None


def select(F, depth, seqs, k, w, gaps=None, canon=True, stats=None):
    """M as a dict: every selected k-mer -> F[k-mer].  stats (a dict, optional) receives windows, mixed (windows holding k-mers of
    two or more depths), ties (windows whose smallest score is held by two or more DIFFERENT k-mers) and valid (valid positions of
    sequences that have a window)."""
    c = comb_of(k, gaps)
    w = max(w, c)
    ws = w - c + 1
    M = {}
    n_win = n_mixed = n_ties = n_valid = 0
    for s in seqs:
        if len(s) < w:
            continue
        km, ok = position_kmers(s, k, gaps, canon)
        kl = km.tolist()
        entries = [(score_of(F, depth, x), x) if v else None for x, v in zip(kl, ok.tolist())]
        n_valid += int(ok.sum())
        for p, best in enumerate(window_minima(entries, ws)):
            n_win += 1
            if stats is not None:
                held = [e for e in entries[p:p + ws] if e is not None]
                if len({e[0] >> 32 for e in held}) >= 2:
                    n_mixed += 1
                if best is not None and len({e[1] for e in held if e[0] == best[0]}) >= 2:
                    n_ties += 1
            if best is not None:
                M[best[1]] = F[best[1]]
    if stats is not None:
        stats.update(windows=n_win, mixed=n_mixed, ties=n_ties, valid=n_valid)
    return M


def sorted_pairs(M):
    """(keys ascending uint64, values uint32) of a dict"""
    keys = np.fromiter(M.keys(), dtype=np.uint64, count=len(M))
    vals = np.fromiter(M.values(), dtype=np.uint32, count=len(M))
    o = np.argsort(keys, kind="stable")
    return keys[o], vals[o]


_EXPECTED = {}


def expected(oracle, world, k, w, gaps=None, canon=True):
    """(keys, values, F, depth) of the edge world `world` (build_cases.make_edge_world) in one form; computed once and shared"""
    key = (world.seed, world.c, world.w, k, w, tuple(gaps) if gaps is not None else None, canon)
    if key not in _EXPECTED:
        F = full_map(oracle, world.tax, world.seqs, world.taxids, k, gaps, canon)
        depth = depths(world.parent)
        ks, vs = sorted_pairs(select(F, depth, world.seqs, k, w, gaps, canon))
        ks.setflags(write=False); vs.setflags(write=False)
        _EXPECTED[key] = (ks, vs, F, depth)
    return _EXPECTED[key]
