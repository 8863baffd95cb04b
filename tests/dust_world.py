"""A small world whose genomes hold low-complexity tracts, reads simulated from it, and the substitution that is the truth of every
bns_set_dust test: a call with masking on for input x equals the same call with it off for substitute(x, mask(x)).  A helper, not a
test."""
import numpy as np

import dust_ref as D
import synth

W, T = 64, 20


def gen_tract(rng):
    """a homopolymer of 20-60 bases, or a unit of 2-6 bases repeated to 24-72"""
    if rng.random() < 0.4:
        seg = np.full(int(rng.integers(20, 61)), int(rng.integers(0, 4)))
    else:
        seg = np.tile(rng.integers(0, 4, size=int(rng.integers(2, 7))), 12)[:int(rng.integers(24, 73))]
    return synth.ACGT[seg]


def tract_genomes(rng, genome_len=6000):
    """synth.make_genomes with a tract every 120-320 bases"""
    g = synth.make_genomes(rng, genome_len)
    for leaf in g:
        seq = g[leaf].copy()
        at = int(rng.integers(40, 160))
        while at + 80 < seq.size:
            t = gen_tract(rng)
            seq[at:at + t.size] = t
            at += t.size + int(rng.integers(120, 320))
        g[leaf] = seq
    return g


def make_world(oracle, seed=31, k=31, genome_len=6000, gaps=None, canon=True):
    rng = np.random.default_rng(seed)
    w = synth.World()
    w.k, w.gaps, w.canon = k, gaps, canon
    w.tax = oracle.Taxonomy(pairs=synth.TAX_PAIRS)
    w.parent = w.tax.parent
    w.genomes = tract_genomes(rng, genome_len)
    w.table = oracle.Table()
    for leaf, g in w.genomes.items():
        oracle.lca_map_add(w.table, w.tax, k, g.tobytes(), leaf, gaps=gaps, canon=canon)
    w.flags, w.keys, w.vals = w.table.arrays()
    w.n_buckets = w.table.n_buckets
    w.rng = rng
    return w


def substituted(seqs, W=W, T=T):
    """uint8 arrays (or bytes) -> (uint8 arrays with 'N' at every masked base, the masks)"""
    raw = [s.tobytes() if hasattr(s, "tobytes") else bytes(s) for s in seqs]
    masks = D.batch_masks(raw, W, T)
    return [np.frombuffer(D.substitute(s, m), dtype=np.uint8) for s, m in zip(raw, masks)], masks


def same_units(a, b, paired=False):
    """taxon, missing, ambig, n_hits and -- where both have them -- the ordered hits / the runs, unit by unit"""
    for k in ("taxon", "missing", "ambig", "n_hits"):
        bad = np.flatnonzero(np.asarray(a[k]) != np.asarray(b[k]))
        assert bad.size == 0, "%s differs at %d units, first %s: %s / %s" % (k, bad.size, bad[:5], np.asarray(a[k])[bad[:5]], np.asarray(b[k])[bad[:5]])
    for k in ("hits",):
        if k in a and k in b:
            assert len(a[k]) == len(b[k])
            for u, (x, y) in enumerate(zip(a[k], b[k])):
                assert np.array_equal(x, y), "hits of unit %d" % u
    if "runs" in a and "runs" in b:
        for u, (x, y) in enumerate(zip(a["runs"], b["runs"])):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), "runs of unit %d" % u


def changed_share(a, b):
    """the share of units of which some per-unit output differs between two runs"""
    d = np.zeros(len(a["taxon"]), dtype=bool)
    for k in ("taxon", "missing", "ambig", "n_hits"):
        d |= np.asarray(a[k]) != np.asarray(b[k])
    return float(d.mean())
