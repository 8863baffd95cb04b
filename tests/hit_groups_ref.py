"""The minimum number of hit groups (bns_set_min_hit_groups, `bonsai classify -M`) restated from its definition in DESIGN.md: keys from the
oracle's encoder, look-ups in the oracle's table, numpy's unique -- nothing here calls the code under test.  Test infrastructure only.

  G(u) = the number of DISTINCT keys among the k-mers of all mates of u that the table holds;  the taxon of u becomes 0 when it was not
  0 and G(u) < N (N = 0: off)."""
import numpy as np

import synth


def unit_keys(oracle, mates, k, gaps=None, canon=True, spaced_intended=True):
    """the keys classify looks up for one unit, mate after mate, in order (uint64)"""
    ks = [oracle.encode(bytes(m.tobytes() if hasattr(m, "tobytes") else m), k, gaps=gaps, canon=canon, spaced_intended=spaced_intended)
          for m in mates]
    return np.concatenate(ks) if ks else np.zeros(0, np.uint64)


def groups(oracle, table, mates, k, **kw):
    """(G, found positions) of one unit"""
    keys = unit_keys(oracle, mates, k, **kw)
    if keys.size == 0:
        return 0, 0
    found = table.get_batch(keys)[1] != 0
    return int(np.unique(keys[found]).size), int(found.sum())


def units_of(reads, paired):
    return [tuple(reads[2 * i:2 * i + 2]) for i in range(len(reads) // 2)] if paired else [(r,) for r in reads]


def groups_of(oracle, table, reads, paired, k, **kw):
    """(G int64[n_units], found positions int64[n_units])"""
    gf = [groups(oracle, table, u, k, **kw) for u in units_of(reads, paired)]
    return np.array([g for g, _ in gf], dtype=np.int64), np.array([f for _, f in gf], dtype=np.int64)


def apply(taxon, g, n):
    """the taxa the setting n leaves: arrays (or scalars) of taxa and of G"""
    taxon, g = np.asarray(taxon, dtype=np.uint32), np.asarray(g, dtype=np.int64)
    return np.where((taxon != 0) & (g < int(n)), np.uint32(0), taxon).astype(np.uint32)


# ---- the worlds the tests share (built once per process) ----------------------------------------------------------------------------------
_CACHE = {}


def thinned_world(oracle, base):
    """base's genomes and taxonomy with a db of the minimizers of windows of 50 bases (lexicographic score), as the benchmark's `-w 50`
    dbs: a 150-base read of a genome finds a handful of keys"""
    if "thin" not in _CACHE:
        w = synth.World()
        w.k, w.gaps, w.canon, w.tax, w.parent, w.genomes = 31, None, True, base.tax, base.parent, base.genomes
        w.table = oracle.Table()
        for leaf, g in w.genomes.items():
            oracle.lca_map_add_windowed(w.table, w.tax, 31, 50, 0, g.tobytes(), leaf)
        w.flags, w.keys, w.vals = w.table.arrays()
        w.n_buckets = w.table.n_buckets
        _CACHE["thin"] = w
    return _CACHE["thin"]


def parity_reads(base, paired):
    """about 600 simulated reads: variable length, 2 % substitutions, 1 % N, 15 % random"""
    return synth.simulate_reads(np.random.default_rng(51 + int(paired)), base.genomes, 600, var_len=True, sub_rate=0.02, n_rate=0.01, random_frac=0.15)


def oracle_units(oracle, w, reads, paired, **kw):
    """[(taxon, missing, ambig, hits)] per unit"""
    return [oracle.classify_seq(w.table, w.tax, w.k, u[0].tobytes(), u[1].tobytes() if len(u) > 1 else None, **kw) for u in units_of(reads, paired)]


def parity_case(oracle, base, paired):
    """(world, reads, oracle units, G, found positions) of the API parity test, single or paired"""
    key = ("parity", bool(paired))
    if key not in _CACHE:
        w = thinned_world(oracle, base)
        reads = parity_reads(base, paired)
        units = oracle_units(oracle, w, reads, paired)
        g, f = groups_of(oracle, w.table, reads, paired, 31)
        _CACHE[key] = (w, reads, units, g, f)
    return _CACHE[key]


PERIOD = 7
REPEAT_UNIT = np.frombuffer(b"ACGGTCA", dtype=np.uint8)       # no shorter period


def repeat_world(oracle):
    """an every-k-mer db of one genome that holds a 400-base tandem repeat of period 7 between random flanks -> (world, repeat start)"""
    if "repeat" not in _CACHE:
        rng = np.random.default_rng(77)
        rep = np.tile(REPEAT_UNIT, 400 // PERIOD + 1)[:400]
        g = np.concatenate([synth.rand_seq(rng, 800), rep, synth.rand_seq(rng, 800)])
        w = synth.World()
        w.k, w.gaps, w.canon = 31, None, True
        w.tax = oracle.Taxonomy(pairs=synth.TAX_PAIRS)
        w.parent = w.tax.parent
        w.genomes = {1001: g}
        w.table = oracle.Table()
        oracle.lca_map_add(w.table, w.tax, 31, g.tobytes(), 1001)
        w.flags, w.keys, w.vals = w.table.arrays()
        w.n_buckets = w.table.n_buckets
        _CACHE["repeat"] = (w, 800)
    return _CACHE["repeat"]


def two_strand_world(oracle):
    """an encoder that does not canonicalise, over a db that holds the forward k-mers of one genome AND those of its reverse
    complement: a read and its reverse complement then find two disjoint sets of keys (k is odd: no k-mer is its own)"""
    if "two" not in _CACHE:
        rng = np.random.default_rng(78)
        g = synth.rand_seq(rng, 3000)
        w = synth.World()
        w.k, w.gaps, w.canon = 31, None, False
        w.tax = oracle.Taxonomy(pairs=synth.TAX_PAIRS)
        w.parent = w.tax.parent
        w.genomes = {1003: g}
        w.table = oracle.Table()
        for s in (g, synth.revcomp(g)):
            oracle.lca_map_add(w.table, w.tax, 31, s.tobytes(), 1003, canon=False)
        w.flags, w.keys, w.vals = w.table.arrays()
        w.n_buckets = w.table.n_buckets
        _CACHE["two"] = w
    return _CACHE["two"]


def long_world(oracle):
    """synth's world with 24-kb genomes, every k-mer in the db (test_gpu_confidence's long units)"""
    if "long" not in _CACHE:
        _CACHE["long"] = synth.make_world(oracle, seed=17, k=31, genome_len=24000)
    return _CACHE["long"]


def late_key_reads(oracle, w, n, length=10000):
    """Two reads of `length` bases over w's first genome, built from n segments of 31 bases (one key each; they come from places 370
    bases apart, so they are n distinct keys).  Between two segments stands one base, chosen so that the table holds no k-mer across
    the junction (the genomes share sequence: the base that follows a segment in one genome need not in another).
      * `never`: the first n - 1 segments, over and over, to the end.
      * `late`:  the same with the n-th segment in place of the last 31 bases: its key is the last k-mer of the read."""
    g = next(iter(w.genomes.values()))
    # (370: no two of them a multiple of the genomes' 500-base segments apart; 57: none begins or ends where such a segment does -- there
    # every base is some genome's continuation)
    at = [370 * i + 57 for i in range(n)]
    segs = [g[a:a + 31] for a in at]

    def separator(left, right, one=True):
        """x such that left + x + right holds the keys of left and right and no other"""
        for x in [(a,) for a in synth.ACGT if one] + [(a, b) for a in synth.ACGT for b in synth.ACGT]:     # (one base; two where no one base does)
            x = np.array(x, dtype=np.uint8)
            if groups(oracle, w.table, (np.concatenate([left, x, right]),), 31)[1] == (1 if left.size < 31 else 2):
                return x
        raise AssertionError("no separator")

    parts, size, i = [], 0, 0
    while size < length:
        a, b = segs[i % (n - 1)], segs[(i + 1) % (n - 1)]
        parts += [a, separator(a, b)]
        size += 31 + parts[-1].size
        i += 1
    never = np.concatenate(parts)[:length].copy()
    late = never.copy()
    late[length - 31:] = segs[n - 1]
    late[length - 33:length - 31] = separator(never[length - 63:length - 33], segs[n - 1], one=False)    # (left: 30 bases, no key of their own)
    return never, late
