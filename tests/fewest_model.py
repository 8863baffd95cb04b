"""The model of fewest-genome minimizer selection ("Defined behaviour"; bns_build_count_*, bns_build_minimize_begin_score,
`bonsai build -G`), in numpy and plain Python.  A helper module, not a conftest.  Nothing here comes from the device: the k-mers of
every position are minimize_model's, F is the oracle's, the counts are the sizes of plain sets of genome ids, and the windows are
selected by the rule as it is written down:

  n(x)      distinct genome ids among the sequences that hold x as a valid k-mer
  score(x)  n(x) << 32 | F[x], smaller is better: fewer genomes, then the smaller taxid, then the smaller k-mer
  window p  as in minimize_model: the smallest (score, k-mer) among the valid k-mers starting at p .. p + w - c; none valid: nothing
  M         every selected k-mer -> F[k-mer]
"""
import minimize_model as mm
from minimize_model import full_map, position_kmers, sorted_pairs, window_minima  # noqa: F401  (what the tests use beside the two below)


def genome_counts(seqs, genome_ids, k, gaps=None, canon=True):
    """{k-mer: n}: per valid k-mer of any sequence, the number of distinct genome ids among the sequences that hold it"""
    held = {}
    for s, g in zip(seqs, genome_ids):
        km, ok = position_kmers(s, k, gaps, canon)
        for x in set(km[ok].tolist()):
            held.setdefault(x, set()).add(int(g))
    return {x: len(ids) for x, ids in held.items()}


def score_of(F, n, x):
    return (n[x] << 32) | F[x]


def select_fewest(F, n, seqs, k, w, gaps=None, canon=True):
    """M as a dict: every selected k-mer -> F[k-mer]"""
    c = mm.comb_of(k, gaps)
    w = max(w, c)
    ws = w - c + 1
    M = {}
    for s in seqs:
        if len(s) < w:
            continue
        km, ok = position_kmers(s, k, gaps, canon)
        entries = [(score_of(F, n, x), x) if v else None for x, v in zip(km.tolist(), ok.tolist())]
        for best in window_minima(entries, ws):
            if best is not None:
                M[best[1]] = F[best[1]]
    return M


def deal_genomes(n_seqs, per_genome=3):
    """genome ids for the sequences of an edge world, in stream order: `per_genome` consecutive sequences are one genome.  The world
    deals its length classes three in a row and its taxids at random, so genomes of several sequences, sequences shorter than the comb
    and the window, and genomes that share a taxid all occur (tests/test_fewest_model.py checks that they do)."""
    return [i // per_genome for i in range(n_seqs)]


_EXPECTED = {}


def expected(oracle, world, genome_ids, k, w, gaps=None, canon=True):
    """(keys, values, F, n) of the edge world `world` (build_cases.make_edge_world) in one form under one dealing of genome ids;
    computed once and shared, and handed out read-only"""
    key = (world.seed, world.c, world.w, tuple(genome_ids), k, w, tuple(gaps) if gaps is not None else None, canon)
    if key not in _EXPECTED:
        F = mm.expected(oracle, world, k, w, gaps, canon)[2]
        n = genome_counts(world.seqs, genome_ids, k, gaps, canon)
        ks, vs = sorted_pairs(select_fewest(F, n, world.seqs, k, w, gaps, canon))
        ks.setflags(write=False); vs.setflags(write=False)
        _EXPECTED[key] = (ks, vs, F, n)
    return _EXPECTED[key]
