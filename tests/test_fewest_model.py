"""CPU tier of fewest-genome minimizer selection: the model the GPU tests compare against (tests/fewest_model.py) selects what a
brute-force reading of the rule selects, its counts depend on the partition of the sequences into genomes and on nothing else, and
the hand-made input of the GPU rule test really separates the three levels of the score."""
import numpy as np
import pytest

import build_cases as bc
import fewest_model as fm
import minimize_model as mm
import synth
from test_minimize_model import BY_NAME, FORMS, world_of

NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def brute_select(F, n, seqs, k, w, gaps, canon):
    """rules 2-4 read literally: per sequence the (score, k-mer) of every position, per window the minimum over its slice -- first of
    the scores, then of the k-mers that hold that score -- with no deque and no running state"""
    c = mm.comb_of(k, gaps)
    w = max(w, c)
    ws = w - c + 1
    M = {}
    for s in seqs:
        if len(s) < w:
            continue
        km, ok = mm.position_kmers(s, k, gaps, canon)
        sc = np.array([(n[x] << 32) | F[x] if v else int(NONE) for x, v in zip(km.tolist(), ok.tolist())], dtype=np.uint64)
        el = np.where(ok, km, NONE)
        vs = np.lib.stride_tricks.sliding_window_view(sc, ws)
        ve = np.lib.stride_tricks.sliding_window_view(el, ws)
        assert vs.shape[0] == len(s) - w + 1
        best = vs.min(axis=1)
        who = np.where(vs == best[:, None], ve, NONE).min(axis=1)
        for x in np.unique(who[best != NONE]).tolist():
            M[x] = F[x]
    return M


@pytest.mark.parametrize("seed", [bc.SEED, bc.SEED + 1], ids=["committed-world", "second-world"])
@pytest.mark.parametrize("name", [f[0] for f in FORMS])
def test_select_fewest_against_brute_force(oracle, name, seed):
    _, k, gaps, w, canon = BY_NAME[name]
    wld = bc.make_edge_world(oracle, seed, mm.comb_of(k, gaps), w)
    ids = fm.deal_genomes(len(wld.seqs))
    F = mm.full_map(oracle, wld.tax, wld.seqs, wld.taxids, k, gaps, canon)
    n = fm.genome_counts(wld.seqs, ids, k, gaps, canon)
    assert set(n) == set(F)                               # every k-mer of F is held by somebody, and nothing else is
    got = fm.select_fewest(F, n, wld.seqs, k, w, gaps, canon)
    assert got == brute_select(F, n, wld.seqs, k, w, gaps, canon)
    if w <= mm.comb_of(k, gaps):
        assert got == F
    else:
        assert 0 < len(got) < len(F)


def test_the_dealt_genomes_hold_what_the_gpu_tests_rely_on(oracle):
    wld = world_of(oracle, BY_NAME["k31-w50-canon"])
    ids = fm.deal_genomes(len(wld.seqs))
    assert ids == sorted(ids) and len(set(ids)) * 3 >= len(ids) > len(set(ids)) * 2          # several sequences a genome
    tax_of = {}
    for g, t in zip(ids, wld.taxids):
        tax_of.setdefault(t, set()).add(g)
    assert any(len(gs) >= 2 for gs in tax_of.values())                                        # two genomes share a taxid
    assert any(len(s) < 31 for s in wld.seqs) and any(31 <= len(s) < 50 for s in wld.seqs)    # shorter than c, shorter than w
    n = fm.genome_counts(wld.seqs, ids, 31)
    hist = np.bincount(np.fromiter(n.values(), dtype=np.int64))
    print("counts: %s" % hist[:12].tolist(), "largest", hist.size - 1)
    assert hist[1] > 1000 and hist[2:].sum() > 1000 and hist.size - 1 > 8                     # private, shared and widely shared k-mers
    # a k-mer that occurs in two sequences of one genome counts once: some k-mer's count is below its number of carriers
    carriers = {}
    for s in wld.seqs:
        km, ok = mm.position_kmers(s, 31)
        for x in set(km[ok].tolist()):
            carriers[x] = carriers.get(x, 0) + 1
    assert sum(1 for x in n if carriers[x] > n[x]) > 100


def test_counts_depend_on_the_partition_alone(oracle):
    wld = world_of(oracle, BY_NAME["k31-w50-canon"])
    seqs = wld.seqs
    ids = fm.deal_genomes(len(seqs))
    n = fm.genome_counts(seqs, ids, 31)
    # renumbered: an injective map of the ids, neither monotonic nor dense
    rng = np.random.default_rng(5)
    new = rng.permutation(4000000000 + np.arange(len(set(ids)), dtype=np.int64) * 7919 % 1000003)
    assert np.unique(new).size == len(set(ids))
    assert fm.genome_counts(seqs, [int(new[g]) for g in ids], 31) == n
    # the sequences in another order, each with its id
    o = rng.permutation(len(seqs)).tolist()
    assert fm.genome_counts([seqs[i] for i in o], [ids[i] for i in o], 31) == n
    # another partition is another answer
    assert fm.genome_counts(seqs, list(range(len(seqs))), 31) != n


# ---- the hand-made input of tests/test_gpu_build_fewest.py's rule test ------------------------------------------------------------
# 1 - 2 - 4 - 6        depths 1, 2, 3, 4
#       \ 5            3
#   \ 3 - 7 - 8        2, 3, 4
PAIRS8 = [(1, 1), (2, 1), (3, 1), (4, 2), (5, 2), (6, 4), (7, 3), (8, 7)]


def rule_input():
    """k 31, w 32: a sequence of 32 bases is one window of two k-mers.  Returns seqs, taxids, genome ids (non-decreasing) and the
    k-mers named below."""
    rng = np.random.default_rng(271)
    other = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}

    def km(s):
        k, ok = mm.position_kmers(s, 31, None, True)
        assert ok.all()
        return [int(x) for x in k]
    # (a) x0 in A (genome 0) and A2 (genome 1): n = 2; x1 in A alone: n = 1.  Depth agrees: F[x0] = lca(6, 7) = 1, F[x1] = 6
    A = synth.rand_seq(rng, 32).tobytes()
    A2 = A[:31] + other[A[31]]
    # (b) e0 in E (genome 2) and E2 (genome 3), both under 6: n = 2, F = 6, depth 4.  e1 in E and E3 (7) of the SAME genome: n = 1,
    #     F = lca(6, 7) = 1, depth 1.  The count keeps e1, the depth keeps e0
    E = synth.rand_seq(rng, 32).tobytes()
    E3 = other[E[0]] + E[1:]
    E2 = E[:31] + other[E[31]]
    # (c) equal counts, the taxid decides: y0 in B (5) alone, y1 in B and B2 (6) of one genome: n = 1 both, F = 5 and lca(5, 6) = 2
    B = synth.rand_seq(rng, 32).tobytes()
    B2 = other[B[0]] + B[1:]
    # (d) equal scores, the k-mer decides: both k-mers of C under 5 alone
    C = synth.rand_seq(rng, 32).tobytes()
    seqs = [A, A2, E, E3, E2, B, B2, C]
    taxids = [6, 7, 6, 7, 6, 5, 6, 5]
    genomes = [0, 1, 2, 2, 3, 4, 4, 5]
    x0, x1 = km(A); e0, e1 = km(E); y0, y1 = km(B); c0, c1 = km(C)
    return seqs, taxids, genomes, dict(x0=x0, x1=x1, e0=e0, e1=e1, y0=y0, y1=y1, c0=c0, c1=c1)


def test_rule_input_separates_the_three_levels(oracle):
    tax = oracle.Taxonomy(pairs=PAIRS8)
    seqs, taxids, genomes, q = rule_input()
    assert genomes == sorted(genomes)
    F = mm.full_map(oracle, tax, seqs, taxids, 31)
    n = fm.genome_counts(seqs, genomes, 31)
    assert len(F) == 12                                   # 8 sequences of two k-mers, four of them shared
    assert (n[q["x0"]], n[q["x1"]], F[q["x0"]], F[q["x1"]]) == (2, 1, 1, 6)
    assert (n[q["e0"]], n[q["e1"]], F[q["e0"]], F[q["e1"]]) == (2, 1, 6, 1)
    assert (n[q["y0"]], n[q["y1"]], F[q["y0"]], F[q["y1"]]) == (1, 1, 5, 2)
    assert (n[q["c0"]], n[q["c1"]], F[q["c0"]], F[q["c1"]]) == (1, 1, 5, 5)
    # which level decides every window
    levels = {"count": 0, "taxid": 0, "kmer": 0}
    for s in seqs:
        a, b = (int(x) for x in mm.position_kmers(s, 31)[0])
        assert a != b
        levels["count" if n[a] != n[b] else "taxid" if F[a] != F[b] else "kmer"] += 1
    print(levels)
    assert min(levels.values()) >= 1
    G = fm.select_fewest(F, n, seqs, 31, 32)
    D = mm.select(F, mm.depths(tax.parent), seqs, 31, 32)
    assert q["x1"] in G and q["x0"] not in G
    assert q["e1"] in G and q["e0"] not in G and G[q["e1"]] == 1      # (E2 keeps its private k-mer, not e0)
    assert q["y1"] in G and q["y0"] not in G and G[q["y1"]] == 2
    assert min(q["c0"], q["c1"]) in G and max(q["c0"], q["c1"]) not in G
    assert q["e0"] in D and q["e1"] not in D and q["y0"] in D
    assert set(G) != set(D)
