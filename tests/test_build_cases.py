"""CPU tier of the device build's edge tests: the worlds of tests/build_cases.py hold what tests/test_gpu_build_edges.py relies
on, shown with the oracle alone.  These are conditions on the inputs, not measurements of the build: a GPU test that passes on a
world without them proves nothing."""
import collections
import re

import numpy as np
import pytest

import build_cases as bc

IDS = [c.name for c in bc.CASES]


@pytest.fixture(scope="module")
def contributions(oracle):
    """per case: (world, expected keys, expected values, per-sequence arrays of distinct keys)"""
    memo = {}

    def get(case):
        if case.name not in memo:
            w = bc.world_for(oracle, case)
            k, v, _ = bc.expected(oracle, w, case)
            memo[case.name] = (w, k, v, [np.unique(bc.stream(oracle, case, s)) for s in w.seqs])
        return memo[case.name]
    return get


def test_case_table():
    """every build form once; the seeds that take the run form and the one that does not"""
    assert len(set(IDS)) == len(IDS) >= 15
    for c in bc.CASES:
        assert bc.comb(c) <= c.w and (c.score == 0 or bc.windowed(c))
        assert c.gaps is None or len(c.gaps) == c.k - 1
    assert bc.encoder_runs(31, bc.G_HALF) == 16 and bc.encoder_runs(31, bc.G_TRIP) == 21      # extract_spaced_runs (p.n_runs > 0),
    assert bc.encoder_runs(31, bc.G_TWO) == 2                                                 # ... compress network above 4 runs
    assert bc.encoder_runs(31, bc.G_LONG) == 0 and bc.encoder_runs(31, None) == 0             # extract_spaced
    w131, w1031 = bc.BY_NAME["w131-forward"], bc.BY_NAME["w1031-canon"]
    assert w131.w - w131.k + 1 > 64 and bc.emitted_stream(w131)                               # the win_scratch form
    assert (2048 - (w1031.w - 1)) // 64 == 15                                                 # rounds per chunk


def test_world_shape(oracle):
    """the taxonomy and the sequences as the module's docstring describes them"""
    w = bc.make_edge_world(oracle, bc.SEED, 31, 50)
    ids = [t for t, _ in w.pairs]
    assert len(ids) == len(set(ids)) == bc.N_NODES and all(1 <= t < 5000 for t in ids)
    assert max(w.depth.values()) >= 25
    assert all(bc.ancestors_of(w.par, t)[-1] == 1 for t in ids)                               # every node reachable from the root
    assert sum(c < p for c, p in w.pairs[1:] if p != 1) >= 100                                # children numbered below their parents
    assert len(w.seqs) == 260 and set(w.cls) == set(bc.length_classes(31, 50))
    assert all(len(s) == L for s, L in zip(w.seqs, w.cls))
    assert set(w.taxids) <= set(ids)
    per_tax = collections.Counter(w.taxids)
    assert sum(1 for t in w.taxids if per_tax[t] > 1) >= 40                                   # contigs of one genome
    children = {p for _, p in w.pairs[1:]}
    assert sum(1 for t in w.taxids if t in children) >= 40                                    # internal nodes as genome taxids
    for r in range(3):                                                                        # a mobile element: met at the root
        who = w.repeat_carriers[r]
        assert len(who) >= 100
        common = set.intersection(*[set(bc.ancestors_of(w.par, w.taxids[i])) for i in who])
        assert max(w.depth[t] for t in common) <= 1
    who = w.repeat_carriers[3]
    assert len(who) >= 8 and all(w.deep_root in bc.ancestors_of(w.par, w.taxids[i]) for i in who)
    assert w.depth[w.deep_root] >= 20
    text = b"|".join(w.seqs)
    for run in (1, 5, 40):
        assert sum(1 for s in w.seqs if re.search(b"[^N]N{%d}[^N]" % run, s)) >= 10
    assert any(s[2028:2068] == b"N" * 40 for s in w.seqs)                                     # across base 2048 (a multiple of 32 too)
    assert any(s[32 * j - 2:32 * j + 3] == b"N" * 5 for s in w.seqs for j in range(1, len(s) // 32))
    assert sum(1 for s in w.seqs if len(s) >= 2047 and any(ch in s for ch in b"acgt")) >= 30
    assert all(ch in text for ch in b"RYK")
    assert len(w.poly) == 4 and len({w.taxids[i] for i in w.poly}) == 4
    assert all(b"A" * 40 in w.seqs[i] for i in w.poly[:2]) and all(b"T" * 40 in w.seqs[i] for i in w.poly[2:])
    assert set(w.seqs[w.all_n]) == {ord("N")} and len(w.seqs[w.all_n]) >= 2047
    # the same world whatever the form, but for the short lengths
    w2 = bc.make_edge_world(oracle, bc.SEED, 46, 46)
    assert w2.taxids == w.taxids and all(a == b for a, b, L in zip(w.seqs, w2.seqs, w.cls) if L >= 2047)


@pytest.mark.parametrize("name", IDS)
def test_world_has_what_the_build_tests_rely_on(oracle, contributions, name):
    case = bc.BY_NAME[name]
    w, keys, vals, per_seq = contributions(case)
    exp = dict(zip(keys.tolist(), vals.tolist()))
    n_win = case.w - bc.comb(case) + 1                   # k-mers per window
    # sequences that contribute: all but the short ones (and the one of nothing but N)
    n_contrib = sum(1 for u in per_seq if u.size)
    assert n_contrib >= 200, n_contrib
    # a real LCA was formed
    own = set(w.taxids)
    n_lca = sum(1 for v in vals.tolist() if v not in own)
    assert n_lca >= 30, n_lca
    assert all(int(v) in w.depth for v in np.unique(vals).tolist())
    depths = {w.depth[int(v)] for v in np.unique(vals).tolist()}
    assert len(depths) >= 10, sorted(depths)
    # contention: 100 keys that 50 or more sequences fold into -- where a world of this size can hold as many.  Such a key costs 50
    # contributions; a window of n_win k-mers keeps about 2 / (n_win + 1) of a sequence's positions, so at n_win = 1001 a sequence of
    # 4100 bases (3070 windows) contributes about 6 keys and all 260 sequences fewer than 1600: no more than 32 keys could have 50
    # contributors if every sequence were the same.  There the count asked for shrinks with the density of the minima: 100 at the
    # 20 k-mers a window of `-w 50`, 100 * 21 / (n_win + 1) = 2 at n_win = 1001.
    allk, cnt = np.unique(np.concatenate(per_seq), return_counts=True)
    assert np.array_equal(allk, keys)                    # the map's keys are the union of the streams
    need = 100 if sum(u.size for u in per_seq) >= 2 * 100 * 50 else (100 * 21) // (n_win + 1)
    assert need == (2 if name == "w1031-canon" else 100)
    n_hot = int((cnt >= 50).sum())
    assert n_hot >= need, (n_hot, need)
    # key 0 is a real key
    if not bc.windowed(case) and not bc.is_spaced(case) and case.canon:
        lca = 0
        for i in w.poly:
            lca = w.taxids[i] if lca == 0 else w.tax.lca(w.taxids[i], lca)
        assert exp.get(0) == lca and sum(1 for u in per_seq if u.size and u[0] == 0) == 4
    # every length class, with the number of keys the oracle says: zero below the comb, one flushed minimum in the emitted-stream
    # forms below the window
    for L, i in w.clean.items():
        assert len(w.seqs[i]) == L
        got = bc.stream(oracle, case, w.seqs[i]).size
        assert got == bc.clean_stream_len(case, L), (L, got)
        assert (per_seq[i].size == 0) == (got == 0)
    assert any(bc.clean_stream_len(case, L) == 0 for L in w.clean) and any(bc.clean_stream_len(case, L) == 1 for L in w.clean)
    # ignoring the N mask cannot pass
    plain = [bc.unmasked(s) for s in w.seqs]
    assert sum(1 for a, b in zip(plain, w.seqs) if a != b) == len(w.masked) >= 100
    k2, v2 = bc.table_pairs(bc.oracle_table(oracle, w.tax, case, plain, w.taxids))
    assert not (np.array_equal(k2, keys) and np.array_equal(v2, vals))
    assert set(k2.tolist()) - set(exp)                   # (k-mers across an N that the reference never emits)


@pytest.mark.parametrize("name", bc.FOLD_TWICE + ("k21-canon",))
def test_fold_route_checks_itself(oracle, name):
    """the fold over the oracle's stream (the only route for the string overload's score) against the oracle's own lca_map, on
    forms that have both"""
    case = bc.BY_NAME[name]
    w = bc.world_for(oracle, case)
    assert bc.oracle_supports(case)
    assert bc.folded_map(oracle, w.tax, case, w.seqs, w.taxids) == bc.expected_map(oracle, w, case)


def test_buckets_for():
    assert [bc.buckets_for(n) for n in (0, 1, 3, 4, 6, 7, 12, 13, 49, 50)] == [4, 4, 4, 8, 8, 16, 16, 32, 64, 128]
