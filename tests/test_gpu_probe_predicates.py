"""The two-key probe (probe_minbucket2) leaves undone in its FIRST pass what only a later pass needs: the value is the slot's as
read, not selected under the hit (later passes select); the overflow table is asked only by a call that had a later pass (a lane
that walks down its chain sets one); and "found" is one compare of the 0 / 1 / 2 state, which the caller's ballot and its lane
predicate share.

These cases pin taxon, missing, ambig, n_hits and the ordered hit stream to the oracle, and the packed entry point to the ASCII
one (test_gpu_wide_stage.check), where those predicates have edges:
(a) missing / ambig with valid lanes that are not found and invalid lanes between them: one N at the first, a middle and the last
    base of reads of 65, 66, 120, 127 and 128 k-mers, reads of 129 and 192 k-mers (a single round behind a double round), and a
    short read behind a long one, whose lanes past its end would be valid by what the image held before;
(b) first-pass verdicts that must survive later passes: k = 21 under its window of 3 m-mers, k = 31 and 32 under a window of 9, where
    a double round has more than 24 run leaders, with a db of chosen k-mers only -- a lane's half A only, half B only, both --
    in lanes ranked below 16 and at 24 and above, a taxon per k-mer so that every value is told from its neighbours';
(c) chain walks and the overflow table: tables of 4, 8 and 16 home buckets filled to the loader's limit, where lanes walk their
    chains and keys live in the overflow table, units with no active lane and single-round units directly between units with
    walkers;
(d) the same batch with and without the hit stream;
(e) single and paired, ASCII and packed, k = 31 (double rounds) and k = 32 (pairs of rounds)."""
import numpy as np
import pytest

import classify_forms as F
import synth
import test_gpu_wide_stage as W

_WORLDS = {}


def world(oracle, k):
    if k not in _WORLDS:
        _WORLDS[k] = synth.make_world(oracle, seed=1200 + k, k=k, genome_len=3000)
    return _WORLDS[k]


def load(ctx, w, span, n_mb=0):
    """test_gpu_wide_stage.load with a fixed number of home buckets"""
    ctx.set_table_buckets(n_mb)
    try:
        return W.load(ctx, w, span)
    finally:
        ctx.set_table_buckets(0)


def check_both(ctx, oracle, w, reads, span, paired):
    """W.check (hit stream wanted), then the same batch without it: the same four arrays"""
    got, exp_hits, form = W.check(ctx, oracle, w, reads, span, paired)
    bases, offsets = synth.concat(reads)
    plain = ctx.classify(bases, offsets, paired=paired, want_hits=False)
    for key in ("taxon", "missing", "ambig", "n_hits"):
        assert np.array_equal(plain[key], got[key]), "without the hit stream: " + key
    return got, exp_hits, form


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("k", [31, 32])
def test_missing_and_ambig_between_invalid_lanes(gpu_ctx, oracle, k, paired):
    span = 15
    w = world(oracle, k)
    try:
        load(gpu_ctx, w, span)
        rng = np.random.default_rng(5 * k)
        g = np.concatenate(list(w.genomes.values()))

        def cut(nk, n_at=None, sub=0.02):
            L = nk + k - 1
            at = int(rng.integers(0, g.size - L))
            r = synth.mutate(rng, g[at:at + L], sub, 0.0)          # substitutions: valid k-mers that are not found
            if n_at is not None:
                r[n_at] = ord("N")
            return r
        reads = []
        for nk in (65, 66, 120, 127, 128):
            L = nk + k - 1
            for n_at in (0, L // 2, L - 1):
                reads.append(cut(nk, n_at))
        reads += [cut(129), cut(192), cut(129, 130), cut(192, 100), cut(127)]
        reads += [cut(220, None, 0.0), cut(66)]                     # a short read behind a long one
        reads += [synth.rand_seq(rng, 150), cut(120, None, 0.0)]    # nothing found, everything found
        assert len(reads) % 2 == 0
        if paired:                                                  # a read of every kind as a first and as a second mate
            reads = reads + reads[1:] + reads[:1]
        got, exp_hits, _ = check_both(gpu_ctx, oracle, w, reads, span, paired)
        assert (got["missing"] > 0).sum() >= 10 and (got["ambig"] > 0).sum() >= 10 and (got["n_hits"] > 0).sum() >= 10
    finally:
        gpu_ctx.debug_set(0)


def chosen_kmers_world(oracle, k, m, seed, patterns, n_kmers=128, min_runs=32):
    """a db that holds, of one random read per pattern, only the k-mers at the pattern's positions -- each under a taxon of its own
    position (three leaves by turns), so a value that belongs to another lane or another pass shows.  The reads are random
    sequences with min_runs window minima or more (a window of 9 m-mers gives 128 k-mers 25.6 on average: drawn again until)"""
    rng = np.random.default_rng(seed)
    tax = oracle.Taxonomy(pairs=[(1, 1), (2, 1), (3, 1), (100, 2), (101, 2), (102, 3)])
    table = oracle.Table()
    reads = []
    for pos in patterns:
        r = synth.rand_seq(rng, n_kmers + k - 1)
        while W.window_runs(r, k, m) < min_runs:
            r = synth.rand_seq(rng, n_kmers + k - 1)
        for j in pos:
            oracle.lca_map_add(table, tax, k, r[j:j + k].tobytes(), 100 + (j * 2654435761 >> 7) % 3)
        reads.append(r)
    w = synth.World()
    w.k, w.gaps, w.canon, w.tax, w.table, w.parent = k, None, True, tax, table, tax.parent
    w.flags, w.keys, w.vals = table.arrays()
    w.n_buckets = table.n_buckets
    return w, reads


PATTERNS = ([j for j in range(128) if j % 2 == 0],                  # a lane's half A only
            [j for j in range(128) if j % 2 == 1],                  # half B only
            [j for j in range(128) if j % 4 < 2],                   # both halves of every other lane
            [j for j in range(128) if j % 6 in (0, 3)],             # half A and half B by turns, neighbours missing
            list(range(128)),
            [0, 1, 126, 127],
            [])


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("k,span", [(21, 11), (31, 8), (32, 8)])
def test_first_pass_verdicts_survive_later_passes(gpu_ctx, oracle, k, span, paired):
    m = F.minimizer_len(k, span)
    assert k - m == (2 if k == 21 else span)
    if ("chosen", k) not in _WORLDS:
        _WORLDS[("chosen", k)] = chosen_kmers_world(oracle, k, m, 77 + k, PATTERNS)
    w, reads = _WORLDS[("chosen", k)]
    try:
        geo = load(gpu_ctx, w, span)
        n_mb = geo["buckets"]
        reads = list(reads) + [synth.revcomp(r) for r in reads]
        got, exp_hits, _ = check_both(gpu_ctx, oracle, w, reads, span, paired)
        # the data reaches its branches: more than 24 run leaders in the double round, hits ranked inside the first pass's stage
        # and beyond it, on either half
        seen = set()
        for i, pos in enumerate(PATTERNS):
            (_, nl, _, rk), = W.pair_stats(W.buckets_of(reads[i], k, m, n_mb), k)
            assert nl > 24, (i, nl)
            for j in pos:
                seen.add((j % 2, "first" if rk[j] < 16 else "later" if rk[j] >= 24 else "either"))
        assert seen >= {(0, "first"), (1, "first"), (0, "later"), (1, "later")}
        inc = 2 if paired else 1
        n_hits = np.array([len(pos) for pos in PATTERNS] * 2).reshape(-1, inc).sum(axis=1)
        assert np.array_equal(got["n_hits"], n_hits)
        assert any(len(set(h.tolist())) == 3 for h in exp_hits)
    finally:
        gpu_ctx.debug_set(0)


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("k,n_mb", [(31, 4), (31, 8), (31, 16), (32, 8)])
def test_walks_and_overflow_table_per_probe(gpu_ctx, oracle, k, n_mb, paired):
    """The loader takes 9.7 keys per home bucket: a db of that many CONSECUTIVE k-mers of one sequence -- a few minimizer groups, so
    homes with more keys than slots -- in 4, 8 and 16 home buckets.  Its keys are found down their chains and in the overflow
    table, and k-mers that are no keys walk the same chains to their ends."""
    span = 15
    n_keys = int(n_mb * 10 * 0.97) - 1
    if ("tiny", k, n_mb) not in _WORLDS:
        _WORLDS[("tiny", k, n_mb)] = chosen_kmers_world(oracle, k, F.minimizer_len(k, span), 300 + k + n_mb, [range(n_keys)], n_kmers=n_keys, min_runs=0)
    w, (seq,) = _WORLDS[("tiny", k, n_mb)]
    try:
        geo = load(gpu_ctx, w, span, n_mb)
        assert geo["buckets"] == n_mb and geo["spilled_keys"] > 0
        assert geo["overflow_keys"] > 0 or n_mb == 4               # (37 keys in 4 + 3 buckets: chains only)
        rng = np.random.default_rng(9 * k + n_mb)

        def embed(L, at):
            r = synth.rand_seq(rng, max(L, at + seq.size))
            r[at:at + seq.size] = seq
            return r

        def no_lane(L):                                             # an N in every k-mer: a probe with no active lane
            r = embed(L, 3)
            r[k // 2::k - 2] = ord("N")
            return r
        reads = []
        for i in range(6):
            # walkers | nobody | walkers | a single round | walkers, one k-mer in fifty lost | nobody | walkers | misses only
            reads += [embed(150, 7 * i), no_lane(150), synth.revcomp(embed(160 + i, 5 + i)), seq[i:i + 40 + k].copy(),
                      synth.mutate(rng, embed(250, 60 + i), 0.02, 0.0), no_lane(100 + k), seq.copy(), synth.rand_seq(rng, 150)]
        assert len(reads) % 2 == 0
        if paired:
            reads = reads + reads[1:] + reads[:1]
        got, exp_hits, _ = check_both(gpu_ctx, oracle, w, reads, span, paired)
        assert (got["n_hits"] >= n_keys).sum() >= 6 and (got["missing"] >= 64).sum() >= 6
        if not paired:
            assert (got["n_hits"] == n_keys).sum() >= 18 and (got["n_hits"] == 0).sum() >= 12
    finally:
        gpu_ctx.debug_set(0)
