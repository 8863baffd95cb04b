"""classify_kernel runs the k-mer rounds of a read through the clustered-table probe two at a time (probe_minbucket2): one
set of probe passes and one vote for rounds 2p and 2p + 1.  These cases pin the device result -- taxon, missing, ambig and
the ordered hit stream -- to the oracle where that pairing has edges: k-mer counts around the round and pair boundaries, an
odd last round, chunks of 2048 bases (31 rounds: every chunk ends on a one-round probe), minimizer groups that straddle
k-mer 64, pairs with more distinct groups than the 16-bucket stage holds, chain walks and overflow-table keys in the second
round only, N bases at the round boundary, and units with more than 64 taxa.  Each case checks that its data reaches its
branch, from a host restatement of the minimizer bucket (bucket_of / round_minhash, bns_device.hpp)."""
import numpy as np
import pytest

import synth
from classify_forms import kmer_buckets

pytestmark = pytest.mark.gpu


def pair_runs(b):
    """Runs of equal buckets per pair of rounds (positions 128 p .. 128 p + 127 of a chunk-free read), and whether k-mers 63
    and 64 share a bucket."""
    runs = []
    for p0 in range(0, len(b), 128):
        seg = b[p0:p0 + 128]
        runs.append(sum(1 for i, x in enumerate(seg) if x is not None and (i == 0 or seg[i - 1] != x)))
    straddle = len(b) > 64 and b[63] is not None and b[63] == b[64]
    return runs, straddle


def check(ctx, oracle, w, reads, paired=False):
    bases, offsets = synth.concat(reads)
    exp = oracle.classify_batch(w.table, w.tax, w.k, bases, offsets, paired=paired, canon=True)
    got = ctx.classify(bases, offsets, paired=paired, want_hits=True)
    for key in ("taxon", "missing", "ambig", "n_hits"):
        assert np.array_equal(got[key], exp[key]), key
    inc = 2 if paired else 1
    for u in range(len(reads) // inc):
        s2 = reads[u * inc + 1].tobytes() if paired else None
        _, _, _, hits = oracle.classify_seq(w.table, w.tax, w.k, reads[u * inc].tobytes(), s2, canon=True)
        assert np.array_equal(got["hits"][u], hits), u
    import bonsai_amd
    words, bw, bm = bonsai_amd.pack_reads(bases, offsets, threads=2)
    gp = ctx.classify_packed(words, bw, bm, offsets, paired=paired, want_hits=True)
    for key in ("taxon", "missing", "ambig", "n_hits"):
        assert np.array_equal(gp[key], got[key]), "packed " + key
    assert all(np.array_equal(a, b) for a, b in zip(gp["hits"], got["hits"])), "packed hits"
    return got


def load(ctx, w, n_mb=0):
    ctx.set_encoder(w.k, None, canonicalize=True)
    ctx.set_table_buckets(n_mb)
    ctx.set_minimizer_identity(32)
    try:
        ctx.load_table(w.n_buckets, w.flags, w.keys, w.vals, layout=2)
    finally:
        ctx.set_table_buckets(0)
        ctx.set_minimizer_identity(0)
    ctx.load_taxonomy(w.parent)
    g = ctx.table_geometry()
    assert g["identity_bits"] == 32                                     # (the wide identity keeps the one-round kernel)
    return g


_WORLDS = {}


def world(oracle, k):
    if k not in _WORLDS:
        _WORLDS[k] = synth.make_world(oracle, seed=40 + k, k=k, genome_len=6000)
    return _WORLDS[k]


NK = [1, 63, 64, 65, 120, 127, 128, 129, 191, 192, 193]


def shaped_reads(w, rng, n_per):
    """Reads from the genomes with the k-mer counts above, reads past one and two 2048-base chunks, and N bases on either
    side of the round boundary (k-mers 63 / 64)."""
    g = np.concatenate(list(w.genomes.values()))
    reads = []
    for nk in NK * n_per + [2100 - w.k + 1, 4200 - w.k + 1, 2048 - w.k + 1 + 64]:
        L = nk + w.k - 1
        st = int(rng.integers(0, g.size - L))
        r = synth.mutate(rng, g[st:st + L], 0.005, 0.0)
        reads.append(r if rng.random() < 0.5 else synth.revcomp(r))
    for pos in (62, 63, 64, 65, 63 + w.k - 1, 64 + w.k - 1):
        st = int(rng.integers(0, g.size - 200))
        r = g[st:st + 120 + w.k - 1].copy()
        r[pos] = ord("N")
        reads.append(r)
    return reads


@pytest.mark.parametrize("k", [31, 21, 25, 27, 32])
@pytest.mark.parametrize("paired", [False, True])
def test_round_pairs_shapes(gpu_ctx, oracle, k, paired):
    w = world(oracle, k)
    geo = load(gpu_ctx, w)
    rng = np.random.default_rng(7 * k + paired)
    reads = shaped_reads(w, rng, 4)
    if paired and len(reads) % 2:
        reads.append(reads[0])
    got = check(gpu_ctx, oracle, w, reads, paired)
    assert (got["taxon"] != 0).mean() > 0.5
    # branches: an odd last round (a one-round probe), a chunk of 31 rounds, the straddling group ranked once, a pair with
    # more runs than the stage holds (a second pass)
    nks = [r.size - k + 1 for r in reads]
    assert any(nk > 0 and ((nk + 63) // 64) % 2 == 1 for nk in nks)
    assert any(nk > 2048 - k + 1 for nk in nks)
    runs, straddles = [], []
    for r in reads:
        if r.size - k + 1 > 2048 - k + 1:
            continue
        rr, s = pair_runs(kmer_buckets(r, k, geo["m"], geo["buckets"]))
        runs += rr
        straddles.append(s)
    assert any(straddles)
    assert max(runs) > 16


def test_round_pairs_dense_table_second_round(gpu_ctx, oracle):
    """A crowded table (keys down their chains, buckets whose keys went to the overflow table), probed by reads whose first
    round is random sequence and whose second round comes from the genomes: the chain walks and overflow-table lookups are
    half B's.  Arrival-order fill and the per-lane overflow walk: the kernel form that runs rounds in pairs."""
    w = world(oracle, 31)
    n_keys = int(w.table.header()[1])
    gpu_ctx.debug_set(0x10 | 0x2000 | 0x100)                 # plain fill, never the cooperative lookup, forced overflow buckets
    try:
        geo = load(gpu_ctx, w, n_mb=max(16, n_keys * 10 // 85))
        assert geo["spilled_keys"] > 0 and gpu_ctx.table_stats()["n_overflow_keys"] > 0
        rng = np.random.default_rng(99)
        g = np.concatenate(list(w.genomes.values()))
        reads = []
        for i in range(600):
            nk = int(rng.integers(65, 129))
            tail = nk - 64 + w.k - 1
            st0 = int(rng.integers(0, g.size - tail))
            reads.append(np.concatenate([synth.rand_seq(rng, 64), g[st0:st0 + tail]]))
        got = check(gpu_ctx, oracle, w, reads)
        assert (got["n_hits"] > 0).mean() > 0.9
        # every found k-mer sits in round B: the first 64 k-mers are random (k-mers 34..63 straddle into the genome part)
        check(gpu_ctx, oracle, w, reads, paired=True)
    finally:
        gpu_ctx.debug_set(0)


def test_round_pairs_many_taxa(gpu_ctx, oracle):
    """Units with more than 64 distinct taxa (the counter past its registers) and with exactly tied scores, where the
    insertion order of the vote -- round A's taxa before round B's -- feeds the tie fold."""
    k = 31
    n_leaf = 90
    pairs = [(1, 1), (2, 1), (3, 1)] + [(100 + i, 2 + (i % 2)) for i in range(n_leaf)]
    tax = oracle.Taxonomy(pairs=pairs)
    rng = np.random.default_rng(5)
    table = oracle.Table()
    segs = []
    for i in range(n_leaf):
        s = synth.rand_seq(rng, 40)
        segs.append(s)
        oracle.lca_map_add(table, tax, k, s.tobytes(), 100 + i)
    w = synth.World()
    w.k, w.gaps, w.canon, w.tax, w.table, w.parent = k, None, True, tax, table, tax.parent
    w.flags, w.keys, w.vals = table.arrays()
    w.n_buckets = table.n_buckets
    load(gpu_ctx, w)
    reads = []
    for rep in range(40):
        order = rng.permutation(n_leaf)[: int(rng.integers(3, n_leaf + 1))]
        reads.append(np.concatenate([segs[i] for i in order]))
    for rep in range(40):                                   # two taxa, each once per round: a tie whose fold order is A, B
        a, b = rng.choice(n_leaf, 2, replace=False)
        reads.append(np.concatenate([segs[a], synth.rand_seq(rng, 40), segs[b]]))
    got = check(gpu_ctx, oracle, w, reads)
    assert (got["n_hits"] > 0).all()
    d = [len(set(h.tolist())) for h in got["hits"]]
    assert max(d) > 64


def test_round_by_round_tie_order(gpu_ctx, oracle):
    """A form that votes round by round -- k = 29 on the clustered table: the generic kernel -- on units with two sibling taxa
    of exactly equal counts, the taxon seen first in round 0 and the other in round 1 (reads of 65 and 129 k-mers; in a read
    of 64 k-mers, one round, the first is at the lower lanes).  The vote's insertion order is the hit stream's and feeds the
    tie fold; taxon, missing, ambig, n_hits and the hit stream are the oracle's."""
    from classify_forms import expected_form
    k = 29
    ta, tb = 100, 101
    tax = oracle.Taxonomy(pairs=[(1, 1), (2, 1), (ta, 2), (tb, 2)])
    rng = np.random.default_rng(29)
    table = oracle.Table()
    seg_a, seg_b = synth.rand_seq(rng, 60), synth.rand_seq(rng, 60)
    oracle.lca_map_add(table, tax, k, seg_a.tobytes(), ta)
    oracle.lca_map_add(table, tax, k, seg_b.tobytes(), tb)
    w = synth.World()
    w.k, w.gaps, w.canon, w.tax, w.table, w.parent = k, None, True, tax, table, tax.parent
    w.flags, w.keys, w.vals = table.arrays()
    w.n_buckets = table.n_buckets
    geo = load(gpu_ctx, w)
    assert expected_form(k, True, None, 2, geo["m"], geo["identity_bits"], False, False, False)[2] == 0     # no fixed-k form

    def unit(nk, c, pa, pb):
        """nk k-mers: c of taxon a from k-mer pa on, c of taxon b from k-mer pb on, random sequence around them (the base on
        either side of a piece is not the one its segment goes on with: the piece's c k-mers are all the read has of it)"""
        n = c + k - 1
        r = synth.rand_seq(rng, nk + k - 1)
        oa, ob = int(rng.integers(0, 60 - n + 1)), int(rng.integers(0, 60 - n + 1))
        r[pa:pa + n] = seg_a[oa:oa + n]
        r[pb:pb + n] = seg_b[ob:ob + n]
        avoid = {}
        for pos, seg, o in ((pa, seg_a, oa), (pb, seg_b, ob)):
            if pos > 0 and o > 0:
                avoid.setdefault(pos - 1, set()).add(int(seg[o - 1]))
            if pos + n < r.size and o + n < seg.size:
                avoid.setdefault(pos + n, set()).add(int(seg[o + n]))
        for f, bad in avoid.items():
            r[f] = next(x for x in b"ACGT" if x not in bad)
        return r

    reads, where = [], []
    for rep in range(8):
        c = 1 + rep % 3                                         # 64 k-mers, one round: a at the lower lanes
        pa = int(rng.integers(0, 64 - 2 * c - k + 1))
        pb = int(rng.integers(pa + c + k, 64 - c + 1))
        reads.append(unit(64, c, pa, pb)); where.append((c, pa, pb))
        pa = int(rng.integers(0, 64 - k))                       # 65 k-mers: round 1 is k-mer 64 alone
        reads.append(unit(65, 1, pa, 64)); where.append((1, pa, 64))
        c = 1 + rep                                             # 129 k-mers: b in round 1, from k-mer 64 + rep on
        pa = int(rng.integers(0, 64 - c - k + 1))
        reads.append(unit(129, c, pa, 64 + rep)); where.append((c, pa, 64 + rep))
    for r, (c, pa, pb) in zip(reads, where):
        nk = r.size - k + 1
        b = kmer_buckets(r, k, geo["m"], geo["buckets"])
        assert len(b) == nk and all(x is not None for x in b)
        assert pa + c <= 64 and pa + c + k <= pb and pb + c <= nk and (nk == 64 or pb >= 64)     # a in round 0, b behind it
        _, _, _, hits = oracle.classify_seq(table, tax, k, r.tobytes(), None, canon=True)
        assert list(hits) == [ta] * c + [tb] * c                # the tie, and its order
    got = check(gpu_ctx, oracle, w, reads)
    assert (got["taxon"] == 2).all() and (got["n_hits"] == [2 * c for c, _, _ in where]).all()
