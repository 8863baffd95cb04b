"""The two-round probe (probe_minbucket2) stages 24 buckets in a pass while the unit's counter has at most 64 distinct taxa: the
counter's LDS arrays lie directly behind the 16-bucket stage and are its third KiB until the 65th taxon needs them.  These cases
pin taxon, missing, ambig, n_hits and the ordered hit stream to the oracle (and the packed entry point to the ASCII one) where
that has edges: pairs of rounds with at most 16 run leaders, 17 to 23, exactly 24, 25 to 32 and 33 or more; the group that
straddles k-mers 63 / 64 ranked 15, 16, 23 and 24; units whose vote stands at exactly 64 and at 65 distinct taxa when a pair with
more than 16 runs comes, next to units for the overflow kernel and ordinary ones in one batch; mate pairs; k = 21, 25, 27, 32.

Every case restates the run leaders of each pair of rounds on the host (bucket_of / round_minhash of bns_device.hpp, from the
loaded table's geometry) and asserts that the classes it names are there.  The genomes do not yield the rare classes (a pair of
a 150-bp read has 15.0 +- 1.9 leaders under the window of 16 m-mers), so sequences changed base by base towards many window minima
(climb()) are planted in the genomes before the db is built: their k-mers are keys, and a hit ranked 16 or above is read from the
third KiB."""
import numpy as np
import pytest

import classify_forms as F
import synth

M32 = F.M32


# ---- the host model ----------------------------------------------------------------------------------------------------
def buckets_of(seq, k, m, n_mb):
    """classify_forms.kmer_buckets for a whole sequence at once: int64 array, -1 for a k-mer with a non-ACGT base"""
    h = F.mmer_hashes(seq, m)
    n = len(seq) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    win = np.lib.stride_tricks.sliding_window_view(h, k - m + 1)[:n]
    lo = win.min(axis=1)
    bad = win.max(axis=1) >= F.INVALID
    x = (np.where(bad, 0, lo).astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    r = np.zeros_like(x)
    for i in range(32):
        r |= ((x >> np.uint64(i)) & np.uint64(1)) << np.uint64(31 - i)
    b = ((r * np.uint64(n_mb)) >> np.uint64(32)).astype(np.int64)
    return np.where(bad, -1, b)


def probes(n_kmers, k):
    """(first k-mer, k-mers) of every two-round probe of a read: chunks of 2048 bases, rounds of 64 k-mers taken two at a time, a
    chunk's odd last round left to the one-round probe"""
    per_chunk = (2048 - (k - 1)) // 64 * 64
    out = []
    for j0 in range(0, n_kmers, per_chunk):
        cn = min(n_kmers - j0, per_chunk)
        for r0 in range(0, cn, 128):
            if r0 + 64 < cn:
                out.append((j0 + r0, min(128, cn - r0)))
    return out


def ranks_of(seg):
    """(leaders, rank per position) of one two-round probe's first pass: a leader is a valid position whose left neighbour wants
    another bucket; rank = leaders at or before the position, less one"""
    lead = (seg >= 0) & np.concatenate([[True], seg[1:] != seg[:-1]])
    return int(lead.sum()), np.cumsum(lead) - 1


def pair_stats(b, k):
    """per two-round probe of a read with k-mer buckets b: (first k-mer, leaders, straddle rank or None, ranks)"""
    out = []
    for j0, n in probes(len(b), k):
        seg = b[j0:j0 + n]
        nl, rk = ranks_of(seg)
        st = int(rk[63]) if (seg[63] >= 0 and seg[63] == seg[64]) else None
        out.append((j0, nl, st, rk))
    return out


def leader_class(nl):
    return "le16" if nl <= 16 else "17-23" if nl <= 23 else "24" if nl == 24 else "25-32" if nl <= 32 else "ge33"


# ---- sequences with many window minima ------------------------------------------------------------------------------------
def window_runs(seq, k, m):
    """runs of equal window minima over the k-mers of seq (the run leaders of a table with a bucket per minimizer)"""
    lo = np.lib.stride_tricks.sliding_window_view(F.mmer_hashes(seq, m), k - m + 1).min(axis=1)
    return 1 + int((lo[1:] != lo[:-1]).sum())


def climb(rng, n, k, m, rate, tries=5000):
    """n random bases, then single-base changes that do not lower the number of runs, until there are `rate` runs per k-mer
    (plain sequence has 2 / (window + 1))"""
    seq = synth.rand_seq(rng, n)
    target, cur = int(rate * (n - k + 1)), window_runs(seq, k, m)
    for _ in range(tries):
        if cur >= target:
            break
        i = int(rng.integers(0, n))
        old = seq[i]
        seq[i] = synth.ACGT[int(rng.integers(0, 4))]
        r = window_runs(seq, k, m)
        if r >= cur:
            cur = r
        else:
            seq[i] = old
    return seq


def climb_straddle(rng, k, m, rank, tries=4000):
    """128 k-mers whose k-mers 63 and 64 share a window minimum that is the (rank + 1)-th of the read"""
    n = 128 + k - 1
    seq = synth.rand_seq(rng, n)

    def off(s):
        lo = np.lib.stride_tricks.sliding_window_view(F.mmer_hashes(s, m), k - m + 1).min(axis=1)
        return abs(int((lo[1:64] != lo[:63]).sum()) - rank) + (0.5 if lo[63] != lo[64] else 0.0)
    cur = off(seq)
    for _ in range(tries):
        if cur == 0:
            break
        i = int(rng.integers(0, 64 + k))
        old = seq[i]
        seq[i] = synth.ACGT[int(rng.integers(0, 4))]
        r = off(seq)
        if r <= cur:
            cur = r
        else:
            seq[i] = old
    return seq


RATES = (0.0, 0.19, 0.25, 0.31)
PLANT_LEN = 400


def planted_world(oracle, k, m, seed, straddles=()):
    """synth.make_world with a sequence of PLANT_LEN bases per entry of RATES, and a read per entry of straddles, planted in the
    genomes (w.plants)"""
    rng = np.random.default_rng(seed)
    w = synth.World()
    w.k, w.gaps, w.canon = k, None, True
    w.tax = oracle.Taxonomy(pairs=synth.TAX_PAIRS)
    w.parent = w.tax.parent
    w.genomes = synth.make_genomes(rng, 6000)
    w.plants = []
    leaves = list(w.genomes)
    plants = [climb(rng, PLANT_LEN, k, m, rate) for rate in RATES] + [climb_straddle(rng, k, m, r) for r in straddles]
    for i, s in enumerate(plants):
        g = w.genomes[leaves[i % len(leaves)]].copy()
        at = 300 + (i // len(leaves)) * (PLANT_LEN + 300)
        g[at:at + s.size] = s
        w.genomes[leaves[i % len(leaves)]] = g
        w.plants.append(s)
    w.table = oracle.Table()
    for leaf, g in w.genomes.items():
        oracle.lca_map_add(w.table, w.tax, k, g.tobytes(), leaf, canon=True)
    w.flags, w.keys, w.vals = w.table.arrays()
    w.n_buckets = w.table.n_buckets
    return w


_WORLDS = {}


def world(oracle, k, span):
    if (k, span) not in _WORLDS:
        _WORLDS[(k, span)] = planted_world(oracle, k, F.minimizer_len(k, span), 900 + 10 * k + span,
                                          straddles=(23, 23, 23, 24, 24, 24) if (k, span) == (31, 15) else ())
    return _WORLDS[(k, span)]


def load(ctx, w, span):
    ctx.set_encoder(w.k, None, canonicalize=True)
    ctx.debug_set(F.DBG_OVC_OFF)                               # the per-lane overflow lookup: the forms that probe two rounds at a time
    ctx.set_minimizer_span(span)
    ctx.set_minimizer_identity(32)
    try:
        ctx.load_table(w.n_buckets, w.flags, w.keys, w.vals, layout=2)
    finally:
        ctx.set_minimizer_span(0)
        ctx.set_minimizer_identity(0)
    ctx.load_taxonomy(w.parent)
    geo = ctx.table_geometry()
    assert geo["identity_bits"] == 32 and geo["m"] == F.minimizer_len(w.k, span)
    return geo


def check(ctx, oracle, w, reads, span, paired=False):
    """taxon, missing, ambig, n_hits and the hit stream against the oracle, the packed entry point against the ASCII one, and the
    kernel forms both calls launched"""
    import bonsai_amd
    bases, offsets = synth.concat(reads)
    exp = oracle.classify_batch(w.table, w.tax, w.k, bases, offsets, paired=paired, canon=True)
    got = ctx.classify(bases, offsets, paired=paired, want_hits=True)
    form = ctx.last_classify_form()
    for key in ("taxon", "missing", "ambig", "n_hits"):
        bad = np.flatnonzero(got[key] != exp[key])
        assert bad.size == 0, "%s differs at units %s: got %s, expected %s" % (key, bad[:8], got[key][bad[:8]], exp[key][bad[:8]])
    inc = 2 if paired else 1
    exp_hits = []
    for u in range(len(reads) // inc):
        s2 = reads[u * inc + 1].tobytes() if paired else None
        _, _, _, hits = oracle.classify_seq(w.table, w.tax, w.k, reads[u * inc].tobytes(), s2, canon=True)
        assert np.array_equal(got["hits"][u], hits), u
        exp_hits.append(hits)
    words, bw, bm = bonsai_amd.pack_reads(bases, offsets, threads=2)
    gp = ctx.classify_packed(words, bw, bm, offsets, paired=paired, want_hits=True)
    pform = ctx.last_classify_form()
    for key in ("taxon", "missing", "ambig", "n_hits"):
        assert np.array_equal(gp[key], got[key]), "packed " + key
    assert all(np.array_equal(a, b) for a, b in zip(gp["hits"], got["hits"])), "packed hits"
    m = F.minimizer_len(w.k, span)
    nm = 2 if paired else 1
    assert form["kernel"] == F.expected_form(w.k, True, None, 2, m, 32, False, False, paired) == (0, 2, w.k, nm, w.k - m, 0, 0, 0)
    assert pform["kernel"] == F.expected_form(w.k, True, None, 2, m, 32, False, True, paired)
    return got, exp_hits, form


def candidates(w, rng, lengths, n_natural):
    """reads cut from the planted sequences at every eighth offset, and from the genomes at random places (forward or reverse
    complement, one base in 200 substituted: misses and ambiguous k-mers among the hits)"""
    out = []
    for s in w.plants:
        for L in lengths:
            for at in range(0, s.size - L + 1, 8):
                out.append(s[at:at + L].copy())
    g = np.concatenate(list(w.genomes.values()))
    for i in range(n_natural):
        L = int(lengths[i % len(lengths)])
        at = int(rng.integers(0, g.size - L))
        r = synth.mutate(rng, g[at:at + L], 0.005, 0.002)
        out.append(r if i % 2 else synth.revcomp(r))
    return out


def select(cands, k, m, n_mb, want, per_class):
    """up to per_class reads per class name that want(pair_stats) gives (a read counts for every class it is given)"""
    have = {}
    picked = []
    for r in cands:
        st = pair_stats(buckets_of(r, k, m, n_mb), k)
        names = [c for c in want(st) if have.get(c, 0) < per_class]
        if names:
            for c in names:
                have[c] = have.get(c, 0) + 1
            picked.append(r)
    return picked, have


def classes_of(st):
    out = set()
    for _, nl, straddle, _ in st:
        out.add(leader_class(nl))
        if straddle in (15, 16, 23, 24):
            out.add("straddle%d" % straddle)
    return out


def assert_high_rank_hits(reads, got, k, m, n_mb, names, paired=False):
    """in every class of `names`, some unit whose pair has a hit ranked 16 or above: a unit without a base outside ACGT whose
    k-mers are all found (n_hits, which check() has held against the oracle) has its hits at the k-mer positions of its reads"""
    seen = set()
    inc = 2 if paired else 1
    for u in range(len(reads) // inc):
        mates = reads[u * inc:(u + 1) * inc]
        n = sum(max(0, r.size - k + 1) for r in mates)
        if n <= 0 or got["n_hits"][u] != n:
            continue
        for r in mates:
            for _, nl, _, rk in pair_stats(buckets_of(r, k, m, n_mb), k):
                if rk.max() >= 16:
                    seen.add(leader_class(nl))
    assert seen >= set(names), (seen, names)


# ---- the cases ------------------------------------------------------------------------------------------------------------
def test_buckets_of_is_kmer_buckets():
    rng = np.random.default_rng(3)
    for k, m in ((31, 16), (31, 23), (21, 16), (32, 17)):
        r = synth.rand_seq(rng, 120)
        r[57] = ord("N")
        ref = F.kmer_buckets(r, k, m, 12345)
        assert [(-1 if x is None else x) for x in ref] == buckets_of(r, k, m, 12345).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("span", [15, 8])
def test_wide_stage_leader_classes(gpu_ctx, oracle, span):
    k = 31
    w = world(oracle, k, span)
    try:
        geo = load(gpu_ctx, w, span)
        m, n_mb = geo["m"], geo["buckets"]
        rng = np.random.default_rng(50 + span)
        need = (["le16", "17-23", "24", "25-32"] + ["straddle%d" % r for r in (15, 16, 23, 24)]) if span == 15 else ["ge33"]
        cands = candidates(w, rng, (128 + k - 1, 150, 120 + k - 1, 250), 60)
        reads, have = select(cands, k, m, n_mb, lambda st: classes_of(st) & set(need), 12)
        reads += cands[-60:]
        for c in need:
            assert have.get(c, 0) >= (2 if c.startswith("straddle") else 8), (c, have)
        got, exp_hits, _ = check(gpu_ctx, oracle, w, reads, span)
        assert (got["taxon"] != 0).mean() > 0.5 and got["missing"].any()
        assert_high_rank_hits(reads, got, k, m, n_mb, [c for c in need if c in ("17-23", "24", "25-32", "ge33")])
    finally:
        gpu_ctx.debug_set(0)


@pytest.mark.gpu
@pytest.mark.parametrize("k,paired", [(31, True)] + [(k, p) for k in (21, 25, 27, 32) for p in (False, True)])
def test_wide_stage_forms(gpu_ctx, oracle, k, paired):
    """mate pairs (the ASCII two-mate forms keep the 16-bucket stage, the packed ones take the third load) and the other
    compile-time k, each with its widest window"""
    span = F.distinct_windows(k)[0][0]
    w = world(oracle, k, span)
    try:
        geo = load(gpu_ctx, w, span)
        m, n_mb = geo["m"], geo["buckets"]
        rng = np.random.default_rng(70 + k)
        need = ["le16", "17-23", "24", "25-32"]
        # (shorter second rounds too: under a narrow window 128 k-mers hold 30 runs and more)
        cands = candidates(w, rng, (128 + k - 1, 66 + k - 1, 72 + k - 1, 88 + k - 1, 104 + k - 1, 150), 40)
        reads, have = select(cands, k, m, n_mb, lambda st: classes_of(st) & set(need), 6)
        reads += cands[-40:]
        if len(reads) % 2:
            reads.append(reads[0])
        for c in need:
            assert have.get(c, 0) >= 2, (c, have)
        if paired:                                           # a class on either mate: the first half reversed against the second
            h = len(reads) // 2
            reads = [x for a, b in zip(reads[:h], reads[h:][::-1]) for x in (a, b)]
        got, exp_hits, _ = check(gpu_ctx, oracle, w, reads, span, paired)
        assert (got["taxon"] != 0).mean() > 0.5
        assert_high_rank_hits(reads, got, k, m, n_mb, ["17-23", "24", "25-32"], paired)
    finally:
        gpu_ctx.debug_set(0)


_SEG_KMERS = {}


def pieced_read(w, pieces, k):
    """(bases, taxon per k-mer or -1) of a read put together from pieces of the many-taxa world's segments: a k-mer (or its reverse
    complement) that lies in a segment is that segment's taxon's key -- one across a joint only when the next piece happens to go on as
    the segment does"""
    if not _SEG_KMERS:
        for t, s in enumerate(w.segs):
            for x in (s, synth.revcomp(s)):
                b = x.tobytes()
                for j in range(len(b) - k + 1):
                    _SEG_KMERS[b[j:j + k]] = t
    b = np.concatenate(pieces).tobytes()
    return np.frombuffer(b, dtype=np.uint8), np.array([_SEG_KMERS.get(b[j:j + k], -1) for j in range(len(b) - k + 1)])


def taxa_before_wide_pairs(seq, tax, k, m, n_mb, min_leaders=17):
    """distinct taxa the vote holds in front of every two-round probe with min_leaders run leaders or more"""
    out = []
    for j0, nl, _, _ in pair_stats(buckets_of(seq, k, m, n_mb), k):
        if nl >= min_leaders:
            seen = tax[:j0]
            out.append(len(set(seen[seen >= 0].tolist())))
    return out


@pytest.mark.gpu
def test_wide_stage_counter_boundary(gpu_ctx, oracle):
    """The counter and the stage's third KiB are the same memory.  Units whose vote holds exactly 64 taxa when a pair with more
    than 16 runs comes (24 buckets staged, every entry in a register), units that hold 65 (entry 64 lives where buckets 18 and 22
    would land: 16 staged; it is the taxon with the most k-mers, and it is looked up again after those pairs), units for the
    overflow kernel, and ordinary units with such pairs between them, so that a wavefront goes from one stage to the other within
    a claim."""
    k, span = 31, 15
    w = F.world(oracle, k, kind="many")
    try:
        geo = load(gpu_ctx, w, span)
        m, n_mb = geo["m"], geo["buckets"]
        rng = np.random.default_rng(64)
        segs = w.segs

        def unit(n_taxa, base):
            """n_taxa taxa, ten k-mers each but thirty for the last, then a tail of the first ones again with a pair of 19 runs or more
            (a third load would reach bucket 18), then the last taxon once more"""
            head = [segs[base + i][:40] for i in range(n_taxa - 1)] + [segs[base + n_taxa - 1]]
            for _ in range(400):
                tail = [segs[base + int(i)][:int(rng.integers(45, 61))] for i in rng.choice(n_taxa - 1, 6, replace=False)]
                seq, tax = pieced_read(w, head + tail + [segs[base + n_taxa - 1][:50]], k)
                if n_taxa in taxa_before_wide_pairs(seq, tax, k, m, n_mb, 19):
                    return seq, tax
            raise AssertionError("no tail with a pair of 19 runs")

        def ordinary(min_leaders):
            for _ in range(400):
                seq, tax = pieced_read(w, [segs[int(i)] for i in rng.choice(F.MANY_LEAVES, 3, replace=False)], k)
                if taxa_before_wide_pairs(seq, tax, k, m, n_mb, min_leaders):
                    return seq, tax
            raise AssertionError("no ordinary read with a pair of %d runs" % min_leaders)

        many = F.many_taxa_reads(w)
        units = []
        for g in range(6):
            units += [ordinary(17), unit(65, 70 * g), ordinary(19), unit(64, 70 * g + 3)]
            units += [ordinary(17), (many[2 * g], None), ordinary(17), (many[2 * g + 1], None)]
        units += [(r, None) for r in many[12:]]
        reads = [np.ascontiguousarray(s, dtype=np.uint8) for s, _ in units]
        got, exp_hits, form = check(gpu_ctx, oracle, w, reads, span)
        assert form["overflow_kernel"] == F.expected_overflow_form(None, 2, 32, False) and form["overflow_units"] >= 3
        # the model's taxa are the oracle's; the classes are there; a claim (chunk >= 4 consecutive units) holds both stages
        stage = []                                               # per unit: the set of stages its wide pairs were probed with
        for u, (seq, tax) in enumerate(units):
            if tax is None:
                stage.append(set())
                continue
            assert np.array_equal(exp_hits[u], 1000 + tax[tax >= 0]), u
            d = taxa_before_wide_pairs(seq, tax, k, m, n_mb)
            stage.append({24 if x <= 64 else 16 for x in d})
        before = [x for seq, tax in units if tax is not None for x in taxa_before_wide_pairs(seq, tax, k, m, n_mb, 19)]
        assert before.count(64) >= 6 and before.count(65) >= 6
        assert form["chunk"] >= 4 and len(units) >= 2 * form["chunk"]
        c = form["chunk"]
        assert any(16 in stage[u] and 24 in stage[v] for u in range(len(units)) for v in range(u + 1, (u // c + 1) * c) if v < len(units))
        win = [u for u, (seq, tax) in enumerate(units) if tax is not None and 65 in taxa_before_wide_pairs(seq, tax, k, m, n_mb, 19)]
        for u in win:                                            # the 65th taxon decides the unit: a lost entry 64 changes the result
            assert got["taxon"][u] == exp_hits[u][np.flatnonzero(np.diff(exp_hits[u]) != 0)[63] + 1]
    finally:
        gpu_ctx.debug_set(0)
