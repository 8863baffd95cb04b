"""classify_kernel takes the rounds of a read two at a time as DOUBLE rounds (k <= 31): lane l holds the adjacent k-mers 2 l and
2 l + 1 of 128, cut from one 64-bit window and one reverse complement, their minimizer windows reduced in one pass, ranked by
probe_minbucket2 in position order.  A double round is taken while more than 64 k-mers of a chunk remain; what is left goes
through the one-round probe.  k = 32 keeps rounds 2 p and 2 p + 1 in lanes l and l (two 32-mers are 33 bases).

These cases pin taxon, missing, ambig, n_hits and the ordered hit stream to the oracle, and the packed entry point to the ASCII
one, where that layout has edges: k-mer counts at every seam of single round / double round / chunk under every start
alignment, window and compile-time k; one N that splits a lane's two k-mers; a tie of two sibling taxa whose insertion order
follows the k-mer order through both halves of a lane; more than 64 run leaders in one double round (ranks beyond the bucket
list); units with 65 and more distinct taxa and units for the overflow kernel beside ordinary ones.  Every case but the host arithmetic of
rounds_of() is marked gpu.  Each case asserts from the
host model (classify_forms.kmer_buckets / mmer_hashes, through test_gpu_wide_stage's whole-sequence form) that its data reaches
its branch."""
import numpy as np
import pytest

import classify_forms as F
import synth
import test_gpu_wide_stage as W

_WORLDS = {}


def world(oracle, k):
    if k not in _WORLDS:
        _WORLDS[k] = synth.make_world(oracle, seed=610 + k, k=k, genome_len=6000)
    return _WORLDS[k]


def rounds_of(nk, k):
    """[(first k-mer, k-mers, 'double' | 'single')] of a read of nk k-mers: chunks of 2048 bases, a double round while more than
    64 k-mers of the chunk remain"""
    per_chunk = (2048 - (k - 1)) // 64 * 64
    out = []
    for j0 in range(0, max(nk, 0), per_chunk):
        cn = min(nk - j0, per_chunk)
        r0 = 0
        while r0 < cn:
            if r0 + 64 < cn:
                out.append((j0 + r0, min(128, cn - r0), "double"))
                r0 += 128
            else:
                out.append((j0 + r0, cn - r0, "single"))
                r0 += 64
    return out


def test_rounds_of_is_the_probe_schedule():
    for k in (21, 31):
        for nk in (1, 64, 65, 128, 129, 192, 193, 257, 1984, 1985, 2050, 4100):
            assert [(a, n) for a, n, kind in rounds_of(nk, k) if kind == "double"] == W.probes(nk, k)
            assert sum(n for _, n, _ in rounds_of(nk, k)) == nk


def aligned(rng, g, wanted):
    """the reads of `wanted` = [(read, start alignment)], each behind a filler read cut so that the read starts at a base
    offset of that alignment modulo 4 in the batch"""
    reads, off = [], 0
    for r, a in wanted:
        n = 36 + (a - off - 36) % 4
        at = int(rng.integers(0, g.size - n))
        reads += [g[at:at + n].copy(), r]
        off += n
        assert off % 4 == a
        off += r.size
    return reads


SEAM_COUNTS = (1, 2, 63, 64, 65, 66, 67, 127, 128, 129, 130, 191, 192, 193, 194, 255, 256, 257)
CHUNK_COUNTS = (1983, 1984, 1985, 2047, 2048, 2049, 2050)


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("k,span", [(31, 15), (31, 11), (31, 8), (21, 15), (25, 15), (27, 15), (32, 15)])
def test_kmer_counts_at_every_seam(gpu_ctx, oracle, k, span, paired):
    w = world(oracle, k)
    try:
        W.load(gpu_ctx, w, span)
        rng = np.random.default_rng(100 * k + span)
        g = np.concatenate(list(w.genomes.values()))
        wanted = []
        for i, nk in enumerate(SEAM_COUNTS + CHUNK_COUNTS):
            for a in range(4):
                L = nk + k - 1
                at = int(rng.integers(0, g.size - L))
                r = synth.mutate(rng, g[at:at + L], 0.004, 0.0)
                wanted.append((r if (i + a) % 2 else synth.revcomp(r), a))
        half = len(wanted) // 2
        reads = aligned(rng, g, wanted[:half])
        if paired:                                           # the second half's reads are first mates, the first half's second mates
            reads.append(g[:40].copy())
        off = sum(r.size for r in reads)
        reads += aligned(rng, g, [(r, (a - off) % 4) for r, a in wanted[half:]])
        if len(reads) % 2:
            reads.append(g[100:150].copy())
        if paired:
            where = {id(r): i % 2 for i, r in enumerate(reads)}
            assert {where[id(r)] for r, _ in wanted} == {0, 1}
        got, _, _ = W.check(gpu_ctx, oracle, w, reads, span, paired)
        assert (got["taxon"] != 0).mean() > 0.5
        # branches: a single round alone, one double round, an odd count in a double round (its last lane holds half A only), a
        # double and a single round, two double rounds, a chunk of 15 double rounds and a single one, a second chunk of every kind
        kinds = {}
        for r, _ in wanted:
            rs = rounds_of(r.size - k + 1, k)
            kinds.setdefault(tuple(x[2] for x in rs[:3]) if len(rs) <= 3 else ("chunk", len(rs), rs[-1][2], rs[-1][1]), True)
            if any(kind == "double" and n % 2 for _, n, kind in rs):
                kinds["odd double"] = True
        for want in (("single",), ("double",), ("double", "single"), ("double", "double"), ("double", "double", "single"), "odd double"):
            assert want in kinds, (want, sorted(map(str, kinds)))
        per_chunk = (2048 - (k - 1)) // 64 * 64
        assert per_chunk // 64 % 2 == 1                      # (31 rounds a chunk: its last is a single round)
        assert ("chunk", 16, "single", 63) in kinds and ("chunk", 16, "single", 64) in kinds and ("chunk", 17, "single", 1) in kinds
        assert ("chunk", 17, "double", 65) in kinds and ("chunk", 17, "double", 66) in kinds
    finally:
        gpu_ctx.debug_set(0)


@pytest.mark.gpu
@pytest.mark.parametrize("k,span", [(31, 15), (31, 8), (21, 11)])
def test_one_n_splits_a_lane(gpu_ctx, oracle, k, span):
    """An N at base 2 l + k ends k-mer 2 l + 1's window and leaves k-mer 2 l whole; an N at base 2 l is in k-mer 2 l and not in
    2 l + 1: the two validity tests of one N-field window.  Then an N in the first and the last base, and on either side of the
    seam between a double round and the single round behind it."""
    w = world(oracle, k)
    try:
        geo = W.load(gpu_ctx, w, span)
        m, n_mb = geo["m"], geo["buckets"]
        rng = np.random.default_rng(7 * k + span)
        g = np.concatenate(list(w.genomes.values()))

        def cut(nk, n_at):
            L = nk + k - 1
            at = int(rng.integers(0, g.size - L))
            r = g[at:at + L].copy()
            r[n_at] = ord("N")
            return r
        reads, expect = [], []                               # expect: (read index, k-mer, valid?)
        for l in (0, 1, 31, 32, 59, 63):
            reads.append(cut(128, 2 * l + k))
            expect += [(len(reads) - 1, 2 * l, True), (len(reads) - 1, 2 * l + 1, False)]
            reads.append(cut(128 + 30, 2 * l))
            expect += [(len(reads) - 1, 2 * l, False), (len(reads) - 1, 2 * l + 1, True)]
        reads += [cut(128, 0), cut(128, -1), cut(120, 0), cut(120, -1)]
        for n_at in (127, 128, 129, 127 + k - 1, 128 + k - 1, 128 + k):    # k-mers 127 | 128: the double round's last and the single round's first
            reads.append(cut(160, n_at))
            assert rounds_of(160, k)[-1] == (128, 32, "single")
        for i, j, valid in expect:
            b = W.buckets_of(reads[i], k, m, n_mb)
            assert (b[j] >= 0) == valid and (b[j ^ 1] >= 0) != valid, (i, j)
            assert rounds_of(b.size, k)[0][2] == "double"
        got, _, _ = W.check(gpu_ctx, oracle, w, reads, span)
        assert (got["n_hits"] > 0).all() and (got["ambig"] > 0).all()
        if len(reads) % 2 == 0:
            W.check(gpu_ctx, oracle, w, reads, span, paired=True)
    finally:
        gpu_ctx.debug_set(0)


@pytest.mark.gpu
def test_insertion_order_follows_kmer_order(gpu_ctx, oracle):
    """An every-k-mer db of two sibling taxa: k-mers 0 .. s - 1 of a read are one taxon's keys, k-mers s .. 2 s - 1 the other's,
    the rest of the read is in no db.  Both have s hits: the vote is a tie, folded in insertion order, and the hit stream is the
    k-mer order.  s = 1 .. 8 and 61 .. 68, both orders of the two taxa: the second taxon's first hit is a lane's half A (s even)
    and a lane's half B (s odd).  With lead = 0 the first taxon's first hit is k-mer 0, lane 0's half A, which every order of the halves
    takes first; so each case runs again behind lead = 1 and 3 bases of no db: the first taxon then starts on a half B (position 1 or 3)
    and the second on position lead + s -- a half A for odd s -- and a vote that took half A's hits before half B's would insert the
    second taxon first."""
    k, span = 31, 15
    tax = oracle.Taxonomy(pairs=[(1, 1), (2, 1), (3, 1), (100, 2), (101, 2), (102, 3)])
    rng = np.random.default_rng(12)
    table = oracle.Table()
    reads, plan = [], []
    for lead in (0, 1, 3):
        for s in list(range(1, 9)) + list(range(61, 69)):
            for first, second in ((100, 101), (101, 100)):
                core = synth.rand_seq(rng, 2 * s + k - 1)
                oracle.lca_map_add(table, tax, k, core[:s + k - 1].tobytes(), first)
                oracle.lca_map_add(table, tax, k, core[s:].tobytes(), second)
                nk = max(2 * s + 40, 120)
                reads.append(np.concatenate([synth.rand_seq(rng, lead), core, synth.rand_seq(rng, nk - 2 * s)]))
                plan.append((s, first, second, lead))
    w = synth.World()
    w.k, w.gaps, w.canon, w.tax, w.table, w.parent = k, None, True, tax, table, tax.parent
    w.flags, w.keys, w.vals = table.arrays()
    w.n_buckets = table.n_buckets
    try:
        W.load(gpu_ctx, w, span)
        got, exp_hits, _ = W.check(gpu_ctx, oracle, w, reads, span)
        for u, (s, first, second, lead) in enumerate(plan):
            assert rounds_of(reads[u].size - k + 1, k)[0][2] == "double"
            assert exp_hits[u].tolist() == [first] * s + [second] * s, u
            assert got["n_hits"][u] == 2 * s
        # the second taxon's first hit on a half A and on a half B; the first taxon's on a half B with the second's on a LATER lane's half A
        assert {(lead + s) % 2 for s, _, _, lead in plan} == {0, 1}
        assert any(lead % 2 == 1 and (lead + s) % 2 == 0 for s, _, _, lead in plan)
        W.check(gpu_ctx, oracle, w, reads, span, paired=True)
    finally:
        gpu_ctx.debug_set(0)


def many_runs_world(oracle, k, m, seed, n_plants):
    """synth.make_world with sequences of 128 k-mers that hold 70 window minima and more (plain sequence under a window of 3
    m-mers has 64) planted in the genomes: their k-mers are keys"""
    rng = np.random.default_rng(seed)
    w = synth.World()
    w.k, w.gaps, w.canon = k, None, True
    w.tax = oracle.Taxonomy(pairs=synth.TAX_PAIRS)
    w.parent = w.tax.parent
    w.genomes = synth.make_genomes(rng, 3000)
    w.plants = [W.climb(rng, 128 + k - 1, k, m, 72 / 128.0, tries=400) for _ in range(n_plants)]
    leaves = list(w.genomes)
    for i, s in enumerate(w.plants):
        g = w.genomes[leaves[i % len(leaves)]].copy()
        at = 200 + (i // len(leaves)) * 400
        g[at:at + s.size] = s
        w.genomes[leaves[i % len(leaves)]] = g
    w.table = oracle.Table()
    for leaf, g in w.genomes.items():
        oracle.lca_map_add(w.table, w.tax, k, g.tobytes(), leaf, canon=True)
    w.flags, w.keys, w.vals = w.table.arrays()
    w.n_buckets = w.table.n_buckets
    return w


@pytest.mark.gpu
@pytest.mark.parametrize("paired", [False, True])
def test_more_than_64_leaders_in_a_double_round(gpu_ctx, oracle, paired):
    """k = 21 under a window of 3 m-mers (m = 19): a double round with 65 run leaders and more has ranks beyond the 64 entries of
    the bucket list in BOTH halves (a lane's half A is an even position), and takes five passes of 16 buckets (three of 24)."""
    k, span = 21, 11
    m = F.minimizer_len(k, span)
    assert k - m == 2
    if "runs" not in _WORLDS:
        _WORLDS["runs"] = many_runs_world(oracle, k, m, 33, 8)
    w = _WORLDS["runs"]
    try:
        geo = W.load(gpu_ctx, w, span)
        n_mb = geo["buckets"]
        rng = np.random.default_rng(8)
        g = np.concatenate(list(w.genomes.values()))
        reads = [s.copy() for s in w.plants] + [synth.revcomp(s) for s in w.plants]
        reads += [np.concatenate([s, g[500:560]]) for s in w.plants[:4]]                    # a single round behind it
        reads += [g[at:at + 150].copy() for at in rng.integers(0, g.size - 150, size=8)]
        assert len(reads) % 2 == 0
        got, _, _ = W.check(gpu_ctx, oracle, w, reads, span, paired)
        inc = 2 if paired else 1
        deep = 0
        for u in range(len(reads) // inc):
            mates = reads[u * inc:(u + 1) * inc]
            if got["n_hits"][u] != sum(r.size - k + 1 for r in mates) or any((r == ord("N")).any() for r in mates):
                continue                                     # (every k-mer found: the hits are at the k-mer positions)
            for r in mates:
                for j0, nl, _, rk in W.pair_stats(W.buckets_of(r, k, m, n_mb), k):
                    if nl >= 65 and (rk[0::2] >= 64).any() and (rk[1::2] >= 64).any():
                        deep += 1
        assert deep >= 4, deep
    finally:
        gpu_ctx.debug_set(0)


@pytest.mark.gpu
def test_mixed_batch_many_taxa_and_overflow(gpu_ctx, oracle):
    """Units with 65 and more distinct taxa (the counter past its registers: the 16-bucket stage), units for the overflow kernel
    (more than 128), and ordinary reads between them, in one batch."""
    k, span = 31, 15
    w = F.world(oracle, k, kind="many")
    try:
        W.load(gpu_ctx, w, span)
        rng = np.random.default_rng(3)
        many = F.many_taxa_reads(w)
        plain = [np.concatenate([w.segs[int(i)] for i in rng.choice(F.MANY_LEAVES, 4, replace=False)])[:int(rng.integers(100, 241))]
                 for _ in range(len(many))]
        reads = [x for pair in zip(plain, many) for x in pair]
        got, exp_hits, form = W.check(gpu_ctx, oracle, w, reads, span)
        assert form["overflow_kernel"] == F.expected_overflow_form(None, 2, 32, False) and form["overflow_units"] >= 3
        d = [len(set(h.tolist())) for h in exp_hits]
        assert sum(1 for x in d if 65 <= x <= F.LDS_CAP) >= 3 and sum(1 for x in d if x > F.LDS_CAP) >= 3 and sum(1 for x in d if 0 < x <= 4) >= 10
        W.check(gpu_ctx, oracle, w, reads, span, paired=True)
    finally:
        gpu_ctx.debug_set(0)
