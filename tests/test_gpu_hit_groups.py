"""The minimum number of hit groups on the device (bns_set_min_hit_groups: hit_groups_kernel behind every classify launch) against
tests/hit_groups_ref.py: G = the distinct found keys of a unit from the oracle's encoder and table, the taxon the oracle's (or
confidence_ref's walk of it) zeroed where G < N, everything else as the oracle says at every N."""
from fractions import Fraction

import numpy as np
import pytest

import bonsai_amd
import confidence_ref as CR
import dust_world as DW
import hit_groups_ref as HG
import minq_lib
import synth
from bonsai_amd import _lib

pytestmark = pytest.mark.gpu

NS = [0, 1, 2, 3, 5, 8, 64]
LAYOUTS = [_lib.LAYOUT_MINBUCKET, _lib.LAYOUT_BUCKET, _lib.LAYOUT_KHASH]
SPACED_GAPS = [1] * 15 + [0] * 15
ERR_ARG, ERR_STATE = -1, -4


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    c = gpu_ctx
    c.windows_end()
    c.set_min_hit_groups(0); c.set_confidence(0); c.set_dust(0); c.set_min_base_quality(0)
    c.debug_set(0); c.set_minimizer_span(0); c.set_minimizer_identity(0)


def load(c, w, layout=_lib.LAYOUT_MINBUCKET, spaced_intended=True):
    c.set_encoder(w.k, w.gaps, canonicalize=w.canon, spaced_intended=spaced_intended)
    c.load_table(w.n_buckets, w.flags, w.keys, w.vals, layout=layout)
    c.load_taxonomy(w.parent)


def fastq(reads, quals=None):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bytes(r.tobytes()), quals[i] if quals else b"I" * r.size) for i, r in enumerate(reads))


def text_of(reads, paired):
    return [fastq(reads[0::2]), fastq(reads[1::2])] if paired else fastq(reads)


def entry_points(c, reads, paired, text=False, hits=True):
    """(name, result) of the batch through classify / classify_packed, with and without the caller's hit buffer, and classify_text"""
    bases, offsets = synth.concat(reads)
    words, bw, bm = bonsai_amd.pack_reads(bases, offsets)
    for wh in ((True, False) if hits else (False,)):
        yield "classify hits=%d" % wh, c.classify(bases, offsets, paired=paired, want_hits=wh)
        yield "classify_packed hits=%d" % wh, c.classify_packed(words, bw, bm, offsets, paired=paired, want_hits=wh)
    if text:
        got = c.classify_text(text_of(reads, paired), final=True)
        assert got["n_records"] == len(reads)
        yield "classify_text", got


def check_units(got, units, taxon, what):
    """taxon as the model says; missing, ambig, n_hits and the hits as the oracle says"""
    bad = np.flatnonzero(got["taxon"] != taxon)
    assert bad.size == 0, (what, [(int(u), int(got["taxon"][u]), int(taxon[u])) for u in bad[:5]])
    assert got["missing"].tolist() == [u[1] for u in units], what
    assert got["ambig"].tolist() == [u[2] for u in units], what
    assert got["n_hits"].tolist() == [u[3].size for u in units], what
    if "hits" in got:
        assert all(np.array_equal(a, u[3]) for a, u in zip(got["hits"], units)), what


def check_every_n(c, reads, paired, units, g, ns, taxa=None, text=False, hits=True):
    """every N of ns through every entry point -> {N: the taxa}"""
    taxa = np.array([u[0] for u in units], dtype=np.uint32) if taxa is None else taxa
    out = {}
    for n in ns:
        c.set_min_hit_groups(n)
        want = HG.apply(taxa, g, n)
        for name, got in entry_points(c, reads, paired, text=text, hits=hits):
            check_units(got, units, want, (n, paired, name))
        out[n] = want
    return out


# ---- 1. API parity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_api_parity(ctx, oracle, small_world, paired):
    w, reads, units, g, found = HG.parity_case(oracle, small_world, paired)
    load(ctx, w)
    got = check_every_n(ctx, reads, paired, units, g, NS, text=True)
    base = np.array([u[0] for u in units], dtype=np.uint32)
    assert np.array_equal(got[0], base) and np.array_equal(got[1], base)
    changed, kept = np.count_nonzero(got[5] != base), np.count_nonzero(got[5])
    assert changed >= base.size // 10 and kept >= base.size // 10        # (tests/test_hit_groups_ref.py: the same shares on the CPU)


# ---- 2. distinct keys are not hits --------------------------------------------------------------------------------------------------
def test_distinct_is_not_hits(ctx, oracle):
    w, at = HG.repeat_world(oracle)
    genome = w.genomes[1001]
    reads = [genome[at + 100 + off:at + 250 + off].copy() for off in range(HG.PERIOD)]
    reads.append(reads[3].copy())                                        # (an even number: the same reads two by two as well)
    load(ctx, w)
    for paired in (False, True):
        units = HG.oracle_units(oracle, w, reads, paired)
        g, found = HG.groups_of(oracle, w.table, reads, paired, 31)
        G = int(g[0])
        assert (g == G).all() and 1 <= G <= HG.PERIOD and (found >= 120).all() and all(u[0] != 0 for u in units)
        got = check_every_n(ctx, reads, paired, units, g, [0, G, G + 1, 64])
        assert (got[G] != 0).all() and (got[G + 1] == 0).all()


# ---- 3. a key in both mates counts once ---------------------------------------------------------------------------------------------
def test_across_mates(ctx, oracle, small_world):
    # mate 2 = the reverse complement of mate 1: under a canonical encoder the same keys again
    w = small_world
    rng = np.random.default_rng(5)
    singles = [w.genomes[leaf][st:st + 60].copy() for leaf, st in zip(synth.LEAVES, rng.integers(0, 5000, size=6))]
    pairs = [x for r in singles for x in (r, synth.revcomp(r))]
    load(ctx, w)
    g1, _ = HG.groups_of(oracle, w.table, singles, False, 31)
    g2, f2 = HG.groups_of(oracle, w.table, pairs, True, 31)
    assert np.array_equal(g1, g2) and (f2 == 2 * g1).all() and (g1 == 30).all()
    units = HG.oracle_units(oracle, w, pairs, True)
    got = check_every_n(ctx, pairs, True, units, g2, [0, 30, 31, 60, 61])
    assert (got[30] != 0).all() and (got[31] == 0).all()
    # without the strand rule, over a db that holds both strands: two disjoint sets of keys
    t = HG.two_strand_world(oracle)
    gen = t.genomes[1003]
    singles = [gen[st:st + 60].copy() for st in (10, 700, 1500, 2900)]
    pairs = [x for r in singles for x in (r, synth.revcomp(r))]
    load(ctx, t)
    kw = {"canon": False}
    g1, _ = HG.groups_of(oracle, t.table, singles, False, 31, **kw)
    g2, _ = HG.groups_of(oracle, t.table, pairs, True, 31, **kw)
    assert (g1 == 30).all() and (g2 == 60).all()
    got = check_every_n(ctx, pairs, True, HG.oracle_units(oracle, t, pairs, True, **kw), g2, [0, 31, 60, 61])
    assert (got[60] != 0).all() and (got[61] == 0).all()
    got = check_every_n(ctx, singles, False, HG.oracle_units(oracle, t, singles, False, **kw), g1, [30, 31])
    assert (got[30] != 0).all() and (got[31] == 0).all()


# ---- 4. long units ------------------------------------------------------------------------------------------------------------------
def test_long_units(ctx, oracle):
    w = HG.long_world(oracle)
    load(ctx, w)
    rng = np.random.default_rng(29)
    plain = synth.simulate_reads(rng, w.genomes, 6, length=10000, sub_rate=0.004, n_rate=0.002, random_frac=0.0)
    made = {n: HG.late_key_reads(oracle, w, n) for n in (2, 33, 64)}
    singles = plain + [r for n in made for r in made[n]]
    # pairs: the late key in mate 2's last chunk; both mates without it
    pairs = plain + [x for n in made for x in (made[n][0], made[n][1], made[n][0], made[n][0])]
    for paired, reads in ((False, singles), (True, pairs)):
        units = HG.oracle_units(oracle, w, reads, paired)
        g, found = HG.groups_of(oracle, w.table, reads, paired, 31)
        assert found.max() > 5000 and found.min() > 150 and all(u[0] != 0 for u in units)
        got = check_every_n(ctx, reads, paired, units, g, [0, 2, 33, 64], hits=False)
        n_plain = len(plain) // (2 if paired else 1)
        for i, n in enumerate(made):
            never, late = (n_plain + 2 * i + 1, n_plain + 2 * i) if paired else (n_plain + 2 * i, n_plain + 2 * i + 1)
            assert g[never] == n - 1 and g[late] == n
            assert got[n][never] == 0 and got[n][late] != 0
        assert (got[64][:n_plain] != 0).all()


# ---- 5. with the confidence threshold -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_with_confidence(ctx, oracle, small_world, paired):
    w, reads, units, g, found = HG.parity_case(oracle, small_world, paired)
    load(ctx, w)
    par = CR.parent_map(w.parent)
    theta, n = Fraction(1, 10), 5                                        # (a thinned db: most of a unit's k-mers are missing, and count in Q)
    base = np.array([u[0] for u in units], dtype=np.uint32)
    walked = np.array([CR.walk(par, theta, t, m, h.tolist()) for t, m, _, h in units], dtype=np.uint32)
    want = HG.apply(walked, g, n)
    # theta walks a unit up and N leaves it alone; theta leaves a unit alone and N zeroes it
    assert np.count_nonzero((walked != base) & (walked != 0) & (want == walked)) >= 1
    assert np.count_nonzero((walked == base) & (base != 0) & (want == 0)) >= 1
    ctx.set_confidence(theta)
    got = check_every_n(ctx, reads, paired, units, g, [0, 1, n, 8], taxa=walked, text=True)
    assert np.array_equal(got[0], walked) and np.array_equal(got[n], want)


# ---- 6. the forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS, ids=["minbucket", "bucket", "khash"])
def test_layouts(ctx, oracle, small_world, layout):
    w, reads, units, g, found = HG.parity_case(oracle, small_world, False)
    load(ctx, w, layout)
    check_every_n(ctx, reads, False, units, g, NS, hits=False)


@pytest.mark.parametrize("layout", LAYOUTS, ids=["minbucket", "bucket", "khash"])
def test_spaced_seed(ctx, oracle, layout):
    w = synth.make_world(oracle, seed=14, k=31, genome_len=3000, gaps=SPACED_GAPS)
    reads = synth.simulate_reads(np.random.default_rng(8), w.genomes, 300, var_len=True, sub_rate=0.02)
    kw = {"gaps": SPACED_GAPS, "spaced_intended": True}
    for paired in (False, True):
        units = HG.oracle_units(oracle, w, reads, paired, **kw)
        g, found = HG.groups_of(oracle, w.table, reads, paired, 31, **kw)
        assert found.tolist() == [u[3].size for u in units]
        load(ctx, w, layout, spaced_intended=True)
        got = check_every_n(ctx, reads, paired, units, g, [0, 2, 33, 64], hits=False)
        assert 0 < np.count_nonzero(got[64]) < np.count_nonzero(got[33]) < np.count_nonzero(got[0])
    # through the string for_each a spaced seed looks nothing up: G = 0, and every unit is unclassified already
    kw = {"gaps": SPACED_GAPS, "spaced_intended": False}
    units = HG.oracle_units(oracle, w, reads, False, **kw)
    g, found = HG.groups_of(oracle, w.table, reads, False, 31, **kw)
    assert not g.any() and not found.any() and all(u[0] == 0 for u in units)
    load(ctx, w, layout, spaced_intended=False)
    check_every_n(ctx, reads, False, units, g, [0, 2, 64], hits=False)


@pytest.mark.parametrize("span, identity", [(15, 32), (11, 52), (8, 52), (15, 52)])
def test_minimizer_windows_and_identities(ctx, oracle, small_world, span, identity):
    """the clustered table as tests/classify_forms.py reaches its forms: the window asked for, the 32- or the 52-bit identity"""
    w, reads, units, g, found = HG.parity_case(oracle, small_world, False)
    ctx.set_minimizer_span(span)
    ctx.set_minimizer_identity(identity)
    load(ctx, w)
    geo = ctx.table_geometry()
    assert geo["m"] == 31 - span and geo["identity_bits"] == identity
    check_every_n(ctx, reads, False, units, g, [0, 3, 5, 64], hits=False)


# ---- 7. the masks: G is counted on the image classify saw ----------------------------------------------------------------------------
def test_with_dust(ctx, oracle):
    w = DW.make_world(oracle)
    reads = synth.simulate_reads(np.random.default_rng(41), w.genomes, 300, var_len=True, sub_rate=0.02, n_rate=0.002)
    load(ctx, w)
    ctx.set_dust(64, 20)
    masks = ctx.dust_mask(*synth.concat(reads))
    masked = [np.where(m, np.uint8(ord("N")), r).astype(np.uint8) for r, m in zip(reads, masks)]
    units = HG.oracle_units(oracle, w, masked, False)
    g, found = HG.groups_of(oracle, w.table, masked, False, 31)
    g_plain, _ = HG.groups_of(oracle, w.table, reads, False, 31)
    assert found.tolist() == [u[3].size for u in units] and np.count_nonzero(g < g_plain) >= 30
    got = check_every_n(ctx, reads, False, units, g, [0, 2, 33, 64], text=True)
    plain = HG.apply(np.array([u[0] for u in HG.oracle_units(oracle, w, reads, False)], dtype=np.uint32), g_plain, 33)
    assert np.count_nonzero((got[33] == 0) & (plain != 0)) >= 1          # (a unit that only the masked image leaves below N)


def test_with_min_base_quality(ctx, oracle, small_world):
    w = small_world
    rng = np.random.default_rng(21)
    reads = synth.simulate_reads(rng, w.genomes, 300, var_len=True, sub_rate=0.01)
    quals = [(33 + rng.choice([5, 30], p=[0.03, 0.97], size=r.size)).astype(np.uint8).tobytes() for r in reads]
    masked = [np.frombuffer(minq_lib.mask(r.tobytes(), q, 20), dtype=np.uint8) for r, q in zip(reads, quals)]
    units = HG.oracle_units(oracle, w, masked, False)
    g, found = HG.groups_of(oracle, w.table, masked, False, 31)
    g_plain, _ = HG.groups_of(oracle, w.table, reads, False, 31)
    taxa = np.array([u[0] for u in units], dtype=np.uint32)
    assert np.count_nonzero(g < g_plain) >= 100
    load(ctx, w)
    ctx.set_min_base_quality(20)
    doc = fastq(reads, quals)
    for n in (0, 2, 33, 64):
        ctx.set_min_hit_groups(n)
        got = ctx.classify_text(doc, final=True)
        assert got["n_records"] == len(reads)
        check_units(got, units, HG.apply(taxa, g, n), n)
    assert 0 < np.count_nonzero(HG.apply(taxa, g, 33)) < np.count_nonzero(taxa)
    assert np.count_nonzero(HG.apply(taxa, g, 33) != HG.apply(taxa, g_plain, 33)) >= 1


# ---- 8. state and arguments ---------------------------------------------------------------------------------------------------------
def test_state_and_arguments(ctx, oracle, small_world):
    w, reads, units, g, found = HG.parity_case(oracle, small_world, False)
    c, L = ctx, _lib.load()
    load(c, w)
    bases, offsets = synth.concat(reads)
    off = c.classify(bases, offsets, want_hits=True)
    assert L.bns_set_min_hit_groups(None, 3) == ERR_ARG
    assert L.bns_set_min_hit_groups(c.h, 65) == ERR_ARG and L.bns_set_min_hit_groups(c.h, 0xFFFFFFFF) == ERR_ARG
    with pytest.raises(bonsai_amd.BonsaiAmdError):
        c.set_min_hit_groups(65)
    assert np.array_equal(c.classify(bases, offsets)["taxon"], off["taxon"])           # (a refused value sets nothing)
    assert L.bns_set_min_hit_groups(c.h, 64) == 0 and L.bns_set_min_hit_groups(c.h, 0) == 0
    # a window session: the setting is refused while one is open, and none opens while the setting is on
    c.windows_begin(100)
    assert L.bns_set_min_hit_groups(c.h, 3) == ERR_STATE and L.bns_set_min_hit_groups(c.h, 0) == ERR_STATE
    c.windows_end()
    c.set_min_hit_groups(3)
    assert L.bns_windows_begin(c.h, 100, 1 << 10) == ERR_STATE and L.bns_windows_begin_conf(c.h, 100, 1 << 10, 1, 2) == ERR_STATE
    c.set_min_hit_groups(1)
    assert L.bns_windows_begin(c.h, 100, 1 << 10) == ERR_STATE
    # a build session
    c.set_min_hit_groups(0)
    c.build_begin()
    try:
        assert L.bns_set_min_hit_groups(c.h, 3) == ERR_STATE
    finally:
        c.build_end()
    # table and taxonomy reloads keep it; back to 0 it is as if it had never been on
    c.set_min_hit_groups(5)
    load(c, w)
    on = c.classify(bases, offsets, want_hits=True)
    assert np.array_equal(on["taxon"], HG.apply(off["taxon"], g, 5)) and not np.array_equal(on["taxon"], off["taxon"])
    c.set_min_hit_groups(0)
    for wh in (True, False):
        DW.same_units(c.classify(bases, offsets, want_hits=wh), off)


def test_tally_counts_the_new_taxa_and_the_sketches_stay(ctx, oracle, small_world):
    """-R sees the filter, -u does not: the tally holds the taxa N leaves, the sketches go by each k-mer's own taxon"""
    import sketch_model as SM
    import taxonomy_ref as tr
    w, reads, units, g, found = HG.parity_case(oracle, small_world, False)
    c = ctx
    load(c, w)
    bases, offsets = synth.concat(reads)
    want_sketch = SM.sketches(oracle, w.table, w.parent, reads, 31)
    taxa = HG.apply(np.array([u[0] for u in units], dtype=np.uint32), g, 5)
    dep = tr.depths(w.parent)
    want = np.bincount(tr.bins(w.parent, taxa, dep >= 0), minlength=w.parent.size + 1).astype(np.uint64)
    c.tally_enable(True)
    c.sketch_enable(64)
    try:
        c.set_min_hit_groups(5)
        for call in (lambda: c.classify(bases, offsets), lambda: c.classify_packed(*bonsai_amd.pack_reads(bases, offsets), offsets),
                     lambda: c.classify_text(fastq(reads), final=True)):
            assert np.array_equal(call()["taxon"], taxa)
            direct, _ = c.tally(reset=True)
            assert np.array_equal(direct, want)
            bins, regs, dropped = c.sketch(reset=True)
            assert bins.tolist() == want_sketch[0].tolist() and np.array_equal(regs, want_sketch[1]) and dropped == 0
    finally:
        c.tally_enable(False)
        c.sketch_enable(0)
