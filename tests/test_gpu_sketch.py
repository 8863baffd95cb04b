"""The distinct k-mer sketches on the device (bns_sketch_enable / bns_sketch_read: sketch_seen_kernel, sketch_assign_kernel,
sketch_kernel) against the numpy model of tests/sketch_model.py: keys from the oracle's encoder, values from the oracle's table,
registers compared byte for byte."""
import numpy as np
import pytest

import bonsai_amd
import minq_lib
import sketch_model as SM
import synth
from bonsai_amd import _lib

pytestmark = pytest.mark.gpu

LAYOUTS = [_lib.LAYOUT_KHASH, _lib.LAYOUT_BUCKET, _lib.LAYOUT_MINBUCKET]
BATCH_TINY, MANY_PIECES = 0x40, 0x4000


def load(c, w, layout=_lib.LAYOUT_MINBUCKET, spaced_intended=True, arrays=None, max_taxa=64):
    flags, keys, vals = arrays or (w.flags, w.keys, w.vals)
    c.set_encoder(w.k, w.gaps, canonicalize=w.canon, spaced_intended=spaced_intended)
    c.load_table(keys.size, flags, keys, vals, layout=layout)
    c.load_taxonomy(w.parent)
    c.sketch_enable(max_taxa)


def model(oracle, w, reads, table=None, spaced_intended=True):
    return SM.sketches(oracle, table or w.table, w.parent, reads, w.k, gaps=w.gaps, canon=w.canon, spaced_intended=spaced_intended)


def check(c, want, reset=True, what=""):
    bins, regs, dropped = c.sketch(reset=reset)
    assert bins.dtype == np.uint32 and regs.dtype == np.uint8 and regs.shape == (bins.size, 4096)
    assert bins.tolist() == want[0].tolist(), what
    assert np.array_equal(regs, want[1]), what
    assert dropped == 0, what


def fastq(reads, quals=None):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, bytes(r.tobytes()), quals[i] if quals else b"I" * r.size) for i, r in enumerate(reads))


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.debug_set(0)
    gpu_ctx.sketch_enable(0)


@pytest.fixture(scope="module")
def exact(oracle, small_world):
    reads = synth.simulate_reads(np.random.default_rng(2024), small_world.genomes, 2000)
    want = model(oracle, small_world, reads)
    assert want[0].size >= 8 and (want[1] != 0).sum() > 10000          # leaves and inner nodes, thousands of registers set
    return reads, want


def dense_nmask(words, bad_word, bad_mask):
    m = np.zeros(words.size, dtype=np.uint32)
    m[bad_word.astype(np.int64)] = bad_mask
    return m


def run_device(c, bases, offsets, paired, packed):
    n_reads, total = offsets.size - 1, int(offsets[-1])
    bufs = []

    def up(a):
        a = np.ascontiguousarray(a)
        p = c.dev_alloc(max(a.nbytes, 8) + 8)
        if a.nbytes:
            c.dev_upload(p, a)
        bufs.append(p)
        return p
    try:
        d_off = up(offsets)
        d_tax = c.dev_alloc(4 * n_reads + 8); bufs.append(d_tax)
        if packed:
            words, bw, bm = bonsai_amd.pack_reads(bases, offsets)
            c.classify_packed_device(up(words), up(dense_nmask(words, bw, bm)), d_off, n_reads, total, 0, paired, d_tax)
        else:
            c.classify_device(up(bases), d_off, n_reads, total, 0, paired, d_tax)
        c.sync()
    finally:
        for p in bufs:
            c.dev_free(p)


@pytest.mark.parametrize("paired", [False, True])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_exact_every_layout_and_entry_point(ctx, small_world, exact, layout, paired):
    c, (reads, want) = ctx, exact
    load(c, small_world, layout)
    bases, offsets = synth.concat(reads)
    c.classify(bases, offsets, paired=paired)
    check(c, want, what="classify_batch")
    words, bw, bm = bonsai_amd.pack_reads(bases, offsets)
    assert bw.size                                                       # (reads with N: the flag words matter)
    c.classify_packed(words, bw, bm, offsets, paired=paired)
    check(c, want, what="classify_batch_packed")
    c.classify(bases, offsets, paired=paired, want_hits=True)            # the caller's own hit buffer
    check(c, want, what="classify_batch with hits")
    c.classify_runs(bases, offsets, paired=paired)
    check(c, want, what="classify_batch_runs")
    run_device(c, bases, offsets, paired, packed=False)
    check(c, want, what="classify_batch_device")
    run_device(c, bases, offsets, paired, packed=True)
    check(c, want, what="classify_batch_packed_device")
    c.debug_set(MANY_PIECES)                                             # the upload in slices: shifted offsets, one launch per slice
    c.classify(bases, offsets, paired=paired)
    check(c, want, what="sliced")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_shapes_where_the_walk_can_go_wrong(ctx, oracle, small_world, layout):
    w = small_world
    table = oracle.Table()
    for leaf, g in w.genomes.items():
        oracle.lca_map_add(table, w.tax, 31, g.tobytes(), leaf)
    oracle.lca_map_add(table, w.tax, 31, b"A" * 100, 1002)              # key 0: poly-A, canonical
    assert table.get_batch(np.zeros(1, np.uint64))[1][0]
    g = w.genomes[1001]
    rng = np.random.default_rng(3)
    every31 = g[200:500].copy(); every31[::31] = ord("N")               # no window of 31 without an N
    spaced_n = g[600:900].copy(); spaced_n[::40] = ord("N")             # some windows between the Ns
    # lengths 0, 30 (< k), 31, then 93 .. 96: 63, 64, 65 and 66 k-mers, either side of a round of 64; 5000 bases: three chunks
    reads = [g[:0], g[10:40], g[10:41], g[100:193], g[100:194], g[100:195], g[100:196], g[300:5300], g[5000:5150], np.full(150, ord("N"), np.uint8), every31,
             spaced_n, np.full(200, ord("A"), np.uint8), np.full(64, ord("a"), np.uint8)] + synth.simulate_reads(rng, w.genomes, 20)
    want = model(oracle, w, reads, table=table)
    assert oracle.encode(every31.tobytes(), 31).size == 0 and oracle.encode(g[100:194].tobytes(), 31).size == 64
    c = ctx
    load(c, w, layout, arrays=table.arrays())
    for paired in (False, True):
        for one_by_one in (False, True):                                  # each read (pair) a launch of its own as well
            step = (2 if paired else 1) if one_by_one else len(reads)
            for i in range(0, len(reads), step):
                bases, offsets = synth.concat(reads[i:i + step])
                c.classify(bases, offsets, paired=paired)
                words, bw, bm = bonsai_amd.pack_reads(bases, offsets)
                c.classify_packed(words, bw, bm, offsets, paired=paired)
            check(c, want, what=(paired, one_by_one))
    # the poly-A reads alone: one bin, one register
    bases, offsets = synth.concat([np.full(200, ord("A"), np.uint8)])
    c.classify(bases, offsets)
    bins, regs, _ = c.sketch()
    assert bins.tolist() == [1002] and np.array_equal(regs[0], SM.registers(np.zeros(1, np.uint64)))


def test_bins_outside_the_taxonomy(ctx, oracle, small_world, exact):
    """a table value below n that is no node, and one >= n: bin n"""
    w, (reads, _) = small_world, exact
    vals = w.vals.copy()
    vals[vals == 1003] = 1500
    vals[vals == 1004] = 7777
    n = w.parent.size
    assert n == 2003 and (vals == 1500).any() and (vals == 7777).any()
    table = oracle.Table.wrap(*w.table.header(), w.flags.copy(), w.keys.copy(), vals)
    want = model(oracle, w, reads[:500], table=table)
    assert want[0][-1] == n and 1003 not in want[0] and 1004 not in want[0]
    for layout in LAYOUTS:
        load(ctx, w, layout, arrays=(w.flags, w.keys, vals))
        ctx.classify(*synth.concat(reads[:500]))
        check(ctx, want, what=layout)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_spaced_seeds(ctx, oracle, layout):
    w = synth.make_world(oracle, seed=14, k=31, genome_len=3000, gaps=[1] * 15 + [0] * 15)
    reads = synth.simulate_reads(np.random.default_rng(8), w.genomes, 300, var_len=True)
    want = model(oracle, w, reads, spaced_intended=True)
    assert want[0].size >= 6
    load(ctx, w, layout, spaced_intended=True)
    for paired in (False, True):
        ctx.classify(*synth.concat(reads), paired=paired)
        check(ctx, want, what=paired)
    # through the string for_each a spaced seed emits nothing: no bin at all
    load(ctx, w, layout, spaced_intended=False)
    ctx.classify(*synth.concat(reads))
    bins, regs, dropped = ctx.sketch()
    assert bins.size == 0 and regs.shape == (0, 4096) and dropped == 0


def test_spaced_seed_with_many_runs(ctx, oracle):
    gaps = [1, 0] * 15                                                   # comb of 46 bases in sixteen runs
    w = synth.make_world(oracle, seed=15, k=31, genome_len=3000, gaps=gaps)
    reads = synth.simulate_reads(np.random.default_rng(9), w.genomes, 200)
    load(ctx, w, _lib.LAYOUT_MINBUCKET)
    ctx.classify(*synth.concat(reads))
    check(ctx, model(oracle, w, reads))


@pytest.mark.parametrize("k, canon", [(21, True), (32, True), (31, False)])
def test_other_k_and_uncanonical(ctx, oracle, k, canon):
    w = synth.make_world(oracle, seed=40 + k, k=k, genome_len=3000, canon=canon)
    reads = synth.simulate_reads(np.random.default_rng(k), w.genomes, 400, var_len=True)
    want = model(oracle, w, reads)
    load(ctx, w, _lib.LAYOUT_MINBUCKET)
    bases, offsets = synth.concat(reads)
    ctx.classify(bases, offsets)
    check(ctx, want)
    ctx.classify_packed(*bonsai_amd.pack_reads(bases, offsets), offsets, paired=True)
    check(ctx, want)
    # a window (bns_set_window) changes what encode emits, not what classify looks up: window = k
    if canon:
        ctx.set_window(k + 10)
        try:
            ctx.classify(bases, offsets)
            check(ctx, want, what="windowed encoder")
        finally:
            ctx.set_window(0)


def test_min_base_quality_follows_the_masked_image(ctx, oracle, small_world, exact):
    w, reads = small_world, exact[0][:400]
    rng = np.random.default_rng(21)
    quals = [(33 + rng.choice([5, 30], p=[0.1, 0.9], size=r.size)).astype(np.uint8).tobytes() for r in reads]
    doc = fastq(reads, quals)
    masked = [np.frombuffer(minq_lib.mask(r.tobytes(), q, 20), dtype=np.uint8) for r, q in zip(reads, quals)]
    want, plain = model(oracle, w, masked), model(oracle, w, reads)
    assert not np.array_equal(want[1], plain[1][np.isin(plain[0], want[0])])
    load(ctx, w)
    ctx.set_min_base_quality(20)
    try:
        got = ctx.classify_text(doc, final=True)
        assert got["n_records"] == len(reads)
        check(ctx, want)
    finally:
        ctx.set_min_base_quality(0)
    ctx.classify_text(doc, final=True)
    check(ctx, plain)


def test_idempotence_and_lifecycle(ctx, oracle, small_world, exact):
    c, w, (reads, want) = ctx, small_world, exact
    c.set_encoder(31, None, canonicalize=True)
    c.load_table(w.n_buckets, w.flags, w.keys, w.vals)
    c.load_taxonomy(w.parent)
    c.sketch_enable(0)
    with pytest.raises(bonsai_amd.BonsaiAmdError):
        c.sketch()                                                       # not enabled
    c.sketch_enable(64)
    bins, regs, dropped = c.sketch()
    assert bins.size == 0 and dropped == 0
    bases, offsets = synth.concat(reads)
    t0 = c.classify(bases, offsets)["taxon"]
    check(c, want, reset=False)
    c.classify(bases, offsets)                                           # the same batch again: nothing changes
    check(c, want, reset=False)
    c.classify(*synth.concat(reads[:100]))                               # ... nor does a part of it, in a launch of its own
    check(c, want, reset=True)
    bins, regs, dropped = c.sketch()                                     # reset: no bin, and the next batch starts from zero
    assert bins.size == 0 and dropped == 0
    half = model(oracle, w, reads[:1000])
    c.classify(*synth.concat(reads[:1000]))
    check(c, half, reset=False)
    c.classify(*synth.concat(reads[1000:]))                              # bins of a later launch take later slots: still ascending
    check(c, want, reset=False)
    c.load_taxonomy(w.parent)                                            # a new taxonomy zeroes
    assert c.sketch()[0].size == 0
    # the confidence walk changes taxa, not one register: a k-mer goes by its own taxon
    c.set_confidence(0.5)
    try:
        t1 = c.classify(bases, offsets)["taxon"]
        assert not np.array_equal(t0, t1)
        check(c, want)
        c.set_confidence(0)                                              # confidence off, sketches on: the hit buffer stays
        c.classify(bases, offsets)
        check(c, want)
    finally:
        c.set_confidence(0)
    c.sketch_enable(0)
    with pytest.raises(bonsai_amd.BonsaiAmdError):
        c.sketch()
    assert np.array_equal(c.classify(bases, offsets)["taxon"], t0)       # off: classify as before
    c.sketch_enable(64)                                                  # on again: from zero
    assert c.sketch()[0].size == 0


def test_sketch_enable_needs_a_taxonomy():
    c = bonsai_amd.Context(0)
    try:
        with pytest.raises(bonsai_amd.BonsaiAmdError):
            c.sketch_enable(16)
        c.sketch_enable(0)
    finally:
        c.close()


def test_capacity(ctx, small_world, exact):
    c, w, (reads, want) = ctx, small_world, exact
    load(c, w, max_taxa=2)
    bases, offsets = synth.concat(reads)
    c.classify(bases, offsets)
    for _ in range(2):                                                   # (the second round: a launch that brings nothing new)
        bins, regs, dropped = c.sketch()
        assert bins.tolist() == want[0][:2].tolist()                     # the two smallest bins, exact
        assert np.array_equal(regs, want[1][:2])
        assert dropped == want[0].size - 2
        c.classify(bases, offsets)
    # room for all but one: the largest bin is the one left out
    load(c, w, max_taxa=want[0].size - 1)
    c.classify(bases, offsets)
    bins, regs, dropped = c.sketch()
    assert bins.tolist() == want[0][:-1].tolist() and np.array_equal(regs, want[1][:-1]) and dropped == 1


def test_text_paths(ctx, small_world, exact):
    c, w, (reads, want) = ctx, small_world, exact
    load(c, w)
    doc = fastq(reads)
    c.debug_set(BATCH_TINY | MANY_PIECES)                                # many pieces of text, a classify launch per >= 64 records
    got = c.classify_text(doc, final=True)
    assert got["n_records"] == len(reads) and got["n_launches"] > 4
    check(c, want, what="several launches")
    half = len(reads) // 2
    pair = c.classify_text([fastq(reads[:half]), fastq(reads[half:])], final=True, defer=True)
    assert pair["n_records"] == len(reads)
    check(c, want, what="a pair of texts, in two halves")
    # calls whose run arrays fill up end early (BNS_TEXT_CAP) and hand launches back: their units are classified again by the next call
    pos, done, cap, capped = 0, 0, 400, 0
    while pos < len(doc):
        part = c.classify_text(doc[pos:], final=True, want_runs=True, runs_cap=cap)
        capped += part["status"] == _lib.TEXT_CAP
        done += part["n_records"]; pos += part["consumed"][0]
        if part["n_records"] == 0:
            cap *= 2
    assert done == len(reads) and capped > 2
    check(c, want, what="roll-back")


def test_estimate_of_one_genome(ctx, oracle, small_world):
    """20x coverage of one leaf genome: the estimate of the bin with the most distinct k-mers lies within six standard errors
    (6 x 1.04 / sqrt(4096) = 9.75 %) of the exact count"""
    from bonsai_amd import hostio
    w = small_world
    reads = synth.simulate_reads(np.random.default_rng(77), {1001: w.genomes[1001]}, 800)
    kb = SM.keys_by_bin(oracle, w.table, w.parent, reads, 31)
    top = max(kb, key=lambda b: np.unique(kb[b]).size)
    exact_n = np.unique(kb[top]).size
    assert exact_n > 1000
    load(ctx, w)
    ctx.classify(*synth.concat(reads))
    bins, regs, _ = ctx.sketch()
    est = hostio.hll_estimate(regs[bins.tolist().index(top)])
    print("bin %d: exact %d, estimate %d (%.2f %%)" % (top, exact_n, est, 100.0 * abs(est - exact_n) / exact_n))
    assert est == SM.estimate(SM.registers(kb[top]))
    assert abs(est - exact_n) / exact_n <= 6 * 1.04 / 64
