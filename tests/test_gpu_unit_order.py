"""The hand-over between consecutive units of classify_kernel.

A wavefront classifies the units of a claim one after the other, and three things cross from one unit to the next: the first
256 bases (or packed words) of the NEXT unit, asked for behind the current unit's first pack; the record of the PREVIOUS unit,
stored at the same place; and, in a pair, the first bases of the second mate.  A unit that packs nothing -- empty, shorter than
k -- still has to ask and to store.  The batches below sit on the edges of that: every length at which the pack takes another
path, every alignment of a read's first base, non-ACGT bases at either end of a read, empty and short units at every place of
a batch and of a claim, batches of a few units, and a batch large enough that every resident wavefront works through full claims
(31 units) and takes a freshly claimed one over.  Every unit's taxon, missing, ambig and n_hits, and the ordered hit
stream, are held against the oracle, through the ASCII and the packed entry point, which must also agree with each other."""
import numpy as np
import pytest

import classify_forms as F
import synth

pytestmark = pytest.mark.gpu

# the bench form (k = 31, clustered table, window 15), a generic-k form, a spaced seed on the clustered table
FORMS = {
    "k31": dict(k=31, gaps=None, span=15),
    "k24": dict(k=24, gaps=None, span=F.distinct_windows(24)[0][0]),
    "spaced": dict(k=31, gaps=F.SPACED_GAPS, span=0),
}
CASES = [(f, paired) for f in FORMS for paired in (False, True)]
IDS = ["%s-%s" % (f, "paired" if p else "single") for f, p in CASES]
FULL_CLAIM = 31                                          # units of a full claim, reads or pairs (classify_chunk, bns_kernels.hpp)
PER_WAVE = {False: 63, True: 31}                         # units per resident wavefront in the large batch: two full claims and one
CUS = 256                                                # MI355X; 32 resident wavefronts each (the test asserts what this is for)


class Loaded:
    """the form's world on the device for the length of a with block"""

    def __init__(self, ctx, oracle, form):
        self.ctx, self.f = ctx, FORMS[form]
        f = self.f
        self.w = F.world(oracle, f["k"], True, f["gaps"], "std")
        self.gaps = list(f["gaps"]) if f["gaps"] is not None else None

    def __enter__(self):
        ctx, f, w = self.ctx, self.f, self.w
        ctx.set_encoder(f["k"], self.gaps, canonicalize=True)
        ctx.debug_set(F.DBG_OVC_OFF)
        if f["gaps"] is None:
            ctx.set_minimizer_span(f["span"])
            ctx.set_minimizer_identity(32)
        ctx.load_table(w.n_buckets, w.flags, w.keys, w.vals, layout=F.LAYOUT_MINBUCKET)
        ctx.load_taxonomy(w.parent)
        return self

    def __exit__(self, *exc):
        self.ctx.debug_set(0)
        self.ctx.set_minimizer_span(0)
        self.ctx.set_minimizer_identity(0)


def check(ld, oracle, bases, offsets, paired, reads=None, hit_units=None):
    """ASCII and packed against the oracle (every unit's four numbers; the hit stream of hit_units, all when reads are given and
    hit_units is None) and against each other (everything); returns the ASCII call's form record"""
    import bonsai_amd
    ctx, w = ld.ctx, ld.w
    inc = 2 if paired else 1
    n_units = (len(offsets) - 1) // inc
    exp = oracle.classify_batch(w.table, w.tax, w.k, bases, offsets, paired=paired, gaps=ld.gaps, canon=True, spaced_intended=True)
    got = ctx.classify(bases, offsets, paired=paired, want_hits=True)
    form = ctx.last_classify_form()
    words, bw, bm = bonsai_amd.pack_reads(bases, offsets, threads=2)
    gotp = ctx.classify_packed(words, bw, bm, offsets, paired=paired, want_hits=True)
    for name, g in (("ascii", got), ("packed", gotp)):
        for key in ("taxon", "missing", "ambig", "n_hits"):
            bad = np.flatnonzero(g[key] != exp[key])
            assert bad.size == 0, "%s: %s differs at units %s of %d: got %s, expected %s" % (name, key, bad[:8], n_units, g[key][bad[:8]], exp[key][bad[:8]])
    assert len(got["hits"]) == len(gotp["hits"]) == n_units
    for u in range(n_units):
        assert np.array_equal(got["hits"][u], gotp["hits"][u]), "hit stream of unit %d: packed differs from ASCII" % u
    if hit_units is None:
        hit_units = range(n_units)
    for u in hit_units:
        o = [int(x) for x in offsets[u * inc:u * inc + inc + 1]]
        s1 = bases[o[0]:o[1]].tobytes()
        s2 = bases[o[1]:o[2]].tobytes() if paired else None
        h = oracle.classify_seq(w.table, w.tax, w.k, s1, s2, gaps=ld.gaps, canon=True, spaced_intended=True)[3]
        assert np.array_equal(got["hits"][u], h), "hit stream of unit %d" % u
    return form, got


def cutter(w, seed):
    rng = np.random.default_rng(seed)
    g = np.concatenate(list(w.genomes.values()))

    def cut(n):
        st = int(rng.integers(0, g.size - n))
        return synth.mutate(rng, g[st:st + n], 0.005, 0.0)
    return rng, cut


def edge_lengths(w):
    """every length at which the pack or the rounds take another path; c = the comb (k for a contiguous seed)"""
    k, c = w.k, F.comb(w.k, w.gaps)
    return sorted({0, 1, k - 1, k, k + 63, k + 64, c - 1, c, c + 63, c + 64, 150, 255, 256, 257, 2047, 2048, 2049, 4300})


def edge_reads(w):
    """The edge lengths between ordinary reads, ragged so that the reads start at every residue mod 4; an N at the first and at
    the last base of a read; short units first, last and several in a row."""
    rng, cut = cutter(w, 5)
    c = F.comb(w.k, w.gaps)
    shorts = [0, 1, c - 1, 0]
    reads = [cut(n) for n in shorts[:2]]                                     # the batch begins with an empty and a 1-base read
    for i, n in enumerate(edge_lengths(w)):
        reads += [cut(n), cut(150 + (i % 4))]                                # ragged: offsets run through all residues mod 4
    for pos in (0, -1):
        for n in (c, 150, 257):
            r = cut(n)
            r[pos] = ord("N")
            reads.append(r)
    reads += [cut(151)] + [cut(n) for n in shorts] + [cut(149)]              # a run of four units that pack nothing
    reads += [cut(n) for n in (c - 1, 0, 1)]                                 # ... and three of them end the batch
    assert {int(x) & 3 for x in np.cumsum([r.size for r in reads])} == {0, 1, 2, 3}
    return [np.ascontiguousarray(r, dtype=np.uint8) for r in reads]


def edge_pairs(w):
    """pairs with mate 1 or mate 2 (or both) empty or shorter than k, between ordinary pairs, first and last of the batch"""
    rng, cut = cutter(w, 6)
    c = F.comb(w.k, w.gaps)
    reads = []
    for a, b in ((0, 150), (150, 0), (c - 1, 151), (149, c - 1), (0, 0), (150, 150), (1, c - 1), (c, c), (257, 2049), (2048, 255), (4300, 150),
                 (151, 4300), (c + 63, c + 64), (153, 0), (0, 152), (c - 1, 1)):
        reads += [cut(a), cut(b)]
    for pos in (0, -1):
        r1, r2 = cut(150), cut(150)
        r1[pos] = ord("N")
        r2[pos] = ord("N")
        reads += [r1, cut(150), cut(150), r2]
    reads += [cut(0), cut(1)]
    return [np.ascontiguousarray(r, dtype=np.uint8) for r in reads]


@pytest.mark.parametrize("form,paired", CASES, ids=IDS)
def test_edge_lengths(gpu_ctx, oracle, form, paired):
    with Loaded(gpu_ctx, oracle, form) as ld:
        batches = [edge_reads(ld.w)]
        if paired:
            batches.append(edge_pairs(ld.w))
        for reads in batches:
            if len(reads) % 2:
                reads = reads + [reads[3]]
            bases, offsets = synth.concat(reads)
            _, got = check(ld, oracle, bases, offsets, paired)
            assert int(got["n_hits"].sum()) > 0 and (got["taxon"] != 0).any()
            assert any(r.size > 4096 for r in reads)


@pytest.mark.parametrize("form,paired", CASES, ids=IDS)
def test_small_batches(gpu_ctx, oracle, form, paired):
    """1, 2, 3, 4, 5 and 9 units (claims of 4, the last one short): ordinary units, units that pack nothing at either end, and
    nothing but such units"""
    inc = 2 if paired else 1
    with Loaded(gpu_ctx, oracle, form) as ld:
        rng, cut = cutter(ld.w, 7)
        c = F.comb(ld.w.k, ld.w.gaps)
        short = (0, c - 1, 1)
        for n in (1, 2, 3, 4, 5, 9):
            plans = [[150 + i for i in range(n * inc)],
                     [short[i % 3] if (i // inc in (0, n - 1) or i // inc == 4) else 150 + i for i in range(n * inc)],
                     [short[i % 3] if i % inc == 0 else 150 + i for i in range(n * inc)],
                     [1 if i == 0 else short[i % 3] for i in range(n * inc)]]
            for lens in plans:
                reads = [np.ascontiguousarray(cut(L), dtype=np.uint8) for L in lens]
                bases, offsets = synth.concat(reads)
                form_rec, _ = check(ld, oracle, bases, offsets, paired)
                assert form_rec["chunk"] == 4 and form_rec["grid"] >= 1


def large_batch(w, paired):
    """Short reads, 63 (pairs: 31) per resident wavefront plus an odd remainder: every wavefront claims full chunks and goes on into
    a further one.  Units that pack nothing sit at the first and the last place of every third claim, five in a row inside every
    fifth, and at random; a few reads are long enough for a second pack pass."""
    full = FULL_CLAIM
    inc = 2 if paired else 1
    n_units = PER_WAVE[paired] * 32 * CUS + 37
    rng = np.random.default_rng(91 + inc)
    c = F.comb(w.k, w.gaps)
    lens = rng.integers(c - 4, c + 40, size=n_units * inc).astype(np.int64)
    lens[rng.random(lens.size) < 0.002] = 300
    u = np.arange(n_units)
    claim, at = u // full, u % full
    nothing = (((claim % 3) == 0) & ((at == 0) | (at == full - 1))) | (((claim % 5) == 1) & (at >= 20) & (at < 25)) | (rng.random(n_units) < 0.01)
    nothing[0] = nothing[-1] = True
    idx = np.flatnonzero(nothing)
    short = np.array([0, c - 1, 1], dtype=np.int64)
    if paired:
        which = rng.integers(0, 3, size=idx.size)                        # mate 1, mate 2 or both
        lens[idx[which != 1] * 2] = short[idx[which != 1] % 3]
        lens[idx[which != 0] * 2 + 1] = short[(idx[which != 0] + 1) % 3]
    else:
        lens[idx] = short[idx % 3]
    offsets = np.zeros(lens.size + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    total = int(offsets[-1])
    g = np.concatenate(list(w.genomes.values()))
    starts = rng.integers(0, g.size - 400, size=lens.size)
    src = np.repeat(starts - offsets[:-1].astype(np.int64), lens) + np.arange(total, dtype=np.int64)
    bases = g[src]
    sub = rng.random(total) < 0.004
    bases[sub] = synth.ACGT[rng.integers(0, 4, size=int(sub.sum()))]
    bases[rng.random(total) < 0.0005] = ord("N")
    return np.ascontiguousarray(bases, dtype=np.uint8), offsets, n_units


@pytest.mark.parametrize("form,paired", CASES, ids=IDS)
def test_full_claims(gpu_ctx, oracle, form, paired):
    with Loaded(gpu_ctx, oracle, form) as ld:
        bases, offsets, n_units = large_batch(ld.w, paired)
        assert bases.size < 100_000_000
        full = FULL_CLAIM
        # the hit stream against the oracle at both ends of every 17th claim and every 997th unit; ASCII against packed everywhere
        sample = sorted({u for cl in range(0, n_units // full, 17) for u in (cl * full, cl * full + full - 1)} | set(range(0, n_units, 997)) | {n_units - 1})
        form_rec, got = check(ld, oracle, bases, offsets, paired, hit_units=sample)
        assert form_rec["chunk"] == full, "the batch is meant to run full claims"
        assert form_rec["grid"] * 4 * full < n_units, "... and every wavefront is meant to go on into a further claim"
        assert (got["taxon"] != 0).mean() > 0.2 and int(got["n_hits"].sum()) > 0
