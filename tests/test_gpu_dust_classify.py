"""Low-complexity masking in front of classify (bns_set_dust), through every classifying entry point.

The truth throughout: a call with masking ON for input x equals the same call with masking OFF for substitute(x, dust_ref(x)) --
taxon, missing, ambig, n_hits, the ordered hit stream, and the runs / Kraken lines where the entry point gives them.  The reads come
from genomes that hold low-complexity tracts (tests/dust_world.py), so that the mask changes at least a fifth of them."""
import numpy as np
import pytest

import bonsai_amd
from bonsai_amd import _lib
import dust_ref as D
import dust_world as DW
import minq_lib as M
import synth

pytestmark = pytest.mark.gpu

W, T = DW.W, DW.T
BATCH_TINY, SLICE_8K = 0x40, 0x4000
N_READS = 1200
u32 = np.uint32


class Dev:
    """device buffers of one test, through the context's own allocator"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def up(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.ctx.dev_alloc(arr.nbytes + 16)
        self.ptrs.append(p)
        if arr.nbytes:
            self.ctx.dev_upload(p, arr)
        return p

    def down(self, p, n, dtype):
        a = np.zeros(n, dtype=dtype)
        if n:
            self.ctx.dev_download(p, a)
        return a

    def free(self):
        for p in self.ptrs:
            self.ctx.dev_free(p)
        self.ptrs = []


@pytest.fixture(scope="module")
def world(oracle):
    w = DW.make_world(oracle, seed=31)
    c = bonsai_amd.Context(0)
    c.set_encoder(31, None, canonicalize=True)
    c.load_table(w.n_buckets, w.flags, w.keys, w.vals)
    c.load_taxonomy(w.parent)
    w.ctx = c
    rng = np.random.default_rng(5)
    w.reads = synth.simulate_reads(rng, w.genomes, N_READS, n_rate=0.002, lower_rate=0.01)
    w.reads[3] = w.reads[3][:0]; w.reads[4] = w.reads[4][:2]; w.reads[5] = w.reads[5][:40]
    w.reads[6] = np.concatenate([w.reads[6], w.genomes[1003][200:2500]])      # a long read: more than one piece of the mask pass
    w.sub, w.masks = DW.substituted(w.reads)
    w.clean = synth.simulate_reads(rng, w.genomes, N_READS, n_rate=0.0)      # no invalid base: a packed image without flag words
    w.clean_sub, _ = DW.substituted(w.clean)
    share = sum(int(m.sum()) for m in w.masks) / sum(r.size for r in w.reads)
    assert 0.05 <= share <= 0.70, share
    yield w
    c.close()


@pytest.fixture(autouse=True)
def as_found(world):
    yield
    c = world.ctx
    c.debug_set(0); c.set_dust(0); c.set_confidence(0); c.tally_enable(False); c.sketch_enable(0); c.set_min_base_quality(0)


def on_off(ctx, call, x, sub):
    """call(x) with masking on, call(sub) with it off -> (on, off, the form of each)"""
    ctx.set_dust(W, T)
    a = call(x)
    fa = ctx.last_classify_form()
    ctx.set_dust(0)
    b = call(sub)
    fb = ctx.last_classify_form()
    return a, b, fa, fb


# ---- host batches ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_classify_host_ascii(world, paired):
    c = world.ctx
    call = lambda reads: c.classify(*synth.concat(reads), paired=paired, want_hits=True)
    a, b, fa, fb = on_off(c, call, world.reads, world.sub)
    DW.same_units(a, b)
    # ASCII input is classified in a packed form while masking is on, and in exactly today's form while it is off
    assert fa["kernel"][7] == 1 and fb["kernel"][7] == 0
    plain = call(world.reads)
    assert c.last_classify_form() == fb
    share = DW.changed_share(a, plain)
    print("units changed by the mask: %.3f" % share)
    assert share >= 0.20
    assert (a["n_hits"] > 0).mean() >= 0.5                      # ... without wiping the reads out


def test_classify_host_sliced(world):
    c = world.ctx
    c.debug_set(SLICE_8K)
    call = lambda reads: c.classify(*synth.concat(reads), want_hits=True)
    a, b, _, _ = on_off(c, call, world.reads, world.sub)
    DW.same_units(a, b)
    c.debug_set(0)
    DW.same_units(a, call(world.sub))


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_classify_runs(world, paired):
    c = world.ctx
    call = lambda reads: c.classify_runs(*synth.concat(reads), paired=paired)
    a, b, fa, _ = on_off(c, call, world.reads, world.sub)
    DW.same_units(a, b)
    assert a["n_runs_total"] == b["n_runs_total"] and fa["kernel"][7] == 1


@pytest.mark.parametrize("which", ["flagged", "clean"])
def test_classify_packed_host(world, which):
    """the packed host form with and without words that hold an invalid base"""
    c = world.ctx
    reads, sub = (world.reads, world.sub) if which == "flagged" else (world.clean, world.clean_sub)

    def call(rs):
        bases, offsets = synth.concat(rs)
        words, bw, bm = bonsai_amd.pack_reads(bases, offsets)
        call.n_bad.append(bw.size)
        keep = words.copy()
        out = c.classify_packed(words, bw, bm, offsets, want_hits=True)
        assert np.array_equal(words, keep)
        return out
    call.n_bad = []
    a, b, fa, fb = on_off(c, call, reads, sub)
    assert (call.n_bad[0] > 0) == (which == "flagged")
    DW.same_units(a, b)
    assert fa["kernel"][7] == 1 and fb["kernel"][7] == 1
    c.debug_set(SLICE_8K)
    a2, b2, _, _ = on_off(c, call, reads, sub)
    DW.same_units(a2, b2); DW.same_units(a2, a)


# ---- device batches ----------------------------------------------------------------------------------------------------------------
def device_ascii(ctx, reads, paired, max_len):
    dev = Dev(ctx)
    try:
        bases, offsets = synth.concat(reads)
        n, total = len(reads), int(offsets[-1])
        inc = 2 if paired else 1
        nu = n // inc
        d_b, d_o = dev.up(np.concatenate([bases, np.zeros(8, np.uint8)])), dev.up(offsets)
        outs = [dev.up(np.zeros(nu, u32)) for _ in range(4)] + [dev.up(np.zeros(total + 1, u32))]
        ctx.classify_device(d_b, d_o, n, total, max_len, paired, *outs)
        res = {k: dev.down(p, nu, u32) for k, p in zip(("taxon", "missing", "ambig", "n_hits"), outs)}
        hits = dev.down(outs[4], total + 1, u32)
        res["hits"] = [hits[int(offsets[u * inc]):int(offsets[u * inc]) + int(res["n_hits"][u])].copy() for u in range(nu)]
        assert np.array_equal(dev.down(d_b, bases.size, np.uint8), bases)
        return res
    finally:
        dev.free()


@pytest.mark.parametrize("paired,max_len", [(False, 0), (False, 4000), (True, 0)], ids=["single-len-read-back", "single-len-given", "paired"])
def test_classify_device(world, paired, max_len):
    c = world.ctx
    call = lambda reads: device_ascii(c, reads, paired, max_len)
    a, b, fa, fb = on_off(c, call, world.reads, world.sub)
    DW.same_units(a, b)
    assert fa["kernel"][7] == 1 and fb["kernel"][7] == 0


def device_packed(ctx, reads, with_nmask, max_len=0):
    dev = Dev(ctx)
    try:
        bases, offsets = synth.concat(reads)
        n, total = len(reads), int(offsets[-1])
        words, bw, bm = bonsai_amd.pack_reads(bases, offsets)
        nmask = M.dense_flags(words.size, bw, bm)
        assert with_nmask or not bw.size
        d_w, d_m, d_o = dev.up(words), dev.up(nmask) if with_nmask else None, dev.up(offsets)
        outs = [dev.up(np.zeros(n, u32)) for _ in range(4)] + [dev.up(np.zeros(total + 1, u32))]
        ctx.classify_packed_device(d_w, d_m, d_o, n, total, max_len, False, *outs)
        res = {k: dev.down(p, n, u32) for k, p in zip(("taxon", "missing", "ambig", "n_hits"), outs)}
        hits = dev.down(outs[4], total + 1, u32)
        res["hits"] = [hits[int(offsets[u]):int(offsets[u]) + int(res["n_hits"][u])].copy() for u in range(n)]
        # the caller's image is never written to
        assert np.array_equal(dev.down(d_w, words.size, np.uint64), words)
        if with_nmask:
            assert np.array_equal(dev.down(d_m, nmask.size, u32), nmask)
        return res
    finally:
        dev.free()


def test_classify_packed_device_with_flags(world):
    c = world.ctx
    a, b, fa, fb = on_off(c, lambda rs: device_packed(c, rs, True), world.reads, world.sub)
    DW.same_units(a, b)
    assert fa["kernel"][7] == 1 and fb["kernel"][7] == 1


def test_classify_packed_device_without_flags(world):
    """the caller hands no flag words in (no read holds an invalid base); the off run's substituted reads need theirs"""
    c = world.ctx
    c.set_dust(W, T)
    a = device_packed(c, world.clean, False, max_len=150)
    c.set_dust(0)
    b = device_packed(c, world.clean_sub, True, max_len=150)
    DW.same_units(a, b)
    assert DW.changed_share(a, device_packed(c, world.clean, False, max_len=150)) >= 0.20


# ---- text ------------------------------------------------------------------------------------------------------------------------
def text_of(reads, fasta=False, tag=b"r", suffix=b""):
    names = [tag + b"%d" % i + suffix for i in range(len(reads))]
    quals = [None if (fasta or i % 7 == 3) else b"I" * len(r) for i, r in enumerate(reads)]
    return M.fastq_text(names, reads, quals, wrap_seq=70 if fasta else 0)


@pytest.mark.parametrize("fasta", [False, True], ids=["fastq", "fasta"])
@pytest.mark.parametrize("dbg", [0, SLICE_8K, SLICE_8K | BATCH_TINY], ids=["one-slice", "slices", "slices-tiny-batches"])
def test_classify_text(world, fasta, dbg):
    c = world.ctx
    c.debug_set(dbg)
    call = lambda reads: c.classify_text(text_of(reads, fasta), final=True, want_runs=True, want_lines=True)
    a, b, fa, _ = on_off(c, call, world.reads, world.sub)
    assert a["status"] == _lib.TEXT_OK and a["n_records"] == len(world.reads) == b["n_records"]
    assert dbg == 0 or a["n_slices"] > 10
    DW.same_units(a, b)
    assert a["lines"] == b["lines"] and np.array_equal(a["line_off"], b["line_off"])
    assert fa["kernel"][7] == 1
    if dbg == 0:
        assert DW.changed_share(a, call(world.reads)) >= 0.20


def test_classify_text_pair(world):
    c = world.ctx
    n = len(world.reads) // 2
    for dbg in (0, SLICE_8K | BATCH_TINY):
        c.debug_set(dbg)
        call = lambda reads: c.classify_text([text_of(reads[:n], suffix=b"/1"), text_of(reads[n:2 * n], suffix=b"/2")], final=True, trim_readno=True,
                                             want_runs=True, want_lines=True)
        a, b, _, _ = on_off(c, call, world.reads, world.sub)
        assert a["status"] == _lib.TEXT_OK and a["n_records"] == 2 * n
        DW.same_units(a, b)
        assert a["lines"] == b["lines"]


def test_parse_only_returns_the_masked_image(world):
    """(one slice: the packed words come back for one-slice calls only)"""
    c = world.ctx
    reads, sub = world.reads[:300], world.sub[:300]
    call = lambda rs: c.classify_text(text_of(rs), final=True, parse_only=True, want_words=True)
    a, b, _, _ = on_off(c, call, reads, sub)
    assert a["status"] == _lib.TEXT_OK and a["n_records"] == len(reads)
    assert np.array_equal(a["seq_len"], b["seq_len"]) and a["names"] == b["names"]
    assert np.array_equal(M.read_words(a["words"], a["seq_len"]), M.read_words(b["words"], b["seq_len"]))
    assert np.array_equal(M.read_words(a["nmask"], a["seq_len"]), M.read_words(b["nmask"], b["seq_len"]))
    assert M.unpack(a["words"], a["nmask"], a["seq_len"]) == [M.norm(s.tobytes()) for s in sub]
    plain = call(reads)
    assert not np.array_equal(M.read_words(a["nmask"], a["seq_len"]), M.read_words(plain["nmask"], plain["seq_len"]))


# ---- what sits behind the image ----------------------------------------------------------------------------------------------------
def test_with_confidence(world):
    c = world.ctx
    c.set_confidence(0.1)
    call = lambda reads: c.classify(*synth.concat(reads), want_hits=True)
    a, b, _, _ = on_off(c, call, world.reads, world.sub)
    DW.same_units(a, b)
    c.set_confidence(0)
    c.set_dust(W, T)
    assert np.count_nonzero(call(world.reads)["taxon"] != a["taxon"]) > 0        # the walk did move calls


def test_with_tally(world):
    c = world.ctx
    c.tally_enable(True)

    def call(reads):
        c.tally(reset=True)
        out = c.classify(*synth.concat(reads))
        out["tally"] = c.tally(reset=True)
        return out
    a, b, _, _ = on_off(c, call, world.reads, world.sub)
    DW.same_units(a, b)
    assert np.array_equal(a["tally"][0], b["tally"][0]) and np.array_equal(a["tally"][1], b["tally"][1])
    assert int(a["tally"][0].sum()) == len(world.reads)
    plain = call(world.reads)
    assert not np.array_equal(plain["tally"][0], a["tally"][0])


def test_with_sketch(world):
    c = world.ctx
    c.sketch_enable(64)

    def call(reads):
        c.sketch(reset=True)
        out = c.classify(*synth.concat(reads))
        out["sketch"] = c.sketch(reset=True)
        return out
    a, b, _, _ = on_off(c, call, world.reads, world.sub)
    DW.same_units(a, b)
    assert np.array_equal(a["sketch"][0], b["sketch"][0]) and np.array_equal(a["sketch"][1], b["sketch"][1]) and a["sketch"][2] == b["sketch"][2]
    plain = call(world.reads)
    assert not np.array_equal(plain["sketch"][1], a["sketch"][1])                 # the tracts' k-mers are no longer sketched


def test_with_min_base_quality(world):
    """quality masking comes first (it happens in the pack); DUST runs on the result"""
    c = world.ctx
    rng = np.random.default_rng(8)
    reads = world.reads[:600]
    quals = [M.illumina_qual(rng, r.size, low=0.03) for r in reads]
    names = [b"q%d" % i for i in range(len(reads))]
    by_q = [np.frombuffer(M.mask(r.tobytes(), q, 20), dtype=np.uint8) for r, q in zip(reads, quals)]
    final, _ = DW.substituted(by_q)
    assert sum(int(np.count_nonzero(a != b)) for a, b in zip(by_q, reads)) > 100
    assert sum(int(np.count_nonzero(a != b)) for a, b in zip(final, by_q)) > 1000
    c.set_min_base_quality(20); c.set_dust(W, T)
    a = c.classify_text(M.fastq_text(names, reads, quals), final=True, want_runs=True, want_lines=True)
    c.set_min_base_quality(0); c.set_dust(0)
    b = c.classify_text(M.fastq_text(names, final, quals), final=True, want_runs=True, want_lines=True)
    assert a["status"] == _lib.TEXT_OK and a["n_records"] == len(reads)
    DW.same_units(a, b)
    assert a["lines"] == b["lines"]
    c.set_dust(W, T)
    only_dust = c.classify_text(M.fastq_text(names, reads, quals), final=True)
    assert DW.changed_share(a, only_dust) > 0


@pytest.mark.parametrize("gaps,canon", [([1] * 15 + [0] * 15, True), (None, False)], ids=["spaced", "not-canonical"])
def test_generic_forms(oracle, gaps, canon):
    """a spaced seed and a forward-only encoder: the generic kernel forms, ASCII (packed while on) and packed"""
    w = DW.make_world(oracle, seed=32, genome_len=3000, gaps=gaps, canon=canon)
    reads = synth.simulate_reads(np.random.default_rng(9), w.genomes, 500, n_rate=0.002)
    sub, _ = DW.substituted(reads)
    c = bonsai_amd.Context(0)
    try:
        c.set_encoder(31, gaps, canonicalize=canon)
        c.load_table(w.n_buckets, w.flags, w.keys, w.vals)
        c.load_taxonomy(w.parent)
        for paired in (False, True):
            call = lambda rs: c.classify(*synth.concat(rs), paired=paired, want_hits=True)
            a, b, fa, fb = on_off(c, call, reads, sub)
            DW.same_units(a, b)
            assert fa["kernel"][7] == 1 and fb["kernel"][7] == 0 and fa["kernel"][2] == 0 and fa["kernel"][0] == (1 if gaps else 0)
            assert DW.changed_share(a, call(reads)) >= 0.20
        a, b, _, _ = on_off(c, lambda rs: device_packed(c, rs, True), reads, sub)
        DW.same_units(a, b)
    finally:
        c.close()


# ---- states ------------------------------------------------------------------------------------------------------------------------
def test_states(world):
    c = world.ctx
    for w_, t_ in ((7, 20), (65, 20), (64, 0), (64, 1001)):
        with pytest.raises(bonsai_amd.BonsaiAmdError):
            c.set_dust(w_, t_)
    # refused while a session is open, either kind
    c.build_begin(64)
    try:
        with pytest.raises(bonsai_amd.BonsaiAmdError, match="build session"):
            c.set_dust(W, T)
    finally:
        c.build_end()
    c.windows_begin(100)
    try:
        with pytest.raises(bonsai_amd.BonsaiAmdError, match="window session"):
            c.set_dust(W, T)
    finally:
        c.windows_end()
    # a window session is refused while masking is on, and the message says why
    c.set_dust(W, T)
    with pytest.raises(bonsai_amd.BonsaiAmdError, match="mask of a substring"):
        c.windows_begin(100)
    with pytest.raises(bonsai_amd.BonsaiAmdError):
        c.windows_begin(100, confidence=0.5)
    c.set_dust(0)
    with pytest.raises(bonsai_amd.BonsaiAmdError):
        c.dust_mask(*synth.concat(world.reads[:4]))
    c.windows_begin(100)
    c.windows_end()


def test_off_again_is_as_if_never_on(world):
    """after on -> off a context gives byte-identical results to one that never had the setting, in the same form"""
    c = world.ctx
    fresh = bonsai_amd.Context(0)
    try:
        fresh.set_encoder(31, None, canonicalize=True)
        fresh.load_table(world.n_buckets, world.flags, world.keys, world.vals)
        fresh.load_taxonomy(world.parent)
        bases, offsets = synth.concat(world.reads)
        c.set_dust(W, T)
        c.classify(bases, offsets, want_hits=True)
        c.set_dust(0)
        got, want = c.classify(bases, offsets, want_hits=True), fresh.classify(bases, offsets, want_hits=True)
        DW.same_units(got, want)
        assert c.last_classify_form() == fresh.last_classify_form()
        doc = text_of(world.reads)
        a, b = c.classify_text(doc, final=True, want_lines=True), fresh.classify_text(doc, final=True, want_lines=True)
        DW.same_units(a, b)
        assert a["lines"] == b["lines"]
    finally:
        fresh.close()
