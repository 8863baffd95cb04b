"""Minimum base quality on the device (bns_set_min_base_quality: pack_text_minq_kernel, csrc/bns_minqual.hpp).

The truth throughout: a call with threshold q on a text equals the call WITHOUT the feature on the same records with every base of
low quality replaced by 'N' (tests/minq_lib.py substitutes through tests/kseq_py.py and re-emits plain four-line FASTQ) -- the packed
image at the parse level; taxon, missing, ambig, n_hits, the ordered hits (as runs) and the device's Kraken lines at the classify
level, there against the oracle itself.  Everything else of a call -- seq_len, names, rec_pos, consumed[], status, why -- is that of
the same call with q = 0 on the same text."""
import gzip
import os

import numpy as np
import pytest

import bonsai_amd
from bonsai_amd import _lib
import ingest_fuzz
import kseq_py
import minq_lib as M
import synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
QS = (1, 20, 41, 93)
BATCH_TINY, SLICE_8K = 0x40, 0x4000


@pytest.fixture(scope="module")
def ctx():
    c = bonsai_amd.Context(0)
    c.set_encoder(31, None, canonicalize=True)
    yield c
    c.close()


def parse(ctx, q, doc, **kw):
    ctx.set_min_base_quality(q)
    try:
        return ctx.classify_text(doc, parse_only=True, want_words=True, **kw)
    finally:
        ctx.set_min_base_quality(0)


def check_parse(ctx, doc, q, final=True, limit=None, trim=False):
    """one parse-only call with threshold q on `doc`: everything but the image is the same call's with q = 0; the image -- words and flag
    words -- is that of a q = 0 call on the substituted text of the records taken"""
    kw = dict(final=final, limit=limit, trim_readno=trim)
    base = parse(ctx, 0, doc, **kw)
    got = parse(ctx, q, doc, **kw)
    for k in ("n_records", "consumed", "status", "why", "names", "total_bases"):
        assert got[k] == base[k], (k, got[k], base[k])
    assert np.array_equal(got["seq_len"], base["seq_len"]) and np.array_equal(got["rec_pos"], base["rec_pos"])
    n = got["n_records"]
    if not n:
        return got, base
    sub, recs = M.substituted_text(doc, q, n)
    truth = parse(ctx, 0, sub, final=True, trim_readno=trim)
    assert truth["status"] == _lib.TEXT_OK and truth["n_records"] == n and truth["consumed"][0] == len(sub)
    assert np.array_equal(truth["seq_len"], got["seq_len"]) and truth["names"] == got["names"]
    # (the image proper: the slack word between two reads is never written by the device packer)
    assert np.array_equal(M.read_words(got["words"], got["seq_len"]), M.read_words(truth["words"], truth["seq_len"])), "packed words"
    assert np.array_equal(M.read_words(got["nmask"], got["seq_len"]), M.read_words(truth["nmask"], truth["seq_len"])), "flag words"
    # ... and read back base by base against the parser's own records
    assert M.unpack(got["words"], got["nmask"], got["seq_len"]) == [M.norm(M.mask(r[2], r[3], q)) for r in recs]
    return got, base


def test_parse_reference_vectors(ctx):
    """the crafted texts of ingest_ref.npz: those the device takes get the masked image; those it hands back are handed back the same"""
    IN = np.load(os.path.join(GOLD, "ingest_ref.npz"))
    seen_ok = seen_irregular = masked = 0
    for ci in range(int(IN["n_cases"])):
        f1, f2 = str(IN["case%d_file1" % ci]), str(IN["case%d_file2" % ci])
        if f2:
            continue
        raw = IN["text_" + f1].tobytes()
        doc = gzip.decompress(raw) if f1.endswith("_gz") else raw
        for q in QS:
            got, base = check_parse(ctx, doc, q)
            if got["n_records"]:
                masked += int(not np.array_equal(M.read_words(got["nmask"], got["seq_len"]), M.read_words(base["nmask"], base["seq_len"])))
        if got["status"] == _lib.TEXT_OK:
            seen_ok += 1
        else:
            seen_irregular += 1
            assert got["why"] != 0 and got["n_records"] == 0
    assert seen_ok >= 9 and seen_irregular >= 1 and masked >= 9, (seen_ok, seen_irregular, masked)


@pytest.mark.parametrize("crlf", [False, True])
@pytest.mark.parametrize("seed", range(3))
def test_parse_independent_wrapping(ctx, seed, crlf):
    """sequence and quality wrapped independently (one line or several each), quality lines that start with '@', '>' or '+' (the
    compaction's slow path), quality bytes over the whole printable range and below 33, empty sequences, FASTA mixed in, a missing last
    newline"""
    rng = np.random.default_rng(500 + 2 * seed + crlf)
    slow = differ = 0
    for it in range(10):
        doc = M.make_qdoc(rng, int(rng.integers(1, 250)), crlf=crlf, final_newline=bool(it % 3), headerish=0.3 if it % 2 else 0.0)
        assert kseq_py.reads_cleanly(doc)
        recs = M.records(doc)
        for q in QS:
            got, base = check_parse(ctx, doc, q)
            assert got["status"] == _lib.TEXT_OK and got["consumed"][0] == len(doc) and got["n_records"] == len(recs), (seed, it, q, got["why"])
            differ += int(not np.array_equal(M.read_words(got["nmask"], got["seq_len"]), M.read_words(base["nmask"], base["seq_len"])))
        lines = doc.split(b"\n")
        slow += int(any(l[:1] in (b"@", b">") and lines[i - 1][:1] == b"+" for i, l in enumerate(lines) if i))
    assert slow >= 3 and differ >= 30


@pytest.mark.parametrize("seed", range(3))
def test_parse_fuzz_regular(ctx, seed):
    """ingest_fuzz's regular documents, LF and CRLF, wrapped quality or not, as tests/test_gpu_ingest.py draws them"""
    rng = np.random.default_rng(100 + seed)
    n_ok = 0
    for it in range(25):
        kinds = (("fastq",), ("fasta",), ("fastq", "fasta"))[it % 3]
        doc = ingest_fuzz.make_doc(rng, int(rng.integers(1, 200)), wild=0.0, kinds=kinds, final_newline=bool(it % 4),
                                   crlf=(0.0, 0.4, 1.0)[it % 3] if it % 5 else 0.0, wrapq=0.5 if it % 2 else 0.0)
        if it % 7 == 0:
            doc = b"\n\n" + doc
        q = QS[it % 4]
        got, base = check_parse(ctx, doc, q, trim=bool(it % 2))
        if kseq_py.reads_cleanly(doc):
            n_ok += 1
            assert got["status"] == _lib.TEXT_OK and got["consumed"][0] == len(doc)
        else:
            assert got["status"] == _lib.TEXT_IRREGULAR and got["n_records"] == 0
    assert n_ok >= 15


@pytest.mark.parametrize("window", [97, 1000, 30000])
def test_parse_in_windows(ctx, window):
    """a window of the text per call, the next one from consumed[] on: the masked records are those of one parse of the whole text"""
    rng = np.random.default_rng(7)
    doc = M.make_qdoc(rng, 600, final_newline=False)
    recs = M.records(doc)
    q = 20
    pos, seqs, w, n_calls = 0, [], window, 0
    while pos < len(doc):
        end = min(len(doc), pos + w)
        got, base = check_parse(ctx, doc[pos:end], q, final=end == len(doc))
        n_calls += 1
        assert got["status"] in (_lib.TEXT_OK, _lib.TEXT_NO_RECORD), got["why"]
        if got["n_records"]:
            seqs += M.unpack(got["words"], got["nmask"], got["seq_len"])
        if got["consumed"][0] == 0 and end < len(doc):
            w *= 2
            continue
        pos += got["consumed"][0]
        w = window
    assert seqs == [M.norm(M.mask(r[2], r[3], q)) for r in recs] and n_calls > 3


def test_parse_with_a_limit(ctx):
    """stretches of one text (the records that START in front of the limit): the masked records concatenate to those of the whole"""
    rng = np.random.default_rng(8)
    doc = M.make_qdoc(rng, 900, crlf=True)
    recs = M.records(doc)
    q = 41
    for n_cuts in (1, 3, 8):
        nominal = sorted(int(x) for x in rng.integers(1, len(doc), size=n_cuts)) + [len(doc)]
        seqs, begin = [], 0
        for end in nominal:
            if begin >= len(doc):
                break
            hi = min(len(doc), end + 4096)
            got, base = check_parse(ctx, doc[begin:hi], q, final=hi == len(doc), limit=max(0, end - begin))
            assert got["status"] == _lib.TEXT_OK
            if got["n_records"]:
                seqs += M.unpack(got["words"], got["nmask"], got["seq_len"])
            begin += got["consumed"][0]
        assert begin == len(doc) and seqs == [M.norm(M.mask(r[2], r[3], q)) for r in recs], n_cuts


def test_setting_is_per_context_and_can_be_turned_off(ctx):
    """q = 0 after q > 0 on one context gives the image of a context that never had the setting; another context is not affected;
    q = 94 is refused and leaves the setting alone"""
    rng = np.random.default_rng(9)
    doc = M.make_qdoc(rng, 200)
    fresh = bonsai_amd.Context(0)
    try:
        fresh.set_encoder(31, None, canonicalize=True)
        plain = fresh.classify_text(doc, parse_only=True, want_words=True)
        ctx.set_min_base_quality(20)
        on = ctx.classify_text(doc, parse_only=True, want_words=True)
        other = fresh.classify_text(doc, parse_only=True, want_words=True)
        with pytest.raises(bonsai_amd.BonsaiAmdError):
            ctx.set_min_base_quality(94)
        still = ctx.classify_text(doc, parse_only=True, want_words=True)
        ctx.set_min_base_quality(0)
        off = ctx.classify_text(doc, parse_only=True, want_words=True)
    finally:
        ctx.set_min_base_quality(0)
        fresh.close()
    def image(a):                                                # (the words of the reads: slack words are not written, M.read_words)
        return M.read_words(a["words"], a["seq_len"]), M.read_words(a["nmask"], a["seq_len"])
    assert not np.array_equal(image(on)[1], image(plain)[1])
    for a in (other, off):
        assert np.array_equal(image(a)[0], image(plain)[0]) and np.array_equal(image(a)[1], image(plain)[1])
    assert np.array_equal(image(still)[0], image(on)[0]) and np.array_equal(image(still)[1], image(on)[1])
    recs = M.records(doc)
    assert M.unpack(off["words"], off["nmask"], off["seq_len"]) == [M.norm(r[2]) for r in recs]


# ---- classify level ---------------------------------------------------------------------------------------------------------------
Q = 20


@pytest.fixture(scope="module")
def world(oracle):
    w = synth.make_world(oracle, seed=21, k=31, genome_len=5000)
    w.oracle = oracle
    c = bonsai_amd.Context(0)
    c.set_encoder(31, None, canonicalize=True)
    c.load_table(w.n_buckets, w.flags, w.keys, w.vals)
    c.load_taxonomy(w.parent)
    w.ctx = c
    yield w
    c.set_min_base_quality(0)
    c.close()


def oracle_units(w, reads, quals, q, paired):
    """per unit: (taxon, missing, ambig, hits) of the oracle on the reads with low-quality bases replaced by 'N'"""
    sub = [M.mask(r.tobytes() if hasattr(r, "tobytes") else bytes(r), ql or b"", q) for r, ql in zip(reads, quals)]
    inc = 2 if paired else 1
    return [w.oracle.classify_seq(w.table, w.tax, 31, sub[u * inc], sub[u * inc + 1] if paired else None) for u in range(len(sub) // inc)]


def assert_bites(w, reads, quals, paired):
    """the quality model bites without wiping the reads out -- by the oracle alone: at least a tenth of the units differ from the unmasked
    run in taxon, missing or hits, and at least a tenth still have hits"""
    plain, masked = oracle_units(w, reads, quals, 0, paired), oracle_units(w, reads, quals, Q, paired)
    differ = sum(1 for a, b in zip(plain, masked) if a[0] != b[0] or a[1] != b[1] or not np.array_equal(a[3], b[3]))
    with_hits = sum(1 for b in masked if b[3].size)
    assert differ * 10 >= len(masked) and with_hits * 10 >= len(masked), (differ, with_hits, len(masked))
    return masked


def assert_units(w, got, exp, names, first_len, emit_all=True):
    n = len(exp)
    assert got["status"] == _lib.TEXT_OK and got["n_records"] in (n, 2 * n) and got["taxon"].size == n
    assert got["taxon"].tolist() == [e[0] for e in exp]
    assert got["missing"].tolist() == [e[1] for e in exp]
    assert got["ambig"].tolist() == [e[2] for e in exp]
    assert got["n_hits"].tolist() == [e[3].size for e in exp]
    lines = []
    for u, e in enumerate(exp):
        tax, ln = M.rle(e[3])                                    # (the ordered hits, as the runs the formatter prints)
        assert np.array_equal(got["runs"][u][0], tax) and np.array_equal(got["runs"][u][1], ln), u
        lines.append(w.oracle.kraken_line(names[u].decode(), e[0], first_len[u], e[1], e[2], e[3]) if (emit_all or e[0]) else b"")
    assert got["lines"] == b"".join(lines)
    assert np.array_equal(got["line_off"], np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.uint64))


def single_file(w, n=2500, seed=3):
    rng = np.random.default_rng(seed)
    reads = synth.simulate_reads(rng, w.genomes, n)
    reads[5] = reads[5][:10]
    reads[6] = reads[6][:0]
    reads[7] = reads[7][:33]
    quals = [M.illumina_qual(rng, r.size) for r in reads]
    for i in range(9, n, 10):                                    # every tenth record is FASTA: no quality, untouched
        quals[i] = None
    names = [b"read%d" % i for i in range(n)]
    return reads, quals, names


def test_classify_one_file(world):
    """one file: results, runs and the device's Kraken lines equal the oracle's on the substituted reads -- one slice, many 8 KiB slices,
    many batches; quality on one line and wrapped; classified units only"""
    w, c = world, world.ctx
    reads, quals, names = single_file(w)
    exp = assert_bites(w, reads, quals, False)
    lens = [r.size for r in reads]
    try:
        for wrap_seq, wrap_qual in ((0, 0), (60, 47)):
            doc = M.fastq_text(names, reads, quals, wrap_seq=wrap_seq, wrap_qual=wrap_qual)
            for dbg in (0, SLICE_8K, SLICE_8K | BATCH_TINY):
                c.debug_set(dbg)
                c.set_min_base_quality(Q)
                got = c.classify_text(doc, final=True, want_runs=True, want_lines=True)
                assert dbg == 0 or got["n_slices"] > 10
                assert_units(w, got, exp, names, lens)
        c.debug_set(0)
        got = c.classify_text(doc, final=True, want_runs=True, want_lines=True, emit_all=False)
        assert_units(w, got, exp, names, lens, emit_all=False)
        # the same call without the feature on the substituted text: the existing path agrees with the oracle, and with the feature
        c.set_min_base_quality(0)
        sub, _ = M.substituted_text(doc, Q)
        old = c.classify_text(sub, final=True, want_runs=True, want_lines=True, emit_all=False)
        assert old["lines"] == got["lines"] and np.array_equal(old["taxon"], got["taxon"])
        unmasked = c.classify_text(doc, final=True)
        assert np.count_nonzero((unmasked["missing"] != got["missing"]) | (unmasked["taxon"] != got["taxon"])) * 10 >= len(reads)
    finally:
        c.debug_set(0)
        c.set_min_base_quality(0)


def pair_files(w, n=1500, seed=4):
    rng = np.random.default_rng(seed)
    r1 = synth.simulate_reads(rng, w.genomes, n)
    r2 = [r[:int(rng.integers(40, len(r) + 1))] for r in synth.simulate_reads(rng, w.genomes, n)]
    q1 = [M.illumina_qual(rng, r.size) for r in r1]
    q2 = [M.illumina_qual(rng, r.size) if i % 3 else None for i, r in enumerate(r2)]      # (a FASTA mate beside a FASTQ mate is legal)
    return r1, r2, q1, q2


def test_classify_pair_of_files(world):
    """a pair: each mate masked by its own quality; every third second mate is a FASTA record"""
    w, c = world, world.ctx
    r1, r2, q1, q2 = pair_files(w)
    inter = [x for p in zip(r1, r2) for x in p]
    interq = [x for p in zip(q1, q2) for x in p]
    exp = assert_bites(w, inter, interq, True)
    names = [b"p%d" % i for i in range(len(r1))]
    d1 = M.fastq_text([b"p%d/1" % i for i in range(len(r1))], r1, q1)
    d2 = M.fastq_text([b"p%d/2" % i for i in range(len(r2))], r2, q2, wrap_seq=70, wrap_qual=33)
    try:
        for dbg in (0, SLICE_8K | BATCH_TINY):
            c.debug_set(dbg)
            c.set_min_base_quality(Q)
            got = c.classify_text([d1, d2], final=True, trim_readno=True, want_runs=True, want_lines=True)
            assert got["consumed"] == [len(d1), len(d2)] and got["n_records"] == 2 * len(r1)
            assert_units(w, got, exp, names, [r.size for r in r1])
    finally:
        c.debug_set(0)
        c.set_min_base_quality(0)


def test_classify_in_two_halves_and_from_device_text(world):
    """BNS_TEXT_DEFER + bns_text_finish (the mask is the first half's: turning the setting off in between changes nothing), text that is in
    HBM already, and both"""
    w, c = world, world.ctx
    reads, quals, names = single_file(w, n=2000, seed=5)
    exp = assert_bites(w, reads, quals, False)
    lens = [r.size for r in reads]
    doc = M.fastq_text(names, reads, quals)
    ptr = c.dev_alloc(len(doc) + 256)
    try:
        c.dev_upload(ptr, np.frombuffer(doc, dtype=np.uint8))
        for dbg in (0, SLICE_8K | BATCH_TINY):
            c.debug_set(dbg)
            for kw in (dict(defer=True), dict(device_ptrs=[(ptr, len(doc))]), dict(device_ptrs=[(ptr, len(doc))], defer=True)):
                c.set_min_base_quality(Q)
                if "defer" in kw and not dbg:
                    kw = dict(kw, between=lambda: c.set_min_base_quality(0))
                got = c.classify_text([] if "device_ptrs" in kw else doc, final=True, want_runs=True, want_lines=True, **kw)
                assert_units(w, got, exp, names, lens)
                if "first_half" in got:
                    assert got["first_half"]["n_records"] == len(reads)
    finally:
        c.debug_set(0)
        c.set_min_base_quality(0)
        c.dev_free(ptr)


def test_classify_with_confidence_and_tally(world):
    """the confidence walk and the tally see the masked image: both as the existing path gives them for the substituted text"""
    w, c = world, world.ctx
    reads, quals, names = single_file(w, n=2000, seed=6)
    assert_bites(w, reads, quals, False)
    doc = M.fastq_text(names, reads, quals)
    sub, _ = M.substituted_text(doc, Q)
    try:
        c.set_confidence(0.5)
        c.tally_enable(True)
        c.tally(reset=True)
        old = c.classify_text(sub, final=True, want_runs=True, want_lines=True)
        d0, c0 = c.tally(reset=True)
        unmasked = c.classify_text(doc, final=True)
        c.tally(reset=True)
        c.set_min_base_quality(Q)
        got = c.classify_text(doc, final=True, want_runs=True, want_lines=True)
        d1, c1 = c.tally(reset=True)
        assert got["status"] == _lib.TEXT_OK and got["n_records"] == len(reads)
        for k in ("taxon", "missing", "ambig", "n_hits"):
            assert np.array_equal(got[k], old[k]), k
        assert got["lines"] == old["lines"] and np.array_equal(got["line_off"], old["line_off"])
        assert np.array_equal(d0, d1) and np.array_equal(c0, c1) and int(d1.sum()) == len(reads)
        # (the threshold counts masked k-mers out of Q: the walk's outcome moves with the mask)
        assert np.count_nonzero(got["taxon"] != unmasked["taxon"]) > 0
        c.set_confidence(0)
        no_conf = c.classify_text(doc, final=True)
        assert np.count_nonzero(no_conf["taxon"] != got["taxon"]) > 0
    finally:
        c.set_confidence(0)
        c.tally_enable(False)
        c.set_min_base_quality(0)
