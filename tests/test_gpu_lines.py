"""Kraken lines assembled on the device (bns_classify_text with out->lines: lines_len_kernel / lines_write_kernel, csrc/bns_lines.hpp)
against (1) the reference's own append_kraken_classification bytes frozen in tests/golden/classify_ref.npz and (2) the checker's
kraken_line fed with the same call's results, at sizes and in corners the frozen vectors do not reach; then batches, capacities, device
text, the call in two halves, the confidence threshold and the tally."""
import os

import numpy as np
import pytest

import bonsai_amd
import synth
from bonsai_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
ABSENT = 0xFFFFFFFF
K = 31
BATCH_TINY, SLICE_8K = 0x40, 0x4000


# ---- 1. the reference's bytes ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def CL():
    return np.load(os.path.join(GOLD, "classify_ref.npz"))


def flat_parent(child, parent):
    p = np.full(int(max(child.max(), parent.max())) + 1, ABSENT, dtype=np.uint32)
    p[child] = parent
    p[1] = 0                       # build_parent_map forces the root (util.h:780-781)
    return p


def golden_texts(CL, paired):
    """the frozen reads as text, named as the CLI test of the frozen lines names them: r<u>, mate 2 r<u>_m; every 20th record FASTQ"""
    def qual(u, n):
        return bytes((33 + (i * 7 + u) % 40) for i in range(n))

    def rec(u, name, s):
        return (b"@%s\n%s\n+\n%s\n" % (name, s, qual(u, len(s)))) if u % 20 == 0 else (b">%s\n%s\n" % (name, s))

    if not paired:
        sb, so = CL["s_bases"], CL["s_offs"]
        return [b"".join(rec(u, b"r%d" % u, sb[int(so[u]):int(so[u + 1])].tobytes()) for u in range(so.size - 1))]
    pb, po = CL["p_bases"], CL["p_offs"]
    n = (po.size - 1) // 2
    d1 = b"".join(rec(u, b"r%d" % u, pb[int(po[2 * u]):int(po[2 * u + 1])].tobytes()) for u in range(n))
    d2 = b"".join(b">r%d_m\n%s\n" % (u, pb[int(po[2 * u + 1]):int(po[2 * u + 2])].tobytes()) for u in range(n))
    return [d1, d2]


def first_difference(a, b):
    n = min(len(a), len(b))
    x = np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8)
    bad = int(np.count_nonzero(x)) + abs(len(a) - len(b))
    at = int(np.argmax(x)) if x.any() else n
    return bad, at, a[max(0, at - 40):at + 40], b[max(0, at - 40):at + 40]


def assert_same_bytes(got, exp, what):
    if got != exp:
        bad, at, g, e = first_difference(got, exp)
        raise AssertionError("%s: %d bytes differ (lengths %d / %d), first at %d:\n got %r\n exp %r" % (what, bad, len(got), len(exp), at, g, e))


@pytest.mark.parametrize("layout", [bonsai_amd.LAYOUT_MINBUCKET, bonsai_amd.LAYOUT_BUCKET, bonsai_amd.LAYOUT_KHASH])
@pytest.mark.parametrize("paired", [False, True])
def test_lines_equal_the_reference_bytes(CL, layout, paired):
    """res["lines"] == the reference's append_kraken_classification output for the frozen reads, byte for byte; without emit_all the
    frozen lines of the classified units only (classifier.h:239); line_off cuts them where s_lines_offs / p_lines_offs does"""
    pre = "p_" if paired else "s_"
    lines, lo = CL[pre + "lines"].tobytes(), CL[pre + "lines_offs"]
    taxon = CL[pre + "res"][:, 0]
    c = bonsai_amd.Context(0)
    try:
        c.set_encoder(int(CL["k"]), None, canonicalize=True)
        c.load_table(int(CL["db_hdr"][0]), CL["db_flags"], CL["db_keys_arr"], CL["db_vals_arr"], layout=layout)
        c.load_taxonomy(flat_parent(CL["tax_child"], CL["tax_parent"]))
        texts = golden_texts(CL, paired)
        res = c.classify_text(texts, final=True, want_lines=True, emit_all=True)
        assert res["status"] == _lib.TEXT_OK and res["n_records"] == taxon.size * len(texts)
        assert np.array_equal(res["taxon"], taxon)
        assert_same_bytes(res["lines"], lines, "emit_all")
        assert np.array_equal(res["line_off"], lo.astype(np.uint64)) and res["lines_bytes"] == len(lines)
        only = b"".join(lines[int(lo[u]):int(lo[u + 1])] for u in range(taxon.size) if taxon[u])
        res = c.classify_text(texts, final=True, want_lines=True, emit_all=False)
        assert_same_bytes(res["lines"], only, "classified only")
        keep = np.where(taxon != 0, np.diff(lo.astype(np.int64)), 0)
        assert np.array_equal(res["line_off"], np.concatenate([[0], np.cumsum(keep)]).astype(np.uint64))
        assert 0 < len(only) < len(lines)
    finally:
        c.close()


# ---- 2. the checker, where the vectors do not reach -----------------------------------------------------------------------------
BIG_IDS = [4_000_000_001, 3_999_999_999, 4_294_967_294, 1_000_000_000]     # ten decimal digits; no key of the taxonomy (ids >= n)


@pytest.fixture(scope="module")
def world(oracle):
    """synth's six genomes and taxonomy, and in the same table: a 10 kb sequence whose k-mers alternate between two taxa (a run per
    k-mer), one that changes taxon every 97 k-mers, and 40-bp segments whose k-mers all carry one ten-digit id -- or the value 0 (printed
    'U') or 0xFFFFFFFF (printed 'A')"""
    w = synth.make_world(oracle, seed=23, k=K, genome_len=5000)
    rng = np.random.default_rng(77)
    w.alt = synth.rand_seq(rng, 10_000)
    w.slow = synth.rand_seq(rng, 10_000)
    w.segs = [synth.rand_seq(rng, 40) for _ in BIG_IDS]
    w.zero_seg, w.amb_seg = synth.rand_seq(rng, 40), synth.rand_seq(rng, 40)
    keys, vals = [], []
    e = oracle.encode(w.alt.tobytes(), K)
    keys.append(e); vals.append(np.where(np.arange(e.size) % 2 == 0, 1001, 2001))
    e = oracle.encode(w.slow.tobytes(), K)
    keys.append(e); vals.append(np.where((np.arange(e.size) // 97) % 2 == 0, 1003, 2002))
    for s, t in zip(w.segs + [w.zero_seg, w.amb_seg], BIG_IDS + [0, ABSENT]):
        e = oracle.encode(s.tobytes(), K)
        keys.append(e); vals.append(np.full(e.size, t))
    keys = np.concatenate(keys); vals = np.concatenate(vals).astype(np.uint32)
    assert np.unique(keys).size == keys.size
    w.table.insert_many(keys, vals)
    w.flags, w.keys, w.vals = w.table.arrays()
    w.n_buckets = w.table.n_buckets
    w.oracle = oracle
    c = bonsai_amd.Context(0)
    c.set_encoder(K, None, canonicalize=True)
    c.load_table(w.n_buckets, w.flags, w.keys, w.vals)
    c.load_taxonomy(w.parent)
    w.ctx = c
    yield w
    c.close()


def fastq(recs, eol=b"\n", fasta=False, wrap=0):
    out = []
    for name, s in recs:
        s = s.tobytes() if hasattr(s, "tobytes") else bytes(s)
        body = eol.join(s[j:j + wrap] for j in range(0, len(s), wrap)) if wrap and s else s
        if fasta:
            out.append(b">" + name + b" some comment" + eol + body + eol)
        else:
            out.append(b"@" + name + eol + body + eol + b"+" + eol + b"I" * len(s) + eol)
    return b"".join(out)


def trimmed(name):
    return name[:-2] if len(name) > 2 and name[-2:-1] == b"/" and name[-1:].isdigit() else name


def expected_lines(oracle, res, ns, emit_all):
    """per unit, the checker's kraken_line on what the SAME call returned: name and length of the first mate, taxon, missing, ambig and
    the hit stream expanded from its runs"""
    out = []
    for u in range(res["n_records"] // ns):
        t = int(res["taxon"][u])
        if not (emit_all or t):
            out.append(b"")
            continue
        tax, ln = res["runs"][u]
        out.append(oracle.kraken_line(res["names"][u * ns].decode("latin-1"), t, int(res["seq_len"][u * ns]), int(res["missing"][u]),
                                      int(res["ambig"][u]), np.repeat(tax, ln)))
    return out


def check_lines(oracle, res, ns, emit_all, what):
    exp = expected_lines(oracle, res, ns, emit_all)
    assert_same_bytes(res["lines"], b"".join(exp), what)
    off = np.concatenate([[0], np.cumsum([len(x) for x in exp])]).astype(np.uint64)
    assert np.array_equal(res["line_off"], off), what
    assert res["lines_bytes"] == int(off[-1])
    for u in (0, len(exp) // 2, len(exp) - 1):
        assert res["lines"][int(res["line_off"][u]):int(res["line_off"][u + 1])] == exp[u]
    return exp


def corner_records(w, rng):
    """(name, sequence) of every corner the issue lists; the simulated reads around them carry N (A: counts) and misses (M:, U runs)"""
    recs = [(b"r%d/1" % i, r) for i, r in enumerate(synth.simulate_reads(rng, w.genomes, 700, n_rate=0.004, var_len=True))]
    nohit = lambda n: synth.rand_seq(rng, n)                         # noqa: E731
    alln = lambda n: np.full(n, ord("N"), np.uint8)                  # noqa: E731
    g = w.genomes[1001]
    special = [(b"x", g[100:250]), (b"n" * 300 + b"/2", g[300:450]), (b"empty", np.zeros(0, np.uint8)), (b"short", g[:12]),
               (b"alt10k", w.alt), (b"slow10k", w.slow), (b"alt_rc", synth.revcomp(w.alt[:6000])),
               (b"big0", w.segs[0]), (b"big_mixed", np.concatenate([w.segs[1], w.segs[2], w.segs[3]])), (b"big3/1", w.segs[3]),
               (b"u_and_a_runs", np.concatenate([g[800:900], w.zero_seg, g[1000:1100], w.amb_seg, w.zero_seg, g[1200:1260]])),
               (b"only_u", w.zero_seg), (b"only_a", w.amb_seg),
               (b"some_N", np.concatenate([g[500:560], alln(1), g[561:700], alln(3), g[703:800]]))]
    special += [(b"miss%d" % n, nohit(n)) for n in (31, 50, 200, 2000, 20_000)]
    special += [(b"ambig%d" % n, alln(n)) for n in (31, 40, 130, 1030, 10_030)]
    special += [(b"mixN%d" % n, np.concatenate([alln(n), nohit(n + 30)])) for n in (35, 300)]
    for i, s in enumerate(special):
        recs.insert(13 + 29 * i, s)
    return recs


def digits(a):
    return {len(str(int(x))) for x in a if x}


def assert_coverage(res, crlf=False):
    """the call reached what this test is there for"""
    nr = np.array([r[0].size for r in res["runs"]])
    assert nr.max() > 4096 and np.any((nr > 64) & (nr <= 4096)) and np.any(nr == 0)
    assert digits(res["missing"]) >= {1, 2, 3, 4, 5} and digits(res["ambig"]) >= {1, 2, 3, 4, 5}
    assert digits(res["taxon"]) >= {4, 10} and np.any(res["taxon"] == 0)
    alltax = np.concatenate([r[0] for r in res["runs"]])
    assert np.any(alltax == 0) and np.any(alltax == ABSENT) and 10 in digits(alltax[alltax != ABSENT])
    cl = res["taxon"] != 0
    assert np.any(cl & (res["missing"] != 0)) and np.any(cl & (res["ambig"] != 0)) and np.any(~cl & (res["ambig"] != 0))
    # (CRLF text: the lone '\r' of an empty sequence line stays in the sequence, klib/kseq.h:135 -- length 1, not 0)
    assert (1 if crlf else 0) in res["seq_len"].tolist()
    nl = [len(n) for n in res["names"]]
    assert min(nl) == 1 and max(nl) > 255


@pytest.mark.parametrize("form", ["fastq", "fastq_crlf", "fasta_wrapped"])
@pytest.mark.parametrize("emit_all", [True, False])
def test_lines_equal_the_checker_single(world, form, emit_all):
    w, c = world, world.ctx
    recs = corner_records(w, np.random.default_rng(5))
    doc = fastq(recs, eol=b"\r\n" if form == "fastq_crlf" else b"\n", fasta=form == "fasta_wrapped", wrap=70 if form == "fasta_wrapped" else 0)
    res = c.classify_text(doc, final=True, trim_readno=True, want_runs=True, want_lines=True, emit_all=emit_all)
    assert res["status"] == _lib.TEXT_OK and res["n_records"] == len(recs)
    assert res["names"] == [trimmed(n) for n, _ in recs]
    assert_coverage(res, crlf=form == "fastq_crlf")
    exp = check_lines(w.oracle, res, 1, emit_all, form)
    assert emit_all or any(x == b"" for x in exp)
    # lines without the run arrays: the runs are made all the same
    alone = c.classify_text(doc, final=True, trim_readno=True, want_lines=True, emit_all=emit_all)
    assert "runs" not in alone
    assert_same_bytes(alone["lines"], res["lines"], "lines without run arrays")
    assert np.array_equal(alone["line_off"], res["line_off"])


@pytest.mark.parametrize("emit_all", [True, False])
def test_lines_equal_the_checker_paired(world, emit_all):
    """a pair's line: the FIRST mate's name and length, the unit's result and runs"""
    w, c = world, world.ctx
    r1 = corner_records(w, np.random.default_rng(6))
    r2 = [(n.replace(b"/1", b"/2") + b"_m", s) for n, s in corner_records(w, np.random.default_rng(7))][::-1]
    r2 = [(n, s[:max(0, len(s) - 7)]) for n, s in r2]
    d1, d2 = fastq(r1), fastq(r2, fasta=True, wrap=80)
    res = c.classify_text([d1, d2], final=True, trim_readno=True, want_runs=True, want_lines=True, emit_all=emit_all)
    assert res["status"] == _lib.TEXT_OK and res["n_records"] == 2 * len(r1)
    assert res["names"][0::2] == [trimmed(n) for n, _ in r1]
    assert np.any(res["seq_len"][0::2] != res["seq_len"][1::2])
    check_lines(w.oracle, res, 2, emit_all, "paired")


# ---- 3. batches and capacities ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many(world):
    rng = np.random.default_rng(9)
    reads = synth.simulate_reads(rng, world.genomes, 3000, n_rate=0.002)
    recs = [(b"read%d" % i, r) for i, r in enumerate(reads)]
    recs[40] = (b"alt10k", world.alt)                                # (a long line inside a small batch)
    doc = fastq(recs)
    one = world.ctx.classify_text(doc, final=True, want_runs=True, want_lines=True)
    assert one["status"] == _lib.TEXT_OK and one["n_records"] == len(recs) and one["n_launches"] == 1
    check_lines(world.oracle, one, 1, True, "one batch")
    return doc, recs, one


@pytest.mark.parametrize("emit_all", [True, False])
def test_lines_across_batches(world, many, emit_all):
    """many batches (a classify launch per >= 64 records) and many 8 KiB slices: the same bytes as the call in one batch"""
    doc, recs, one = many
    c = world.ctx
    ref = one if emit_all else c.classify_text(doc, final=True, want_lines=True, emit_all=False)
    try:
        for dbg in (SLICE_8K, SLICE_8K | BATCH_TINY):
            c.debug_set(dbg)
            got = c.classify_text(doc, final=True, want_lines=True, emit_all=emit_all)
            assert got["status"] == _lib.TEXT_OK and got["n_records"] == len(recs)
            assert got["n_launches"] > 10 if dbg & BATCH_TINY else got["n_launches"] == 1
            assert_same_bytes(got["lines"], ref["lines"], "dbg %#x" % dbg)
            assert np.array_equal(got["line_off"], ref["line_off"])
    finally:
        c.debug_set(0)


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("dbg", [0, SLICE_8K | BATCH_TINY])
def test_lines_cap_too_small(world, many, defer, dbg):
    """lines_cap one byte short: BNS_TEXT_CAP; the records, consumed[] and line bytes reported are those of the batches that fit -- a
    prefix of the full output that ends at a unit boundary -- and a call with room from consumed[] on delivers the rest"""
    doc, recs, one = many
    c = world.ctx
    full, off = one["lines"], one["line_off"]
    try:
        c.debug_set(dbg)
        got = c.classify_text(doc, final=True, want_lines=True, lines_cap=len(full) - 1, defer=defer)
        assert got["status"] == _lib.TEXT_CAP
        n = got["n_records"]
        assert n < len(recs) and (n > 0 if dbg else n == 0)
        if defer and not dbg:
            assert got["first_half"]["n_records"] == len(recs)       # (the first half had parsed them all; the second found no room)
        assert got["lines_bytes"] == int(off[n]) and got["lines"] == full[:int(off[n])]
        assert np.array_equal(got["line_off"], off[:n + 1])
        assert np.array_equal(got["taxon"], one["taxon"][:n])
        assert got["consumed"][0] == int(one["rec_pos"][n])
        rest = c.classify_text(doc[got["consumed"][0]:], final=True, want_lines=True, lines_cap=len(full) - int(off[n]), defer=defer)
        assert rest["status"] == _lib.TEXT_OK and rest["n_records"] == len(recs) - n
        assert_same_bytes(got["lines"] + rest["lines"], full, "two calls")
        exact = c.classify_text(doc, final=True, want_lines=True, lines_cap=len(full), defer=defer)
        assert exact["status"] == _lib.TEXT_OK
        assert_same_bytes(exact["lines"], full, "room to the byte")
    finally:
        c.debug_set(0)


# ---- 4. device text, two halves --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dbg", [0, SLICE_8K | BATCH_TINY])
def test_lines_device_text_and_two_halves(world, many, dbg):
    doc, recs, one = many
    c = world.ctx
    ptr = c.dev_alloc(len(doc) + 256)
    try:
        c.debug_set(dbg)
        c.dev_upload(ptr, np.frombuffer(doc, dtype=np.uint8))
        for kw in (dict(device_ptrs=[(ptr, len(doc))]), dict(defer=True), dict(device_ptrs=[(ptr, len(doc))], defer=True)):
            got = c.classify_text([] if "device_ptrs" in kw else doc, final=True, want_lines=True, **kw)
            assert got["status"] == _lib.TEXT_OK and got["n_records"] == len(recs)
            assert_same_bytes(got["lines"], one["lines"], str(sorted(kw)))
            assert np.array_equal(got["line_off"], one["line_off"])
    finally:
        c.debug_set(0)
        c.dev_free(ptr)


def test_lines_argument_errors(world):
    with pytest.raises(Exception):
        world.ctx.classify_text(b"@a\nAC\n+\nII\n", parse_only=True, want_lines=True)


# ---- 5. confidence and tally -----------------------------------------------------------------------------------------------------
def test_lines_follow_the_confidence_walk_and_leave_the_tally_alone(world, many):
    doc, recs, one = many
    c = world.ctx
    try:
        c.set_confidence(0.5)
        c.tally_enable(True)
        c.tally(reset=True)
        plain = c.classify_text(doc, final=True, want_runs=True)
        d0, c0 = c.tally(reset=True)
        got = c.classify_text(doc, final=True, want_runs=True, want_lines=True)
        d1, c1 = c.tally(reset=True)
        assert np.array_equal(d0, d1) and np.array_equal(c0, c1) and int(d0.sum()) == len(recs)
        assert np.array_equal(got["taxon"], plain["taxon"])
        changed = got["taxon"] != one["taxon"]
        assert np.count_nonzero(changed) > 0
        exp = check_lines(world.oracle, got, 1, True, "confidence 0.5")
        for u in np.nonzero(changed)[0][:50]:
            f = exp[u].split(b"\t")
            assert f[0] == (b"C" if got["taxon"][u] else b"U") and int(f[2]) == int(got["taxon"][u])
        # a rolled-back batch leaves the tally too: what fits is counted once
        c.debug_set(SLICE_8K | BATCH_TINY)
        part = c.classify_text(doc, final=True, want_lines=True, lines_cap=len(got["lines"]) // 2)
        d2, _ = c.tally(reset=True)
        n = part["n_records"]
        assert part["status"] == _lib.TEXT_CAP and 0 < n < len(recs) and int(d2.sum()) == n
        assert part["lines"] == got["lines"][:int(got["line_off"][n])]
    finally:
        c.debug_set(0)
        c.tally_enable(False)
        c.set_confidence(0)
