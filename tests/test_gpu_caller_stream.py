"""The nine entry points that take a `void *stream`, called the way bench.py and every torch caller call them: on a
torch.cuda.Stream of the caller's, the inputs produced on that stream immediately before the call, the device never drained in
between (the rule: include/bonsai_amd.h, "the `void *stream` argument").  Every scenario uses tests/stream_lib.py's late input: the
stream is busy for a calibrated 250 ms, the real input A lands behind the delay over a poison P (a valid input of the same geometry
whose answers differ), the call follows, its outputs are taken in stream order.  A step of the call enqueued anywhere but on the
caller's stream reads P, or a sentinel, or writes too late: a wrong answer, never a fault.  The expectation is the CPU oracle's (or
a numpy model's) of A, never the device's.

The control (the `env` fixture) gives the scenarios their power: the same set-up with the call on the library's own stream must
return expected(P) -- once through probe_device, once through classify_device, a multi-kernel call.  Where a candidate stream
returns expected(A) instead it shares a hardware queue with the context's stream; the next torch.cuda.Stream() is taken, four at
the most, and without an independent one the fixture fails.

What the technique cannot see: a call that synchronises the stream part-way (a read-back of a counter, a hipFree) has drained the
delay by then, so only the steps up to its first wait are held to the stream; the results are checked throughout.  Calls are
warmed up once on P, so that the late run enlarges (frees) no workspace buffer."""
from fractions import Fraction

import numpy as np
import pytest

import build_cases as bc
import classify_forms as F
import confidence_ref as CR
import minimize_model as mm
import sketch_model as SM
import stream_lib as SL
import synth
import taxonomy_ref as tr
from test_gpu_build import present_pairs
from test_gpu_build_session import check_table, khash_size
from test_gpu_windows_conf import Model as WindowsModel

pytestmark = pytest.mark.gpu

K, N_READS, READ_LEN = 31, 2048, 100
LAYOUT_KHASH, LAYOUT_BUCKET, LAYOUT_MINBUCKET = 0, 1, 2
SCORE_LEX = 0
THETA = Fraction(1, 10)
LEAVES_B = [1002, 1003, 1004, 2001, 2002, 1001]         # the taxids of the second genome set: the leaves, rotated


def can_overflow(nmates, max_read_len, c=K):
    """unit_can_overflow (bns_classify_plan.hpp) restated: the call then reads the overflow count back, i.e. waits for its stream"""
    return max_read_len >= c and nmates * (max_read_len - c + 1) > F.LDS_CAP


# ---- inputs and what the oracle says of them -------------------------------------------------------------------------------------
def make_reads(w, seed, n_rate=0.002):
    return synth.simulate_reads(np.random.default_rng(seed), w.genomes, N_READS, length=READ_LEN, n_rate=n_rate)


_EXPECT = {}


def expect_classify(oracle, w, tag, reads, paired):
    """{"taxon", "missing", "ambig", "n_hits": uint32 arrays, "hits": one array per unit}; once per (tag, paired)"""
    key = (tag, paired)
    if key not in _EXPECT:
        bases, offsets = synth.concat(reads)
        res = oracle.classify_batch(w.table, w.tax, w.k, bases, offsets, paired=paired, nthreads=8)
        inc = 2 if paired else 1
        hits = [oracle.classify_seq(w.table, w.tax, w.k, reads[u * inc].tobytes(), reads[u * inc + 1].tobytes() if paired else None)[3]
                for u in range(len(reads) // inc)]
        exp = {name: np.ascontiguousarray(res[name]) for name in ("taxon", "missing", "ambig", "n_hits")}
        assert all(h.size == n for h, n in zip(hits, exp["n_hits"]))
        exp["hits"] = hits
        _EXPECT[key] = exp
    return _EXPECT[key]


def differ_enough(a, p):
    """the condition on a poison: at least half of the units are called differently"""
    return float((a["taxon"] != p["taxon"]).mean()) >= 0.5


def check_units(got, exp, offsets, inc, taxon=None):
    """the five outputs as they stood on the stream behind the call against the oracle's, every unit; the hit stream where it is
    defined (n_hits entries from the unit's first base on)"""
    arrs = [SL.to_host(g, np.uint32) for g in got]
    want = dict(exp)
    if taxon is not None:
        want["taxon"] = taxon
    for name, a in zip(("taxon", "missing", "ambig", "n_hits"), arrs):
        bad = np.flatnonzero(a != want[name])
        assert bad.size == 0, "%s differs at %d units, first %s: got %s, expected %s" % (name, bad.size, bad[:6], a[bad[:6]], want[name][bad[:6]])
    at = np.concatenate([int(offsets[u * inc]) + np.arange(h.size, dtype=np.int64) for u, h in enumerate(exp["hits"])])
    bad = np.flatnonzero(arrs[4][at] != np.concatenate(exp["hits"]))
    assert bad.size == 0, "hit stream differs at %d entries" % bad.size


class Env:
    """the module's context, stream, delay and inputs"""

    def dev(self, a, pad=0):
        return SL.to_dev(self.torch, a, pad)

    def empty(self, n, dtype=None):
        return self.torch.zeros(int(n), dtype=dtype or self.torch.int32, device="cuda")

    def table(self, layout):
        """the world's own db in `layout`, the world's taxonomy"""
        w = self.w
        if self.tax_loaded != "world":
            self.ctx.load_taxonomy(w.parent)
            self.tax_loaded = "world"
        if self.loaded != layout:
            self.ctx.load_table(w.n_buckets, w.flags, w.keys, w.vals, layout=layout)
            self.loaded = layout


class ReadBatch:
    """reads A and their poison P, the same offsets: A and P resident, the offsets complete and never late, one buffer the call reads"""

    def __init__(self, e, reads_a, reads_p):
        ba, off = synth.concat(reads_a)
        bp, off_p = synth.concat(reads_p)
        assert np.array_equal(off, off_p)
        self.reads_a, self.n, self.total, self.offsets = reads_a, len(reads_a), int(off[-1]), off
        self.bases_a, self.bases_p = ba, bp
        self.d_off = e.dev(off)
        self.d_bases = e.empty(self.total + 8, e.torch.uint8)
        self.fills = [(self.d_bases[:self.total], e.dev(ba), e.dev(bp))]

    def outs(self, e, paired):
        nu = self.n // (2 if paired else 1)
        return [e.empty(nu) for _ in range(4)] + [e.empty(self.total)]


def classify_call(e, b, paired, max_len, outs):
    def call(stream):
        e.ctx.classify_device(b.d_bases.data_ptr(), b.d_off.data_ptr(), b.n, b.total, max_len, paired, *(o.data_ptr() for o in outs), stream=stream)
    return call


def probe_inputs(oracle, w):
    """4096 queries, half of them keys of the db: A and P present and absent at opposite positions, so every query differs in its
    found flag"""
    rng = np.random.default_rng(4096)
    keys, _ = bc.table_pairs(w.table)
    cand = np.unique(np.concatenate([oracle.encode(synth.rand_seq(rng, 3000).tobytes(), K) for _ in range(2)]))
    absent = cand[~np.isin(cand, keys)]
    assert absent.size >= 4096 and keys.size >= 4096
    pa, pp = rng.choice(keys, 2048, replace=False), rng.choice(keys, 2048, replace=False)
    aa, ap = absent[:2048], absent[2048:4096]
    where = rng.permutation(4096)
    a, p = np.zeros(4096, np.uint64), np.zeros(4096, np.uint64)
    a[where[:2048]], a[where[2048:]] = pa, aa
    p[where[:2048]], p[where[2048:]] = ap, pp
    ea, ep = w.table.get_batch(a), w.table.get_batch(p)
    assert int(ea[1].sum()) == 2048 and int(ep[1].sum()) == 2048 and (ea[1] != ep[1]).all()
    return a, p, ea, ep


def same_probe(got, exp):
    return np.array_equal(SL.to_host(got[0], np.uint32), exp[0]) and np.array_equal(SL.to_host(got[1], np.uint8), exp[1])


@pytest.fixture(scope="module")
def env(oracle, small_world):
    import torch                                           # (before the library maps its own HIP runtime: see conftest.py)
    assert torch.cuda.is_available()
    torch.cuda.init()
    torch.cuda.set_device(0)
    import bonsai_amd
    e = Env()
    e.torch, e.oracle, e.w, e.A = torch, oracle, small_world, bonsai_amd
    e.ctx = bonsai_amd.Context(0)
    try:
        e.loaded = e.tax_loaded = None
        e.ctx.set_encoder(K, None, canonicalize=True)
        e.table(LAYOUT_MINBUCKET)

        # ---- the inputs, and that every poison deserves the name
        w = small_world
        e.reads_a, e.reads_p = make_reads(w, 1), make_reads(w, 2)
        for paired in (False, True):
            assert differ_enough(expect_classify(oracle, w, "A", e.reads_a, paired), expect_classify(oracle, w, "P", e.reads_p, paired))
        e.batch = ReadBatch(e, e.reads_a, e.reads_p)
        rng = np.random.default_rng(77)
        e.genomes_a = [w.genomes[leaf] for leaf in synth.LEAVES]
        e.genomes_b = [synth.rand_seq(rng, g.size) for g in e.genomes_a]          # disjoint from the world's
        e.genomes_c = [synth.rand_seq(rng, g.size) for g in e.genomes_a]

        # ---- the delay, and a stream that runs independently of the context's own
        first = torch.cuda.Stream()
        e.delay = SL.Delay(torch, first)
        print("\ndelay: %s" % e.delay)
        qa, qp, exp_a, exp_p = probe_inputs(oracle, w)
        e.probe = (qa, qp, exp_a, exp_p)
        d_q, d_vals, d_found = e.empty(4096, torch.int64), e.empty(4096), e.empty(4096, torch.uint8)
        fills = [(d_q, e.dev(qa), e.dev(qp))]
        e.streams, e.late, seen = [], None, []
        for i in range(4):
            S = first if i == 0 else torch.cuda.Stream()
            e.streams.append(S)
            assert S.cuda_stream != 0
            late = SL.Late(torch, e.ctx, S, e.delay)
            got = late.control(fills, [d_vals, d_found], lambda st: e.ctx.probe_device(d_q.data_ptr(), 4096, d_vals.data_ptr(), d_found.data_ptr(), stream=st))
            if same_probe(got, exp_p):
                e.late, e.S = late, S
                print("stream: candidate %d of 4 (handle %#x); control through probe_device(stream=None): all 4096 queries answered as "
                             "expected(P)" % (i + 1, S.cuda_stream))
                break
            seen.append("candidate %d: %s" % (i + 1, "expected(A): serialised with the context's stream" if same_probe(got, exp_a) else "neither expected(A) nor expected(P)"))
            print("stream: " + seen[-1])
        if e.late is None:
            pytest.fail("delay / stream independence not established: " + "; ".join(seen))

        # ---- the same control through a multi-kernel call
        b = e.batch
        outs = b.outs(e, False)
        got = e.late.control(b.fills, outs, classify_call(e, b, False, READ_LEN, outs))
        check_units(got, expect_classify(oracle, w, "P", e.reads_p, False), b.offsets, 1)
        print("control through classify_device(stream=None): all %d units and their hit streams as expected(P)" % b.n)
        yield e
    finally:
        e.ctx.close()


@pytest.fixture(autouse=True)
def as_found(env):
    yield
    c = env.ctx
    c.build_end(); c.windows_end()
    c.set_timing(False); c.debug_set(0)
    c.set_confidence(0); c.tally_enable(False); c.sketch_enable(0)
    env.torch.cuda.synchronize()


# ---- 1. classify, the longest read known -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
@pytest.mark.parametrize("layout", [LAYOUT_MINBUCKET, LAYOUT_BUCKET], ids=["minbucket", "bucket"])
def test_classify_device(env, layout, paired):
    e, b = env, env.batch
    e.table(layout)
    outs = b.outs(e, paired)
    call = classify_call(e, b, paired, READ_LEN, outs)
    e.late.warm(b.fills, outs, call)
    got = e.late.run(b.fills, outs, call)
    print("host side of the call: %.2f ms, stream busy at return: %s" % (e.late.host_ms, e.late.busy_at_return))
    check_units(got, expect_classify(e.oracle, e.w, "A", e.reads_a, paired), b.offsets, 2 if paired else 1)
    # a single 100-base read holds 70 k-mers: no overflow count to read back, the call returns with its work queued; a pair holds
    # 140 (> 128): the call waits for the count
    assert can_overflow(2 if paired else 1, READ_LEN) == paired
    if not paired:
        assert e.late.busy_at_return


# ---- 2. classify, the longest read found on the device; the overflow pass ---------------------------------------------------------
@pytest.mark.parametrize("long_read", [False, True], ids=["reads-of-100", "one-read-of-5000"])
def test_classify_device_max_len_read_back(env, long_read):
    e, w = env, env.w
    e.table(LAYOUT_MINBUCKET)
    if long_read:
        ra, rp = list(e.reads_a), list(e.reads_p)
        ra[7], rp[7] = w.genomes[1003][500:5500].copy(), w.genomes[2001][700:5700].copy()
        b, tag = ReadBatch(e, ra, rp), "long"
        assert can_overflow(1, 5000)
    else:
        ra, b, tag = e.reads_a, e.batch, ""
    outs = b.outs(e, False)
    call = classify_call(e, b, False, 0, outs)
    e.late.warm(b.fills, outs, call)
    got = e.late.run(b.fills, outs, call)
    check_units(got, expect_classify(e.oracle, w, "A" + tag, ra, False), b.offsets, 1)
    # sixteen taxa: with the long read the overflow pass reads its count back, and finds no unit for classify_overflow_kernel
    # (test_classify_device_overflow_kernel has units for it)
    form = e.ctx.last_classify_form()
    assert form["kernel"] is not None and form["overflow_kernel"] is None and form["overflow_units"] == 0


def overflow_reads(segs, shift):
    """reads over classify_forms' 700 private segments, taken from `shift` on: runs of 64 to 300 segments (129 and more: past the
    cap of 128 distinct taxa) that hold their first segment twice -- that leaf outweighs the rest, so the unit is called there and
    every shift gives other calls --, single segments, and a run with an N"""
    s = segs[shift:] + segs[:shift]
    reads = [np.concatenate(s[20 * u:20 * u + n] + [s[20 * u]]) for u, n in enumerate((129, 130, 140, 200, 300, 128, 127, 64))]
    reads += [s[i].copy() for i in (500, 501, 502, 503)]
    r = np.concatenate(s[400:540] + [s[400]])
    r[1000] = ord("N")
    return [np.ascontiguousarray(x, dtype=np.uint8) for x in reads + [r]]


def test_classify_device_overflow_kernel(env):
    """units with more than 128 distinct taxa (classify_forms' world of 700 leaves): the overflow list is written by classify_kernel
    on the caller's stream, its count read back there, classify_overflow_kernel follows.  max_read_len is given, so the first wait
    is the one for the count: the classify kernel runs inside the delay."""
    e = env
    mw = F.world(e.oracle, K, True, None, "many")
    ra, rp = overflow_reads(mw.segs, 0), overflow_reads(mw.segs, 350)
    exp_a, exp_p = expect_classify(e.oracle, mw, "manyA", ra, False), expect_classify(e.oracle, mw, "manyP", rp, False)
    assert (exp_a["taxon"] != exp_p["taxon"]).all() and (exp_a["taxon"] >= 1000).all()
    over = sum(1 for h in exp_a["hits"] if np.unique(h).size > F.LDS_CAP)
    assert over == 6
    b = ReadBatch(e, ra, rp)
    max_len = max(r.size for r in ra)
    try:
        e.ctx.load_table(mw.n_buckets, mw.flags, mw.keys, mw.vals, layout=LAYOUT_MINBUCKET)
        e.ctx.load_taxonomy(mw.parent)
        e.loaded = e.tax_loaded = None
        geo = e.ctx.table_geometry()
        outs = b.outs(e, False)
        call = classify_call(e, b, False, max_len, outs)
        e.late.warm(b.fills, outs, call)
        got = e.late.run(b.fills, outs, call)
        check_units(got, exp_a, b.offsets, 1)
        form = e.ctx.last_classify_form()
        assert form["overflow_units"] == over and 1 <= form["overflow_grid"] <= over
        assert form["overflow_kernel"] == F.expected_overflow_form(None, LAYOUT_MINBUCKET, geo["identity_bits"], False)
    finally:
        e.table(LAYOUT_MINBUCKET)


# ---- 3. confidence, tally and sketches behind the classify kernel -----------------------------------------------------------------
def test_classify_device_confidence_tally_sketch(env):
    e, b, w, c = env, env.batch, env.w, env.ctx
    e.table(LAYOUT_MINBUCKET)
    exp = expect_classify(e.oracle, w, "A", e.reads_a, False)
    par = CR.parent_map(synth.TAX_PAIRS)
    taxon = np.array([CR.walk(par, THETA, t, m, h.tolist()) for t, m, h in zip(exp["taxon"], exp["missing"], exp["hits"])], dtype=np.uint32)
    assert 0 < int((taxon != exp["taxon"]).sum())                        # (the threshold moves some units up)
    want_sketch = SM.sketches(e.oracle, w.table, w.parent, e.reads_a, K)
    c.tally_enable(True)
    c.sketch_enable(64)
    c.set_confidence(THETA)
    outs = b.outs(e, False)
    call = classify_call(e, b, False, READ_LEN, outs)
    e.late.warm(b.fills, outs, call)
    c.tally(reset=True)                                                  # (what the warm-up counted of P)
    c.sketch(reset=True)
    got = e.late.run(b.fills, outs, call)
    assert e.late.busy_at_return
    check_units(got, exp, b.offsets, 1, taxon=taxon)
    # the stream is complete (Late.run waited for it): the readers work on the context's own
    dep = tr.depths(w.parent)
    want = np.bincount(tr.bins(w.parent, taxon, dep >= 0), minlength=w.parent.size + 1).astype(np.uint64)
    direct, clade = c.tally()
    assert np.array_equal(direct, want) and int(direct.sum()) == b.n     # A's units, nothing of P
    assert np.array_equal(clade, tr.clade_sums(w.parent, want, dep))
    bins, regs, dropped = c.sketch()
    assert bins.tolist() == want_sketch[0].tolist() and np.array_equal(regs, want_sketch[1]) and dropped == 0


# ---- 4. packed reads ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nmask", ["dense", "none"])
def test_classify_packed_device(env, nmask):
    e, w, torch = env, env.w, env.torch
    e.table(LAYOUT_MINBUCKET)
    if nmask == "dense":
        ra, rp, tag = e.reads_a, e.reads_p, ""
    else:
        ra, rp, tag = make_reads(w, 3, n_rate=0.0), make_reads(w, 4, n_rate=0.0), "noN"
    exp, exp_p = expect_classify(e.oracle, w, "A" + tag, ra, False), expect_classify(e.oracle, w, "P" + tag, rp, False)
    assert differ_enough(exp, exp_p)
    images = []
    for reads in (ra, rp):
        bases, offsets = synth.concat(reads)
        words, bw, bm = e.A.pack_reads(bases, offsets)
        dense = np.zeros(words.size, dtype=np.uint32)
        dense[bw.astype(np.int64)] = bm
        assert (bw.size > 0) == (nmask == "dense")
        images.append((words, dense))
    n, total = len(ra), int(offsets[-1])
    d_off = e.dev(offsets)
    d_words, d_nmask = e.empty(images[0][0].size + 2, torch.int64), e.empty(images[0][0].size + 2)
    nw = images[0][0].size
    fills = [(d_words[:nw], e.dev(images[0][0]), e.dev(images[1][0]))]
    if nmask == "dense":
        fills.append((d_nmask[:nw], e.dev(images[0][1]), e.dev(images[1][1])))
    outs = [e.empty(n) for _ in range(4)] + [e.empty(total)]

    def call(stream):
        e.ctx.classify_packed_device(d_words.data_ptr(), d_nmask.data_ptr() if nmask == "dense" else None, d_off.data_ptr(), n, total, READ_LEN, False,
                                     *(o.data_ptr() for o in outs), stream=stream)
    e.late.warm(fills, outs, call)
    got = e.late.run(fills, outs, call)
    assert e.late.busy_at_return
    check_units(got, exp, offsets, 1)


# ---- 5. probe -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [LAYOUT_MINBUCKET, LAYOUT_BUCKET, LAYOUT_KHASH], ids=["minbucket", "bucket", "khash"])
def test_probe_device(env, layout):
    e, torch = env, env.torch
    e.table(layout)
    qa, qp, exp_a, _ = e.probe
    d_q, d_vals, d_found = e.empty(4096, torch.int64), e.empty(4096), e.empty(4096, torch.uint8)
    fills = [(d_q, e.dev(qa), e.dev(qp))]

    def call(stream):
        e.ctx.probe_device(d_q.data_ptr(), 4096, d_vals.data_ptr(), d_found.data_ptr(), stream=stream)
    e.late.warm(fills, [d_vals, d_found], call)
    got = e.late.run(fills, [d_vals, d_found], call)
    assert e.late.busy_at_return
    assert np.array_equal(SL.to_host(got[1], np.uint8), exp_a[1])
    assert np.array_equal(SL.to_host(got[0], np.uint32), exp_a[0])


# ---- 6. encode ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [0, 50], ids=["every-kmer", "w50-lex"])
def test_encode_device(env, window):
    e, b, c, torch = env, env.batch, env.ctx, env.torch
    if window:
        want = [e.oracle.encode_windowed(r.tobytes(), K, window, SCORE_LEX) for r in e.reads_a]
        poison = [e.oracle.encode_windowed(r.tobytes(), K, window, SCORE_LEX) for r in e.reads_p[:64]]
    else:
        want = [e.oracle.encode(r.tobytes(), K) for r in e.reads_a]
        poison = [e.oracle.encode(r.tobytes(), K) for r in e.reads_p[:64]]
    assert all(not np.array_equal(x, y) for x, y in zip(want, poison))
    d_kmers, d_n = e.empty(b.total + 8, torch.int64), e.empty(b.n)

    def call(stream):
        c.encode_device(b.d_bases.data_ptr(), b.d_off.data_ptr(), b.n, b.total, d_kmers.data_ptr(), d_n.data_ptr(), stream=stream)
    try:
        if window:
            c.set_window(window, SCORE_LEX)
        e.late.warm(b.fills, [d_kmers, d_n], call)
        got = e.late.run(b.fills, [d_kmers, d_n], call)
        assert e.late.busy_at_return
    finally:
        c.set_encoder(K, None, canonicalize=True)            # (resets the window)
        e.loaded = None
    kmers, n_k = SL.to_host(got[0], np.uint64), SL.to_host(got[1], np.uint32)
    assert np.array_equal(n_k, np.array([x.size for x in want], dtype=np.uint32))
    for r, x in enumerate(want):                             # read by read
        o = int(b.offsets[r])
        assert np.array_equal(kmers[o:o + x.size], x), r


# ---- 7. the one-shot build ------------------------------------------------------------------------------------------------------------
def genome_fills(e, real, poison, real_tax, poison_tax):
    """-> d_bases, d_offsets, d_taxid, total, fills: bases and taxids late, the offsets in place"""
    ba, off = synth.concat([np.ascontiguousarray(g) for g in real])
    bp, off_p = synth.concat([np.ascontiguousarray(g) for g in poison])
    assert np.array_equal(off, off_p)
    total = int(off[-1])
    d_bases, d_tax = e.empty(total + 16, e.torch.uint8), e.empty(len(real))
    fills = [(d_bases[:total], e.dev(ba), e.dev(bp)),
             (d_tax, e.dev(np.asarray(real_tax, dtype=np.uint32)), e.dev(np.asarray(poison_tax, dtype=np.uint32)))]
    return d_bases, e.dev(off), d_tax, total, fills


def oracle_map(e, genomes, taxids):
    t = e.oracle.Table()
    for g, tx in zip(genomes, taxids):
        e.oracle.lca_map_add(t, e.w.tax, K, g.tobytes(), int(tx))
    return bc.table_pairs(t)


def test_build_table_device(env):
    e, c, torch = env, env.ctx, env.torch
    exp_keys, exp_vals = bc.table_pairs(e.w.table)
    nb = khash_size(exp_keys.size)
    d_bases, d_off, d_tax, total, fills = genome_fills(e, e.genomes_a, e.genomes_b, synth.LEAVES, LEAVES_B)
    outs = [e.empty(max(1, nb >> 4)), e.empty(nb, torch.int64), e.empty(nb)]
    hdrs = []

    def call(stream):
        hdrs.append(c.build_table_device(d_bases.data_ptr(), d_off.data_ptr(), 6, total, d_tax.data_ptr(), nb, *(o.data_ptr() for o in outs), stream=stream))
    e.late.warm(fills, outs, call)
    got = e.late.run(fills, outs, call)
    check_table(e.oracle, hdrs[-1], SL.to_host(got[0], np.uint32), SL.to_host(got[1], np.uint64), SL.to_host(got[2], np.uint32), exp_keys, exp_vals)


# ---- 8. table load --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def khash_arrays(env):
    """the khash arrays of two dbs of one size, built on the device: A from the world's genomes, P from disjoint random ones; each is
    the oracle's map (so what a probe of the loaded table must answer comes from the oracle)"""
    e, c, torch = env, env.ctx, env.torch
    nb = 1 << 16
    out = {"nb": nb}
    for tag, genomes, taxids in (("A", e.genomes_a, synth.LEAVES), ("P", e.genomes_b, LEAVES_B)):
        d_bases, d_off, d_tax, total, fills = genome_fills(e, genomes, genomes, taxids, taxids)
        arrs = [e.empty(nb >> 4), e.empty(nb, torch.int64), e.empty(nb)]
        fills[0][0].copy_(fills[0][1]); fills[1][0].copy_(fills[1][1])
        torch.cuda.synchronize()
        c.build_table_device(d_bases.data_ptr(), d_off.data_ptr(), 6, total, d_tax.data_ptr(), nb, *(a.data_ptr() for a in arrs))
        keys, vals = present_pairs(SL.to_host(arrs[0], np.uint32), SL.to_host(arrs[1], np.uint64), SL.to_host(arrs[2], np.uint32), nb)
        want = oracle_map(e, genomes, taxids)
        assert np.array_equal(keys, want[0]) and np.array_equal(vals, want[1])
        out[tag] = arrs
        out[tag + "_pairs"] = (keys, vals)
    assert not np.isin(out["P_pairs"][0], out["A_pairs"][0]).any()
    return out


@pytest.mark.parametrize("layout", [LAYOUT_KHASH, LAYOUT_BUCKET, LAYOUT_MINBUCKET], ids=["khash", "bucket", "minbucket"])
def test_load_table_device(env, khash_arrays, layout):
    """the arrays arrive late; a probe queued behind the load on the same stream answers from A's table, for A's keys and for P's.
    (A load frees the table it replaces, which drains the device: the delay holds the steps before that to the stream, the results
    hold the rest.)"""
    e, c, torch, ka = env, env.ctx, env.torch, khash_arrays
    nb = ka["nb"]
    queries = np.concatenate([ka["A_pairs"][0], ka["P_pairs"][0]])
    want = e.w.table.get_batch(queries)
    assert int(want[1].sum()) == ka["A_pairs"][0].size and np.array_equal(want[0][:ka["A_pairs"][0].size], ka["A_pairs"][1])
    d_q = e.dev(queries)
    table = [e.empty(nb >> 4), e.empty(nb, torch.int64), e.empty(nb)]
    fills = [(t, a, p) for t, a, p in zip(table, ka["A"], ka["P"])]
    outs = [e.empty(queries.size), e.empty(queries.size, torch.uint8)]

    def call(stream):
        c.load_table_device(nb, *(t.data_ptr() for t in table), layout=layout, stream=stream)
        c.probe_device(d_q.data_ptr(), queries.size, outs[0].data_ptr(), outs[1].data_ptr(), stream=stream)
    try:
        e.late.warm(fills, outs, call)
        got = e.late.run(fills, outs, call)
        assert np.array_equal(SL.to_host(got[1], np.uint8), want[1])
        assert np.array_equal(SL.to_host(got[0], np.uint32), want[0])
        assert c.table_info()["n_keys"] == ka["A_pairs"][0].size and c.table_info()["layout"] == layout
    finally:
        e.loaded = None
        e.table(LAYOUT_MINBUCKET)                            # (the borrowed arrays of the KHASH load are let go before they are freed)


# ---- 9. the build session and the minimizing pass ---------------------------------------------------------------------------------
def late_add(e, real, poison, real_tax, poison_tax):
    d_bases, d_off, d_tax, total, fills = genome_fills(e, real, poison, real_tax, poison_tax)
    e.late.run(fills, [], lambda st: e.ctx.build_add(d_bases.data_ptr(), d_off.data_ptr(), len(real), total, d_tax.data_ptr(), stream=st))


def test_build_session_adds(env):
    """two adds on the caller's stream into a table that starts at 4 buckets: it grows inside the streamed add"""
    e, c = env, env.ctx
    exp_keys, exp_vals = oracle_map(e, e.genomes_a + e.genomes_b, list(synth.LEAVES) + LEAVES_B)
    c.build_begin(4)
    late_add(e, e.genomes_a, e.genomes_c, synth.LEAVES, LEAVES_B)
    late_add(e, e.genomes_b, e.genomes_c, LEAVES_B, synth.LEAVES)
    hdr, flags, keys, vals = c.build_finish()
    stats = c.build_stats()
    c.build_end()
    check_table(e.oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
    assert stats["batches"] == 2 and stats["grows"] >= 10 and stats["keys"] == exp_keys.size


def test_build_minimize_add(env):
    """F holds the k-mers of both genome sets; the sequences of the first arrive late over those of the second -- all of them
    k-mers F knows --, so M is the selection over the first set's windows alone"""
    e, c = env, env.ctx
    w = e.w
    seqs = [g.tobytes() for g in e.genomes_a + e.genomes_b]
    taxids = list(synth.LEAVES) + LEAVES_B
    full = mm.full_map(e.oracle, w.tax, seqs, taxids, K)
    depth = mm.depths(w.parent)
    exp_keys, exp_vals = mm.sorted_pairs(mm.select(full, depth, seqs[:6], K, 50))
    other = mm.sorted_pairs(mm.select(full, depth, seqs[6:], K, 50))
    assert 0 < exp_keys.size < len(full) and not np.isin(other[0], exp_keys).all()
    c.build_begin(4)
    for genomes, tx in ((e.genomes_a, synth.LEAVES), (e.genomes_b, LEAVES_B)):
        d_bases, d_off, d_tax, total, fills = genome_fills(e, genomes, genomes, tx, tx)
        for dst, a, _ in fills:
            dst.copy_(a)
        e.torch.cuda.synchronize()
        c.build_add(d_bases.data_ptr(), d_off.data_ptr(), 6, total, d_tax.data_ptr())
    assert c.build_stats()["keys"] == len(full)
    c.build_minimize_begin(50, 4)
    d_bases, d_off, _, total, fills = genome_fills(e, e.genomes_a, e.genomes_b, synth.LEAVES, LEAVES_B)
    e.late.run(fills[:1], [], lambda st: c.build_minimize_add(d_bases.data_ptr(), d_off.data_ptr(), 6, total, stream=st))
    hdr, flags, keys, vals = c.build_finish()
    mstats = c.build_minimize_stats()
    c.build_end()
    check_table(e.oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
    assert mstats["batches"] == 1 and mstats["grows"] >= 8 and mstats["keys"] == exp_keys.size and mstats["scored_keys"] == len(full)


# ---- 10. the window session -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def windows_model(env):
    w = env.w
    return WindowsModel(env.oracle, w.table, w.tax, CR.parent_map(w.parent), env.genomes_a, list(synth.LEAVES), 150)


@pytest.mark.parametrize("theta", [0, THETA], ids=["plain", "confidence"])
def test_windows_add(env, windows_model, theta):
    """P: the same genomes one place on, under other taxids: other calls at (nearly) every base, other pairs throughout"""
    e, c = env, env.ctx
    e.table(LAYOUT_MINBUCKET)
    want_image, want_pairs = windows_model.at(theta)
    rot = e.genomes_a[1:] + e.genomes_a[:1]
    d_bases, d_off, d_tax, total, fills = genome_fills(e, e.genomes_a, rot, synth.LEAVES, LEAVES_B[1:] + LEAVES_B[:1])
    d_taxon = e.empty(total + 2)
    outs = [d_taxon[:total]]

    def call(stream):
        c.windows_add(d_bases.data_ptr(), d_off.data_ptr(), 6, total, d_tax.data_ptr(), d_taxon.data_ptr(), stream=stream)
    c.windows_begin(150, pair_cap=1 << 12, confidence=theta)
    e.late.warm(fills, outs, call)
    c.windows(reset=True)                                    # (the warm-up's pairs)
    got = e.late.run(fills, outs, call)
    assert e.late.busy_at_return                             # an untimed add returns with its work queued
    image = SL.to_host(got[0], np.uint32)
    assert np.array_equal(image, want_image), np.flatnonzero(image != want_image)[:5].tolist()
    seq, called, count, dropped = c.windows()
    assert dropped == 0 and all(np.array_equal(g, x) for g, x in zip((seq, called, count), want_pairs))
    c.windows_end()


# ---- 11. the timing events ------------------------------------------------------------------------------------------------------------
def test_timing_events_bracket_the_kernel_not_the_delay(env):
    e, b, c = env, env.batch, env.ctx
    e.table(LAYOUT_MINBUCKET)
    outs = b.outs(e, False)
    call = classify_call(e, b, False, READ_LEN, outs)
    e.late.warm(b.fills, outs, call)
    c.set_timing(True)
    got = e.late.run(b.fills, outs, call)
    ms = c.last_kernel_ms()
    print("last_kernel_ms: %.3f (delay %.1f ms)" % (ms, e.delay.ms))
    check_units(got, expect_classify(e.oracle, e.w, "A", e.reads_a, False), b.offsets, 1)
    assert 0 < ms < e.delay.ms
