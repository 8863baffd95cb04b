"""Low-complexity masking on a busy caller's stream: classify_device, classify_packed_device, build_add and build_minimize_add with
bns_set_dust on, held to the stream the call was given by tests/stream_lib.py's late input (the technique and its control are
described there and in tests/test_gpu_caller_stream.py).  The real input A lands behind a 250 ms delay over a poison P of the same
geometry; a pack, mark or apply launch enqueued anywhere but on the caller's stream works on P's image -- other tracts, another
mask -- and the answer is wrong.  The expectation is the CPU oracle's of substitute(A, dust_ref(A))."""
import numpy as np
import pytest

import build_cases as bc
import dust_world as DW
import minimize_model as mm
import stream_lib as SL
import synth
from test_gpu_build_session import check_table
from test_gpu_caller_stream import check_units, differ_enough

pytestmark = pytest.mark.gpu

K, N_READS, READ_LEN = 31, 1024, 100
W, T = DW.W, DW.T
LEAVES_B = [1002, 1003, 1004, 2001, 2002, 1001]


def expect(oracle, w, reads, paired=False):
    """the oracle on the substituted reads: per-unit arrays and the hit streams"""
    sub, masks = DW.substituted(reads)
    bases, offsets = synth.concat(sub)
    res = oracle.classify_batch(w.table, w.tax, K, bases, offsets, paired=paired, nthreads=8)
    exp = {name: np.ascontiguousarray(res[name]) for name in ("taxon", "missing", "ambig", "n_hits")}
    exp["hits"] = [oracle.classify_seq(w.table, w.tax, K, s.tobytes(), None)[3] for s in sub]
    exp["masked"] = sum(int(m.sum()) for m in masks) / sum(len(r) for r in reads)
    return exp


class Env:
    def dev(self, a, pad=0):
        return SL.to_dev(self.torch, a, pad)

    def empty(self, n, dtype=None):
        return self.torch.zeros(int(n), dtype=dtype or self.torch.int32, device="cuda")


@pytest.fixture(scope="module")
def env(oracle):
    import torch                                           # (before the library maps its own HIP runtime: see conftest.py)
    assert torch.cuda.is_available()
    torch.cuda.init()
    torch.cuda.set_device(0)
    import bonsai_amd
    e = Env()
    e.torch, e.oracle, e.A = torch, oracle, bonsai_amd
    e.w = w = DW.make_world(oracle, seed=51)
    e.ctx = c = bonsai_amd.Context(0)
    try:
        c.set_encoder(K, None, canonicalize=True)
        c.load_table(w.n_buckets, w.flags, w.keys, w.vals)
        c.load_taxonomy(w.parent)
        e.reads_a = synth.simulate_reads(np.random.default_rng(1), w.genomes, N_READS, length=READ_LEN, n_rate=0.002)
        e.reads_p = synth.simulate_reads(np.random.default_rng(2), w.genomes, N_READS, length=READ_LEN, n_rate=0.002)
        e.exp_a, e.exp_p = expect(oracle, w, e.reads_a), expect(oracle, w, e.reads_p)
        assert differ_enough(e.exp_a, e.exp_p) and e.exp_a["masked"] >= 0.05
        # (and the mask matters: the unmasked reads are called differently often enough)
        ba, off = synth.concat(e.reads_a)
        plain = oracle.classify_batch(w.table, w.tax, K, ba, off, nthreads=8)
        assert float(((plain["n_hits"] != e.exp_a["n_hits"]) | (plain["ambig"] != e.exp_a["ambig"])).mean()) >= 0.20
        e.genomes_a = [w.genomes[leaf] for leaf in synth.LEAVES]
        e.genomes_b = list(DW.tract_genomes(np.random.default_rng(77)).values())        # disjoint from the world's, tracts of their own
        e.genomes_c = list(DW.tract_genomes(np.random.default_rng(78)).values())

        # ---- the delay, and a stream that runs independently of the context's own: the control is the masked classify call itself
        bp, off_p = synth.concat(e.reads_p)
        assert np.array_equal(off, off_p)
        e.offsets, e.total = off, int(off[-1])
        e.d_off = e.dev(off)
        e.d_bases = e.empty(e.total + 8, torch.uint8)
        e.fills = [(e.d_bases[:e.total], e.dev(ba), e.dev(bp))]
        e.outs = [e.empty(N_READS) for _ in range(4)] + [e.empty(e.total)]
        first = torch.cuda.Stream()
        e.delay = SL.Delay(torch, first)
        e.late = None
        c.set_dust(W, T)
        for i in range(4):
            S = first if i == 0 else torch.cuda.Stream()
            late = SL.Late(torch, c, S, e.delay)
            got = late.control(e.fills, e.outs, classify_call(e))
            if np.array_equal(SL.to_host(got[3], np.uint32), e.exp_p["n_hits"]):
                check_units(got, e.exp_p, e.offsets, 1)
                e.late, e.S = late, S
                print("\nstream: candidate %d of 4; control through classify_device(stream=None) with masking on: expected(P)" % (i + 1))
                break
        c.set_dust(0)
        if e.late is None:
            pytest.fail("delay / stream independence not established")
        yield e
    finally:
        c.close()


@pytest.fixture(autouse=True)
def as_found(env):
    env.ctx.set_dust(W, T)
    yield
    env.ctx.build_end()
    env.ctx.set_dust(0)
    env.torch.cuda.synchronize()


def classify_call(e):
    def call(stream):
        e.ctx.classify_device(e.d_bases.data_ptr(), e.d_off.data_ptr(), N_READS, e.total, READ_LEN, False, *(o.data_ptr() for o in e.outs), stream=stream)
    return call


def test_classify_device(env):
    e = env
    call = classify_call(e)
    e.late.warm(e.fills, e.outs, call)
    got = e.late.run(e.fills, e.outs, call)
    print("host side of the call: %.2f ms, stream busy at return: %s" % (e.late.host_ms, e.late.busy_at_return))
    check_units(got, e.exp_a, e.offsets, 1)
    assert e.late.busy_at_return                              # 70 k-mers a read: nothing is read back, masking adds no wait
    assert e.ctx.last_classify_form()["kernel"][7] == 1


@pytest.mark.parametrize("nmask", ["dense", "none"])
def test_classify_packed_device(env, nmask):
    e, torch = env, env.torch
    if nmask == "dense":
        ra, rp, exp = e.reads_a, e.reads_p, e.exp_a
    else:
        ra = synth.simulate_reads(np.random.default_rng(3), e.w.genomes, N_READS, length=READ_LEN, n_rate=0.0)
        rp = synth.simulate_reads(np.random.default_rng(4), e.w.genomes, N_READS, length=READ_LEN, n_rate=0.0)
        exp = expect(e.oracle, e.w, ra)
        assert differ_enough(exp, expect(e.oracle, e.w, rp))
    images = []
    for reads in (ra, rp):
        bases, offsets = synth.concat(reads)
        words, bw, bm = e.A.pack_reads(bases, offsets)
        dense = np.zeros(words.size, dtype=np.uint32)
        dense[bw.astype(np.int64)] = bm
        assert (bw.size > 0) == (nmask == "dense")
        images.append((words, dense))
    nw = images[0][0].size
    d_words, d_nmask = e.empty(nw + 2, torch.int64), e.empty(nw + 2)
    fills = [(d_words[:nw], e.dev(images[0][0]), e.dev(images[1][0]))]
    if nmask == "dense":
        fills.append((d_nmask[:nw], e.dev(images[0][1]), e.dev(images[1][1])))
    outs = [e.empty(N_READS) for _ in range(4)] + [e.empty(e.total)]

    def call(stream):
        e.ctx.classify_packed_device(d_words.data_ptr(), d_nmask.data_ptr() if nmask == "dense" else None, e.d_off.data_ptr(), N_READS, e.total,
                                     READ_LEN, False, *(o.data_ptr() for o in outs), stream=stream)
    e.late.warm(fills, outs, call)
    got = e.late.run(fills, outs, call)
    assert e.late.busy_at_return
    check_units(got, exp, offsets, 1)
    # the caller's image as it was put there: never written
    assert np.array_equal(SL.to_host(d_words[:nw], np.uint64), images[0][0])
    if nmask == "dense":
        assert np.array_equal(SL.to_host(d_nmask[:nw], np.uint32), images[0][1])


def genome_fills(e, real, poison, real_tax, poison_tax):
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


def test_build_add(env):
    """two adds on the caller's stream into a table that starts at 4 buckets: the map of the substituted genomes"""
    e, c = env, env.ctx
    sub_a, _ = DW.substituted(e.genomes_a)
    sub_b, _ = DW.substituted(e.genomes_b)
    exp_keys, exp_vals = oracle_map(e, sub_a + sub_b, list(synth.LEAVES) + LEAVES_B)
    unmasked = oracle_map(e, e.genomes_a + e.genomes_b, list(synth.LEAVES) + LEAVES_B)[0].size
    assert exp_keys.size < unmasked
    c.build_begin(4)
    for real, tax, ptax in ((e.genomes_a, synth.LEAVES, LEAVES_B), (e.genomes_b, LEAVES_B, synth.LEAVES)):
        d_bases, d_off, d_tax, total, fills = genome_fills(e, real, e.genomes_c, tax, ptax)
        e.late.run(fills, [], lambda st: c.build_add(d_bases.data_ptr(), d_off.data_ptr(), len(real), total, d_tax.data_ptr(), stream=st))
    hdr, flags, keys, vals = c.build_finish()
    stats = c.build_stats()
    c.build_end()
    check_table(e.oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
    assert stats["batches"] == 2 and stats["keys"] == exp_keys.size


def test_build_minimize_add(env):
    """F holds the masked k-mers of both genome sets; the first set arrives late over the second, and M is the selection over the
    first set's masked windows alone"""
    e, c = env, env.ctx
    sub_a, _ = DW.substituted(e.genomes_a)
    sub_b, _ = DW.substituted(e.genomes_b)
    seqs = [g.tobytes() for g in sub_a + sub_b]
    taxids = list(synth.LEAVES) + LEAVES_B
    full = mm.full_map(e.oracle, e.w.tax, seqs, taxids, K)
    depth = mm.depths(e.w.parent)
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
    assert mstats["batches"] == 1 and mstats["keys"] == exp_keys.size and mstats["scored_keys"] == len(full)
