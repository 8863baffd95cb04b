"""GPU tier at NCBI scale: the per-taxon tally (tally_kernel, clade_scatter / clade_scan / clade_kernel), the confidence walk
(confidence_kernel, conf_required) and `bonsai classify -R / -t` on tests/taxonomy_ref.make_taxonomy's taxonomy -- 2.5 M keys, ids up
to 3.5 M, 5 M Euler positions, a chain 2 100 deep, a genus of 100 k species, a second root, a subtree whose chain breaks -- each held
against taxonomy_ref's plain restatements.  Every test first asserts that its data reaches the branch it is there for (scan tiles,
grid-stride rounds, LDS hash overflow, walk lengths, the 128-bit ceil), so that shrinking the data fails instead of losing coverage."""
import math
import re
import subprocess
import types
from fractions import Fraction

import numpy as np
import pytest

import bonsai_amd
import synth
import taxonomy_ref as tr
from bonsai_amd import _lib, hostio
from bonsai_amd.context import confidence_fraction
from test_gpu_cli import BIN
from test_gpu_confidence import THETAS
from test_gpu_report import fastq

pytestmark = pytest.mark.gpu

K = 31
SEG = 40                                   # template segments: 10 k-mers, all of one taxon
N_CU = 256                                 # MI355X: grid_for caps a grid at n_cu x blocks per CU (bns_api.hip)
TALLY_BLOCK, TALLY_SLOTS = 256, 1024       # tally_kernel (bns_tally.hpp)
SCAN_TILE = 1024 * 4                       # clade_scan_kernel: positions per tile
CLADE_ROUND = N_CU * 8 * 256               # clade_scatter / clade_kernel: ids per grid-stride round
CONF_ROUND = N_CU * 8 * 4 * 16             # confidence_kernel: blocks x waves x CONF_GROUP units per grid-stride round
CONF_CACHED_HITS = 4 * 64                  # confidence_kernel: the hits whose tin stays in registers
UPLOAD_SLICE = 64 << 20                    # bns_classify_batch: host batches go up in min(16, bytes / 64 MiB) slices


def tally_workgroups(n_units):
    """tally_units' launch: grid_for(n_units, TALLY_BLOCK * 16, 2) workgroups; unit i falls to workgroup (i / TALLY_BLOCK) % grid"""
    grid = max(1, min(-(-n_units // (TALLY_BLOCK * 16)), N_CU * 2))
    return grid, (np.arange(n_units) // TALLY_BLOCK) % grid


def fewest_bins_per_workgroup(b):
    grid, wg = tally_workgroups(b.size)
    pairs = np.unique((wg.astype(np.int64) << 32) | b.astype(np.int64))
    return int(np.bincount(pairs >> 32, minlength=grid).min())


def euler_positions(parent):
    """bns_load_taxonomy's clock + 1: two per forest id (every key, and every id that is a key's parent)"""
    parent = np.asarray(parent)
    forest = parent != tr.TAX_ABSENT
    forest[0] = False
    p = parent[forest]
    forest[p[p != 0]] = True
    return 2 * int(np.count_nonzero(forest)) + 1


def upload_slices(n_bytes):
    return min(16, max(1, n_bytes // UPLOAD_SLICE))


@pytest.fixture(scope="module")
def world(oracle):
    """the big taxonomy and one table: a 31-mer for each of ~300 k values (taxa all over the tree, the deep chain, the wide genus, the
    broken subtree, ids that are no key, ids >= n) and 40-bp segments of 10 k-mers of one taxon each for the confidence templates"""
    t = tr.make_taxonomy(0)
    w = types.SimpleNamespace(t=t, n=t.n, parent=t.parent, dep=tr.depths(t.parent))
    w.ok = w.dep >= 0
    rng = np.random.default_rng(41)
    n = t.n
    good = np.nonzero(w.ok)[0]
    w.vals = np.unique(np.concatenate([rng.choice(good, 280_000, replace=False), t.deep, t.wide_kids[:5000], t.broken, t.root2_nodes[:2000],
                                       rng.choice(t.non_keys, 2000, replace=False),
                                       [1, 1001, 2002, t.root2, t.missing_parent, n - 1, n, n + 5, (1 << 24) - 1, (1 << 28) + 1]])).astype(np.uint32)
    kmers = synth.rand_seq(rng, K * w.vals.size).reshape(-1, K)
    keys = oracle.encode(kmers.tobytes(), K)[::K]
    w.seg_tax = np.concatenate([t.deep, rng.choice(t.wide_kids, 800, replace=False), t.broken[:300], rng.choice(t.non_keys, 100, replace=False),
                                [n + 5, (1 << 28) + 1], rng.choice(good, 3000, replace=False), t.root2_nodes[:40]]).astype(np.uint32)
    w.segs = synth.rand_seq(rng, SEG * w.seg_tax.size).reshape(-1, SEG)
    enc = oracle.encode(w.segs.tobytes(), K)
    pos = (np.arange(w.seg_tax.size)[:, None] * SEG + np.arange(SEG - K + 1)).ravel()
    all_keys = np.concatenate([keys, enc[pos]])
    assert keys.size == w.vals.size and np.unique(all_keys).size == all_keys.size
    w.table = oracle.Table()
    w.table.insert_many(all_keys, np.concatenate([w.vals, np.repeat(w.seg_tax, SEG - K + 1)]))
    miss = synth.rand_seq(rng, K * 64).reshape(-1, K)                              # 31-mers no key holds
    _, found = w.table.get_batch(oracle.encode(miss.tobytes(), K)[::K])
    w.pool = np.concatenate([kmers, miss[found == 0]])                             # one 31-bp read per row
    w.pool_vals = np.concatenate([w.vals, np.zeros(int(np.count_nonzero(found == 0)), np.uint32)])
    w.row = {int(v): i for i, v in enumerate(w.vals.tolist())}
    b = tr.bins(w.parent, w.pool_vals, w.ok)
    w.ok_rows = np.nonzero((b != 0) & (b != n))[0]
    w.tax = oracle.Taxonomy(pairs=list(zip(t.keys.tolist(), t.parent[t.keys].tolist())))
    assert np.array_equal(w.tax.parent, t.parent)
    w.flags, w.tkeys, w.tvals = w.table.arrays()
    c = bonsai_amd.Context(0)
    w.ctx = c
    c.set_encoder(K, None, canonicalize=True)
    c.load_table(w.table.n_buckets, w.flags, w.tkeys, w.tvals)
    c.load_taxonomy(t.parent)
    yield w
    c.close()


def kmer_batch(w, rows):
    """31-bp reads, read i the k-mer of pool row rows[i] -> bases, offsets, the value each read classifies to"""
    bases = np.ascontiguousarray(w.pool[rows]).ravel()
    return bases, np.arange(rows.size + 1, dtype=np.uint64) * K, w.pool_vals[rows]


def check_tally(c, taxa, parent, dep, times=1):
    """the device's read-out (then reset) against np.bincount of the bins and clade_sums"""
    want = np.bincount(tr.bins(parent, taxa, dep >= 0), minlength=parent.size + 1).astype(np.uint64) * np.uint64(times)
    direct, clade = c.tally(reset=True)
    bad = np.nonzero(direct != want)[0]
    assert bad.size == 0, [(int(i), int(direct[i]), int(want[i])) for i in bad[:8]]
    wc = tr.clade_sums(parent, want, dep)
    bad = np.nonzero(clade != wc)[0]
    assert bad.size == 0, (bad.size, [(int(i), int(clade[i]), int(wc[i])) for i in bad[:8]])


def test_kmer_taxa_and_tally_at_scale(world):
    w, c = world, world.ctx
    rng = np.random.default_rng(5)
    n_units = 2_100_000
    rows = rng.integers(0, w.pool_vals.size, n_units)
    rows[:w.pool_vals.size] = rng.permutation(w.pool_vals.size)                  # (every value at least once)
    bases, offsets, want = kmer_batch(w, rows)
    b = tr.bins(w.parent, want, w.ok)
    # the data reaches what it is here for
    assert upload_slices(bases.size) == 1                                      # one classify launch, one tally launch
    assert fewest_bins_per_workgroup(b) > TALLY_SLOTS                          # every tally workgroup overflows its LDS hash into direct[]
    assert euler_positions(w.parent) > 1000 * SCAN_TILE                        # the scan carries across > 1000 tiles
    assert w.n + 1 > 6 * CLADE_ROUND                                           # clade_scatter / clade_kernel: several grid-stride rounds
    assert np.count_nonzero(b == 0) and np.count_nonzero(b == w.n) > 5000 and np.isin(w.t.broken, want).all()
    c.tally_enable()
    try:
        c.tally(reset=True)
        got = c.classify(bases, offsets)["taxon"]
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, [(int(i), int(got[i]), int(want[i])) for i in bad[:5]]       # first: the intended taxa
        check_tally(c, want, w.parent, w.dep)
        words, bw, bm = bonsai_amd.pack_reads(bases, offsets)
        assert np.array_equal(c.classify_packed(words, bw, bm, offsets)["taxon"], want)
        check_tally(c, want, w.parent, w.dep)
        ptrs = [c.dev_alloc(bases.size + 64), c.dev_alloc(offsets.nbytes), c.dev_alloc(n_units * 4)]
        try:
            c.dev_upload(ptrs[0], bases)
            c.dev_upload(ptrs[1], offsets)
            c.classify_device(ptrs[0], ptrs[1], n_units, bases.size, K, False, ptrs[2])
            c.sync()
            taxa = np.zeros(n_units, np.uint32)
            c.dev_download(ptrs[2], taxa)
            assert np.array_equal(taxa, want)
        finally:
            for p in ptrs:
                c.dev_free(p)
        check_tally(c, want, w.parent, w.dep)
    finally:
        c.tally_enable(False)


def test_tally_forced_collisions(world):
    """one workgroup: 48 taxa that hash to one LDS slot and one taxon for each of the 31 slots behind it -- at most 32 of the 48 find a
    slot, the others go to direct[] one by one"""
    w, c = world, world.ctx
    v = w.pool_vals[w.ok_rows].astype(np.uint64)
    slot = ((v * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(22)
    h = int(np.bincount(slot.astype(np.int64)).argmax())
    same = w.ok_rows[slot == h][:48]
    nxt = [w.ok_rows[slot == (h + k) % TALLY_SLOTS][0] for k in range(1, 32)]
    rows = np.concatenate([same, nxt])
    assert same.size >= 40 and rows.size == same.size + 31
    rng = np.random.default_rng(8)
    batch = rows[rng.integers(0, rows.size, 4096)]
    batch[:rows.size] = rows
    bases, offsets, want = kmer_batch(w, batch)
    assert tally_workgroups(batch.size)[0] == 1
    c.tally_enable()
    try:
        c.tally(reset=True)
        for _ in range(3):
            assert np.array_equal(c.classify(bases, offsets)["taxon"], want)
        check_tally(c, want, w.parent, w.dep, times=3)
    finally:
        c.tally_enable(False)


def test_tally_handed_back_batches(world, monkeypatch):
    """classify_text whose run arrays fill up (BNS_TEXT_CAP): the batch that did not fit is subtracted again, through the LDS hash and
    through direct[] -- every record its own bin, a batch per slice of 1 MiB (or the rest of the text), > 4 096 records each"""
    w, c = world, world.ctx
    rng = np.random.default_rng(12)
    rows = rng.permutation(w.ok_rows)[:150_000]
    _, _, want = kmer_batch(w, rows)
    assert np.unique(want).size == want.size
    doc = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, w.pool[j].tobytes(), b"I" * K) for i, j in enumerate(rows.tolist()))
    piece = 1 << 20
    per_piece = piece // (len(doc) // rows.size + 1)
    rec_max = len(b"@r%d\n" % (rows.size - 1)) + 2 * K + 4
    assert per_piece > 3 * 4096
    monkeypatch.setenv("BNS_TEXT_PIECE_MB", "1")
    c.tally_enable()
    c.debug_set(0x40)                                                          # (a classify launch per slice)
    try:
        c.tally(reset=True)
        pos, done, capped, cap = 0, 0, 0, 2 * per_piece + per_piece // 2
        while pos < len(doc):
            rest = len(doc) - pos
            part = c.classify_text(doc[pos:], final=True, want_runs=True, runs_cap=cap, cap_records=rows.size - done + 16, names_cap=rest + 16)
            nr = part["n_records"]
            assert np.array_equal(part["taxon"], want[done:done + nr])
            if part["status"] == _lib.TEXT_CAP:
                capped += 1
                # the batch handed back is the next slice: up to the end of the next piece, or of the text -- at least `back` records
                back = (min(rest - part["consumed"][0], piece) - rec_max) // rec_max
                assert back > 4096 and fewest_bins_per_workgroup(want[done + nr:done + nr + back]) > TALLY_SLOTS
            done += nr
            pos += part["consumed"][0]
            if nr == 0:
                cap *= 2
        assert done == rows.size and capped >= 3
        check_tally(c, want, w.parent, w.dep)
    finally:
        c.debug_set(0)
        c.tally_enable(False)


def test_tally_across_reloads(world, small_world):
    """small -> big -> a sparse copy of ids up to 2^24 - 1 -> small: every read-out exact, every taxonomy's tally from zero"""
    w, c = world, world.ctx
    sparse = np.full(1 << 24, tr.TAX_ABSENT, np.uint32)
    sparse[:w.n] = w.parent
    sparse[(1 << 24) - 1] = 1
    rng = np.random.default_rng(13)
    rows = rng.integers(0, w.pool_vals.size, 300_000)
    special = [w.row[x] for x in ((1 << 24) - 1, w.n, w.n + 5, (1 << 28) + 1, w.t.missing_parent, 1001, 2002)] + [w.pool_vals.size - 1]
    rows[:len(special)] = special
    bases, offsets, want = kmer_batch(w, rows)
    c.tally_enable()
    try:
        for parent in (small_world.parent, w.parent, sparse, small_world.parent):
            c.load_taxonomy(parent)
            d0, c0 = c.tally()
            assert d0.size == parent.size + 1 and not d0.any() and not c0.any()
            assert np.array_equal(c.classify(bases, offsets)["taxon"], want)
            dep = w.dep if parent is w.parent else tr.depths(parent)
            assert 0 < np.count_nonzero(tr.bins(parent, want, dep >= 0) == parent.size) < want.size
            check_tally(c, want, parent, dep)
            c.classify(bases, offsets)                                         # (counted, never read: the next load drops it)
    finally:
        c.load_taxonomy(w.parent)
        c.tally_enable(False)


def test_tally_past_2_32(world):
    """2^24 one-k-mer reads of the deepest taxon, 257 launches: every count on its 2 100-node chain is 257 * 2^24 > 2^32"""
    w, c = world, world.ctx
    t = int(w.t.deep[-1])
    n_reads, times = 1 << 24, 257
    total = times * n_reads
    up = tr.up_chain(w.parent, t)
    assert total > 1 << 32 and len(up) > 2000
    bases = np.tile(w.pool[w.row[t]], n_reads)
    offsets = np.arange(n_reads + 1, dtype=np.uint64) * K
    ptrs = [c.dev_alloc(bases.size + 64), c.dev_alloc(offsets.nbytes), c.dev_alloc(n_reads * 4)]
    c.tally_enable()
    try:
        c.dev_upload(ptrs[0], bases)
        c.dev_upload(ptrs[1], offsets)
        for _ in range(times):
            c.classify_device(ptrs[0], ptrs[1], n_reads, n_reads * K, K, False, ptrs[2])
        c.sync()
        taxa = np.zeros(n_reads, np.uint32)
        c.dev_download(ptrs[2], taxa)
        assert (taxa == t).all()
        direct, clade = c.tally(reset=True)
        assert int(direct[t]) == total and int(direct.sum()) == total
        assert (clade[up] == total).all() and np.count_nonzero(clade) == len(up)
    finally:
        for p in ptrs:
            c.dev_free(p)
        c.tally_enable(False)


# ---- the confidence walk


@pytest.fixture(scope="module")
def templates(world, oracle):
    """~3 000 units built from the table's 40-bp segments, each with the oracle's (taxon, missing, ambig, hits) and the fast walker"""
    w = world
    rng = np.random.default_rng(21)
    nd = w.t.deep.size
    wide = nd + np.arange(800)
    odd = nd + 800 + np.arange(402)                                            # broken subtree, ids that are no key, ids >= n
    good = nd + 1202 + np.arange(3000)
    groups = []
    # one segment near the bottom of the deep chain, then 26-40 far above it (deepest first): > 256 hits, walks of >= 500 steps
    for _ in range(36):
        bottom = int(rng.integers(1900, nd))
        body = np.sort(rng.choice(np.arange(300, bottom - 500), size=int(rng.integers(26, 41)), replace=False))[::-1]
        groups.append(("deep", [bottom] + body.tolist()))
    for _ in range(150):
        groups.append(("chain", rng.choice(nd, size=int(rng.integers(1, 6))).tolist()))
    for _ in range(600):                                                       # (one species twice or more: T is that species)
        r = rng.choice(wide, size=int(rng.integers(1, 5)), replace=False).tolist()
        groups.append(("wide", r[:1] * int(rng.integers(1, 4)) + r[1:]))
    for _ in range(300):
        r = rng.choice(odd, size=int(rng.integers(1, 3))).tolist() + rng.choice(good, size=int(rng.integers(0, 3))).tolist()
        groups.append(("odd", rng.permutation(r).tolist()))
    for _ in range(1874):
        groups.append(("good", rng.choice(good, size=int(rng.integers(1, 6))).tolist()))
    groups += [("root2", [int(good[-1]) + 1 + i]) for i in range(40)]           # (below the second root)
    tp = types.SimpleNamespace(kinds=[g[0] for g in groups], seqs=[np.ascontiguousarray(w.segs[r].ravel()) for _, r in groups])
    tp.units = [oracle.classify_seq(w.table, w.tax, K, s.tobytes()) for s in tp.seqs]
    tp.walkers = [tr.walker(w.parent, u[0], u[1], u[3]) for u in tp.units]
    pairs = [(rng.choice(good, size=int(rng.integers(1, 4))), rng.choice(np.concatenate([good, wide, odd]), size=int(rng.integers(1, 4))))
             for _ in range(400)]
    tp.pair_seqs = [(np.ascontiguousarray(w.segs[a].ravel()), np.ascontiguousarray(w.segs[b].ravel())) for a, b in pairs]
    tp.pair_units = [oracle.classify_seq(w.table, w.tax, K, a.tobytes(), b.tobytes()) for a, b in tp.pair_seqs]
    tp.pair_walkers = [tr.walker(w.parent, u[0], u[1], u[3]) for u in tp.pair_units]
    return tp


def steps_of(f, th):
    r = f(th)
    return f.up.index(r) if f.up and r in f.up else -1


def long_path_thetas(tp, rng):
    """thetas whose terms take conf_required's 128-bit long division: c/Q +- 1/(Q 2^40) (R must be c + 1 above, c below), the same
    with a reduced den in (2^63, 2^64) (the division's top bit), 0.37 over the largest prime below 2^64, and 1/(2^64 - 1)"""
    out = []
    deep = [f for f, k in zip(tp.walkers, tp.kinds) if k == "deep"]
    for f in [deep[i] for i in rng.choice(len(deep), 4, replace=False)]:
        c, q = f.counts[len(f.counts) // 2 + 1], f.q
        assert 0 < c < q
        m = (1 << 63) // q + 1
        for mult in (1 << 40, None):
            for s in (1, -1):
                while True:
                    mm = mult or m
                    th = Fraction(c * mm + s, q * mm)
                    if mult or (1 << 63) < th.denominator < (1 << 64):
                        break
                    m += 1
                assert math.ceil(th * q) == (c + 1 if s > 0 else c)
                num, den = confidence_fraction(th)
                assert num >= 1 << 31 and (mult or den > 1 << 63)            # (the long path; its top bit for the second kind)
                out.append(th)
    p = 2 ** 64 - 59
    out += [Fraction(p * 37 // 100, p), Fraction(1, 2 ** 64 - 1)]
    return out


def test_confidence_at_scale(world, templates):
    w, c, tp = world, world.ctx, templates
    rng = np.random.default_rng(33)
    n_t = len(tp.seqs)
    n_units = 600_011
    idx = rng.integers(0, n_t, n_units)
    idx[:n_t] = rng.permutation(n_t)
    bases, offsets = synth.concat([tp.seqs[i] for i in idx])
    deep = [i for i, k in enumerate(tp.kinds) if k == "deep"]
    boundary = sorted({Fraction(x, tp.walkers[i].q) for i in deep for x in tp.walkers[i].counts if 0 < x < tp.walkers[i].q})
    boundary = [boundary[i] for i in sorted(rng.choice(len(boundary), 12, replace=False))]
    long_th = long_path_thetas(tp, rng)
    thetas = THETAS + boundary + long_th
    core = {Fraction("0.25"), boundary[3], long_th[0], long_th[2], long_th[-2]}
    # the data reaches what it is here for
    assert n_units % 16 and n_units // upload_slices(bases.size) > 4 * CONF_ROUND       # the group loop runs > 4 rounds per launch
    far = [i for i in deep if tp.units[i][3].size > CONF_CACHED_HITS and max(steps_of(tp.walkers[i], th) for th in thetas) >= 500]
    assert len(far) >= 20                                                     # long walks that count uncached hits at every step
    assert max(tp.walkers[i].q for i in deep) < 4000 and max(len(tp.walkers[i].up) for i in deep) > 2000
    kinds = {k: [i for i, x in enumerate(tp.kinds) if x == k] for k in set(tp.kinds)}
    assert sum(tp.walkers[i](Fraction(1, 4)) == w.t.wide != tp.units[i][0] for i in kinds["wide"]) > 50      # up to the wide genus
    assert any(tp.walkers[i].up is None and tp.units[i][0] for i in kinds["odd"])          # a broken or outside T: stays
    assert any(h >= w.n for i in kinds["odd"] for h in tp.units[i][3].tolist())
    words, bw, bm = bonsai_amd.pack_reads(bases, offsets)
    base = c.classify(bases, offsets)
    assert np.array_equal(base["taxon"], np.array([u[0] for u in tp.units], np.uint32)[idx])
    assert np.array_equal(base["n_hits"], np.array([u[3].size for u in tp.units], np.uint32)[idx])
    doc = fastq([tp.seqs[i] for i in idx])
    changed = {}
    c.tally_enable()
    try:
        c.tally(reset=True)
        for th in thetas:
            c.set_confidence(th)
            want = np.array([f(th) for f in tp.walkers], np.uint32)[idx]
            runs = [("classify", c.classify(bases, offsets)["taxon"])]
            if th in core:
                got = c.classify(bases, offsets, want_hits=True)
                assert all(np.array_equal(got["hits"][j], tp.units[idx[j]][3]) for j in range(0, n_units, 997))
                runs.append(("hits", got["taxon"]))
                runs.append(("packed", c.classify_packed(words, bw, bm, offsets)["taxon"]))
                got = c.classify_text(doc, final=True, cap_records=n_units + 16, names_cap=len(doc) + 16)
                assert got["n_records"] == n_units
                runs.append(("text", got["taxon"]))
                c.debug_set(0x4000)
                try:
                    runs.append(("sliced", c.classify(bases, offsets)["taxon"]))
                finally:
                    c.debug_set(0)
            for tag, got in runs:
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, (th, tag, bad.size, [(int(idx[u]), tp.kinds[idx[u]], int(got[u]), int(want[u])) for u in bad[:5]])
            direct, _ = c.tally(reset=True)
            wd = np.bincount(tr.bins(w.parent, want, w.ok), minlength=w.n + 1).astype(np.uint64) * np.uint64(len(runs))
            assert np.array_equal(direct, wd), th
            changed[th] = int(np.count_nonzero(want != base["taxon"]))
    finally:
        c.set_confidence(0)
        c.tally_enable(False)
    assert changed[Fraction(1, 2)] > n_units // 10 and all(changed[th] for th in long_th[:-1])


def test_confidence_pairs_at_scale(world, templates):
    w, c, tp = world, world.ctx, templates
    rng = np.random.default_rng(35)
    n_p = len(tp.pair_seqs)
    n_units = 140_003
    idx = rng.integers(0, n_p, n_units)
    idx[:n_p] = rng.permutation(n_p)
    bases, offsets = synth.concat([s for i in idx for s in tp.pair_seqs[i]])
    assert n_units > CONF_ROUND and upload_slices(bases.size) == 1
    base = c.classify(bases, offsets, paired=True)["taxon"]
    assert np.array_equal(base, np.array([u[0] for u in tp.pair_units], np.uint32)[idx])
    try:
        for th in THETAS + long_path_thetas(tp, rng)[:4]:
            c.set_confidence(th)
            want = np.array([f(th) for f in tp.pair_walkers], np.uint32)[idx]
            for wh in (False, True):
                got = c.classify(bases, offsets, paired=True, want_hits=wh)["taxon"]
                assert np.array_equal(got, want), (th, wh, int(np.count_nonzero(got != want)))
    finally:
        c.set_confidence(0)


# ---- the CLI


def test_cli_taxa_and_report_at_scale(world, templates, tmp_path):
    """nodes.dmp / names.dmp of the big taxonomy, its db, 300 k template reads: `-K -b -R -n` with and without -t 0.37, one context
    and two -- the taxa as walked, the report byte for byte as taxonomy_ref restates it"""
    w, tp = world, templates
    nodes, names, db, fq = (str(tmp_path / x) for x in ("nodes.dmp", "names.dmp", "big.db", "reads.fq"))
    tr.write_dmps(w.t, nodes, names)
    h = w.table.header()                                                       # (n_buckets, size, n_occupied, upper_bound)
    hostio.write_db(db, K, K, None, [h[0], h[2], h[1], h[3]], w.flags, w.tkeys, w.tvals)
    rng = np.random.default_rng(37)
    n_t = len(tp.seqs)
    idx = rng.integers(0, n_t, 300_000)
    idx[:n_t] = rng.permutation(n_t)
    with open(fq, "wb") as f:
        f.write(fastq([tp.seqs[i] for i in idx]))
    for th in (None, "0.37"):
        want = np.array([f(Fraction(th)) if th else u[0] for f, u in zip(tp.walkers, tp.units)], np.uint32)[idx]
        report = tr.report_from_taxa(want, w.parent, w.t.ranks, w.t.names)
        assert report.count("\n") > 5000 and "\t(not in taxonomy)\n" in report and ("\tunclassified\n" in report) == bool(th)
        assert re.search(r"\tS\d{3,}\t", report) and "\t-\t%d\t" % w.t.root2 in report               # (the deep chain, the second root)
        for devs in ("0", "0,0"):
            tb, rp = str(tmp_path / "t.bin"), str(tmp_path / "t.report")
            p = subprocess.run([BIN, "classify", "-K", "-g", devs, "-b", tb, "-R", rp, "-n", names] + (["-t", th] if th else []) + [db, nodes, fq],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            assert p.returncode == 0, p.stderr.decode()
            got = np.fromfile(tb, dtype="<u4")
            assert np.array_equal(got, want), (th, devs, int(np.count_nonzero(got != want)))
            assert open(rp, encoding="utf-8").read() == report, (th, devs)
