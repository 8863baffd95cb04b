"""Fewest-genome minimizers on the device (bns_build_count_begin / _add / _get / _stats, bns_build_minimize_begin_score): a build
session that scored every k-mer (F) streams its sequences again with the genome id of each, counts per k-mer the distinct genomes
that hold it, and a third stream keeps, from every window, the k-mer the fewest genomes hold.  The expected counts and table are the
model's (tests/fewest_model.py: the oracle's F, plain sets of ids, the rule as DESIGN.md states it), never the device's."""
import numpy as np
import pytest

import bonsai_amd
import dust_world as DW
import fewest_model as fm
import minimize_model as mm
import synth
from test_fewest_model import PAIRS8, rule_input
from test_gpu_build import present_pairs
from test_gpu_build_minimize import configure, minimize_batch, run_minimize
from test_gpu_build_session import add_batch, check_table, khash_size
from test_gpu_caller_stream import K, LEAVES_B, as_found, env, genome_fills  # noqa: F401  (the fixtures of the stream pattern)
from test_minimize_model import BY_NAME, FORMS, world_of

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_TABLE = -1, -4, -7              # include/bonsai_amd.h
NO_ID = 0xFFFFFFFF


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.build_end()                                  # (a test that failed inside a session must not leave it to the next module)
    gpu_ctx.set_dust(0)
    gpu_ctx.set_encoder(31, None, canonicalize=True)


def count_batch(ctx, seqs, ids):
    """one bns_build_count_add: the sequences uploaded, counted under their genome ids, freed"""
    arrs = [np.ascontiguousarray(np.frombuffer(s, dtype=np.uint8) if isinstance(s, bytes) else s) for s in seqs]
    bases, offsets = synth.concat(arrs)
    pad = (-bases.size) % 8 + 8
    d_bases = ctx.dev_alloc(bases.size + pad); d_off = ctx.dev_alloc(offsets.nbytes)
    try:
        ctx.dev_upload(d_bases, bases); ctx.dev_upload(d_off, offsets)
        ctx.build_count_add(d_bases, d_off, len(arrs), int(offsets[-1]), ids)
    finally:
        for p in (d_bases, d_off):
            ctx.dev_free(p)


def run_fewest(ctx, seqs, taxids, cuts, w, query, hint_f=1 << 18, hint_m=4):
    """begin -> one add of everything -> count_begin -> one count_add per (seqs, ids) of cuts -> the counts of `query` ->
    minimize_begin(w, hint_m, "fewest") -> one minimize_add of everything -> finish.
    Returns hdr, flags, keys, vals, counts of query, count stats, minimize stats"""
    ctx.build_begin(hint_f)
    try:
        add_batch(ctx, seqs, taxids)
        ctx.build_count_begin()
        for s, ids in cuts:
            count_batch(ctx, s, ids)
        counts = ctx.build_count(query)
        cstats = ctx.build_count_stats()
        ctx.build_minimize_begin(w, hint_m, score="fewest")
        minimize_batch(ctx, seqs)
        assert np.array_equal(ctx.build_count(query), counts)          # still answered while minimizing
        hdr, flags, keys, vals = ctx.build_finish()
        assert np.array_equal(ctx.build_count(query), counts)          # and behind the finish
        mstats = ctx.build_minimize_stats()
    finally:
        ctx.build_end()
    return hdr, flags, keys, vals, counts, cstats, mstats


def absent_keys(F, k, n=1000, seed=9):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        x = int(rng.integers(0, 1 << 62)) & ((1 << (2 * k)) - 1 if k < 32 else (1 << 64) - 1)
        if x not in F:
            out.append(x)
    return np.array(out, dtype=np.uint64)


def check_counts(got, fkeys, n):
    want = np.array([n[x] for x in fkeys.tolist()], dtype=np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, [(int(fkeys[i]), int(got[i]), int(want[i])) for i in bad[:5]])


# ---- 1. every form over the edge world of its comb and window ------------------------------------------------------------------
@pytest.mark.parametrize("name", [f[0] for f in FORMS])
def test_forms_equal_the_model(ctx, oracle, name):
    form = BY_NAME[name]
    _, k, gaps, w, canon = form
    wld = world_of(oracle, form)
    ids = fm.deal_genomes(len(wld.seqs))
    exp_keys, exp_vals, F, n = fm.expected(oracle, wld, ids, k, w, gaps, canon)
    fkeys = mm.sorted_pairs(F)[0]
    none = absent_keys(F, k)
    configure(ctx, k, gaps, canon, wld.parent)
    h = len(wld.seqs) // 2                               # (130: genome 43 lies on both sides of the cut)
    assert ids[h - 1] == ids[h]
    hdr, flags, keys, vals, counts, sc, sm = run_fewest(ctx, wld.seqs, wld.taxids, [(wld.seqs[:h], ids[:h]), (wld.seqs[h:], ids[h:])], w,
                                                        np.concatenate([fkeys, none]))
    print("%s: %d scored keys, %d selected, %r, %r" % (name, len(F), exp_keys.size, sc, sm))
    check_counts(counts[:fkeys.size], fkeys, n)
    assert not counts[fkeys.size:].any()
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
    assert sc["batches"] == 2 and sc["genomes"] == len(set(ids)) and sc["launches"] == len(set(ids)) + 1
    assert sc["largest"] == max(n.values())
    valid = sum(int(mm.position_kmers(s, k, gaps, canon)[1].sum()) for s in wld.seqs)
    assert sc["lookups"] == valid                        # every position belongs to one chunk
    assert sm["scored_keys"] == len(F) and sm["keys"] == exp_keys.size
    if w <= mm.comb_of(k, gaps):
        assert exp_keys.size == len(F)
    else:
        assert 0 < exp_keys.size < len(F)


# ---- 2. a genome counts once ------------------------------------------------------------------------------------------------------
def test_once_per_genome(ctx, oracle, small_world):
    """X + Y + X in one record of 4200 bases: the repeat lies in other 2048-base chunks than its first copy; X again as a second
    record of the genome; a second genome holds X once"""
    rng = np.random.default_rng(22)
    X, Y = synth.rand_seq(rng, 1500), synth.rand_seq(rng, 1200)
    seqs = [np.concatenate([X, Y, X]).tobytes(), X.tobytes(), X.tobytes()]
    assert len(seqs[0]) > 4096
    leaves = list(small_world.genomes)
    taxids, ids = [leaves[0], leaves[0], leaves[1]], [0, 0, 1]
    F = mm.full_map(oracle, small_world.tax, seqs, taxids, 31)
    n = fm.genome_counts(seqs, ids, 31)
    fkeys = mm.sorted_pairs(F)[0]
    xk = np.unique(mm.position_kmers(X, 31)[0])
    assert xk.size == 1470 and all(n[x] == 2 for x in xk.tolist())
    configure(ctx, 31, None, True, small_world.parent)
    exp_keys, exp_vals = mm.sorted_pairs(fm.select_fewest(F, n, seqs, 31, 50))
    hdr, flags, keys, vals, counts, sc, sm = run_fewest(ctx, seqs, taxids, [(seqs, ids)], 50, np.concatenate([fkeys, xk]), hint_f=1 << 14)
    check_counts(counts[:fkeys.size], fkeys, n)
    assert (counts[fkeys.size:] == 2).all()
    assert sc["launches"] == 2 and sc["genomes"] == 2 and sc["largest"] == 2
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)


# ---- 3. more genomes than a wavefront has lanes, than a byte counts ------------------------------------------------------------------
def test_three_hundred_genomes(ctx, oracle, small_world):
    rng = np.random.default_rng(300)
    shared = synth.rand_seq(rng, 60)
    seqs = []
    for g in range(300):
        s = synth.rand_seq(rng, 300)
        at = int(rng.integers(0, 241))
        s[at:at + 60] = shared
        seqs.append(s.tobytes())
    leaves = list(small_world.genomes)
    taxids, ids = [leaves[g % len(leaves)] for g in range(300)], list(range(300))
    F = mm.full_map(oracle, small_world.tax, seqs, taxids, 31)
    n = fm.genome_counts(seqs, ids, 31)
    fkeys = mm.sorted_pairs(F)[0]
    sk = np.unique(mm.position_kmers(shared, 31)[0])
    assert sk.size == 30 and all(n[x] == 300 for x in sk.tolist())
    configure(ctx, 31, None, True, small_world.parent)
    exp_keys, exp_vals = mm.sorted_pairs(fm.select_fewest(F, n, seqs, 31, 50))
    hdr, flags, keys, vals, counts, sc, sm = run_fewest(ctx, seqs, taxids, [(seqs, ids)], 50, np.concatenate([fkeys, sk]), hint_f=1 << 18)
    check_counts(counts[:fkeys.size], fkeys, n)
    assert (counts[fkeys.size:] == 300).all()
    assert (sc["batches"], sc["launches"], sc["genomes"], sc["largest"]) == (1, 300, 300, 300)
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)


# ---- 4. M and the counts are a function of the triples ----------------------------------------------------------------------------
def test_cuts_order_and_numbering_change_nothing(ctx, oracle):
    form = BY_NAME["k31-w50-canon"]
    wld = world_of(oracle, form)
    N = 90                                               # the three of every length class and 48 long ones: 30 genomes
    seqs, taxids, ids = wld.seqs[:N], wld.taxids[:N], fm.deal_genomes(N)
    F = mm.full_map(oracle, wld.tax, seqs, taxids, 31)
    n = fm.genome_counts(seqs, ids, 31)
    fkeys = mm.sorted_pairs(F)[0]
    exp_keys, exp_vals = mm.sorted_pairs(fm.select_fewest(F, n, seqs, 31, 50))
    final = khash_size(exp_keys.size)
    configure(ctx, 31, None, True, wld.parent)
    other = [5, 9] + [4000000000 + 1000 * g for g in range(2, N // 3)]           # the same partition under other, increasing names
    renamed = [other[g] for g in ids]
    assert max(renamed) < NO_ID
    cut = 46                                             # inside genome 15 (sequences 45, 46, 47)
    assert ids[cut - 1] == ids[cut]
    ways = {
        "one call": [(seqs, ids)],
        "one sequence per call": [([s], [g]) for s, g in zip(seqs, ids)],
        "a genome spanning two calls": [(seqs[:cut], ids[:cut]), (seqs[cut:], ids[cut:])],
        "other names for the same genomes": [(seqs, renamed)],
    }
    seen = []
    for what, cuts in ways.items():
        for hint_m in (4, final):
            hdr, flags, keys, vals, counts, sc, sm = run_fewest(ctx, seqs, taxids, cuts, 50, fkeys, hint_m=hint_m)
            print(what, hint_m, sc, sm)
            check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
            check_counts(counts, fkeys, n)
            assert (sm["grows"] == 0) == (hint_m == final)
            assert sc["batches"] == len(cuts) and sc["genomes"] == N // 3
            assert sc["launches"] == {1: N // 3, 2: N // 3 + 1}.get(len(cuts), N)
            k2, v2 = present_pairs(flags, keys, vals, int(hdr[0]))
            seen.append((k2.tobytes(), v2.tobytes(), counts.tobytes()))
    assert len(set(seen)) == 1


# ---- 5. the rule itself -------------------------------------------------------------------------------------------------------------
def test_the_rule_on_a_hand_made_taxonomy(ctx, oracle):
    tax = oracle.Taxonomy(pairs=PAIRS8)
    seqs, taxids, genomes, q = rule_input()
    F = mm.full_map(oracle, tax, seqs, taxids, 31)
    n = fm.genome_counts(seqs, genomes, 31)
    exp_keys, exp_vals = mm.sorted_pairs(fm.select_fewest(F, n, seqs, 31, 32))
    fkeys = mm.sorted_pairs(F)[0]
    configure(ctx, 31, None, True, tax.parent)
    hdr, flags, keys, vals, counts, sc, sm = run_fewest(ctx, seqs, taxids, [(seqs, genomes)], 32, fkeys, hint_f=64)
    check_counts(counts, fkeys, n)
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
    gk, gv = present_pairs(flags, keys, vals, int(hdr[0]))
    got = dict(zip(gk.tolist(), gv.tolist()))
    assert q["x1"] in got and q["x0"] not in got                                  # the count decides
    assert q["e1"] in got and q["e0"] not in got and got[q["e1"]] == 1            # ... against the depth
    assert q["y1"] in got and q["y0"] not in got and got[q["y1"]] == 2            # equal counts: the smaller taxid
    assert min(q["c0"], q["c1"]) in got and max(q["c0"], q["c1"]) not in got      # equal scores: the smaller k-mer
    # the device's own -D map of the same session inputs is another one
    d = run_minimize(ctx, [(seqs, taxids)], [seqs], 32, hint_f=64, hint_m=4)
    dk, _ = present_pairs(d[1], d[2], d[3], int(d[0][0]))
    assert q["e0"] in dk.tolist() and q["e1"] not in dk.tolist() and not np.array_equal(dk, gk)


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------
def test_errors_fail_and_fault_nothing(ctx, oracle, small_world):
    wld = small_world
    configure(ctx, 31, None, True, wld.parent)
    L, h = ctx.L, ctx.h
    leaves = list(wld.genomes)
    seqs = [wld.genomes[l].tobytes() for l in leaves]
    n3 = fm.genome_counts(seqs[:3], [0, 1, 1], 31)
    q = np.array(sorted(n3), dtype=np.uint64)
    u64p, u32p = L.bns_build_count_get.argtypes[1], L.bns_build_count_get.argtypes[3]
    out6 = np.zeros(6, dtype=np.uint64)

    def err():
        return L.bns_last_error(h).decode()

    def raw_add(d_b, d_o, nseq, total, ids):
        a = np.ascontiguousarray(ids, dtype=np.uint32)
        return L.bns_build_count_add(h, d_b, d_o, nseq, total, a.ctypes.data_as(u32p), None)
    # without a session; before count_begin
    assert L.bns_build_count_begin(h) == ERR_STATE
    assert L.bns_build_count_add(h, None, None, 0, 0, None, None) == ERR_STATE
    assert L.bns_build_count_stats(h, out6.ctypes.data_as(u64p)) == ERR_STATE
    ctx.build_begin(1 << 16)
    add_batch(ctx, seqs[:3], leaves[:3])
    assert L.bns_build_count_add(h, None, None, 0, 0, None, None) == ERR_STATE and "before bns_build_count_begin" in err()
    assert L.bns_build_count_stats(h, out6.ctypes.data_as(u64p)) == ERR_STATE
    assert L.bns_build_minimize_begin_score(h, 50, 0, 1) == ERR_STATE and "bns_build_count_begin" in err()
    assert L.bns_build_minimize_begin_score(h, 50, 0, 7) == ERR_ARG
    ctx.build_count_begin()
    assert not ctx.build_count(q).any()
    assert L.bns_build_count_begin(h) == ERR_STATE and "twice" in err()
    assert L.bns_build_add(h, None, None, 0, 0, None, None) == ERR_STATE and "frozen" in err()
    fl = np.full(1, 0xAAAAAAAA, dtype=np.uint32); ks = np.zeros(4, dtype=np.uint64); vs = np.zeros(4, dtype=np.uint32)
    sa = L.bns_build_seed.argtypes
    assert L.bns_build_seed(h, 4, fl.ctypes.data_as(sa[2]), ks.ctypes.data_as(sa[3]), vs.ctypes.data_as(sa[4])) == ERR_STATE
    count_batch(ctx, seqs[:2], [3, 5])
    n2 = fm.genome_counts(seqs[:2], [3, 5], 31)
    want = np.array([n2.get(x, 0) for x in q.tolist()], dtype=np.uint32)
    assert np.array_equal(ctx.build_count(q), want) and want.any() and not want.all()
    before = ctx.build_count_stats()
    # the refusals of the ids: on the host, before anything is enqueued -- a real batch is handed in, and nothing is counted
    arrs = [np.frombuffer(s, dtype=np.uint8) for s in seqs[1:3]]
    bases, offsets = synth.concat(arrs)
    d_b = ctx.dev_alloc(bases.size + 16); d_o = ctx.dev_alloc(offsets.nbytes)
    try:
        ctx.dev_upload(d_b, bases); ctx.dev_upload(d_o, offsets)
        for ids, what in (([7, 6], "must not decrease"), ([4, 8], "must not decrease"), ([6, NO_ID], "no genome id"), ([NO_ID, NO_ID], "no genome id")):
            assert raw_add(d_b, d_o, 2, int(offsets[-1]), ids) == ERR_ARG and what in err(), ids
            assert np.array_equal(ctx.build_count(q), want) and ctx.build_count_stats() == before
        assert L.bns_build_count_add(h, d_b, d_o, 2, int(offsets[-1]), None, None) == ERR_ARG
        assert L.bns_build_minimize_begin_score(h, 50, 0, 7) == ERR_ARG
        assert np.array_equal(ctx.build_count(q), want)
        # the session goes on: the same id again (the genome continues), then a larger one
        assert raw_add(d_b, d_o, 2, int(offsets[-1]), [5, 6]) == 0
    finally:
        ctx.dev_free(d_b); ctx.dev_free(d_o)
    n4 = fm.genome_counts(seqs[:2] + seqs[1:3], [3, 5, 5, 6], 31)
    assert np.array_equal(ctx.build_count(q), np.array([n4.get(x, 0) for x in q.tolist()], dtype=np.uint32))
    assert ctx.build_count_stats()["genomes"] == 3 and ctx.build_count_stats()["launches"] == 4
    # a sequence F never saw: the flagged probe, BNS_ERR_TABLE, then only bns_build_end
    with pytest.raises(bonsai_amd.BonsaiAmdError) as ei:
        count_batch(ctx, [seqs[4]], [9])
    assert "not part of the scored build" in str(ei.value) and L.bns_strerror(ERR_TABLE).decode() in str(ei.value)
    assert L.bns_build_count_add(h, None, None, 0, 0, None, None) == ERR_STATE
    assert L.bns_build_count_get(h, q.ctypes.data_as(u64p), q.size, want.ctypes.data_as(u32p)) == ERR_STATE
    assert L.bns_build_minimize_begin_score(h, 50, 0, 1) == ERR_STATE
    assert L.bns_build_end(h) == 0
    # count_add while minimizing and after finish; a window beyond the comb
    ctx.build_begin(1 << 16)
    add_batch(ctx, seqs[:1], leaves[:1])
    ctx.build_count_begin()
    count_batch(ctx, seqs[:1], [0])
    ctx.build_minimize_begin(50, score="fewest")
    assert L.bns_build_count_add(h, None, None, 0, 0, None, None) == ERR_STATE
    assert L.bns_build_count_begin(h) == ERR_STATE
    ctx.build_end()
    ctx.set_window(50, 0)
    ctx.build_begin(64)
    assert L.bns_build_count_begin(h) == ERR_STATE and "bns_set_window" in err()
    ctx.build_end()
    configure(ctx, 31, None, True, wld.parent)
    # a fresh session on the same context works afterwards
    ids = [0, 0, 1, 2, 2, 3]
    F = mm.full_map(oracle, wld.tax, seqs, leaves, 31)
    n = fm.genome_counts(seqs, ids, 31)
    exp_keys, exp_vals = mm.sorted_pairs(fm.select_fewest(F, n, seqs, 31, 50))
    fkeys = mm.sorted_pairs(F)[0]
    hdr, flags, keys, vals, counts, sc, sm = run_fewest(ctx, seqs, leaves, [(seqs, ids)], 50, fkeys, hint_f=1 << 16)
    check_counts(counts, fkeys, n)
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)


# ---- 7. on a busy caller's stream ---------------------------------------------------------------------------------------------------
def test_build_count_add_on_the_callers_stream(env):
    """F holds the k-mers of two genome sets; the sequences of the first arrive late over those of the second -- all of them k-mers
    F knows --, so the counts are those of the first set alone and every k-mer private to the second has none"""
    e, c = env, env.ctx
    seqs = [g.tobytes() for g in e.genomes_a + e.genomes_b]
    ids = [0, 0, 1, 2, 2, 3]
    full = mm.full_map(e.oracle, e.w.tax, seqs, list(synth.LEAVES) + LEAVES_B, K)
    fkeys = mm.sorted_pairs(full)[0]
    n_a, n_b = fm.genome_counts(seqs[:6], ids, K), fm.genome_counts(seqs[6:], ids, K)
    want = np.array([n_a.get(x, 0) for x in fkeys.tolist()], dtype=np.uint32)
    poison = np.array([n_b.get(x, 0) for x in fkeys.tolist()], dtype=np.uint32)
    assert float((want != poison).mean()) >= 0.9
    c.build_begin(4)
    for genomes, tx in ((e.genomes_a, synth.LEAVES), (e.genomes_b, LEAVES_B)):
        d_bases, d_off, d_tax, total, fills = genome_fills(e, genomes, genomes, tx, tx)
        for dst, a, _ in fills:
            dst.copy_(a)
        e.torch.cuda.synchronize()
        c.build_add(d_bases.data_ptr(), d_off.data_ptr(), 6, total, d_tax.data_ptr())
    assert c.build_stats()["keys"] == len(full)
    c.build_count_begin()
    d_bases, d_off, _, total, fills = genome_fills(e, e.genomes_a, e.genomes_b, synth.LEAVES, LEAVES_B)
    e.late.run(fills[:1], [], lambda st: c.build_count_add(d_bases.data_ptr(), d_off.data_ptr(), 6, total, ids, stream=st))
    got = c.build_count(fkeys)
    stats = c.build_count_stats()
    c.build_end()
    assert np.array_equal(got, want)
    assert (stats["batches"], stats["launches"], stats["genomes"]) == (1, 4, 4)


# ---- 8. with low-complexity masking on -----------------------------------------------------------------------------------------------
def test_with_dust_on(ctx, oracle):
    """all three passes see one mask: the counts and M are those of the sequences as tests/dust_ref.py masks them"""
    w = DW.make_world(oracle, seed=41)
    leaves = list(w.genomes)
    raw = [w.genomes[l] for l in leaves]
    sub, masks = DW.substituted(raw)
    assert 0.05 <= sum(int(m.sum()) for m in masks) / sum(s.size for s in raw) <= 0.70
    ids = [0, 0, 1, 2, 2, 3]
    sseqs = [s.tobytes() for s in sub]
    F = mm.full_map(oracle, w.tax, sseqs, leaves, 31)
    n = fm.genome_counts(sseqs, ids, 31)
    exp_keys, exp_vals = mm.sorted_pairs(fm.select_fewest(F, n, sseqs, 31, 50))
    fkeys = mm.sorted_pairs(F)[0]
    plain = mm.full_map(oracle, w.tax, [s.tobytes() for s in raw], leaves, 31)
    assert len(F) < len(plain)
    configure(ctx, 31, None, True, w.parent)
    ctx.set_dust(DW.W, DW.T)
    hdr, flags, keys, vals, counts, sc, sm = run_fewest(ctx, raw, leaves, [(raw[:3], ids[:3]), (raw[3:], ids[3:])], 50, fkeys, hint_f=1 << 16)
    check_counts(counts, fkeys, n)
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
    assert sm["scored_keys"] == len(F)


# ---- 9. the depth form is what it was -------------------------------------------------------------------------------------------------
def test_depth_through_the_score_entry_point(ctx, oracle):
    form = BY_NAME["k31-w50-canon"]
    wld = world_of(oracle, form)
    exp_keys, exp_vals, F, _ = mm.expected(oracle, wld, 31, 50)
    configure(ctx, 31, None, True, wld.parent)
    tables = []
    for score in ("depth", 0):                           # bns_build_minimize_begin, bns_build_minimize_begin_score(.., BNS_MINIMIZE_DEPTH)
        ctx.build_begin(1 << 18)
        try:
            add_batch(ctx, wld.seqs, wld.taxids)
            ctx.build_minimize_begin(50, 4, score=score)
            minimize_batch(ctx, wld.seqs)
            hdr, flags, keys, vals = ctx.build_finish()
        finally:
            ctx.build_end()
        check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
        tables.append(present_pairs(flags, keys, vals, int(hdr[0])))
    assert np.array_equal(tables[0][0], tables[1][0]) and np.array_equal(tables[0][1], tables[1][1])
