"""The build session (bns_build_begin / _seed / _add / _finish / _export / _end): a table that stays in the context from batch to
batch, doubles when a batch does not fit, and can start from the present slots of an existing khash table.  Whatever the batches,
their order, the starting size and the seed, the finished table is the oracle's sequential update_lca_map over the union of all
sequences -- the expectation never comes from the device -- in khash's own size, valid for the reference's kh_get."""
import numpy as np
import pytest

import build_cases as bc
import synth
from test_gpu_build import device_build, present_pairs

pytestmark = pytest.mark.gpu

ERR_STATE = -4                                           # include/bonsai_amd.h


def khash_size(n):
    """the smallest power of two nb >= 4 with (uint64_t)(nb * 0.77 + 0.5) >= n: what khash itself has grown to after n puts"""
    nb = 4
    while int(nb * 0.77 + 0.5) < n:
        nb <<= 1
    return nb


def slot_states(flags, nb):
    i = np.arange(nb)
    return (flags[i >> 4] >> ((i & 15) << 1)) & 3


def add_batch(ctx, seqs, taxids):
    """one bns_build_add: the sequences (bytes or uint8 arrays) uploaded, added, freed"""
    arrs = [np.ascontiguousarray(np.frombuffer(s, dtype=np.uint8) if isinstance(s, bytes) else s) for s in seqs]
    bases, offsets = synth.concat(arrs)
    pad = (-bases.size) % 8 + 8
    tx = np.ascontiguousarray(taxids, dtype=np.uint32)
    d_bases = ctx.dev_alloc(bases.size + pad); d_off = ctx.dev_alloc(offsets.nbytes); d_tx = ctx.dev_alloc(max(4, tx.nbytes))
    try:
        ctx.dev_upload(d_bases, bases); ctx.dev_upload(d_off, offsets); ctx.dev_upload(d_tx, tx)
        ctx.build_add(d_bases, d_off, len(arrs), int(offsets[-1]), d_tx)
    finally:
        for p in (d_bases, d_off, d_tx):
            ctx.dev_free(p)


def run_session(ctx, batches, hint, seed=None):
    """begin(hint) [-> seed] -> one add per (seqs, taxids) of batches -> finish; returns hdr, flags, keys, vals, stats"""
    ctx.build_begin(hint)
    try:
        if seed is not None:
            ctx.build_seed(*seed)
        for seqs, taxids in batches:
            add_batch(ctx, seqs, taxids)
        hdr, flags, keys, vals = ctx.build_finish()
        stats = ctx.build_stats()
    finally:
        ctx.build_end()
    return hdr, flags, keys, vals, stats


def check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals):
    """the finished table against the expected pairs: the same map, khash's own size, kh_get finds every key, empty slots zeroed"""
    n = int(exp_keys.size)
    nb = int(hdr[0])
    got_keys, got_vals = present_pairs(flags, keys, vals, nb)
    assert np.array_equal(got_keys, exp_keys)
    bad = np.flatnonzero(got_vals != exp_vals)
    assert bad.size == 0, (bad.size, [(int(exp_keys[i]), int(got_vals[i]), int(exp_vals[i])) for i in bad[:5]])
    assert [int(x) for x in hdr] == [khash_size(n), n, n, int(khash_size(n) * 0.77 + 0.5)]
    assert flags.size == max(1, nb >> 4) and keys.size == nb and vals.size == nb
    t = oracle.Table.wrap(nb, n, n, int(hdr[3]), flags, keys, vals)
    qv, qf = t.get_batch(exp_keys)
    assert qf.all() and np.array_equal(qv, exp_vals)
    st = slot_states(flags, nb)
    assert set(np.unique(st).tolist()) <= {0, 2} and not keys[st == 2].any() and not vals[st == 2].any()
    if n and exp_keys[0] == 0:                           # key 0 is told from an empty slot by the flag alone
        assert int(((keys == 0) & (st == 0)).sum()) == 1


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.build_end()                                  # (a test that failed inside a session must not leave it to the next module)
    gpu_ctx.set_encoder(31, None, canonicalize=True)


# ---- small_world: 6 genomes x 6000 bp, about 26 k keys at k = 31 ---------------------------------------------------------------
FORMS = {"k31": (31, 0, True, None), "w50-entropy": (50, 1, True, None), "w50-entropy-forward": (50, 1, False, None),
         "spaced-half-w50-entropy": (50, 1, True, list(bc.G_HALF))}
_SMALL = {}


def small_expected(oracle, wld, form, leaves=None):
    """sorted (keys, values) of the oracle's sequential build over the genomes of `leaves` (all six: None), once per (form, leaves)"""
    key = (form, tuple(leaves) if leaves is not None else None)
    if key not in _SMALL:
        w, score, canon, gaps = FORMS[form]
        comb = 31 + (sum(gaps) if gaps else 0)
        t = oracle.Table()
        for leaf, g in wld.genomes.items():
            if leaves is not None and leaf not in leaves:
                continue
            if w > comb:
                oracle.lca_map_add_windowed(t, wld.tax, 31, w, score, g.tobytes(), leaf, gaps=gaps, canon=canon)
            else:
                oracle.lca_map_add(t, wld.tax, 31, g.tobytes(), leaf, gaps=gaps, canon=canon)
        k, v = bc.table_pairs(t)
        k.setflags(write=False); v.setflags(write=False)
        _SMALL[key] = (k, v, t)
    return _SMALL[key]


def configure_small(ctx, wld, form):
    w, score, canon, gaps = FORMS[form]
    ctx.set_encoder(31, gaps, canonicalize=canon, spaced_intended=True)
    ctx.set_window(w, score)
    ctx.load_taxonomy(wld.parent)


@pytest.mark.parametrize("form", list(FORMS))
def test_session_equals_one_shot(ctx, oracle, small_world, form):
    """three batches of two genomes into a table that starts large enough: the oracle's map, compacted to khash's own size"""
    wld = small_world
    exp_keys, exp_vals, _ = small_expected(oracle, wld, form)
    configure_small(ctx, wld, form)
    leaves = list(wld.genomes)
    batches = [([wld.genomes[l] for l in leaves[i:i + 2]], leaves[i:i + 2]) for i in (0, 2, 4)]
    hdr, flags, keys, vals, stats = run_session(ctx, batches, 1 << 17)
    print("%s: %d keys in %d buckets, %r" % (form, exp_keys.size, int(hdr[0]), stats))
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
    assert stats == {"batches": 3, "grows": 0, "seeded": 0, "keys": exp_keys.size}
    if form == "k31":
        assert exp_keys.size > 20000 and int(hdr[0]) == 1 << 16


@pytest.mark.parametrize("per_batch", [6, 1])
def test_session_grows_from_the_minimum(ctx, oracle, small_world, per_batch):
    """4 buckets to start with: pass 1 fills the table up, the table doubles, the same batch is applied again -- 14 times over on
    the way to 2^16 buckets --, and nothing is lost or folded wrongly on the way"""
    wld = small_world
    exp_keys, exp_vals, _ = small_expected(oracle, wld, "k31")
    configure_small(ctx, wld, "k31")
    leaves = list(wld.genomes)
    batches = [([wld.genomes[l] for l in leaves[i:i + per_batch]], leaves[i:i + per_batch]) for i in range(0, 6, per_batch)]
    hdr, flags, keys, vals, stats = run_session(ctx, batches, 4)
    print("%d per batch: %r" % (per_batch, stats))
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
    assert stats["batches"] == len(batches) and stats["grows"] >= 13 and stats["keys"] == exp_keys.size


@pytest.mark.parametrize("name", ["k11-canon", "w50-entropy-forward"])
def test_session_idempotent_and_order_free(ctx, oracle, name):
    """A, B, A again, then B backwards: a key found again is left alone and lca(tx, lca(tx, cur)) is what it was.  k11-canon: keys
    that a hundred sequences share, key 0 among them; w50-entropy-forward: windows over the emitted stream"""
    case = bc.BY_NAME[name]
    w = bc.world_for(oracle, case)
    exp_keys, exp_vals, _ = bc.expected(oracle, w, case)
    ctx.set_encoder(case.k, None, canonicalize=case.canon, spaced_intended=True)
    if bc.windowed(case):
        ctx.set_window(case.w, case.score)
    ctx.load_taxonomy(w.parent)
    h = len(w.seqs) // 2
    a = (w.seqs[:h], w.taxids[:h])
    b = (w.seqs[h:], w.taxids[h:])
    hdr, flags, keys, vals, stats = run_session(ctx, [a, b, a, (b[0][::-1], b[1][::-1])], 4)
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
    assert stats["batches"] == 4 and stats["keys"] == exp_keys.size


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_session_edge_worlds_in_two_batches(ctx, oracle, name):
    """every build form over its edge world (N runs, short sequences, deep folds, key 0), cut in two batches, from 4 buckets"""
    case = bc.BY_NAME[name]
    w = bc.world_for(oracle, case)
    exp_keys, exp_vals, _ = bc.expected(oracle, w, case)
    ctx.set_encoder(case.k, list(case.gaps) if case.gaps is not None else None, canonicalize=case.canon, spaced_intended=True)
    if bc.windowed(case):
        ctx.set_window(case.w, case.score)
    ctx.load_taxonomy(w.parent)
    h = len(w.seqs) // 2
    hdr, flags, keys, vals, stats = run_session(ctx, [(w.seqs[:h], w.taxids[:h]), (w.seqs[h:], w.taxids[h:])], 4)
    print("%s: %d keys expected, %d buckets, %r" % (name, exp_keys.size, int(hdr[0]), stats))
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
    if not bc.windowed(case) and not bc.is_spaced(case) and case.canon:
        assert exp_keys[0] == 0


def test_session_seed_then_add(ctx, oracle, small_world):
    """a db of genomes 0-2 with 50 slots deleted and garbage in 50 empty ones, plus genomes 3-5: the fold of what the seed still
    holds and the new genomes; without the damage, the one-shot build of all six"""
    wld = small_world
    leaves = list(wld.genomes)
    old, new = leaves[:3], leaves[3:]
    _, _, old_t = small_expected(oracle, wld, "k31", old)
    new_keys, new_vals, _ = small_expected(oracle, wld, "k31", new)
    all_keys, all_vals, _ = small_expected(oracle, wld, "k31")
    f0, k0, v0 = old_t.arrays()
    nb = old_t.n_buckets
    configure_small(ctx, wld, "k31")
    new_batch = [([wld.genomes[l] for l in new], new)]

    # untouched seed: the build over all six genomes
    hdr, flags, keys, vals, stats = run_session(ctx, new_batch, 0, seed=(nb, f0, k0, v0))
    check_table(oracle, hdr, flags, keys, vals, all_keys, all_vals)
    n_old = int((slot_states(f0, nb) == 0).sum())
    assert stats["seeded"] == n_old and stats["batches"] == 1

    # 50 present slots deleted (key and value words left as they are), 50 empty slots given key and value words
    rng = np.random.default_rng(50)
    st = slot_states(f0, nb)
    dele = rng.choice(np.flatnonzero(st == 0), size=50, replace=False)
    junk = rng.choice(np.flatnonzero(st == 2), size=50, replace=False)
    f1, k1, v1 = f0.copy(), k0.copy(), v0.copy()
    for i in dele.tolist():
        f1[i >> 4] |= np.uint32(1 << ((i & 15) << 1))
    k1[junk] = rng.integers(1, 1 << 62, size=50, dtype=np.uint64)
    v1[junk] = rng.integers(1, 1 << 20, size=50, dtype=np.uint32)
    st1 = slot_states(f1, nb)
    assert (st1[dele] == 1).all() and (st1[junk] == 2).all() and int((st1 == 0).sum()) == n_old - 50
    rem_keys, rem_vals = present_pairs(f1, k1, v1, nb)
    # (the two halves really meet: keys of both with different values, so the seeded value is folded, not kept or overwritten)
    common, ia, ib = np.intersect1d(rem_keys, new_keys, return_indices=True)
    assert int((rem_vals[ia] != new_vals[ib]).sum()) >= 100
    exp_t = oracle.Table()
    for key, val in zip(rem_keys.tolist(), rem_vals.tolist()):
        exp_t.put(key, val)
    for leaf in new:
        oracle.lca_map_add(exp_t, wld.tax, 31, wld.genomes[leaf].tobytes(), leaf)
    exp_keys, exp_vals = bc.table_pairs(exp_t)
    hdr, flags, keys, vals, stats = run_session(ctx, new_batch, 0, seed=(nb, f1, k1, v1))
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
    assert stats["seeded"] == n_old - 50
    assert not np.isin(k1[junk], keys).any()             # (nothing of an empty slot's words went in)


def test_session_state_refusals(ctx, oracle, small_world):
    """what is out of order returns BNS_ERR_STATE and harms nothing; a session without a key is an empty table of 4 buckets"""
    wld = small_world
    configure_small(ctx, wld, "k31")
    L, h = ctx.L, ctx.h
    hdr = np.zeros(4, dtype=np.uint64)
    fl = np.zeros(1, dtype=np.uint32); ks = np.zeros(4, dtype=np.uint64); vs = np.zeros(4, dtype=np.uint32)
    u32p, u64p = L.bns_build_export.argtypes[1], L.bns_build_export.argtypes[2]

    def p(a, t):
        return a.ctypes.data_as(t)
    seed_flags = np.full(1, 0xAAAAAAAA, dtype=np.uint32)

    def calls():
        return {"add": L.bns_build_add(h, None, None, 0, 0, None, None), "finish": L.bns_build_finish(h, p(hdr, u64p)),
                "export": L.bns_build_export(h, p(fl, u32p), p(ks, u64p), p(vs, u32p)),
                "seed": L.bns_build_seed(h, 4, p(seed_flags, u32p), p(ks, u64p), p(vs, u32p)),
                "stats": L.bns_build_stats(h, p(np.zeros(6, dtype=np.uint64), u64p))}
    assert calls() == {"add": ERR_STATE, "finish": ERR_STATE, "export": ERR_STATE, "seed": ERR_STATE, "stats": ERR_STATE}
    assert L.bns_build_end(h) == 0                       # legal at any point
    # begin twice; the encoder, the window and the taxonomy stay while a session is open
    ctx.build_begin(64)
    assert L.bns_build_begin(h, 64) == ERR_STATE
    assert L.bns_set_encoder(h, 21, None, 1, 1) == ERR_STATE
    assert L.bns_set_window(h, 50, 0) == ERR_STATE
    par = np.ascontiguousarray(wld.parent, dtype=np.uint32)
    assert L.bns_load_taxonomy(h, p(par, L.bns_load_taxonomy.argtypes[1]), par.size) == ERR_STATE
    assert L.bns_build_export(h, p(fl, u32p), p(ks, u64p), p(vs, u32p)) == ERR_STATE          # before finish
    # seed after an add
    leaf = list(wld.genomes)[0]
    add_batch(ctx, [wld.genomes[leaf]], [leaf])
    assert L.bns_build_seed(h, 4, p(seed_flags, u32p), p(ks, u64p), p(vs, u32p)) == ERR_STATE
    # ... and the session is none the worse for any of it (k is still 31: one genome's keys under its own taxid)
    one_keys = np.unique(oracle.encode(wld.genomes[leaf].tobytes(), 31))
    hdr1, flags, keys, vals = ctx.build_finish()
    check_table(oracle, hdr1, flags, keys, vals, one_keys, np.full(one_keys.size, leaf, dtype=np.uint32))
    assert L.bns_build_add(h, None, None, 0, 0, None, None) == ERR_STATE                      # after finish
    assert L.bns_build_finish(h, p(hdr, u64p)) == ERR_STATE
    ctx.build_end()
    ctx.build_end()
    # begin -> finish: a valid empty table
    ctx.build_begin()
    hdr0, flags, keys, vals = ctx.build_finish()
    ctx.build_end()
    assert [int(x) for x in hdr0] == [4, 0, 0, 3] and flags.tolist() == [0xAAAAAAAA] and not keys.any() and not vals.any()
    qv, qf = oracle.Table.wrap(4, 0, 0, 3, flags, keys, vals).get_batch(np.array([0, 1, 12345], dtype=np.uint64))
    assert not qf.any()
    # the refusals of bns_build_table_device hold for a session too
    ctx.set_encoder(32, None, canonicalize=False)
    assert L.bns_build_begin(h, 64) == -1 and "k == 32" in L.bns_last_error(h).decode()
    ctx.set_encoder(31, list(bc.G_HALF), canonicalize=True, spaced_intended=False)
    assert L.bns_build_begin(h, 64) == -1 and "spaced_intended" in L.bns_last_error(h).decode()
    # and the context builds on as before
    configure_small(ctx, wld, "k31")
    exp_keys, exp_vals, _ = small_expected(oracle, wld, "k31")
    hdr2, flags, keys, vals = device_build(ctx, list(wld.genomes.values()), list(wld.genomes.keys()), 1 << 17)
    got_keys, got_vals = present_pairs(flags, keys, vals, 1 << 17)
    assert np.array_equal(got_keys, exp_keys) and np.array_equal(got_vals, exp_vals)
