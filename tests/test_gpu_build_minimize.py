"""Taxonomic-depth minimizers on the device (bns_build_minimize_begin / _add / _stats): a build session that scored every k-mer
(F) streams its sequences again and keeps, from every window, the k-mer whose LCA lies deepest.  The expected table is the model's
(tests/minimize_model.py: the oracle's F, depths from the parent array, the rule as DESIGN.md states it), never the device's."""
import numpy as np
import pytest

import minimize_model as mm
import synth
from test_gpu_build_session import add_batch, check_table, khash_size
from test_minimize_model import BY_NAME, FORMS, world_of

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE, ERR_TABLE = -1, -4, -7              # include/bonsai_amd.h


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.build_end()                                  # (a test that failed inside a session must not leave it to the next module)
    gpu_ctx.set_encoder(31, None, canonicalize=True)


def minimize_batch(ctx, seqs):
    """one bns_build_minimize_add: the sequences uploaded, added, freed"""
    arrs = [np.ascontiguousarray(np.frombuffer(s, dtype=np.uint8) if isinstance(s, bytes) else s) for s in seqs]
    bases, offsets = synth.concat(arrs)
    pad = (-bases.size) % 8 + 8
    d_bases = ctx.dev_alloc(bases.size + pad); d_off = ctx.dev_alloc(offsets.nbytes)
    try:
        ctx.dev_upload(d_bases, bases); ctx.dev_upload(d_off, offsets)
        ctx.build_minimize_add(d_bases, d_off, len(arrs), int(offsets[-1]))
    finally:
        for p in (d_bases, d_off):
            ctx.dev_free(p)


def run_minimize(ctx, batches_a, batches_b, w, hint_f=0, hint_m=0):
    """begin(hint_f) -> add every (seqs, taxids) of batches_a -> minimize_begin(w, hint_m) -> minimize_add every seqs of batches_b
    -> finish; returns hdr, flags, keys, vals, stats of pass A, stats of the minimizing"""
    ctx.build_begin(hint_f)
    try:
        for seqs, taxids in batches_a:
            add_batch(ctx, seqs, taxids)
        stats_a = ctx.build_stats()
        ctx.build_minimize_begin(w, hint_m)
        for seqs in batches_b:
            minimize_batch(ctx, seqs)
        hdr, flags, keys, vals = ctx.build_finish()
        mstats = ctx.build_minimize_stats()
    finally:
        ctx.build_end()
    return hdr, flags, keys, vals, stats_a, mstats


def configure(ctx, k, gaps, canon, parent):
    ctx.set_encoder(k, list(gaps) if gaps is not None else None, canonicalize=canon, spaced_intended=True)
    ctx.load_taxonomy(parent)


# ---- 1. every form over the edge world of its comb and window ------------------------------------------------------------------
@pytest.mark.parametrize("name", [f[0] for f in FORMS])
def test_forms_equal_the_model(ctx, oracle, name):
    form = BY_NAME[name]
    _, k, gaps, w, canon = form
    wld = world_of(oracle, form)
    exp_keys, exp_vals, F, _ = mm.expected(oracle, wld, k, w, gaps, canon)
    configure(ctx, k, gaps, canon, wld.parent)
    h = len(wld.seqs) // 2
    hdr, flags, keys, vals, sa, sm = run_minimize(ctx, [(wld.seqs[:h], wld.taxids[:h]), (wld.seqs[h:], wld.taxids[h:])],
                                                  [wld.seqs[:h], wld.seqs[h:]], w, hint_f=1 << 18, hint_m=4)
    print("%s: %d scored keys, %d selected, %d buckets, %r" % (name, len(F), exp_keys.size, int(hdr[0]), sm))
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
    assert sa["keys"] == len(F) and sm["scored_keys"] == len(F) and sm["keys"] == exp_keys.size and sm["batches"] == 2
    if w <= mm.comb_of(k, gaps):
        assert exp_keys.size == len(F)                   # M = F
    else:
        assert 0 < exp_keys.size < len(F)


# ---- 2. M is a function of the set of sequences --------------------------------------------------------------------------------
def test_order_batches_sizes_change_nothing(ctx, oracle):
    form = BY_NAME["k31-w50-canon"]
    wld = world_of(oracle, form)
    exp_keys, exp_vals, F, _ = mm.expected(oracle, wld, 31, 50)
    configure(ctx, 31, None, True, wld.parent)
    seqs, tx = wld.seqs, wld.taxids
    rs, rt = seqs[::-1], tx[::-1]
    one = [(seqs, tx)]
    final = khash_size(exp_keys.size)
    runs = {
        "one batch, M from 4 buckets, F grows": (one, [seqs], 4, 0),
        "one batch, M at its final size": (one, [seqs], 1 << 18, final),
        "pass A reversed": ([(rs, rt)], [seqs], 1 << 18, final),
        "pass B reversed": (one, [rs], 1 << 18, 0),
        "the same batch twice in pass B": (one, [seqs, seqs], 1 << 18, 0),
    }
    for what, (a, b, hf, hm) in runs.items():
        hdr, flags, keys, vals, sa, sm = run_minimize(ctx, a, b, 50, hint_f=hf, hint_m=hm)
        print(what, sa, sm)
        check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
        assert sm["keys"] == exp_keys.size and sm["scored_keys"] == len(F)
        if hf == 4:
            assert sa["grows"] >= 10
        assert (sm["grows"] == 0) == (hm == final)
    # one sequence per batch in both passes (the long ones only in steps: 260 uploads twice over are the slow part)
    per = [([s], [t]) for s, t in zip(seqs, tx)]
    hdr, flags, keys, vals, sa, sm = run_minimize(ctx, per, [[s] for s in rs], 50, hint_f=4, hint_m=0)
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
    assert sm["batches"] == len(seqs) and sm["keys"] == exp_keys.size


# ---- 3. the rule itself ------------------------------------------------------------------------------------------------------
# 1 - 2 - 4 - 6        depths 1, 2, 3, 4
#       \ 5            3
#   \ 3 - 7 - 8        2, 3, 4
PAIRS8 = [(1, 1), (2, 1), (3, 1), (4, 2), (5, 2), (6, 4), (7, 3), (8, 7)]
NOT_A_NODE = 50


def rule_input(oracle, tax):
    """k 31, w 32: a window holds two k-mers, a sequence of 32 bases is one window.  Returns seqs, taxids and the k-mers named below."""
    rng = np.random.default_rng(314)
    other = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}

    def km(s):
        k, ok = mm.position_kmers(s, 31, None, True)
        assert ok.all()
        return [int(x) for x in k]
    for _ in range(64):
        # (a) x0 in A (6) and A2 (7): LCA 1, depth 1, the k-mer both other scores keep (the smaller Lex hash, and the larger value,
        # which is what the path overloads' entropy score prefers); x1 in A alone: 6, depth 4
        A = synth.rand_seq(rng, 32).tobytes()
        A2 = A[:31] + other[A[31]]
        x0, x1 = km(A)
        lex, ent = oracle.Table(), oracle.Table()
        for s, t in ((A, 6), (A2, 7)):
            oracle.lca_map_add_windowed(lex, tax, 31, 32, 0, s, t)
            oracle.lca_map_add_windowed(ent, tax, 31, 32, 1, s, t)
        if not lex.get_batch(np.array([x1], dtype=np.uint64))[1][0] and not ent.get_batch(np.array([x1], dtype=np.uint64))[1][0]:
            break
    else:
        raise AssertionError("no sequence whose deep k-mer the Lex and entropy builds both leave out")
    # (b) y0 in B alone, whose taxid is no node: F = 50, depth 0; y1 in B and B2 (6): lca = 0xFFFFFFFF, depth 0
    B = synth.rand_seq(rng, 32).tobytes()
    B2 = other[B[0]] + B[1:]
    y0, y1 = km(B)
    # (c) both k-mers of C under 5 alone
    C = synth.rand_seq(rng, 32).tobytes()
    c0, c1 = km(C)
    # (d) z0 in D (6) and D3 (7): 1; z1 in D (6) and D2 (5): 2 -- selected in D, and in D2 beaten by q (5 alone, depth 3)
    D = synth.rand_seq(rng, 32).tobytes()
    D2 = D[1:] + other[D[0]]
    D3 = other[D[31]] + D[:31]
    z0, z1 = km(D)
    q = km(D2)[1]
    seqs = [A, A2, B, B2, C, D, D2, D3]
    taxids = [6, 7, NOT_A_NODE, 6, 5, 6, 5, 7]
    return seqs, taxids, dict(x0=x0, x1=x1, y0=y0, y1=y1, c0=c0, c1=c1, z0=z0, z1=z1, q=q, lex=lex, ent=ent)


def test_the_rule_on_a_hand_made_taxonomy(ctx, oracle):
    tax = oracle.Taxonomy(pairs=PAIRS8)
    seqs, taxids, n = rule_input(oracle, tax)
    F = mm.full_map(oracle, tax, seqs, taxids, 31)
    depth = mm.depths(tax.parent)
    assert depth == {1: 1, 2: 2, 3: 2, 4: 3, 5: 3, 6: 4, 7: 3, 8: 4}
    M = mm.select(F, depth, seqs, 31, 32)
    exp_keys, exp_vals = mm.sorted_pairs(M)
    # what the input was built for, stated on the model first
    assert (F[n["x0"]], F[n["x1"]]) == (1, 6)
    assert (F[n["y0"]], F[n["y1"]]) == (NOT_A_NODE, 0xFFFFFFFF)
    assert F[n["c0"]] == F[n["c1"]] == 5
    assert (F[n["z0"]], F[n["z1"]], F[n["q"]]) == (1, 2, 5)
    configure(ctx, 31, None, True, tax.parent)
    hdr, flags, keys, vals, sa, sm = run_minimize(ctx, [(seqs, taxids)], [seqs], 32, hint_f=64, hint_m=4)
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)
    got = dict(zip(keys[np.isin(keys, exp_keys)].tolist(), vals[np.isin(keys, exp_keys)].tolist()))
    # (a) the deep k-mer, not the shallow one; neither the Lex nor the entropy db of the same input holds it
    assert n["x1"] in got and n["x0"] not in got and got[n["x1"]] == 6
    for t in (n["lex"], n["ent"]):
        assert not t.get_batch(np.array([n["x1"]], dtype=np.uint64))[1][0]
    # (b) equal depth (0): the smaller taxid
    assert n["y0"] in got and n["y1"] not in got and got[n["y0"]] == NOT_A_NODE
    # (c) equal score: the smaller k-mer
    assert min(n["c0"], n["c1"]) in got and max(n["c0"], n["c1"]) not in got
    # (d) selected in D alone, stored with the LCA that D2 -- where q beat it -- took part in
    assert got[n["z1"]] == 2 and n["q"] in got and n["z0"] not in got
    assert sm["keys"] == len(M)


# ---- 4. depth at scale -------------------------------------------------------------------------------------------------------
def test_depth_300_and_sparse_ids(ctx, oracle):
    """ids up to 3 000 000; a chain to depth 299 numbered downwards (every child below its parent), two leaves under its end"""
    top = 2999999
    pairs = [(1, 1), (top, 1)] + [(top - i, top - i + 1) for i in range(1, 298)]
    end = top - 297                                      # depth 299
    l_big, l_small = 3000000, 2000000                    # depth 300 both
    pairs += [(l_big, end), (l_small, end)]
    tax = oracle.Taxonomy(pairs=pairs)
    depth = mm.depths(tax.parent)
    assert depth[end] == 299 and depth[l_big] == 300 and depth[l_small] == 300 and tax.parent.size == 3000001
    rng = np.random.default_rng(300)
    other = {ord("A"): b"C", ord("C"): b"G", ord("G"): b"T", ord("T"): b"A"}
    E = synth.rand_seq(rng, 32).tobytes()                # e0 shared with E2: the LCA is `end`, depth 299; e1 under l_big alone: 300
    E2 = E[:31] + other[E[31]]
    long_seq = synth.rand_seq(rng, 3000).tobytes()       # and a sequence of more than a chunk under a node half way down
    seqs, taxids = [E, E2, long_seq, long_seq[1000:2500]], [l_big, l_small, top - 150, top - 100]
    F = mm.full_map(oracle, tax, seqs, taxids, 31)
    e0, e1 = (int(x) for x in mm.position_kmers(E, 31)[0])
    assert (F[e0], F[e1]) == (end, l_big)                # the deeper one has the LARGER taxid: depth decides, not the id
    M = mm.select(F, depth, seqs, 31, 32)
    assert e1 in M and e0 not in M
    exp_keys, exp_vals = mm.sorted_pairs(M)
    configure(ctx, 31, None, True, tax.parent)
    hdr, flags, keys, vals, sa, sm = run_minimize(ctx, [(seqs, taxids)], [seqs], 32, hint_f=1 << 13, hint_m=4)
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)


# ---- 5. errors ---------------------------------------------------------------------------------------------------------------
def test_errors_fail_and_fault_nothing(ctx, oracle, small_world):
    wld = small_world
    configure(ctx, 31, None, True, wld.parent)
    L, h = ctx.L, ctx.h
    leaves = list(wld.genomes)
    u64p = L.bns_build_minimize_stats.argtypes[1]
    out6 = np.zeros(6, dtype=np.uint64)
    hdr = np.zeros(4, dtype=np.uint64)

    def err():
        return L.bns_last_error(h).decode()
    # without a session
    assert L.bns_build_minimize_begin(h, 50, 0) == ERR_STATE
    assert L.bns_build_minimize_add(h, None, None, 0, 0, None) == ERR_STATE
    assert L.bns_build_minimize_stats(h, out6.ctypes.data_as(u64p)) == ERR_STATE
    # add before begin; windows that are too wide; begin twice; F is frozen; the encoder and the window stay
    ctx.build_begin(1 << 16)
    add_batch(ctx, [wld.genomes[leaves[0]]], [leaves[0]])
    assert L.bns_build_minimize_add(h, None, None, 0, 0, None) == ERR_STATE
    assert L.bns_build_minimize_stats(h, out6.ctypes.data_as(u64p)) == ERR_STATE
    assert L.bns_build_minimize_begin(h, 31 + 1024, 0) == ERR_ARG and "1024 k-mers" in err()
    assert L.bns_build_minimize_begin(h, 1921, 0) == ERR_ARG
    ctx.build_minimize_begin(50)
    assert L.bns_build_minimize_begin(h, 50, 0) == ERR_STATE
    assert L.bns_build_add(h, None, None, 0, 0, None, None) == ERR_STATE and "frozen" in err()
    fl = np.full(1, 0xAAAAAAAA, dtype=np.uint32); ks = np.zeros(4, dtype=np.uint64); vs = np.zeros(4, dtype=np.uint32)
    sa = L.bns_build_seed.argtypes
    assert L.bns_build_seed(h, 4, fl.ctypes.data_as(sa[2]), ks.ctypes.data_as(sa[3]), vs.ctypes.data_as(sa[4])) == ERR_STATE
    assert L.bns_set_window(h, 50, 0) == ERR_STATE
    assert L.bns_set_encoder(h, 21, None, 1, 1) == ERR_STATE
    # a sequence F never saw: BNS_ERR_TABLE, then only bns_build_end
    with pytest.raises(Exception) as ei:
        minimize_batch(ctx, [wld.genomes[leaves[0]], wld.genomes[leaves[1]]])
    assert "not part of the scored build" in str(ei.value) and L.bns_strerror(ERR_TABLE).decode() in str(ei.value)
    d = ctx.dev_alloc(64)
    try:
        assert L.bns_build_minimize_add(h, d, d, 0, 0, None) == ERR_STATE
    finally:
        ctx.dev_free(d)
    assert L.bns_build_minimize_begin(h, 50, 0) == ERR_STATE
    assert L.bns_build_finish(h, hdr.ctypes.data_as(u64p)) == ERR_STATE
    assert L.bns_build_add(h, None, None, 0, 0, None, None) == ERR_STATE
    assert L.bns_build_end(h) == 0
    # a window beyond the comb set on the encoder: the session did not score every k-mer
    ctx.set_window(50, 0)
    ctx.build_begin(64)
    assert L.bns_build_minimize_begin(h, 50, 0) == ERR_STATE and "bns_set_window" in err()
    ctx.build_end()
    configure(ctx, 31, None, True, wld.parent)
    # after finish
    ctx.build_begin(1 << 16)
    add_batch(ctx, [wld.genomes[leaves[0]]], [leaves[0]])
    ctx.build_finish()
    assert L.bns_build_minimize_begin(h, 50, 0) == ERR_STATE
    assert L.bns_build_minimize_add(h, None, None, 0, 0, None) == ERR_STATE
    ctx.build_end()
    ctx.build_begin(1 << 16)
    add_batch(ctx, [wld.genomes[leaves[0]]], [leaves[0]])
    ctx.build_minimize_begin(50)
    minimize_batch(ctx, [wld.genomes[leaves[0]]])
    ctx.build_finish()
    assert L.bns_build_minimize_add(h, None, None, 0, 0, None) == ERR_STATE
    assert L.bns_build_minimize_begin(h, 50, 0) == ERR_STATE
    ctx.build_end()
    # a fresh session on the same context works afterwards
    seqs = [wld.genomes[l].tobytes() for l in leaves]
    F = mm.full_map(oracle, wld.tax, seqs, leaves, 31)
    exp_keys, exp_vals = mm.sorted_pairs(mm.select(F, mm.depths(wld.parent), seqs, 31, 50))
    hdr, flags, keys, vals, sa, sm = run_minimize(ctx, [(seqs, leaves)], [seqs], 50, hint_f=1 << 16)
    check_table(oracle, hdr, flags, keys, vals, exp_keys, exp_vals)


# ---- 6. one lookup per position ----------------------------------------------------------------------------------------------
def test_one_lookup_per_position(ctx, oracle, small_world):
    """four random sequences of 100 000 bases, k 31, w 50: every position is looked up once per 2048-base chunk -- 19 re-read per
    1920 windows --, not once per round that reads it (which would be 2.0)"""
    rng = np.random.default_rng(6)
    seqs = [synth.rand_seq(rng, 100000) for _ in range(4)]
    taxids = list(small_world.genomes)[:4]
    configure(ctx, 31, None, True, small_world.parent)
    valid = sum(s.size - 30 for s in seqs)
    hdr, flags, keys, vals, sa, sm = run_minimize(ctx, [(seqs, taxids)], [seqs], 50, hint_f=1 << 20, hint_m=1 << 18)
    print("valid positions %d, looked up %d (%.4f), %r" % (valid, sm["lookups"], sm["lookups"] / valid, sm))
    assert sm["grows"] == 0 and sm["batches"] == 1
    assert valid <= sm["lookups"] <= 1.05 * valid
    assert 0 < sm["keys"] == int(hdr[2]) < sa["keys"]
