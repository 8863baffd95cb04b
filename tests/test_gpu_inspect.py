"""bns_table_tally / Context.table_tally(): the keys of the loaded table per taxon bin and per clade, walked on the device in every
layout, against the numpy model of tests/inspect_model.py -- exactly, and sum(direct) == table_info()'s key count in every case."""
import ctypes as C

import numpy as np
import pytest

import bonsai_amd
import inspect_model
import synth
from bonsai_amd import _lib
from test_gpu_report import subtree_sums

pytestmark = pytest.mark.gpu

LAYOUTS = [_lib.LAYOUT_MINBUCKET, _lib.LAYOUT_BUCKET, _lib.LAYOUT_KHASH]
ERR_ARG, ERR_STATE = -1, -4
# small_world's 26341 keys in 2750 home buckets (95.8 % load).  Chosen once on an MI355X, where the twelve tables below (fill 1 and 2,
# spans 8 / 11 / 15, identity 32 and 52) came out with 4535 (fill 2, span 8, identity 32) to 6385 (fill 1, span 15, identity 52) keys
# outside their home bucket and 3870 to 5573 keys in the overflow table; 2800 and 2900 buckets gave 3388 to 5408 overflow keys.
CROWDED_BUCKETS = 2750


def khash_arrays(keys, vals, seed=1):
    """khash-shaped arrays holding keys[i] -> vals[i] at arbitrary slots of a power-of-two table (the loader walks the slots; only
    LAYOUT_KHASH's probe needs kh_put's positions, and these tables are never probed in that layout)"""
    keys = np.asarray(keys, dtype=np.uint64); vals = np.asarray(vals, dtype=np.uint32)
    nb = 16
    while nb < 2 * keys.size:
        nb *= 2
    slots = np.random.default_rng(seed).permutation(nb)[:keys.size]
    flags = np.full(nb >> 4, 0xAAAAAAAA, dtype=np.uint32)
    np.bitwise_and.at(flags, slots >> 4, ~(np.uint32(3) << ((slots & 15) << 1).astype(np.uint32)))
    k = np.zeros(nb, np.uint64); v = np.zeros(nb, np.uint32)
    k[slots], v[slots] = keys, vals
    return nb, flags, k, v


def check(ctx, flags, keys, vals, parent, tag=None):
    direct, clade = ctx.table_tally()
    want_d, want_c = inspect_model.model(flags, keys, vals, parent)
    assert direct.dtype == np.uint64 and direct.size == len(parent) + 1
    assert int(direct.sum()) == ctx.table_info()["n_keys"] == int(want_d.sum()), tag
    assert np.array_equal(direct, want_d), tag
    assert np.array_equal(clade, want_c), tag
    return direct, clade


@pytest.fixture()
def ctx():
    c = bonsai_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_small_world_default_sizing(ctx, small_world, layout):
    w = small_world
    ctx.set_encoder(31, None, canonicalize=True)
    ctx.load_table(w.n_buckets, w.flags, w.keys, w.vals, layout=layout)
    ctx.load_taxonomy(w.parent)
    direct, clade = check(ctx, w.flags, w.keys, w.vals, w.parent)
    assert np.array_equal(clade, subtree_sums(direct))                 # (the DFS of the -R tests agrees with the model)
    assert direct[0] == 0 and direct[w.parent.size] == 0 and clade[1] == ctx.table_info()["n_keys"]
    # either output alone
    n = w.parent.size
    only = np.zeros(n + 1, np.uint64)
    assert ctx.L.bns_table_tally(ctx.h, None, only.ctypes.data_as(_lib.u64p), n + 1) == 0 and np.array_equal(only, clade)
    assert ctx.L.bns_table_tally(ctx.h, only.ctypes.data_as(_lib.u64p), None, n + 1) == 0 and np.array_equal(only, direct)
    assert ctx.L.bns_table_tally(ctx.h, None, None, n + 1) == 0
    # whole lines instead of their upper halves (the A/B switch of the clustered walk): the same counts
    ctx.debug_set(0x80)
    try:
        check(ctx, w.flags, w.keys, w.vals, w.parent, "whole lines")
    finally:
        ctx.debug_set(0)


@pytest.mark.parametrize("bits", [32, 52])
@pytest.mark.parametrize("span", [8, 11, 15])
@pytest.mark.parametrize("fill", [1, 2])
def test_crowded_minbucket(ctx, small_world, fill, span, bits):
    """keys down their chains, in spill-only buckets and in the overflow table: nothing counted twice, nothing left out"""
    w = small_world
    ctx.set_encoder(31, None, canonicalize=True)
    ctx.set_table_buckets(CROWDED_BUCKETS)
    ctx.set_table_fill(fill)
    ctx.set_minimizer_span(span)
    ctx.set_minimizer_identity(bits)
    ctx.load_table(w.n_buckets, w.flags, w.keys, w.vals, layout=_lib.LAYOUT_MINBUCKET)
    ctx.load_taxonomy(w.parent)
    geo = ctx.table_geometry()
    assert geo["buckets"] == CROWDED_BUCKETS and geo["spilled_keys"] > 0 and geo["overflow_keys"] > 0, geo
    check(ctx, w.flags, w.keys, w.vals, w.parent, geo)


def fold(key):
    lo, hi = key & 0xFFFFFFFF, key >> 32
    return lo ^ (((hi << 15) | (hi >> 17)) & 0xFFFFFFFF)


def test_bucket_without_a_perfect_hash(ctx):
    """two keys with one fold in one bucket: no multiplier separates them, the bucket's keys move to the overflow table and the bucket
    reads MINB_N_IN_OVF -- counted there, once"""
    keys = [0x0123456789ABCDEF >> 2, 0x1F2E3D4C5B6A7988 >> 2, 0x0000000012345678, 0x2AAAAAAA55555555, 0x3FFFFFFF00000001, 7, 0x1000000000000000]
    a = keys[0]
    hi_b = 0x0BADF00D
    b = (hi_b << 32) | (fold(a) ^ (((hi_b << 15) | (hi_b >> 17)) & 0xFFFFFFFF))
    assert fold(b) == fold(a) and b != a and b < (1 << 62)
    keys.append(b)
    vals = [1001, 1002, 1003, 1004, 2001, 2002, 101, 1001]
    nb, f, k, v = khash_arrays(keys, vals)
    parent = synth_parent()
    ctx.set_encoder(31, None, canonicalize=True)
    ctx.set_table_buckets(1)                                            # 8 keys, one home bucket (the loader wants 9.7 slots per 10 keys)
    ctx.load_table(nb, f, k, v, layout=_lib.LAYOUT_MINBUCKET)
    ctx.load_taxonomy(parent)
    assert ctx.table_geometry()["buckets"] == 1
    assert ctx.table_stats()["n_overflow_keys"] > 0
    direct, _ = check(ctx, f, k, v, parent)
    assert direct[1001] == 2 and direct.sum() == 8


def synth_parent():
    parent = np.full(2003, _lib.TAX_ABSENT, np.uint32)
    for c, p in synth.TAX_PAIRS:
        parent[c] = 0 if c == 1 else p
    return parent


@pytest.mark.parametrize("layout", LAYOUTS)
def test_deleted_flags(ctx, small_world, layout):
    """nine present keys in ten marked deleted: neither empty nor deleted slots count"""
    w = small_world
    flags = w.flags.copy()
    idx = np.arange(w.n_buckets)
    pres_idx = idx[inspect_model.present_mask(flags, w.n_buckets)]
    drop = pres_idx[np.arange(pres_idx.size) % 10 != 0]
    np.bitwise_or.at(flags, drop >> 4, (np.uint32(1) << ((drop & 15) << 1).astype(np.uint32)))      # bit 0 of the pair: deleted
    ctx.set_encoder(31, None, canonicalize=True)
    ctx.load_table(w.n_buckets, flags, w.keys, w.vals, layout=layout)
    ctx.load_taxonomy(w.parent)
    direct, _ = check(ctx, flags, w.keys, w.vals, w.parent)
    assert direct.sum() == pres_idx.size - drop.size


@pytest.mark.parametrize("layout", LAYOUTS)
def test_values_outside_the_taxonomy(ctx, small_world, layout):
    w = small_world
    parent = w.parent.copy()
    n = parent.size
    assert parent[1500] == _lib.TAX_ABSENT and parent[1600] == _lib.TAX_ABSENT and parent[1601] == _lib.TAX_ABSENT
    parent[1600] = 1601                                                 # a key under an id that is not one: a broken chain
    vals = w.vals.copy()
    pres = np.nonzero(inspect_model.present_mask(w.flags, w.n_buckets))[0]
    odd = [0, n, 7777, 0xFFFFFFFF, 1500, 1600, 1601]
    for j, t in enumerate(odd):
        vals[pres[j::40][:50 + j]] = t
    ctx.set_encoder(31, None, canonicalize=True)
    ctx.load_table(w.n_buckets, w.flags, w.keys, vals, layout=layout)
    ctx.load_taxonomy(parent)
    direct, clade = check(ctx, w.flags, w.keys, vals, parent)
    assert direct[0] == 50 and clade[0] == 50
    assert direct[n] == sum(50 + j for j in range(1, len(odd))) and clade[n] == direct[n]
    assert direct[1500] == 0 and direct[1600] == 0 and clade[1600] == 0


def leaf_taxonomy():
    """root 1, fifty inner nodes 2..51, five thousand leaves 100..5099"""
    parent = np.full(5100, _lib.TAX_ABSENT, np.uint32)
    parent[1] = 0
    parent[2:52] = 1
    parent[100:5100] = 2 + np.arange(5000) % 50
    return parent


TINY = 0x8          # bns_debug_set: bns_table_tally launches at most 4 workgroups, which flush their LDS counters every 3 rounds


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", ["one_value", "round_robin"])
def test_combining_paths(ctx, layout, case):
    """200 000 keys on one value: many workgroups add to one counter.  100 000 keys over 5 000 leaf values in round-robin: with the
    full grid a workgroup sees a few hundred keys at most (the grid is sized from the table), so the walk is repeated with at most 4
    workgroups (TINY): each then takes a quarter of the table in hundreds of grid-stride rounds and meets all 5 000 bins, five times
    the TALLY_SLOTS = 1024 its LDS hash holds between two flushes, so bins that find no slot within TALLY_PROBES go straight to HBM;
    the counters are flushed every 3 rounds, in the middle of the walk."""
    parent = leaf_taxonomy()
    rng = np.random.default_rng(9)
    if case == "one_value":
        keys = rng.integers(0, 1 << 62, 200000, dtype=np.uint64)
        vals = np.full(keys.size, 4242, np.uint32)
    else:
        keys = rng.integers(0, 1 << 62, 100000, dtype=np.uint64)
        vals = (100 + np.arange(keys.size) % 5000).astype(np.uint32)
    keys = np.unique(keys)
    vals = vals[:keys.size]
    nb, f, k, v = khash_arrays(keys, vals)
    ctx.set_encoder(31, None, canonicalize=True)
    ctx.load_table(nb, f, k, v, layout=layout)
    ctx.load_taxonomy(parent)
    for bits in (0, TINY):
        ctx.debug_set(bits)
        try:
            direct, clade = check(ctx, f, k, v, parent, bits)
        finally:
            ctx.debug_set(0)
        assert clade[1] == keys.size
        if case == "one_value":
            assert direct[4242] == keys.size
        else:
            assert np.count_nonzero(direct) == 5000


def test_full_lds_hash_in_one_round(ctx):
    """The default layout, the full grid, no switch: 100 000 keys over 5 000 leaf values in 10 400 home buckets (96 % load) are 41
    workgroups of 256 buckets, about 2 400 keys and so about 1 900 distinct bins each -- more than the LDS hash's 1024 slots in a
    workgroup's single round, so the adds past TALLY_PROBES reach HBM one by one."""
    parent = leaf_taxonomy()
    keys = np.unique(np.random.default_rng(10).integers(0, 1 << 62, 100000, dtype=np.uint64))
    vals = (100 + np.random.default_rng(11).permutation(keys.size) % 5000).astype(np.uint32)
    nb, f, k, v = khash_arrays(keys, vals)
    ctx.set_encoder(31, None, canonicalize=True)
    ctx.set_table_buckets(10400)
    ctx.load_table(nb, f, k, v, layout=_lib.LAYOUT_MINBUCKET)
    ctx.load_taxonomy(parent)
    assert ctx.table_geometry()["buckets"] == 10400
    direct, _ = check(ctx, f, k, v, parent)
    assert np.count_nonzero(direct) == 5000


@pytest.mark.parametrize("layout", LAYOUTS)
def test_grid_stride_rounds(ctx, small_world, layout):
    """at most 4 workgroups over small_world's table (TINY): every workgroup runs many rounds of its grid-stride loop, the last of them
    past the table's end, and flushes its counters between them; the crowded clustered table adds chains and the overflow table"""
    w = small_world
    ctx.set_encoder(31, None, canonicalize=True)
    for buckets in ((0, CROWDED_BUCKETS) if layout == _lib.LAYOUT_MINBUCKET else (0,)):
        ctx.set_table_buckets(buckets)
        ctx.load_table(w.n_buckets, w.flags, w.keys, w.vals, layout=layout)
        ctx.load_taxonomy(w.parent)
        ctx.debug_set(TINY)
        try:
            check(ctx, w.flags, w.keys, w.vals, w.parent, buckets)
            ctx.debug_set(TINY | 0x80)                                  # (whole lines)
            check(ctx, w.flags, w.keys, w.vals, w.parent, buckets)
        finally:
            ctx.debug_set(0)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_key_zero_is_a_key(ctx, layout):
    keys = [0, 1, 2, 0x2AAAAAAAAAAAAAAA]
    nb, f, k, v = khash_arrays(keys, [1001, 1002, 1001, 2002])
    ctx.set_encoder(31, None, canonicalize=True)
    ctx.load_table(nb, f, k, v, layout=layout)
    ctx.load_taxonomy(synth_parent())
    direct, _ = check(ctx, f, k, v, synth_parent())
    assert direct[1001] == 2 and direct.sum() == 4


def test_all_ones_key_of_an_uncanonical_k32_table(ctx, oracle):
    """~0 is the all-T 32-mer, and what unused slots of the clustered layout hold: occupancy comes from the header's bits.  probe() finds
    the key in every layout, and the walk counts it."""
    t = oracle.Table()
    keys = np.array([0xFFFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFE, 0x0123456789ABCDEF, 0], dtype=np.uint64)
    vals = np.array([1003, 1001, 1002, 1004], dtype=np.uint32)
    t.insert_many(keys, vals)
    f, k, v = t.arrays()
    for layout in LAYOUTS:
        ctx.set_encoder(32, None, canonicalize=False)
        ctx.load_table(t.n_buckets, f, k, v, layout=layout)
        ctx.load_taxonomy(synth_parent())
        got, found = ctx.probe(keys)
        assert found.all() and np.array_equal(got, vals), layout
        direct, _ = check(ctx, f, k, v, synth_parent(), layout)
        assert direct[1003] == 1 and direct.sum() == 4, layout


def test_state_and_errors(ctx, small_world):
    w = small_world
    n = w.parent.size
    buf = np.zeros(n + 1, np.uint64)
    p = buf.ctypes.data_as(_lib.u64p)
    assert ctx.L.bns_table_tally(ctx.h, p, None, n + 1) == ERR_STATE                      # no table
    with pytest.raises(bonsai_amd.BonsaiAmdError):
        ctx.table_tally()
    ctx.set_encoder(31, None, canonicalize=True)
    ctx.load_table(w.n_buckets, w.flags, w.keys, w.vals)
    assert ctx.L.bns_table_tally(ctx.h, p, None, n + 1) == ERR_STATE                      # no taxonomy
    ctx.load_taxonomy(w.parent)
    assert ctx.L.bns_table_tally(ctx.h, p, None, n) == ERR_ARG
    assert ctx.L.bns_table_tally(ctx.h, p, None, n + 2) == ERR_ARG
    assert ctx.L.bns_table_tally(None, p, None, n + 1) == ERR_ARG
    first, _ = check(ctx, w.flags, w.keys, w.vals, w.parent)
    # a second table: its counts
    nb, f, k, v = khash_arrays([5, 6, 7], [1001, 1001, 2002])
    ctx.load_table(nb, f, k, v, layout=_lib.LAYOUT_BUCKET)
    second, _ = check(ctx, f, k, v, w.parent)
    assert second.sum() == 3 and not np.array_equal(first, second)
    # the read tally and the table tally do not touch each other
    ctx.load_table(w.n_buckets, w.flags, w.keys, w.vals)
    ctx.tally_enable()
    try:
        reads = synth.simulate_reads(np.random.default_rng(2), w.genomes, 500)
        ctx.classify(*synth.concat(reads))
        before = ctx.tally()
        assert before[0].sum() == 500
        table = ctx.table_tally()
        after = ctx.tally()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        again = ctx.table_tally()
        assert np.array_equal(table[0], again[0]) and np.array_equal(table[1], again[1]) and np.array_equal(table[0], first)
    finally:
        ctx.tally_enable(False)


def test_two_contexts_of_a_multi_load(small_world):
    """every context of bns_load_table_multi holds the whole table: each returns the whole answer (callers do not add them up)"""
    w = small_world
    a, b = bonsai_amd.Context(0), bonsai_amd.Context(0)
    try:
        for c in (a, b):
            c.set_encoder(31, None, canonicalize=True)
        arr = (C.c_void_p * 2)(a.h, b.h)
        f, k, v = (np.ascontiguousarray(x) for x in (w.flags, w.keys, w.vals))
        rc = a.L.bns_load_table_multi(arr, 2, w.n_buckets, f.ctypes.data_as(_lib.u32p), k.ctypes.data_as(_lib.u64p), v.ctypes.data_as(_lib.u32p),
                                      _lib.LAYOUT_MINBUCKET)
        assert rc == 0, a.L.bns_last_error(a.h)
        for c in (a, b):
            c.load_taxonomy(w.parent)
        da, ca = check(a, w.flags, w.keys, w.vals, w.parent, "root")
        db, cb = check(b, w.flags, w.keys, w.vals, w.parent, "replica")
        assert np.array_equal(da, db) and np.array_equal(ca, cb)
    finally:
        a.close(); b.close()
