"""The window session on the device (bns_windows_begin / _add / _read / _end: windows_lookup_kernel, windows_vote_kernel) against
tests/windows_model.py: every window cut out and classified by the CPU oracle as a read of its own.  Equality throughout: the whole
d_taxon image, 0xFFFFFFFF positions included, and the pair counts."""
import numpy as np
import pytest

import bonsai_amd
import synth
import windows_model as WM
from bonsai_amd import _lib

pytestmark = pytest.mark.gpu

LAYOUTS = [_lib.LAYOUT_KHASH, _lib.LAYOUT_BUCKET, _lib.LAYOUT_MINBUCKET]
T = _lib.WINDOWS_TILE                     # the vote kernel's tile: window starts per wavefront
FAST_TAXA = _lib.WINDOWS_FAST_TAXA        # distinct taxa of a window the register counter holds
ERR_ARG, ERR_STATE = -1, -4
K = 31


def load(c, w, layout=_lib.LAYOUT_MINBUCKET, spaced_intended=True, arrays=None, parent=None):
    flags, keys, vals = arrays or (w.flags, w.keys, w.vals)
    c.set_encoder(w.k, w.gaps, canonicalize=w.canon, spaced_intended=spaced_intended)
    c.load_table(keys.size, flags, keys, vals, layout=layout)
    c.load_taxonomy(w.parent if parent is None else parent)


class Batch:
    """a batch on the device; add() runs bns_windows_add of the open session and returns the d_taxon image"""

    def __init__(self, c, seqs, taxids):
        self.c = c
        self.bases, self.offsets = synth.concat(seqs)
        self.taxids = np.ascontiguousarray(taxids, dtype=np.uint32)
        self.n, self.total = len(seqs), int(self.offsets[-1])
        self.bufs = []
        self.d_bases, self.d_offsets, self.d_taxid = (self.up(a) for a in (self.bases, self.offsets, self.taxids))
        self.d_taxon = c.dev_alloc(4 * self.total + 8); self.bufs.append(self.d_taxon)

    def up(self, a):
        p = self.c.dev_alloc(a.nbytes + 8)
        if a.nbytes:
            self.c.dev_upload(p, a)
        self.bufs.append(p)
        return p

    def add(self, want_taxon=True):
        self.c.windows_add(self.d_bases, self.d_offsets, self.n, self.total, self.d_taxid, self.d_taxon if want_taxon else None)
        self.c.sync()
        out = np.zeros(self.total, dtype=np.uint32)
        if want_taxon and self.total:
            self.c.dev_download(self.d_taxon, out)
        return out

    def free(self):
        for p in self.bufs:
            self.c.dev_free(p)
        self.bufs = []


def session(c, seqs, taxids, L, pair_cap=1 << 12):
    """one session over one batch -> (image, (seq_taxid, called, count, n_dropped))"""
    bases, offsets = synth.concat(seqs)
    return c.classify_windows(bases, offsets, taxids, L, pair_cap=pair_cap)


def same_pairs(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got[:3], want))


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.windows_end()
    gpu_ctx.set_confidence(0)
    gpu_ctx.tally_enable(False)
    gpu_ctx.sketch_enable(0)


# ---- 1. equality on small_world ------------------------------------------------------------------------------------------------
WINDOW_LENS = [31, 32, 150, 600, 6000, 6001]      # one k-mer per window, two, the usual length, a long one, exactly one window, none


@pytest.fixture(scope="module")
def worlds(oracle, small_world):
    return {True: small_world, False: synth.make_world(oracle, seed=11, k=K, genome_len=6000, canon=False)}


def genome_batch(w):
    seqs, taxids = [], []
    for leaf in synth.LEAVES:
        g = w.genomes[leaf]
        seqs += [g, synth.mutate(np.random.default_rng(leaf), g, 0.01, 0.002)]
        taxids += [leaf, leaf]
    return seqs, taxids


@pytest.fixture(scope="module")
def genome_models(oracle, worlds):
    cache = {}

    def get(canon, L):
        if (canon, L) not in cache:
            w = worlds[canon]
            seqs, taxids = genome_batch(w)
            bases, offsets = synth.concat(seqs)
            cache[(canon, L)] = WM.windows(oracle, w.table, w.tax, K, bases, offsets, taxids, L, canon=canon)
        return cache[(canon, L)]
    return get


def test_the_input_is_not_trivial(genome_models):
    image, _ = genome_models(True, 31)
    called = image[image != WM.NONE]
    leaf = np.isin(called, synth.LEAVES)
    print("L = 31: %d called 0, %d at a leaf, %d above, of %d" % ((called == 0).sum(), leaf.sum(), ((called != 0) & ~leaf).sum(), called.size))
    assert (called == 0).sum() >= 1000 and leaf.sum() >= 1000 and ((called != 0) & ~leaf).sum() >= 1000


@pytest.mark.parametrize("canon", [True, False])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_equality_on_small_world(ctx, worlds, genome_models, layout, canon):
    w = worlds[canon]
    load(ctx, w, layout)
    seqs, taxids = genome_batch(w)
    for L in WINDOW_LENS:
        want_image, want_pairs = genome_models(canon, L)
        image, got = session(ctx, seqs, taxids, L)
        assert (want_image != WM.NONE).sum() == sum(WM.n_windows(s.size, L) for s in seqs)
        assert np.array_equal(image, want_image), L
        assert same_pairs(got, want_pairs) and got[3] == 0, L


def test_a_window_whose_hit_list_does_not_fit_lds(ctx, oracle, small_world):
    """tile + halo beyond WINDOWS_LDS_LIST positions: the vote kernel's other form, the compacted hit list in global memory"""
    w, L = small_world, 12000
    assert T + L - K > _lib.WINDOWS_LDS_LIST and L - K + 1 <= 65535
    seq = np.concatenate([w.genomes[1001], synth.mutate(np.random.default_rng(4), w.genomes[1003], 0.01, 0.002), w.genomes[2001][:2300]])
    seqs, taxids = [seq, w.genomes[1002], seq[:L]], [1001, 1002, 2001]          # 2301 windows, none, one
    bases, offsets = synth.concat(seqs)
    want_image, want_pairs = WM.windows(oracle, w.table, w.tax, K, bases, offsets, taxids, L)
    assert np.unique(want_image).size > 3
    for layout in LAYOUTS:
        load(ctx, w, layout)
        image, got = session(ctx, seqs, taxids, L)
        assert np.array_equal(image, want_image), layout
        assert same_pairs(got, want_pairs) and got[3] == 0


# ---- 2. ties and many taxa -----------------------------------------------------------------------------------------------------
def chimera(w):
    rng = np.random.default_rng(7)
    parts = []
    for i in range(60):
        g = w.genomes[synth.LEAVES[i % 6]]
        at = int(rng.integers(0, g.size - 45))
        parts.append(g[at:at + 45])
    return np.concatenate(parts)


def test_ties_and_many_taxa(ctx, oracle, small_world):
    w = small_world
    seq = chimera(w)
    assert seq.size == 2700
    ties, most = 0, 0
    for p in range(seq.size - 150 + 1):
        taxon, _, _, hits = oracle.classify_seq(w.table, w.tax, K, seq[p:p + 150].tobytes())
        ties += taxon not in hits.tolist()
        most = max(most, np.unique(hits).size)
    print("L = 150: %d windows whose call is not among their hits, up to %d distinct taxa" % (ties, most))
    assert ties >= 100
    for layout in LAYOUTS:
        load(ctx, w, layout)
        for L in (90, 150, 600):
            want_image, want_pairs = WM.windows(oracle, w.table, w.tax, K, seq, [0, seq.size], [7], L)
            image, got = session(ctx, [seq], [7], L)
            assert np.array_equal(image, want_image), (layout, L)
            assert same_pairs(got, want_pairs) and got[3] == 0


# ---- 3. beyond any fixed capacity ----------------------------------------------------------------------------------------------
def test_more_taxa_than_the_fast_path_holds(ctx, oracle):
    pairs = [(1, 1)] + [(i, 1) for i in range(2, 302)]
    tax = oracle.Taxonomy(pairs=pairs)
    seq = synth.rand_seq(np.random.default_rng(5), 12000)
    table = oracle.Table()
    for i in range(300):
        oracle.lca_map_add(table, tax, K, seq[40 * i:40 * i + 40].tobytes(), 2 + i)
    L = 4000
    most = max(np.unique(oracle.classify_seq(table, tax, K, seq[p:p + L].tobytes())[3]).size for p in range(0, seq.size - L + 1, 500))
    assert most > FAST_TAXA, most
    want_image, want_pairs = WM.windows(oracle, table, tax, K, seq, [0, seq.size], [2], L)
    ctx.set_encoder(K, None, canonicalize=True)
    flags, keys, vals = table.arrays()
    ctx.load_taxonomy(tax.parent)
    for layout in LAYOUTS:
        ctx.load_table(keys.size, flags, keys, vals, layout=layout)
        image, got = session(ctx, [seq], [2], L)
        assert np.array_equal(image, want_image), layout
        assert same_pairs(got, want_pairs) and got[3] == 0


# ---- 4. seams and edges --------------------------------------------------------------------------------------------------------
def edge_sequences(w, L):
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 401, size=1000)
    lens[:4] = [0, L - 1, L, L + 1]

    def piece(i, n):
        g = w.genomes[synth.LEAVES[i % 6]]
        at = int(rng.integers(0, g.size - n + 1))
        return g[at:at + n].copy()
    many = [piece(i, int(n)) for i, n in enumerate(lens)]
    assert any(s.size == 0 for s in many) and any(0 < s.size < L for s in many) and any(s.size == L for s in many)
    assert any(o % 2 for o in np.cumsum([s.size for s in many]).tolist())
    seams = [piece(i, n) for i, n in enumerate([L + 63, L + 64, L + 65, T + L - 2, T + L - 1, T + L])]
    g = w.genomes[1001]
    across_chunk = g[:2600].copy(); across_chunk[2048 - 80:2048 + L - 60] = ord("N")         # a run of N longer than L across base 2048
    assert (across_chunk == ord("N")).sum() > L
    head = g[3000:3100].copy()                                                                # (so that the next one starts off a tile edge)
    across_tile = g[1000:2200].copy()
    edge = -(-(sum(s.size for s in seams) + across_chunk.size + head.size + 300) // T) * T    # a tile edge of the batch inside across_tile
    at = edge - (sum(s.size for s in seams) + across_chunk.size + head.size)
    across_tile[at - 70:at + L - 50] = ord("N")
    lower = g[4000:4600].copy(); lower[100:400] |= 0x20
    return many, seams + [across_chunk, head, across_tile, lower]


def test_seams_and_edges(ctx, oracle, small_world):
    w, L = small_world, 150
    vals = w.vals.copy()
    vals[vals == 1003] = 1500                     # a value that is no node of the taxonomy
    vals[vals == 1004] = 0                        # and the value 0: a hit all the same
    assert (vals == 1500).any() and (vals == 0).sum() > 1000 and w.parent[1500] == _lib.TAX_ABSENT
    table = oracle.Table.wrap(*w.table.header(), w.flags.copy(), w.keys.copy(), vals)
    models = []
    for seqs in edge_sequences(w, L):
        taxids = [synth.LEAVES[i % 6] for i in range(len(seqs))]
        bases, offsets = synth.concat(seqs)
        models.append((seqs, taxids, WM.windows(oracle, table, w.tax, K, bases, offsets, taxids, L)))
    for layout in LAYOUTS:
        load(ctx, w, layout, arrays=(w.flags, w.keys, vals))
        for seqs, taxids, (want_image, want_pairs) in models:
            image, got = session(ctx, seqs, taxids, L)
            assert np.array_equal(image, want_image), (layout, len(seqs))
            assert same_pairs(got, want_pairs) and got[3] == 0


# ---- 5. a spaced seed ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_spaced_seed(ctx, oracle, layout):
    w = synth.make_world(oracle, seed=14, k=K, genome_len=3000, gaps=[1] * 15 + [0] * 15)
    seqs = [w.genomes[leaf] for leaf in synth.LEAVES]
    bases, offsets = synth.concat(seqs)
    for intended in (True, False):
        want_image, want_pairs = WM.windows(oracle, w.table, w.tax, K, bases, offsets, synth.LEAVES, 150, gaps=w.gaps, spaced_intended=intended)
        called = want_image[want_image != WM.NONE]
        assert (called != 0).sum() > 10000 if intended else not called.any()      # through the string for_each a spaced seed emits nothing
        load(ctx, w, layout, spaced_intended=intended)
        image, got = session(ctx, seqs, synth.LEAVES, 150)
        assert np.array_equal(image, want_image), intended
        assert same_pairs(got, want_pairs) and got[3] == 0


# ---- 6. pairs ------------------------------------------------------------------------------------------------------------------
def test_pairs(ctx, oracle, small_world):
    w, L, c = small_world, 150, ctx
    load(c, w)
    rng = np.random.default_rng(12)
    halves = []
    for h in range(2):
        seqs = [synth.mutate(rng, w.genomes[leaf][1000 * h:1000 * h + 2500], 0.02, 0.002) for leaf in synth.LEAVES] + [w.genomes[1001][:100]]
        taxids = synth.LEAVES + [1002]
        bases, offsets = synth.concat(seqs)
        halves.append((seqs, taxids, WM.windows(oracle, w.table, w.tax, K, bases, offsets, taxids, L)[1]))
    want = WM.merge_pairs(halves[0][2], halves[1][2])
    assert want[0].size > 4
    batches = [Batch(c, seqs, taxids) for seqs, taxids, _ in halves]
    try:
        c.windows_begin(L, 1 << 10)
        for b in batches:
            b.add()
        got = c.windows()
        assert same_pairs(got, want) and got[3] == 0
        assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and got[2].dtype == np.uint64
        order = (got[0].astype(np.uint64) << np.uint64(32)) | got[1]
        assert (np.diff(order.astype(np.int64)) > 0).all()
        for leaf in set(synth.LEAVES) | {1002}:                       # per genome taxid: every window counted once
            lens = [s.size for seqs, taxids, _ in halves for s, t in zip(seqs, taxids) if t == leaf]
            assert int(got[2][got[0] == leaf].sum()) == sum(WM.n_windows(n, L) for n in lens)
        assert same_pairs(c.windows(reset=True), want)
        empty = c.windows()
        assert empty[0].size == 0 and empty[3] == 0
        for b in batches:                                             # d_taxon = NULL: the same pairs
            b.add(want_taxon=False)
        assert same_pairs(c.windows(), want)
        c.windows_end()
        # a table of 4 slots under more than 4 pairs: what is stored is exact, the rest is counted as dropped
        c.windows_begin(L, 4)
        for b in batches:
            b.add()
        s, t, n, dropped = c.windows()
        full = {(a, b_): k_ for a, b_, k_ in zip(*(x.tolist() for x in want))}
        assert 0 < s.size <= 4 and dropped > 0
        assert all(full.get((a, b_)) == k_ for a, b_, k_ in zip(s.tolist(), t.tolist(), n.tolist()))
        assert int(n.sum()) + dropped == int(want[2].sum())
    finally:
        c.windows_end()
        for b in batches:
            b.free()


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------
def test_errors(ctx, small_world):
    w = small_world
    bare = bonsai_amd.Context(0)
    try:
        assert bare.L.bns_windows_begin(bare.h, 150, 16) == ERR_STATE            # no encoder
        bare.set_encoder(K, None, canonicalize=True)
        assert bare.L.bns_windows_begin(bare.h, 150, 16) == ERR_STATE            # no table
        bare.load_table(w.n_buckets, w.flags, w.keys, w.vals)
        assert bare.L.bns_windows_begin(bare.h, 150, 16) == ERR_STATE            # no taxonomy
        n = np.zeros(1, np.uint64)
        assert bare.L.bns_windows_read(bare.h, None, None, None, 0, n.ctypes.data_as(_lib.u64p), None, 0) == ERR_STATE
        assert bare.L.bns_windows_add(bare.h, None, None, 0, 0, None, None, None) == ERR_STATE
        assert bare.L.bns_windows_end(bare.h) == 0                               # legal at any point
    finally:
        bare.close()
    c = ctx
    load(c, w)
    L_ = c.L
    assert L_.bns_windows_begin(c.h, K - 1, 16) == ERR_ARG
    assert L_.bns_windows_begin(c.h, K + 65535, 16) == ERR_ARG
    assert L_.bns_windows_begin(c.h, 150, 0) == ERR_ARG
    c.set_confidence(0.5)
    assert L_.bns_windows_begin(c.h, 150, 16) == ERR_STATE
    c.set_confidence(0)
    assert L_.bns_windows_begin(c.h, K + 65534, 16) == 0                         # the longest window there is
    assert L_.bns_windows_begin(c.h, 150, 16) == ERR_STATE                       # a second begin
    c.windows_end()
    b = Batch(c, [w.genomes[1001][:1000], w.genomes[2001][:1000]], [1001, 2001])
    try:
        c.windows_begin(150, 16)
        c.set_confidence(0.5)                                                    # turned on during a session
        assert L_.bns_windows_add(c.h, b.d_bases, b.d_offsets, b.n, b.total, b.d_taxid, None, None) == ERR_STATE
        c.set_confidence(0)
        b.add()
        n = np.zeros(1, np.uint64)
        seq = np.zeros(1, np.uint32)
        assert c.windows()[0].size > 1
        rc = L_.bns_windows_read(c.h, seq.ctypes.data_as(_lib.u32p), None, None, 1, n.ctypes.data_as(_lib.u64p), None, 0)
        assert rc == ERR_ARG and int(n[0]) == c.windows()[0].size
    finally:
        c.windows_end()
        b.free()


def test_stage_timing(ctx, small_world):
    c, w = ctx, small_world
    load(c, w)
    b = Batch(c, [w.genomes[1001]], [1001])
    ms = (_lib.C.c_double * 3)()
    try:
        c.windows_begin(150, 16)                                                 # begun with timing off: nothing to report
        assert c.L.bns_windows_timing(c.h, ms, None) == ERR_STATE
        c.windows_end()
        assert c.L.bns_windows_timing(c.h, ms, None) == ERR_STATE                # no session
        c.set_timing(True)
        c.windows_begin(150, 16)
        want = b.add()
        b.add()
        got, n_adds = c.windows_timing()
        assert n_adds == 2 and all(v > 0 for v in got.values()) and sum(got.values()) < 1000.0
        assert c.windows_timing()[1] == 0                                        # read and started again
        assert np.array_equal(b.add(), want)
    finally:
        c.set_timing(False)
        c.windows_end()
        b.free()


# ---- 8. other features stay untouched ------------------------------------------------------------------------------------------
def test_tally_sketch_and_classify_are_untouched(ctx, small_world):
    c, w = ctx, small_world
    load(c, w)
    reads = synth.simulate_reads(np.random.default_rng(31), w.genomes, 300)
    bases, offsets = synth.concat(reads)
    before = c.classify(bases, offsets)
    c.tally_enable(True)
    c.sketch_enable(64)
    c.tally(reset=True)
    seqs = [w.genomes[leaf] for leaf in synth.LEAVES]
    image, pairs = session(c, seqs, synth.LEAVES, 150)
    assert (image != WM.NONE).sum() == 6 * (6000 - 149) and pairs[0].size > 6
    direct, clade = c.tally()[:2]
    assert not np.asarray(direct).any() and not np.asarray(clade).any()
    assert c.sketch()[0].size == 0
    c.tally_enable(False)
    c.sketch_enable(0)
    after = c.classify(bases, offsets)
    for f in ("taxon", "missing", "ambig"):
        assert np.array_equal(before[f], after[f])
