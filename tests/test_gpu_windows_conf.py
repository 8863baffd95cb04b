"""The window session with a confidence threshold of its own (bns_windows_begin_conf: the CONF form of windows_vote_kernel).

Model: every window is cut out as a read and classified by the CPU oracle (oracle.classify_batch: taxon, missing, n_hits per window);
its hits are the range [rank(p), rank(p + L - c + 1)) of the oracle's hit stream of the whole sequence (the positions come from the
oracle run on every single k-mer as a read, and the range's length must equal the window's own n_hits).  The threshold is then applied
as tests/confidence_ref.py states it.  confidence_ref.walker is a Python parent walk per hit, so every window goes through a numpy form
of the same rules built from confidence_ref.chain / in_clade (clade counts as prefix sums along the hit stream), and walker itself
checks a random sample of the windows of every case.  Second witness: the same windows cut as reads and classified on the same GPU
context with set_confidence(theta).  Equality throughout: the whole d_taxon image and the pair counts, n_dropped == 0."""
from fractions import Fraction

import numpy as np
import pytest

import bonsai_amd
import confidence_ref as cr
import synth
import windows_model as WM
from bonsai_amd import _lib
from test_gpu_windows import Batch, chimera, edge_sequences, genome_batch, load, same_pairs

pytestmark = pytest.mark.gpu

LAYOUTS = [_lib.LAYOUT_KHASH, _lib.LAYOUT_BUCKET, _lib.LAYOUT_MINBUCKET]
T = _lib.WINDOWS_TILE
ERR_ARG, ERR_STATE = -1, -4
K = 31


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.windows_end()
    gpu_ctx.set_confidence(0)


# ---- the model -----------------------------------------------------------------------------------------------------------------
def cut(seq, L):
    """every window of L bases as a read of its own -> (bases, offsets)"""
    nw = WM.n_windows(seq.size, L)
    if nw == 0:
        return np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    return (np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(seq, L)).reshape(-1),
            np.arange(nw + 1, dtype=np.uint64) * np.uint64(L))


class SeqModel:
    """one sequence: the oracle's taxon, missing and hit range of every window, and the hit stream the ranges index"""

    def __init__(self, oracle, table, tax, seq, L, c, **kw):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self.nw = WM.n_windows(seq.size, L)
        if self.nw == 0:
            return
        res = oracle.classify_batch(table, tax, K, *cut(seq, L), nthreads=16, **kw)
        one = oracle.classify_batch(table, tax, K, *cut(seq, c), nthreads=16, **kw)          # every k-mer as a read: is it a hit
        assert one["n_hits"].max(initial=0) <= 1
        rank = np.concatenate([[0], np.cumsum(one["n_hits"].astype(np.int64))])
        self.hits = oracle.classify_seq(table, tax, K, seq.tobytes(), **kw)[3].astype(np.int64)
        assert self.hits.size == rank[-1]
        p = np.arange(self.nw)
        self.lo, self.hi = rank[p], rank[p + L - c + 1]
        assert np.array_equal(self.hi - self.lo, res["n_hits"])                              # the window's own hits ARE that range
        self.taxon = res["taxon"].astype(np.int64)
        self.missing = res["missing"].astype(np.int64)

    def walk(self, par, theta):
        """the numpy form of confidence_ref.walker over all windows"""
        theta = Fraction(theta)
        num, den = theta.numerator, theta.denominator
        out = self.taxon.copy()
        if self.nw == 0 or num == 0:
            return out
        q = (self.hi - self.lo) + self.missing
        assert num * 65536 < 2 ** 62
        r = (num * q + den - 1) // den
        vals, inv = np.unique(self.hits, return_inverse=True)
        prefix = {}

        def clade_prefix(a):
            if a not in prefix:
                ind = np.array([cr.in_clade(par, a, int(v)) for v in vals], dtype=np.int64)
                prefix[a] = np.concatenate([[0], np.cumsum(ind[inv])]) if vals.size else np.zeros(1, np.int64)
            return prefix[a]
        for t in np.unique(self.taxon).tolist():
            up = cr.chain(par, t) if t else None
            if up is None:
                continue                                                                     # 0, or no node whose chain reaches a root
            idx = np.nonzero((self.taxon == t) & (r > 0))[0]
            ans = np.zeros(idx.size, dtype=np.int64)
            done = np.zeros(idx.size, dtype=bool)
            for a in up:
                cp = clade_prefix(a)
                ok = ~done & (cp[self.hi[idx]] - cp[self.lo[idx]] >= r[idx])
                ans[ok] = a
                done |= ok
            out[idx] = ans
        return out

    def check_sample(self, par, theta, got, rng, budget):
        """confidence_ref.walker itself on a sample of the windows (at most budget of them, fewer where windows hold many hits)"""
        if self.nw == 0:
            return
        span = int((self.hi - self.lo).max(initial=1))
        for p in rng.choice(self.nw, size=min(self.nw, budget, max(6, 20000 // max(1, span))), replace=False).tolist():
            want = cr.walker(par, self.taxon[p], self.missing[p], self.hits[self.lo[p]:self.hi[p]].tolist())(theta)
            assert int(got[p]) == want, (p, theta)


class Model:
    def __init__(self, oracle, table, tax, par, seqs, taxids, L, gaps=None, **kw):
        self.par, self.L, self.taxids = par, L, taxids
        self.seqs = [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
        c = K + (int(np.sum(gaps)) if gaps is not None else 0)
        self.m = [SeqModel(oracle, table, tax, s, L, c, gaps=gaps, **kw) for s in self.seqs]
        self.cache = {}

    def at(self, theta):
        """-> (image, pairs) as the session with this threshold writes them"""
        theta = Fraction(theta)
        if theta not in self.cache:
            rng = np.random.default_rng(5)
            total = sum(s.size for s in self.seqs)
            image = np.full(total, WM.NONE, dtype=np.uint32)
            who, what, o = [], [], 0
            for s, m, t in zip(self.seqs, self.m, self.taxids):
                if m.nw:
                    calls = m.walk(self.par, theta)
                    m.check_sample(self.par, theta, calls, rng, max(1, 48 // len(self.seqs)))
                    image[o:o + m.nw] = calls.astype(np.uint32)
                    who.append(np.full(m.nw, int(t), dtype=np.uint64)); what.append(calls.astype(np.uint32))
                o += s.size
            who = np.concatenate(who) if who else np.zeros(0, np.uint64)
            what = np.concatenate(what) if what else np.zeros(0, np.uint32)
            self.cache[theta] = (image, WM.pairs_of(who, what))
        return self.cache[theta]


def session(c, seqs, taxids, L, theta, pair_cap=1 << 12):
    bases, offsets = synth.concat(seqs)
    return c.classify_windows(bases, offsets, taxids, L, pair_cap=pair_cap, confidence=theta)


def check(c, model, theta, tag=None):
    want_image, want_pairs = model.at(theta)
    image, got = session(c, model.seqs, model.taxids, model.L, theta)
    assert np.array_equal(image, want_image), (tag, theta, np.nonzero(image != want_image)[0][:5].tolist())
    assert same_pairs(got, want_pairs) and got[3] == 0, (tag, theta)
    return image


def witness(c, model, theta, image):
    """the same windows cut as reads, classified on this context under set_confidence(theta)"""
    o = 0
    try:
        c.set_confidence(theta)
        for s in model.seqs:
            nw = WM.n_windows(s.size, model.L)
            if nw:
                assert np.array_equal(c.classify(*cut(s, model.L))["taxon"], image[o:o + nw]), theta
            o += s.size
    finally:
        c.set_confidence(0)


# ---- a. small world ------------------------------------------------------------------------------------------------------------
THETAS = [Fraction(1, 20), Fraction(1, 2), Fraction(1)]


@pytest.fixture(scope="module")
def genome_models(oracle, small_world):
    w = small_world
    par = cr.parent_map(w.parent)
    seqs, taxids = genome_batch(w)
    cache = {}

    def get(L):
        if L not in cache:
            cache[L] = Model(oracle, w.table, w.tax, par, seqs, taxids, L)
        return cache[L]
    return get


@pytest.mark.parametrize("layout", LAYOUTS)
def test_small_world(ctx, small_world, genome_models, layout):
    load(ctx, small_world, layout)
    for L in (31, 150, 600):
        m = genome_models(L)
        base = m.at(0)[0]
        for th in THETAS:
            image = check(ctx, m, th, (layout, L))
            if L == 150 and th == Fraction(1, 2):                  # not vacuous: calls move, and some stop on the way up
                moved = image != base
                assert moved.sum() >= 1000 and (moved & (image != 0)).sum() >= 100
            if th == Fraction(1, 2) and layout == _lib.LAYOUT_MINBUCKET:
                witness(ctx, m, th, image)


# ---- b. Q changes, the hit range does not --------------------------------------------------------------------------------------
def test_q_changes_without_the_range(ctx, oracle, small_world):
    w, L = small_world, 150
    par = cr.parent_map(w.parent)
    rng = np.random.default_rng(41)
    seq = synth.rand_seq(rng, 600)
    seq[100] = ord("N")
    seq[200:240] = w.genomes[1001][3000:3040]
    m = Model(oracle, w.table, w.tax, par, [seq], [1001], L)
    sm = m.m[0]
    assert (sm.lo[100], sm.hi[100]) == (sm.lo[101], sm.hi[101]) and sm.hi[100] - sm.lo[100] == 10       # the piece's ten k-mers in both
    assert sm.missing[100] + 1 == sm.missing[101]                  # window 100 holds the N: one k-mer fewer is looked up
    thetas = set()
    for p in (100, 101):
        thetas |= cr.boundaries(par, sm.taxon[p], sm.missing[p], sm.hits[sm.lo[p]:sm.hi[p]].tolist())
    thetas = sorted(t for t in thetas if 0 < t <= 1)
    assert thetas
    split = 0
    load(ctx, w)
    for th in thetas:
        image = check(ctx, m, th)
        split += int(image[100] != image[101])
        witness(ctx, m, th, image)
    assert split >= 1                                              # two adjacent windows, equal hit ranges, different calls


# ---- c. exact boundaries -------------------------------------------------------------------------------------------------------
def test_exact_boundaries(ctx, oracle, small_world):
    w, L = small_world, 150
    par = cr.parent_map(w.parent)
    seq = chimera(w)
    m = Model(oracle, w.table, w.tax, par, [seq], [7], L)
    sm = m.m[0]
    load(ctx, w)
    n_changed = 0
    for p in np.random.default_rng(9).choice(sm.nw, size=10, replace=False).tolist():
        q = int(sm.hi[p] - sm.lo[p] + sm.missing[p])
        for th in sorted(cr.boundaries(par, sm.taxon[p], sm.missing[p], sm.hits[sm.lo[p]:sm.hi[p]].tolist())):
            if not 0 < th < 1:
                continue
            above = Fraction(th.numerator * (1 << 20) + 1, th.denominator * (1 << 20))       # the next fraction above c / Q
            assert th * q == th.numerator * q // th.denominator                                # (theta = c / Q: num = c, den = Q)
            at, past = check(ctx, m, th, p), check(ctx, m, above, p)
            want_at, want_past = m.at(th)[0], m.at(above)[0]
            assert want_at[p] != want_past[p] and at[p] != past[p]                           # exactly at c / Q the clade still holds enough
            n_changed += 1
    assert n_changed >= 10
    witness(ctx, m, Fraction(1, 3), check(ctx, m, Fraction(1, 3)))


# ---- d. more taxa than the register counter holds ------------------------------------------------------------------------------
def test_many_taxa(ctx, oracle):
    pairs = [(1, 1)] + [(i, 1) for i in range(2, 302)]
    tax = oracle.Taxonomy(pairs=pairs)
    par = cr.parent_map(pairs)
    seq = synth.rand_seq(np.random.default_rng(5), 12000)
    table = oracle.Table()
    for i in range(300):
        oracle.lca_map_add(table, tax, K, seq[40 * i:40 * i + 40].tobytes(), 2 + i)
    L = 4000
    m = Model(oracle, table, tax, par, [seq], [2], L)
    sm = m.m[0]
    assert max(np.unique(sm.hits[sm.lo[p]:sm.hi[p]]).size for p in range(0, sm.nw, 500)) > _lib.WINDOWS_FAST_TAXA
    root, none = Fraction(1, 5), Fraction(1, 2)
    assert (m.at(0)[0][:sm.nw] == 1).all()                        # so many leaves meet at the root: the walk starts and ends there
    assert (m.at(root)[0][:sm.nw] == 1).all()                     # the root's clade, every hit of the window, holds a fifth of Q
    assert (m.at(none)[0][:sm.nw] == 0).all()                     # and not half of it
    ctx.set_encoder(K, None, canonicalize=True)
    flags, keys, vals = table.arrays()
    ctx.load_taxonomy(tax.parent)
    for layout in LAYOUTS:
        ctx.load_table(keys.size, flags, keys, vals, layout=layout)
        for th in (root, none):
            image = check(ctx, m, th, layout)
    witness(ctx, m, none, image)
    witness(ctx, m, root, m.at(root)[0])


# ---- e. the hit list in global memory ------------------------------------------------------------------------------------------
def test_hit_list_in_global_memory(ctx, oracle, small_world):
    w, L = small_world, 12000
    assert T + L - K > _lib.WINDOWS_LDS_LIST
    seq = np.concatenate([w.genomes[1001], synth.mutate(np.random.default_rng(4), w.genomes[1003], 0.01, 0.002), w.genomes[2001][:2300]])
    m = Model(oracle, w.table, w.tax, cr.parent_map(w.parent), [seq, w.genomes[1002], seq[:L]], [1001, 1002, 2001], L)
    th = Fraction(1, 2)
    base, want = m.at(0)[0], m.at(th)[0]
    assert (want != base).sum() > 100 and (want != 0).sum() > 100
    load(ctx, w, _lib.LAYOUT_MINBUCKET)
    witness(ctx, m, th, check(ctx, m, th))


# ---- f. odd values and seams ---------------------------------------------------------------------------------------------------
def test_odd_values_and_seams(ctx, oracle, small_world):
    w, L = small_world, 150
    vals = w.vals.copy()
    vals[vals == 1003] = 1500                     # a value that is no node of the taxonomy
    vals[vals == 1004] = 0                        # and the value 0: a hit all the same
    table = oracle.Table.wrap(*w.table.header(), w.flags.copy(), w.keys.copy(), vals)
    par = cr.parent_map(w.parent)
    th = Fraction(1, 2)
    models = []
    for seqs in edge_sequences(w, L):
        models.append(Model(oracle, table, w.tax, par, seqs, [synth.LEAVES[i % 6] for i in range(len(seqs))], L))
    assert any(s.size > T + L for s in models[1].seqs)
    for layout in LAYOUTS:
        load(ctx, w, layout, arrays=(w.flags, w.keys, vals))
        images = [check(ctx, m, th, layout) for m in models]
    for m, image in zip(models, images):
        witness(ctx, m, th, image)


# ---- g. a spaced seed ----------------------------------------------------------------------------------------------------------
def test_spaced_seed(ctx, oracle):
    w = synth.make_world(oracle, seed=14, k=K, genome_len=3000, gaps=[1] * 15 + [0] * 15)
    seqs = [w.genomes[leaf] for leaf in synth.LEAVES]
    par = cr.parent_map(w.parent)
    th = Fraction(1, 2)
    for intended in (True, False):
        m = Model(oracle, w.table, w.tax, par, seqs, synth.LEAVES, 150, gaps=w.gaps, spaced_intended=intended)
        want = m.at(th)[0]
        called = want[want != WM.NONE]
        assert ((want != m.at(0)[0]).sum() > 100) if intended else not called.any()
        load(ctx, w, _lib.LAYOUT_MINBUCKET, spaced_intended=intended)
        witness(ctx, m, th, check(ctx, m, th, intended))


# ---- equivalences and errors ---------------------------------------------------------------------------------------------------
def test_no_threshold_is_the_plain_session(ctx, small_world):
    c, w = ctx, small_world
    load(c, w)
    seqs, taxids = genome_batch(w)
    b = Batch(c, seqs, taxids)
    try:
        assert c.L.bns_windows_begin(c.h, 150, 1 << 12) == 0
        plain_image, plain = b.add(), c.windows()
        c.windows_end()
        assert c.L.bns_windows_begin_conf(c.h, 150, 1 << 12, 0, 1) == 0
        image, got = b.add(), c.windows()
        c.windows_end()
        assert np.array_equal(image, plain_image) and same_pairs(got, plain[:3]) and got[3] == plain[3] == 0
        assert c.L.bns_windows_begin_conf(c.h, 150, 1 << 12, 0, 7) == 0          # 0 / 7 is no threshold either
        assert np.array_equal(b.add(), plain_image)
        c.windows_end()
        c.windows_begin(150, 1 << 12, confidence=0.5)
        assert not np.array_equal(b.add(), plain_image)
    finally:
        c.windows_end()
        b.free()


def test_errors_and_the_context_is_untouched(ctx, small_world):
    c, w = ctx, small_world
    load(c, w)
    L_ = c.L
    assert L_.bns_windows_begin_conf(c.h, 150, 16, 2, 1) == ERR_ARG              # bns_set_confidence's codes
    assert L_.bns_windows_begin_conf(c.h, 150, 16, 1, 0) == ERR_ARG
    assert L_.bns_windows_begin_conf(c.h, 150, 16, 0, 0) == ERR_ARG
    assert L_.bns_set_confidence(c.h, 2, 1) == ERR_ARG and L_.bns_set_confidence(c.h, 1, 0) == ERR_ARG
    with pytest.raises(ValueError):
        c.windows_begin(150, 16, confidence=1.5)
    c.set_confidence(0.5)
    assert L_.bns_windows_begin_conf(c.h, 150, 16, 1, 2) == ERR_STATE            # the context's threshold still refuses a session
    assert L_.bns_windows_begin_conf(c.h, 150, 16, 0, 1) == ERR_STATE
    c.set_confidence(0)
    reads = synth.simulate_reads(np.random.default_rng(31), w.genomes, 300)
    bases, offsets = synth.concat(reads)
    before = c.classify(bases, offsets)
    b = Batch(c, [w.genomes[1001][:1000]], [1001])
    try:
        assert L_.bns_windows_begin_conf(c.h, 150, 16, 1, 2) == 0
        assert L_.bns_windows_begin_conf(c.h, 150, 16, 1, 2) == ERR_STATE        # a second begin
        c.set_confidence(0.25)                                                   # turned on during a session
        assert L_.bns_windows_add(c.h, b.d_bases, b.d_offsets, b.n, b.total, b.d_taxid, None, None) == ERR_STATE
        c.set_confidence(0)
        b.add()
        during = c.classify(bases, offsets)                                      # the session's theta is not the context's
        c.windows_end()
        after = c.classify(bases, offsets)
        for f in ("taxon", "missing", "ambig"):
            assert np.array_equal(before[f], during[f]) and np.array_equal(before[f], after[f])
    finally:
        c.windows_end()
        b.free()
