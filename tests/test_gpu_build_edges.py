"""bns_build_table_device against the oracle's sequential update_lca_map on the worlds of tests/build_cases.py: N runs, lower
case and IUPAC letters, sequences shorter than the comb / the window / a 2048-base chunk, keys that 100 sequences fold into over
a tree 30 deep, key 0, every build form (k, seed, strand rule, window, score), tables of 4 to 16 buckets, the exact load-factor
boundary and the argument refusals.  tests/test_build_cases.py (CPU tier) shows that the worlds hold all that."""
import numpy as np
import pytest

import build_cases as bc
import synth
from test_gpu_build import device_build, present_pairs

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_TABLE = -1, -7                              # include/bonsai_amd.h


def configure(ctx, case):
    ctx.set_encoder(case.k, list(case.gaps) if case.gaps is not None else None, canonicalize=case.canon, spaced_intended=True)
    if bc.windowed(case):
        ctx.set_window(case.w, case.score)


def arrays(seqs):
    return [np.frombuffer(s, dtype=np.uint8) for s in seqs]


def slot_states(flags, nb):
    i = np.arange(nb)
    return (flags[i >> 4] >> ((i & 15) << 1)) & 3


def upper_bound(nb):
    return int(nb * 0.77 + 0.5)                          # khash64.h:198


def build_pairs(ctx, seqs, taxids, nb):
    hdr, flags, keys, vals = device_build(ctx, arrays(seqs), taxids, nb)
    k, v = present_pairs(flags, keys, vals, nb)
    assert [int(x) for x in hdr] == [nb, k.size, k.size, upper_bound(nb)]
    return k, v


@pytest.fixture
def ctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.set_encoder(31, None, canonicalize=True)     # (what the other modules expect of the shared context)


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_build_edges(ctx, oracle, name):
    case = bc.BY_NAME[name]
    w = bc.world_for(oracle, case)
    exp_keys, exp_vals, exp_t = bc.expected(oracle, w, case)
    gaps = list(case.gaps) if case.gaps is not None else None
    configure(ctx, case)
    ctx.load_taxonomy(w.parent)
    nb = bc.buckets_for(exp_keys.size)
    hdr, flags, keys, vals = device_build(ctx, arrays(w.seqs), w.taxids, nb)
    got_keys, got_vals = present_pairs(flags, keys, vals, nb)
    print("%s: %d keys expected, %d built, %d buckets" % (name, exp_keys.size, got_keys.size, nb))
    assert np.array_equal(got_keys, exp_keys)
    bad = np.flatnonzero(got_vals != exp_vals)
    assert bad.size == 0, (bad.size, [(int(exp_keys[i]), int(got_vals[i]), int(exp_vals[i])) for i in bad[:5]])
    assert [int(x) for x in hdr] == [nb, exp_keys.size, exp_keys.size, upper_bound(nb)]
    # a valid khash for the reference's kh_get (no empty slot before a key on its probe path); empty slots zeroed
    t = oracle.Table.wrap(int(hdr[0]), int(hdr[2]), int(hdr[1]), int(hdr[3]), flags, keys, vals)
    qv, qf = t.get_batch(exp_keys)
    assert qf.all() and np.array_equal(qv, exp_vals)
    st = slot_states(flags, nb)
    assert set(np.unique(st).tolist()) <= {0, 2} and not keys[st == 2].any() and not vals[st == 2].any()
    if exp_keys.size and exp_keys[0] == 0:               # key 0 is told from an empty slot by the flag alone
        assert int(((keys == 0) & (st == 0)).sum()) == 1
    if not bc.windowed(case) and not bc.is_spaced(case) and case.canon:
        assert exp_keys[0] == 0
    # and it classifies like the oracle's own table: reads cut from the world's sequences, N runs and lower case included.
    # Classify takes every form here (it always looks up every k-mer, w = k; the window and its score only thinned the db), so
    # no case skips this half; for the string overload's score the oracle's table is the one filled from the folded map.
    ctx.set_encoder(case.k, gaps, canonicalize=case.canon, spaced_intended=True)
    ctx.load_table(nb, flags, keys, vals)
    reads = synth.simulate_reads(np.random.default_rng(5), dict(enumerate(arrays(w.seqs))), 300, n_rate=0.003, lower_rate=0.1)
    b, o = synth.concat(reads)
    exp = oracle.classify_batch(exp_t, w.tax, case.k, b, o, gaps=gaps, canon=case.canon, spaced_intended=True)
    got = ctx.classify(b, o)
    assert np.array_equal(got["taxon"], exp["taxon"]) and np.array_equal(got["missing"], exp["missing"])
    if not bc.windowed(case):
        assert int((exp["taxon"] != 0).sum()) >= 100


@pytest.mark.parametrize("name", ["k11-canon", "w50-entropy-canon"])
def test_build_is_order_free(ctx, oracle, name):
    """the fold is a CAS race between the waves of all sequences: whatever the order of the sequences, and from one build to the
    next, the same pairs; contigs of one genome (one taxid, no k-mer across the break) as the reference reads them"""
    case = bc.BY_NAME[name]
    w = bc.world_for(oracle, case)
    exp_keys, exp_vals, _ = bc.expected(oracle, w, case)
    configure(ctx, case)
    ctx.load_taxonomy(w.parent)
    nb = bc.buckets_for(exp_keys.size)
    n = len(w.seqs)
    orders = [list(range(n)), list(range(n)), list(range(n))[::-1], [int(x) for x in np.random.default_rng(9).permutation(n)]]
    for order in orders:                                 # (the first two: twice in a row on the same context)
        k, v = build_pairs(ctx, [w.seqs[i] for i in order], [w.taxids[i] for i in order], nb)
        assert np.array_equal(k, exp_keys) and np.array_equal(v, exp_vals)
    # one long sequence cut in two under its taxid: the k-mers (windows) across the cut are gone, nothing else changes
    i = w.clean[4100]
    s = w.seqs[i]
    seqs = w.seqs[:i] + [s[:2048], s[2048:]] + w.seqs[i + 1:]
    taxids = w.taxids[:i] + [w.taxids[i]] * 2 + w.taxids[i + 1:]
    sk, sv = bc.table_pairs(bc.oracle_table(oracle, w.tax, case, seqs, taxids))
    assert sk.size < exp_keys.size and np.isin(sk, exp_keys).all()
    k, v = build_pairs(ctx, seqs, taxids, nb)
    assert np.array_equal(k, sk) and np.array_equal(v, sv)


@pytest.mark.parametrize("n_keys,nb", [(1, 4), (3, 8), (6, 16), (12, 16)])
def test_build_tiny_tables(ctx, oracle, n_keys, nb):
    """fewer than 16 buckets share one flag word: its bits past n_buckets read as empty"""
    w = bc.make_edge_world(oracle)
    seq = synth.rand_seq(np.random.default_rng(100 + n_keys), 31 + n_keys - 1).tobytes()
    exp_keys = np.unique(oracle.encode(seq, 31))
    assert exp_keys.size == n_keys <= upper_bound(nb)
    tx = w.taxids[0]
    ctx.set_encoder(31, None, canonicalize=True)
    ctx.load_taxonomy(w.parent)
    hdr, flags, keys, vals = device_build(ctx, arrays([seq]), [tx], nb)
    assert [int(x) for x in hdr] == [nb, n_keys, n_keys, upper_bound(nb)]
    assert flags.size == 1
    st = (int(flags[0]) >> (2 * np.arange(16))) & 3
    assert (st[nb:] == 2).all() and set(st[:nb].tolist()) <= {0, 2} and int((st[:nb] == 0).sum()) == n_keys
    got_keys, got_vals = present_pairs(flags, keys, vals, nb)
    assert np.array_equal(got_keys, exp_keys) and (got_vals == tx).all()
    assert not keys[st[:nb] == 2].any() and not vals[st[:nb] == 2].any()
    qv, qf = oracle.Table.wrap(nb, n_keys, n_keys, int(hdr[3]), flags, keys, vals).get_batch(exp_keys)
    assert qf.all() and (qv == tx).all()


def test_build_load_boundary(ctx, oracle):
    """khash's load factor at n_buckets = 64: 49 keys (= upper_bound) build, 50 are refused, and the context builds on"""
    import bonsai_amd
    w = bc.make_edge_world(oracle)
    rng = np.random.default_rng(49)
    seq = synth.rand_seq(rng, 31 + 49).tobytes()         # 50 k-mers; without its last base 49
    assert upper_bound(64) == 49
    assert np.unique(oracle.encode(seq[:-1], 31)).size == 49 and np.unique(oracle.encode(seq, 31)).size == 50
    tx = w.taxids[1]
    ctx.set_encoder(31, None, canonicalize=True)
    ctx.load_taxonomy(w.parent)
    k, v = build_pairs(ctx, [seq[:-1]], [tx], 64)
    assert k.size == 49 and np.array_equal(k, np.unique(oracle.encode(seq[:-1], 31))) and (v == tx).all()
    with pytest.raises(bonsai_amd.BonsaiAmdError) as e:
        build_pairs(ctx, [seq], [tx], 64)
    assert "load factor" in str(e.value)
    k, v = build_pairs(ctx, [seq[:-1]], [tx], 64)
    assert k.size == 49 and (v == tx).all()
    k, v = build_pairs(ctx, [seq], [tx], 128)
    assert k.size == 50


def test_build_argument_refusals(ctx, oracle):
    """the checks that return before anything is launched, each with its error code"""
    w = bc.make_edge_world(oracle)
    seq = np.frombuffer(synth.rand_seq(np.random.default_rng(3), 60).tobytes() + b"N" * 16, dtype=np.uint8)
    off = np.array([0, 60], dtype=np.uint64)
    tx = np.array([w.taxids[0]], dtype=np.uint32)
    nb = 64
    bufs = [ctx.dev_alloc(n) for n in (seq.size, off.nbytes, tx.nbytes, 4 * max(1, nb >> 4), 8 * nb, 4 * nb)]
    d_bases, d_off, d_tx, d_f, d_k, d_v = bufs
    ctx.dev_upload(d_bases, seq); ctx.dev_upload(d_off, off); ctx.dev_upload(d_tx, tx)
    hdr = np.zeros(4, dtype=np.uint64)

    def call(n_buckets):
        rc = ctx.L.bns_build_table_device(ctx.h, d_bases, d_off, 1, 60, d_tx, n_buckets, d_f, d_k, d_v, hdr.ctypes.data_as(ctx.L.bns_build_table_device.argtypes[10]), None)
        return rc, ctx.L.bns_last_error(ctx.h).decode()
    try:
        ctx.load_taxonomy(w.parent)
        ctx.set_encoder(31, None, canonicalize=True)
        for bad in (48, 2, 0):
            rc, msg = call(bad)
            assert rc == ERR_TABLE and "power of two" in msg, (bad, rc, msg)
        ctx.set_encoder(32, None, canonicalize=False)    # ~0, the empty marker while building, is a legal forward 32-mer
        rc, msg = call(nb)
        assert rc == ERR_ARG and "k == 32" in msg, (rc, msg)
        ctx.set_encoder(31, list(bc.G_HALF), canonicalize=True, spaced_intended=False)
        rc, msg = call(nb)
        assert rc == ERR_ARG and "spaced_intended" in msg, (rc, msg)
        assert not hdr.any()
        ctx.set_encoder(31, None, canonicalize=True)     # and the same buffers build once the arguments are right
        rc, msg = call(nb)
        n = np.unique(oracle.encode(seq[:60].tobytes(), 31)).size
        assert rc == 0 and [int(x) for x in hdr] == [nb, n, n, upper_bound(nb)]
    finally:
        for p in bufs:
            ctx.dev_free(p)
