"""Low-complexity masking in front of the device builds (bns_set_dust): bns_build_table_device, bns_build_add and
bns_build_minimize_begin / _add.  The truth: a build with masking ON over genomes g is the build with masking OFF over
substitute(g, dust_ref(g)) -- the same keys, the same values, the same khash arrays' size."""
import numpy as np
import pytest

import bonsai_amd
import build_cases as bc
import dust_world as DW
from test_gpu_build import device_build, present_pairs
from test_gpu_build_minimize import run_minimize
from test_gpu_build_session import check_table, run_session

pytestmark = pytest.mark.gpu

W, T = DW.W, DW.T
K = 31


@pytest.fixture(scope="module")
def genomes(oracle):
    """six genomes of 6 kb with tracts, their substituted forms, and the oracle's table of all k-mers of the substituted ones"""
    w = DW.make_world(oracle, seed=41)
    w.leaves = list(w.genomes)
    w.seqs = [w.genomes[l] for l in w.leaves]
    w.sub, w.masks = DW.substituted(w.seqs)
    share = sum(int(m.sum()) for m in w.masks) / sum(s.size for s in w.seqs)
    assert 0.05 <= share <= 0.70, share
    t = oracle.Table()
    for leaf, g in zip(w.leaves, w.sub):
        oracle.lca_map_add(t, w.tax, K, g.tobytes(), leaf)
    w.sub_keys, w.sub_vals = bc.table_pairs(t)
    return w


@pytest.fixture
def ctx(gpu_ctx, genomes):
    gpu_ctx.set_encoder(K, None, canonicalize=True)
    gpu_ctx.load_taxonomy(genomes.parent)
    yield gpu_ctx
    gpu_ctx.build_end()
    gpu_ctx.set_dust(0)
    gpu_ctx.set_encoder(K, None, canonicalize=True)


def same_tables(a, b):
    """(hdr, flags, keys, vals) twice: the same header and the same map (where a key sits is the order of arrival's to decide)"""
    assert np.array_equal(a[0], b[0])
    ka, va = present_pairs(a[1], a[2], a[3], int(a[0][0]))
    kb, vb = present_pairs(b[1], b[2], b[3], int(b[0][0]))
    assert np.array_equal(ka, kb) and np.array_equal(va, vb)


@pytest.mark.parametrize("w,score", [(31, 0), (50, 1)], ids=["every-kmer", "w50-entropy"])
def test_build_table_device(ctx, genomes, w, score):
    g = genomes
    ctx.set_window(w, score)
    nb = 1 << 17
    ctx.set_dust(W, T)
    on = device_build(ctx, g.seqs, g.leaves, nb)
    ctx.set_dust(0)
    off = device_build(ctx, g.sub, g.leaves, nb)
    plain = device_build(ctx, g.seqs, g.leaves, nb)
    k_on, v_on = present_pairs(on[1], on[2], on[3], nb)
    k_off, v_off = present_pairs(off[1], off[2], off[3], nb)
    assert np.array_equal(k_on, k_off) and np.array_equal(v_on, v_off) and np.array_equal(on[0], off[0])
    if w == K:
        assert np.array_equal(k_on, g.sub_keys) and np.array_equal(v_on, g.sub_vals)
    print("keys: %d masked, %d unmasked" % (int(on[0][2]), int(plain[0][2])))
    assert 0 < int(on[0][2]) < int(plain[0][2])


@pytest.mark.parametrize("per_batch", [6, 2, 1])
def test_build_session(ctx, oracle, genomes, per_batch):
    g = genomes
    cut = lambda seqs: [(seqs[i:i + per_batch], g.leaves[i:i + per_batch]) for i in range(0, len(seqs), per_batch)]
    ctx.set_dust(W, T)
    on = run_session(ctx, cut(g.seqs), 4)
    ctx.set_dust(0)
    off = run_session(ctx, cut(g.sub), 4)
    plain = run_session(ctx, cut(g.seqs), 4)
    same_tables(on[:4], off[:4])
    check_table(oracle, *on[:4], g.sub_keys, g.sub_vals)
    assert on[4]["keys"] == g.sub_keys.size < plain[4]["keys"]


def test_build_session_seeded(ctx, oracle, genomes):
    """-A: a db of the first genomes (masked when it was built), the others added with masking on"""
    g = genomes
    ctx.set_dust(W, T)
    first = run_session(ctx, [(g.seqs[:3], g.leaves[:3])], 4)
    both = run_session(ctx, [(g.seqs[3:], g.leaves[3:])], 4, seed=(int(first[0][0]), first[1], first[2], first[3]))
    check_table(oracle, *both[:4], g.sub_keys, g.sub_vals)


def test_build_minimize(ctx, oracle, genomes):
    """-D, w = 50: both passes see the same mask, so pass B never meets a k-mer pass A did not fold"""
    g = genomes
    a = lambda seqs: [(seqs[:3], g.leaves[:3]), (seqs[3:], g.leaves[3:])]
    b = lambda seqs: [seqs[:2], seqs[2:]]
    ctx.set_dust(W, T)
    on = run_minimize(ctx, a(g.seqs), b(g.seqs), 50)
    ctx.set_dust(0)
    off = run_minimize(ctx, a(g.sub), b(g.sub), 50)
    plain = run_minimize(ctx, a(g.seqs), b(g.seqs), 50)
    same_tables(on[:4], off[:4])
    k_on, v_on = present_pairs(on[1], on[2], on[3], int(on[0][0]))
    check_table(oracle, *on[:4], k_on, v_on)
    assert on[4]["keys"] == g.sub_keys.size and on[5]["scored_keys"] == g.sub_keys.size
    assert 0 < on[5]["keys"] < plain[5]["keys"] and on[5]["keys"] == off[5]["keys"]


def test_set_dust_is_refused_inside_a_session(ctx, genomes):
    ctx.build_begin(4)
    with pytest.raises(bonsai_amd.BonsaiAmdError, match="build session"):
        ctx.set_dust(W, T)
    with pytest.raises(bonsai_amd.BonsaiAmdError, match="build session"):
        ctx.set_dust(0)
    ctx.build_end()
    ctx.set_dust(W, T)
    ctx.set_dust(0)
