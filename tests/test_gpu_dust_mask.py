"""dust_mark_kernel against tests/dust_ref.py, bit for bit (Context.dust_mask).

The kernel cuts the BATCH into pieces of 2048 bases (DUST_PIECE) and every sequence into rounds of 64 start triplets counted from the
sequence's own first base; a piece that ends inside a sequence runs one truncated halo round.  The batches below put sequence ends,
round ends and piece ends in every relation to each other: the lengths around 64 / 128 / 2048, and sequences of other lengths in
front of them that shift where the piece edges fall."""
import numpy as np
import pytest

import dust_ref as D
import synth

pytestmark = pytest.mark.gpu


def _rand(rng, n):
    return synth.rand_seq(rng, n).tobytes()


def _put(seq, at, tract):
    at = max(0, min(at, len(seq) - len(tract)))
    return seq[:at] + tract + seq[at + len(tract):]


def _edge_batch(rng):
    seqs = []
    # lengths at the round, piece and halo edges; generated tracts all over
    for n in [0, 1, 2, 3, 4, 9, 61, 62, 63, 64, 65, 66, 127, 128, 129, 130, 150, 2046, 2047, 2048, 2049, 2050, 4200, 10007]:
        seqs.append(D.gen_seq(rng, n))
    # tracts straddling base offsets 63/64, 127/128, 2047/2048 and the last base, in a random background
    for tract in (b"A" * 30, b"AC" * 15, b"ACG" * 11, b"TTTTTTTTG" * 4):
        s = _rand(rng, 2100)
        for at in (63 - len(tract) // 2, 127 - len(tract) // 2, 2047 - len(tract) // 2, 2100):
            s = _put(s, at, tract)
        seqs.append(s)
        seqs.append(_put(_rand(rng, 2048), 2048, tract))          # the tract ends with the sequence, the sequence with the piece
    # a tract cut by an N, by a byte that is no base, and NOT cut by lower case
    t = b"G" * 40
    seqs.append(_rand(rng, 20) + t[:20] + b"N" + t[21:] + _rand(rng, 20))
    seqs.append(_rand(rng, 20) + t[:9] + b"X" + t[10:] + _rand(rng, 20))
    seqs.append(_rand(rng, 20) + t[:9] + b"g" + t[10:] + _rand(rng, 20))
    seqs.append(_rand(rng, 20) + b"CACACACACACACANCACACACACACACA" + b"-" + b"CACACA")
    # neighbours: one ends and the next begins with the same homopolymer, neither long enough alone (7 are masked at (64, 20))
    for n_left, n_right in ((4, 4), (3, 5), (6, 6)):
        seqs.append(_rand(rng, 60 - n_left) + b"T" * n_left)
        seqs.append(b"T" * n_right + _rand(rng, 64 - n_right))
    seqs.append(b"A" * 6); seqs.append(b"A" * 6); seqs.append(b"A" * 7); seqs.append(b"")
    seqs.append(b"A" * 31 + b"C"); seqs.append(b"A" * 32); seqs.append(b"A" * 33)
    return seqs


@pytest.fixture(scope="module")
def batches():
    rng = np.random.default_rng(77)
    edge = _edge_batch(rng)
    order = rng.permutation(len(edge))
    return {"edges": edge, "edges_shuffled": [edge[i] for i in order], "reads": D.gen_batch(rng, [150] * 5000)}


@pytest.fixture(scope="module")
def expected(batches):
    """the reference of every (batch, W, T), computed once"""
    memo = {}

    def get(name, W, T):
        if (name, W, T) not in memo:
            memo[(name, W, T)] = D.batch_masks(batches[name], W, T)
        return memo[(name, W, T)]
    return get


def _check(ctx, seqs, want, W, T):
    bases, offsets = synth.concat([np.frombuffer(s, dtype=np.uint8) for s in seqs])
    ctx.set_dust(W, T)
    try:
        got = ctx.dust_mask(bases, offsets)
    finally:
        ctx.set_dust(0)
    assert len(got) == len(seqs)
    n_set = 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.size == len(seqs[i])
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError("sequence %d of %d bases at (%d, %d): %d bases differ, first at %d (got %d)" %
                                 (i, len(seqs[i]), W, T, bad.size, int(bad[0]), int(g[bad[0]])))
        n_set += int(w.sum())
    return n_set / max(1, sum(len(s) for s in seqs))


@pytest.mark.parametrize("W,T", D.PARAMS)
@pytest.mark.parametrize("name", ["edges", "edges_shuffled"])
def test_mask_edges(gpu_ctx, batches, expected, name, W, T):
    share = _check(gpu_ctx, batches[name], expected(name, W, T), W, T)
    assert 0.10 <= share <= 0.70


@pytest.mark.parametrize("W,T", D.PARAMS)
def test_mask_5000_reads(gpu_ctx, batches, expected, W, T):
    share = _check(gpu_ctx, batches["reads"], expected("reads", W, T), W, T)
    assert 0.10 <= share <= 0.70


def test_neighbours_do_not_leak(gpu_ctx):
    a, b = b"CGTCAGT" + b"T" * 4, b"T" * 4 + b"CTGACGC"
    bases, offsets = synth.concat([np.frombuffer(s, dtype=np.uint8) for s in (a, b, a + b)])
    gpu_ctx.set_dust(64, 20)
    try:
        got = gpu_ctx.dust_mask(bases, offsets)
    finally:
        gpu_ctx.set_dust(0)
    assert not got[0].any() and not got[1].any()
    assert got[2][7:15].all()                                     # joined, the eight T's are one tract


def test_mask_states_and_arguments(gpu_ctx):
    import bonsai_amd
    bases, offsets = synth.concat([np.frombuffer(b"A" * 40, dtype=np.uint8)])
    gpu_ctx.set_dust(0)
    with pytest.raises(bonsai_amd.BonsaiAmdError):
        gpu_ctx.dust_mask(bases, offsets)                         # off
    for w, t in ((7, 20), (65, 20), (64, 0), (64, 1001), (1, 1)):
        with pytest.raises(bonsai_amd.BonsaiAmdError):
            gpu_ctx.set_dust(w, t)
    with pytest.raises(bonsai_amd.BonsaiAmdError):
        gpu_ctx.dust_mask(bases, offsets)                         # a refused setting leaves it off
    for w, t in ((8, 1), (64, 1000)):
        gpu_ctx.set_dust(w, t)
        assert gpu_ctx.dust_mask(bases, offsets)[0].size == 40
    gpu_ctx.set_dust(0)
