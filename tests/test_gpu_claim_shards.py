"""classify_kernel's eight work counters on the device: a draw d from counter x is claim 8 d + x of the one tiling, and a wavefront
whose counter is past the end goes on to the next one until all eight are.

Context.debug_claim_waves(W) sizes the claims for W wavefronts and caps the grid at W / 4 workgroups; with Context.DBG_SHARD_BY_WAVE a
wavefront's home counter is its index & 7 instead of its XCD number, so that two workgroups are at home on all eight counters and
every one of them has to go round the others at the end.  Reads of 40-60 bases, k = 31 on the clustered table, single and paired.
Every unit's taxon, missing, ambig, n_hits and ordered hit stream are held against the oracle (ASCII and packed, through
test_gpu_unit_order.check), and the same batch is run once more without the bit (the XCD's counter: whichever the two workgroups
land on) and must give the same.

The sizes.  The launcher deals a batch of up to 30 W units out by static claims alone and hands the kernel no counter; from
30 W + 1 units on the dynamic part is what the staggered static claims (36 units for W = 8, 10 for W = 4) leave.  So the dynamic
parts that can be launched are none at all, and 7 claims or more at W = 8 (4 or more at W = 4); a dynamic part of 1 to 6 claims
at W = 8 does not exist.  Tried here: none (240 units: no counter), the smallest at W = 8 (241 units: 7 claims, the last one cut,
counter 7 past the end from its first draw), the smallest at W = 4 (121 units: 3 full claims and a cut one, counters 4-7 past
the end from their first draw, and the four wavefronts at home on 0-3 only), exactly 8 claims and one unit either way (the eighth
claim cut to 30; a ninth of one unit), and about 200 claims with the last one cut."""
import numpy as np
import pytest

import bonsai_amd
import claims_lib as CL
import classify_forms as F
import synth
import test_gpu_unit_order as U

pytestmark = pytest.mark.gpu

FULL = CL.FULL
SHARD_BY_WAVE = bonsai_amd.Context.DBG_SHARD_BY_WAVE


def cases():
    S8, S4 = CL.stagger_total(8), CL.stagger_total(4)
    out = [(8, 240, 0), (8, 241, 7), (4, 121, 4), (8, S8 + 8 * FULL - 1, 8), (8, S8 + 8 * FULL, 8), (8, S8 + 8 * FULL + 1, 9), (8, S8 + 200 * FULL + 5, 201)]
    assert (S8, S4) == (36, 10)
    return out


def make_batch(w, n_units, paired, seed):
    """reads of 40-60 bases cut from the world's genomes, a few substitutions; a unit that packs nothing first and last"""
    inc = 2 if paired else 1
    rng = np.random.default_rng(seed)
    lens = rng.integers(40, 61, size=n_units * inc).astype(np.int64)
    lens[0] = 0
    lens[-1] = 1
    offsets = np.zeros(lens.size + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    total = int(offsets[-1])
    g = np.concatenate(list(w.genomes.values()))
    starts = rng.integers(0, g.size - 100, size=lens.size)
    src = np.repeat(starts - offsets[:-1].astype(np.int64), lens) + np.arange(total, dtype=np.int64)
    bases = g[src]
    sub = rng.random(total) < 0.004
    bases[sub] = synth.ACGT[rng.integers(0, 4, size=int(sub.sum()))]
    return np.ascontiguousarray(bases, dtype=np.uint8), offsets


@pytest.fixture
def claim_waves(gpu_ctx):
    yield gpu_ctx.debug_claim_waves
    gpu_ctx.debug_claim_waves(0)


@pytest.mark.parametrize("paired", (False, True), ids=("single", "paired"))
def test_shards(gpu_ctx, oracle, claim_waves, paired):
    with U.Loaded(gpu_ctx, oracle, "k31") as ld:
        hits_seen = 0
        for W, n, n_dyn in cases():
            claim_waves(W)
            base, cnt, n_static = CL.claims(n, W // 4)
            assert base.size - n_static == n_dyn, "batch of %d units on %d wavefronts: the dynamic part is meant to be %d claims" % (n, W, n_dyn)
            bases, offsets = make_batch(ld.w, n, paired, 14000 + 10 * n + W)
            gpu_ctx.debug_set(F.DBG_OVC_OFF | SHARD_BY_WAVE)
            form, got = U.check(ld, oracle, bases, offsets, paired)
            chunk, grid, _ = CL.geometry(n, W // 4)
            assert (form["chunk"], form["grid"]) == (chunk, grid) and (chunk == FULL) == (n_dyn > 0), "batch of %d units" % n
            assert n_dyn == 0 or grid * 4 == W
            gpu_ctx.debug_set(F.DBG_OVC_OFF)                                 # the same batch from the XCD's own counter
            ref = gpu_ctx.classify(bases, offsets, paired=paired, want_hits=True)
            for key in ("taxon", "missing", "ambig", "n_hits"):
                bad = np.flatnonzero(got[key] != ref[key])
                assert bad.size == 0, "batch of %d units, %s: by XCD differs from by wavefront at units %s" % (n, key, bad[:8])
            assert all(np.array_equal(a, b) for a, b in zip(got["hits"], ref["hits"])), "batch of %d units: hit streams" % n
            hits_seen += int(got["n_hits"].sum())
        assert hits_seen > 0
