"""classify_kernel's claims on the device: the static first claim of every wavefront (even shares for a small batch, staggered
sizes 1..31 otherwise), full dynamic claims behind them, and the cut of the last claim at the end of the batch.

With the real number of resident wavefronts (8192) a batch needs 245 761 units to run a dynamic claim at all.
Context.debug_claim_waves(W) sizes the claims for W = 4 or 8 wavefronts and caps the grid at W / 4 workgroups: a batch of a few
hundred short reads then runs all of it, on wavefronts that go on claiming.  The batch sizes sit on the edges of the deal
(tests/claims_lib.py computes it from the header the kernel and the launcher share): around the static total, around the smallest
batch with full claims, around whole numbers of dynamic claims, around the sizes at which stages of shrinking claims would begin
(the schedule had them once), and a few thousand units.  Units that pack nothing (empty, one base, shorter than k) sit at the
first and at the last place of claims.  Every unit's taxon, missing, ambig and n_hits are held against the oracle, ASCII and
packed, single and paired; the hit stream of the first and the last unit of every claim too."""
import numpy as np
import pytest

import claims_lib as CL
import classify_forms as F
import synth
import test_gpu_unit_order as U

pytestmark = pytest.mark.gpu

FULL = CL.FULL


def batch_sizes(W):
    S = CL.stagger_total(W)
    small = [S - 3, S - 1, S, S + 1, 30 * W]                                 # dealt out by the static part alone (even shares)
    full = [30 * W + 1,                                                      # the smallest batch with full claims
            S + 16 * W + 16 * 3 + 5, S + 24 * W + 3,
            S + 32 * W - 1, S + 32 * W, S + 32 * W + 1,
            S + 32 * W + FULL - 1, S + 32 * W + FULL, S + 32 * W + FULL + 1]
    k = -(-(30 * W + 1 - S) // FULL)                                         # a whole number of dynamic claims, and one unit either way
    full += [S + k * FULL - 1, S + k * FULL, S + k * FULL + 1, S + (k + 1) * FULL + 2]
    full.append(3001 + W)                                                    # many full claims per wavefront
    return small, sorted(set(n for n in full if n > 30 * W))


def make_batch(w, n_units, W, paired, seed):
    """reads of 31-70 bases cut from the world's genomes; units that pack nothing at the first and the last place of every
    second claim (and at both ends of the batch); returns bases, offsets and the units whose hit stream is checked"""
    inc = 2 if paired else 1
    rng = np.random.default_rng(seed)
    c = F.comb(w.k, w.gaps)
    lens = rng.integers(31, 71, size=n_units * inc).astype(np.int64)
    base, cnt, _ = CL.claims(n_units, W // 4)
    first, last = base, base + cnt - 1
    nothing = np.zeros(n_units, dtype=bool)
    nothing[first[::2]] = True
    nothing[last[1::2]] = True
    nothing[0] = nothing[-1] = True
    idx = np.flatnonzero(nothing)
    short = np.array([0, c - 1, 1], dtype=np.int64)
    if paired:
        which = rng.integers(0, 3, size=idx.size)                            # mate 1, mate 2 or both
        lens[idx[which != 1] * 2] = short[idx[which != 1] % 3]
        lens[idx[which != 0] * 2 + 1] = short[(idx[which != 0] + 1) % 3]
    else:
        lens[idx] = short[idx % 3]
    offsets = np.zeros(lens.size + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lens)
    total = int(offsets[-1])
    g = np.concatenate(list(w.genomes.values()))
    starts = rng.integers(0, g.size - 100, size=lens.size)
    src = np.repeat(starts - offsets[:-1].astype(np.int64), lens) + np.arange(total, dtype=np.int64)
    bases = g[src]
    sub = rng.random(total) < 0.004
    bases[sub] = synth.ACGT[rng.integers(0, 4, size=int(sub.sum()))]
    edges = sorted(set(int(u) for u in first) | set(int(u) for u in last))
    return np.ascontiguousarray(bases, dtype=np.uint8), offsets, edges


@pytest.fixture
def claim_waves(gpu_ctx):
    yield gpu_ctx.debug_claim_waves
    gpu_ctx.debug_claim_waves(0)


@pytest.mark.parametrize("paired", (False, True), ids=("single", "paired"))
@pytest.mark.parametrize("W", (4, 8))
def test_schedule_edges(gpu_ctx, oracle, claim_waves, W, paired):
    with U.Loaded(gpu_ctx, oracle, "k31") as ld:
        claim_waves(W)
        small, full = batch_sizes(W)
        hits_seen = 0
        for n in small + full:
            bases, offsets, edges = make_batch(ld.w, n, W, paired, 1000 * W + n)
            form, got = U.check(ld, oracle, bases, offsets, paired, hit_units=edges)
            chunk, grid, _ = CL.geometry(n, W // 4)
            assert (form["chunk"], form["grid"]) == (chunk, grid), "batch of %d units" % n
            assert grid * 4 <= W
            if n in full:
                assert chunk == FULL and grid * 4 == W
                base, cnt, n_static = CL.claims(n, W // 4)
                assert n_static == W and base.size >= W + (n - CL.stagger_total(W)) // FULL > W, "batch of %d units: the wavefronts are meant to go on claiming" % n
            else:
                assert chunk < FULL
            hits_seen += int(got["n_hits"].sum())
        assert hits_seen > 0


@pytest.mark.parametrize("paired", (False, True), ids=("single", "paired"))
def test_real_waves(gpu_ctx, oracle, claim_waves, paired):
    """the smallest batch that runs full claims on the device's own number of wavefronts, against the same batch dealt to 8"""
    with U.Loaded(gpu_ctx, oracle, "k31") as ld:
        n = 30 * 32 * U.CUS + 1
        bases, offsets, _ = make_batch(ld.w, n, 32 * U.CUS, paired, 5 + int(paired))
        got = gpu_ctx.classify(bases, offsets, paired=paired, want_hits=True)
        form = gpu_ctx.last_classify_form()
        assert form["chunk"] == FULL, "the batch is meant to run full claims"
        assert form["grid"] * 4 > 8
        claim_waves(8)
        ref = gpu_ctx.classify(bases, offsets, paired=paired, want_hits=True)
        assert gpu_ctx.last_classify_form()["grid"] == 2
        for key in ("taxon", "missing", "ambig", "n_hits"):
            bad = np.flatnonzero(got[key] != ref[key])
            assert bad.size == 0, "%s differs at units %s of %d" % (key, bad[:8], n)
        assert np.array_equal(np.concatenate(got["hits"]), np.concatenate(ref["hits"]))
        assert (got["taxon"] != 0).mean() > 0.2 and int(got["n_hits"].sum()) > 0
