"""How classify_kernel's batch is dealt out (bonsai_amd/csrc/bns_claims.hpp), on the host: the header is compiled into a small
library (tests/helpers/claim_schedule_harness.cpp, through tests/claims_lib.py) that calls its functions the way the launcher and
the kernel do.

Every wavefront's static claim and every dynamic claim, in that order, must tile [0, n_units) exactly once; no claim is larger
than a full one (cnt * mates + 1 offsets must fit one 64-lane load); the sizes never grow with the dynamic claim index; a claim
index past the last one says so; a small batch is dealt out by the static part alone, by the launcher's old rule (an even share,
at least 4).  (The stages of shrinking claims over the end of a batch that the schedule once had are not in it:
docs/KERNEL_NOTES.md, "Dealing the batch out".)"""
import numpy as np
import pytest

import claims_lib as CL

FULL = CL.FULL
WAVES = (4, 8, 64, 8192)
WHY = {1: "the claims do not tile [0, n_units) in order", 2: "a claim too large", 3: "a dynamic claim larger than the one before it",
       4: "an empty claim, or a wavefront left out in front of one that is not", 5: "a claim index past the end that does not say so",
       7: "small batch: not the even-share rule, or a dynamic claim"}


def boundaries(W, G):
    """every batch size at which the deal changes shape, for W resident and G launched wavefronts"""
    S = CL.stagger_total(G)
    at = {0, 1, 3, 4, 5, 31, 32, 4 * W, 30 * W, 31 * W, S, S + FULL, S + 2 * FULL, 64 * W}
    for tail in (8 * W, 16 * W, 32 * W):                          # (where the stages of a shrinking tail would begin)
        at |= {S + tail, S + tail + FULL}
    out = set()
    for b in at:
        out |= {b + d for d in range(-2, 3) if b + d >= 0}
    return sorted(out)


def sizes(W, G, rng):
    ns = set(boundaries(W, G))
    ns |= {int(x) for x in rng.integers(0, 1 << 24, size=300)}
    ns |= {int(2.0 ** e) for e in rng.uniform(0, 24, size=3000)}
    return sorted(ns)


@pytest.mark.parametrize("W", WAVES)
def test_sweep(W):
    """claim by claim in the harness (its claims_verify says which property it checks under which number); mates 1 and 2 share a
    full claim of 31 units, and the 64-lane bound is checked for 2"""
    rng = np.random.default_rng(1300 + W)
    grids = sorted({W // 4, max(1, W // 8), 1})
    checked = 0
    for blocks in grids:
        for n in sizes(W, blocks * 4, rng):
            rc = CL.lib().claims_verify(n, blocks, FULL)
            assert rc == 0, "n_units %d, %d resident workgroups: %s" % (n, blocks, WHY.get(rc, rc))
            checked += 1
    assert checked > 2000 * len(grids)


@pytest.mark.parametrize("W", WAVES)
def test_claims_listed(W):
    """the same properties from the list of claims itself, for every boundary size and a few random ones -- and what the form
    record reports: chunk 31 and the whole grid for a batch with full claims, the even share for a small one"""
    rng = np.random.default_rng(77 + W)
    blocks = W // 4
    ns = boundaries(W, W) + [int(x) for x in rng.integers(0, 1 << 21, size=40)]
    for n in ns:
        chunk, grid, dyn_base = CL.geometry(n, blocks)
        base, cnt, n_static = CL.claims(n, blocks)
        assert int(cnt.sum()) == n
        assert (cnt > 0).all() and (cnt <= FULL).all() and (cnt * 2 + 1 <= 64).all()
        ends = base + cnt
        assert base.size == 0 or (base[0] == 0 and (base[1:] == ends[:-1]).all() and ends[-1] == n), "n_units %d: not a tiling" % n
        dyn = cnt[n_static:]
        assert (np.diff(dyn) <= 0).all(), "n_units %d: a dynamic claim larger than the one before it" % n
        if n > 30 * W:
            assert chunk == FULL
            assert n_static == grid * 4 and int(cnt[:n_static].sum()) == CL.stagger_total(grid * 4) == dyn_base
            assert (cnt[:n_static] == 1 + np.arange(n_static) % FULL).all()
            assert (dyn[:-1] == FULL).all() and dyn.size == -(-(n - dyn_base) // FULL)
            if n > 31 * W:
                assert grid == blocks
        else:
            assert chunk == min(FULL, max(4, -(-n // W))) and dyn.size == 0 and dyn_base == n
            assert grid == max(1, min(blocks, -(-(-(-n // chunk)) // 4)))
            assert (cnt[:-1] == chunk).all()
