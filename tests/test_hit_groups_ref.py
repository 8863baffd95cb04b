"""The model of the minimum number of hit groups (tests/hit_groups_ref.py) held against the oracle on the CPU, and the worlds of
tests/test_gpu_hit_groups.py checked for what they are built to hold: the found positions of every unit are the oracle's n_hits,
G <= n_hits, a share of the parity units changes at N = 5 and a share stays, the tandem-repeat reads have many hits and few keys, the
long reads bring their N-th key in the last chunk or never."""
import numpy as np
import pytest

import hit_groups_ref as HG


@pytest.mark.parametrize("paired", [False, True])
def test_model_counts_the_oracles_hits(oracle, small_world, paired):
    w, reads, units, g, found = HG.parity_case(oracle, small_world, paired)
    assert len(units) == (300 if paired else 600)
    assert found.tolist() == [u[3].size for u in units]
    assert (g <= found).all()                                           # (fewer: a key at two positions, or in both mates -- the repeat tests)
    taxa = np.array([u[0] for u in units], dtype=np.uint32)
    assert ((taxa != 0) <= (g >= 1)).all()                              # a taxon implies a hit: N = 1 changes nothing
    assert np.array_equal(HG.apply(taxa, g, 0), taxa) and np.array_equal(HG.apply(taxa, g, 1), taxa)
    at5 = HG.apply(taxa, g, 5)
    changed, kept = np.count_nonzero(at5 != taxa), np.count_nonzero(at5)
    print("paired %d: %d units, %d classified, %d changed at N = 5, %d still classified; G max %d" % (paired, taxa.size, np.count_nonzero(taxa), changed, kept, g.max()))
    # the thinned db leaves a 150-base read about ten keys and 2 % substitutions about half of those: N = 5 cuts through the middle
    assert changed >= taxa.size // 10 and kept >= taxa.size // 10
    assert np.count_nonzero(HG.apply(taxa, g, 64)) == 0 or g.max() >= 64
    for n in (2, 3, 8):
        assert np.count_nonzero(HG.apply(taxa, g, n) != HG.apply(taxa, g, n - 1)) > 0, n


def test_apply():
    assert HG.apply([5, 0, 7, 0xFFFFFFFF], [3, 0, 2, 1], 3).tolist() == [5, 0, 0, 0]
    assert HG.apply([5, 0, 7, 0xFFFFFFFF], [3, 0, 2, 1], 0).tolist() == [5, 0, 7, 0xFFFFFFFF]
    assert int(HG.apply(9, 64, 64)) == 9 and int(HG.apply(9, 63, 64)) == 0


def test_tandem_repeat_reads(oracle):
    w, at = HG.repeat_world(oracle)
    g = w.genomes[1001]
    for off in range(HG.PERIOD):
        read = g[at + 100 + off:at + 250 + off]
        G, found = HG.groups(oracle, w.table, (read,), 31)
        assert found == 120 and 1 <= G <= HG.PERIOD, (off, G, found)
        keys = HG.unit_keys(oracle, (read,), 31)
        assert np.unique(keys[:64]).size == G                            # every key of the read is in its first round: later rounds bring duplicates only


@pytest.mark.parametrize("n", [2, 33, 64])
def test_late_key_reads(oracle, n):
    w = HG.long_world(oracle)
    never, late = HG.late_key_reads(oracle, w, n)
    assert never.size == late.size == 10000
    g_never, f_never = HG.groups(oracle, w.table, (never,), 31)
    g_late, f_late = HG.groups(oracle, w.table, (late,), 31)
    assert g_never == n - 1 and g_late == n and f_never > 150
    keys = HG.unit_keys(oracle, (late,), 31)
    found = w.table.get_batch(keys)[1] != 0
    first = {}
    for i in np.flatnonzero(found):
        first.setdefault(int(keys[i]), int(i))
    assert max(first.values()) == keys.size - 1                          # the n-th key is the read's last k-mer: past five chunks of 1984 k-mers
    assert sorted(first.values())[-2] < 2 * 1984                         # ... and all the others are in the first two chunks
