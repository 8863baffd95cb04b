"""CPU tier: the host side of the distinct k-mer column of `bonsai classify -R -u` -- bns::hll_estimate and the eight-column
format_report in libbns_host -- against the numpy model of tests/sketch_model.py, on test_report.py's hand-written taxonomy."""
import numpy as np
import pytest

import sketch_model as SM
import test_report as TR
from test_report import hostio  # noqa: F401  (the module's fixture)


def random_keys(rng, n):
    k = np.unique(rng.integers(0, 1 << 64, size=n + n // 8 + 8, dtype=np.uint64))
    assert k.size >= n
    return rng.permutation(k)[:n]


@pytest.mark.parametrize("n_keys", [1, 10, 120, 1000, 5970, 36000, 200000])
def test_estimate_equals_the_model(hostio, n_keys):
    rng = np.random.default_rng(1000 + n_keys)
    reg = SM.registers(random_keys(rng, n_keys))
    want = SM.estimate(reg)
    assert hostio.hll_estimate(reg) == want
    # six standard errors of a 4096-register sketch (1.04 / sqrt(m)); below m registers' worth of keys the linear count is far closer
    assert abs(want - n_keys) <= max(1, 6 * 1.04 / 64 * n_keys)


def test_estimate_edges(hostio):
    assert hostio.hll_estimate(np.zeros(4096, np.uint8)) == 0
    one = np.zeros(4096, np.uint8); one[77] = 53                    # (a key whose hash ends in 52 zero bits)
    assert hostio.hll_estimate(one) == SM.estimate(one) == 1
    full = np.full(4096, 40, np.uint8)                               # no zero register, nothing for the small-range branch
    assert hostio.hll_estimate(full) == SM.estimate(full) > 1 << 50
    with pytest.raises(ValueError):
        hostio.hll_estimate(np.zeros(100, np.uint8))


def test_model_registers_by_hand():
    """fmix64 and the rank, spelled out in Python integers for a few keys"""
    mask = (1 << 64) - 1
    for x in (0, 1, 0x0123456789ABCDEF, mask, 31337):
        h = x
        h ^= h >> 33; h = h * 0xff51afd7ed558ccd & mask
        h ^= h >> 33; h = h * 0xc4ceb9fe1a85ec53 & mask
        h ^= h >> 33
        assert int(SM.fmix64(np.array([x], np.uint64))[0]) == h
        w = (h << 12) & mask
        rho = 53 if w == 0 else 64 - w.bit_length() + 1
        reg = SM.registers(np.array([x], np.uint64))
        assert reg[h >> 52] == rho and np.count_nonzero(reg) == 1


def test_report_distinct_column(hostio, tmp_path):
    nodes, names = TR.write_dmps(tmp_path)
    parent = hostio.read_nodes_dmp(nodes)
    n = parent.size
    direct = np.zeros(n + 1, np.uint64); clade = np.zeros(n + 1, np.uint64)
    for t, c in TR.DIRECT.items():
        direct[t] = c
    for t, c in TR.CLADE.items():
        clade[t] = c
    direct[0] = clade[0] = TR.UNCLASSIFIED
    direct[n] = clade[n] = TR.NOT_IN_TAX
    ranks, nm = hostio.read_node_ranks(nodes), hostio.read_scientific_names(names)
    seven = hostio.format_report(direct, clade, parent, ranks, nm)
    assert seven == TR.EXPECTED                                      # the seven-column report is what it was

    rng = np.random.default_rng(9)
    pool = random_keys(rng, 60000)
    # sketched bins: leaves and inner nodes, two that share keys (562 and 83333), one whose clade counts no unit (620: not printed, but
    # part of 543's clade), bin 0 (printed nowhere) and bin n
    keys = {83333: pool[:1000], 562: pool[800:1500], 564: pool[2000:2040], 561: pool[3000:3001], 620: pool[4000:9000], 1117: pool[9000:9120],
            2: pool[10000:46000], 12000: pool[50000:50010], 0: pool[51000:51500], n: pool[52000:52300]}
    bins = np.array(sorted(keys), dtype=np.uint32)
    regs = np.stack([SM.registers(keys[int(b)]) for b in bins])
    got = hostio.format_report(direct, clade, parent, ranks, nm, sketch_bins=bins, sketch_registers=regs)
    pairs = [(t, p) for t, p, _, _ in TR.NODES]
    want_d = SM.clade_estimates(bins[(bins != 0) & (bins != n)], regs[(bins != 0) & (bins != n)], pairs)
    want_d[n] = SM.estimate(regs[-1])
    assert got == SM.add_column(seven, want_d, n)
    # the same lines in the same order, one more column after the direct count
    cut = "".join("\t".join(f[:3] + f[4:]) + "\n" for f in (ln.split("\t") for ln in got.splitlines()))
    assert cut == seven
    col = {int(f[5]): int(f[3]) for f in (ln.split("\t") for ln in got.splitlines())}
    assert col[0] == 0                                               # unclassified: no k-mers
    assert col[4294967295] == SM.estimate(SM.registers(keys[n]))
    assert col[83333] == SM.estimate(SM.registers(keys[83333]))
    assert col[562] == SM.estimate(SM.registers(np.concatenate([keys[562], keys[83333]])))      # a clade is a union: shared keys once
    assert col[562] < col[83333] + SM.estimate(SM.registers(keys[562]))
    assert col[543] == SM.estimate(SM.registers(np.concatenate([keys[t] for t in (620, 561, 562, 564, 83333)])))
    assert col[1] == col[131567] == col[2] > col[1224] >= col[543]
    assert col[10239] == col[12000] == 10
    # no sketches at all: zeros in the column
    empty = hostio.format_report(direct, clade, parent, ranks, nm, sketch_bins=np.zeros(0, np.uint32), sketch_registers=np.zeros((0, 4096), np.uint8))
    assert empty == SM.add_column(seven, {}, n)
    assert hostio.format_report(np.zeros(n + 1), np.zeros(n + 1), parent, [], {}, sketch_bins=bins, sketch_registers=regs) == ""
