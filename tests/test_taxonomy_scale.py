"""CPU tier for tests/taxonomy_ref.py, the plain restatements the GPU tier (test_gpu_taxonomy_scale.py) holds the device against at NCBI
scale: its confidence walk against tests/confidence_ref.py, its report against test_report's hand-written one and against
bns::format_report on a 2.5 M-key taxonomy; and the Python binding's refusal of thresholds whose terms do not fit 64 bits."""
import re
import types
from collections import Counter
from fractions import Fraction

import numpy as np
import pytest

import confidence_ref as cr
import synth
import taxonomy_ref as tr
import test_report
from bonsai_amd.context import Context, confidence_fraction
from test_report import hostio  # noqa: F401  (the module's fixture)

THETAS = [Fraction(0), Fraction("0.05"), Fraction("0.1"), Fraction("0.25"), Fraction("0.5"), Fraction("0.75"), Fraction("0.9"), Fraction(1)]


def tax_pairs_parent(pairs=synth.TAX_PAIRS):
    n = max(max(c, p) for c, p in pairs) + 1
    parent = np.full(n, tr.TAX_ABSENT, np.uint32)
    for c, p in pairs:
        parent[c] = 0 if c == 1 else p
    return parent


def random_parent(rng, n):
    """a small parent array: a tree under root 1, a few more roots, ids that are not keys, subtrees below such ids (chains that break)"""
    parent = np.full(n, tr.TAX_ABSENT, np.uint32)
    parent[1] = 0
    ids = rng.permutation(np.arange(2, n))
    keys, absent = ids[: int(n * 0.7)].tolist(), ids[int(n * 0.7):].tolist()
    placed = [1]
    for i in keys:
        r = rng.random()
        if r < 0.05:
            parent[i] = 0
        elif r < 0.1 and absent:
            parent[i] = absent[int(rng.integers(len(absent)))]
        else:
            parent[i] = placed[-1 - int(rng.integers(min(len(placed), 6)))]       # (mostly below a recent node: deep chains)
        placed.append(i)
    return parent


# test_confidence.py's hand-worked cases on synth.TAX_PAIRS: (theta, taxon, missing, hits, answer)
HAND = [(Fraction(3, 10), 1001, 0, [1001] * 3 + [2001] * 7, 1001), (Fraction(31, 100), 1001, 0, [1001] * 3 + [2001] * 7, 1),
        (Fraction(1, 2), 1001, 5, [1001] * 2 + [1002] * 3, 101), (Fraction(1, 5), 1001, 5, [1001] * 2 + [1002] * 3, 1001),
        (1, 1001, 1, [1001] * 10, 0), (1, 1001, 0, [1001] * 10, 1001),
        (Fraction(1, 2), 1500, 0, [1001] * 4, 1500), (Fraction(1, 2), 7777, 0, [1001] * 4, 7777),
        (Fraction(1, 2), 0xFFFFFFFF, 0, [1001] * 4, 0xFFFFFFFF), (1, 2001, 50, [1001], 0),
        (Fraction(1, 2), 1001, 0, [1001] * 5 + [7777] * 3 + [1500] * 2, 1001), (Fraction(3, 5), 1001, 0, [1001] * 5 + [7777] * 3 + [1500] * 2, 0),
        (Fraction("0.1"), 1001, 0, [1001] * 3 + [2001] * 27, 1001), (Fraction("0.1"), 1001, 1, [1001] * 3 + [2001] * 27, 1),
        (Fraction("0.07"), 1001, 0, [1001] * 7 + [2001] * 93, 1001),
        (Fraction(1, 2), 1001, 8, [1001, 1002], 0), (Fraction(1, 2), 1, 8, [1001, 2001], 0)]
HAND += [(0, t, 5, [2001], t) for t in (0, 1, 1001, 2002, 1500, 0xFFFFFFFF)]


def test_fast_walk_hand_worked():
    parent = tax_pairs_parent()
    for th, t, m, h, want in HAND:
        assert tr.walker(parent, t, m, h)(th) == want, (th, t, m, h)
    broken = tax_pairs_parent([(c, p) for c, p in synth.TAX_PAIRS if c != 201])
    assert tr.walker(broken, 2001, 50, [1001])(1) == 2001
    assert tr.up_chain(parent, 1001) == [1001, 101, 11, 2, 1] and tr.up_chain(broken, 2002) is None


def test_fast_walk_matches_confidence_ref():
    rng = np.random.default_rng(3)
    walked, deep = Counter(), 0
    for _ in range(60):
        n = int(rng.integers(6, 160))
        parent = random_parent(rng, n)
        par = cr.parent_map(parent)
        keys = [i for i in range(1, n) if parent[i] != tr.TAX_ABSENT]
        others = [i for i in range(1, n) if parent[i] == tr.TAX_ABSENT] + [n, n + 7, 0xFFFFFFFF]
        pool = keys * 4 + others
        for _ in range(30):
            t = int(rng.choice(pool + [0]))
            hits = [int(x) for x in rng.choice(pool, size=int(rng.integers(0, 40)))]
            m = int(rng.integers(0, 25))
            fast, slow = tr.walker(parent, t, m, hits), cr.walker(par, t, m, hits)
            thetas = THETAS + sorted(cr.boundaries(par, t, m, hits)) + [Fraction(int(rng.integers(0, 97)), 97)]
            for th in thetas:
                got = fast(th)
                assert got == slow(th), (n, t, m, hits, th)
                walked[got == t] += 1
            deep = max(deep, len(fast.up or []))
    assert walked[False] > 1000 and walked[True] > 1000 and deep >= 10       # (walks that climb and walks that stay; chains of some depth)


def hand_written_arrays():
    n = 131568
    parent = np.full(n, tr.TAX_ABSENT, np.uint32)
    ranks = [""] * n
    for t, p, r, _ in test_report.NODES:
        parent[t] = 0 if t == 1 else p
        ranks[t] = r
    names = {t: nm for t, _, _, nm in test_report.NODES if nm is not None}
    direct = np.zeros(n + 1, np.uint64)
    for t, c in test_report.DIRECT.items():
        direct[t] = c
    direct[0], direct[n] = test_report.UNCLASSIFIED, test_report.NOT_IN_TAX
    return parent, ranks, names, direct


def test_report_restatement_hand_written():
    parent, ranks, names, direct = hand_written_arrays()
    clade = tr.clade_sums(parent, direct)
    assert {t: int(clade[t]) for t in test_report.CLADE} == test_report.CLADE
    assert tr.report(direct, parent, ranks, names) == test_report.EXPECTED
    assert tr.report(direct, parent, ranks, {}).splitlines()[2] == " 51.11\t23\t0\tR1\t131567\t  131567"
    assert tr.report(np.zeros(parent.size + 1, np.uint64), parent, [], {}) == ""
    # from the units' taxa: 0 unclassified; ids that are no key, or no id at all, go to bin n
    taxa = [0] * 10 + [t for t, c in test_report.DIRECT.items() for _ in range(c)] + [7, 131600, 0xFFFFFFFF]
    assert tr.report_from_taxa(taxa, parent, ranks, names) == test_report.EXPECTED


@pytest.fixture(scope="module")
def big():
    t = tr.make_taxonomy(0)
    t.dep = tr.depths(t.parent)
    return t


def test_big_taxonomy_shape(big):
    t, dep = big, big.dep
    keys = t.keys
    assert keys.size >= 1_500_000 and t.n >= 3_000_000 and t.parent[t.n - 1] != tr.TAX_ABSENT
    assert np.count_nonzero(keys[1:] < t.parent[keys[1:]]) > keys.size // 4      # (children numbered below their parents)
    ok = dep >= 0
    assert 20 <= np.median(dep[ok]) <= 40 and np.count_nonzero((dep >= 20) & (dep <= 40)) > keys.size // 2
    assert dep[t.deep[-1]] - dep[t.deep[0]] >= 2000 - 1 and np.count_nonzero(t.parent == t.wide) >= 100_000
    assert t.parent[t.root2] == 0 and t.root2 != 1 and tr.LETTER.get(t.ranks[t.root2], "") == ""
    assert not ok[t.broken].any() and t.parent[t.missing_parent] == tr.TAX_ABSENT and t.parent[t.broken[0]] == t.missing_parent
    assert t.non_keys.size > 100_000 and (t.parent[t.non_keys] == tr.TAX_ABSENT).all()
    assert np.count_nonzero(ok) == keys.size - t.broken.size
    assert {tr.LETTER.get(r) for r in set(t.ranks)} >= set(tr.LETTER.values()) | {None}


def test_clade_sums_against_chain_walks(big):
    t, dep = big, big.dep
    rng = np.random.default_rng(9)
    direct = np.zeros(t.n + 1, np.uint64)
    sel = np.concatenate([rng.choice(np.nonzero(dep >= 0)[0], 3000, replace=False), t.deep[-5:], t.wide_kids[:50]])
    direct[sel] = rng.integers(1, 1 << 40, sel.size).astype(np.uint64)
    direct[0], direct[t.n] = 5, 6
    clade = tr.clade_sums(t.parent, direct, dep)
    want = Counter()
    for v in np.unique(sel).tolist():
        for a in tr.up_chain(t.parent, v):
            want[a] += int(direct[v])
    nz = np.nonzero(clade[1:t.n])[0] + 1
    assert {int(v): int(clade[v]) for v in nz} == dict(want)
    assert clade[0] == 5 and clade[t.n] == 6 and clade[1] + clade[t.root2] == direct[1:t.n].sum()
    bad = direct.copy()
    bad[t.broken[3]] = 1
    with pytest.raises(AssertionError):
        tr.clade_sums(t.parent, bad, dep)


def test_bins(big):
    t = big
    n = t.n
    taxa = np.array([0, 1, t.root2, t.deep[-1], t.broken[0], t.broken[-1], t.non_keys[5], t.missing_parent, n - 1, n, n + 5,
                     (1 << 28) + 1, 0xFFFFFFFF], dtype=np.uint32)
    assert tr.bins(t.parent, taxa, t.dep >= 0).tolist() == [0, 1, t.root2, t.deep[-1], n, n, n, n, n - 1, n, n, n, n]


def first_difference(a, b):
    la, lb = a.splitlines(), b.splitlines()
    for i, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            return i, x[:200], y[:200]
    return min(len(la), len(lb)), len(la), len(lb)


def test_report_matches_the_formatter_at_scale(hostio, big):  # noqa: F811
    t, dep = big, big.dep
    n = t.n
    rng = np.random.default_rng(17)
    direct = np.zeros(n + 1, np.uint64)
    sel = rng.choice(np.nonzero(dep >= 0)[0], 40_000, replace=False)
    direct[sel] = rng.integers(0, 100, sel.size).astype(np.uint64)              # (zeros among them)
    direct[sel[:300]] = rng.integers(1 << 30, 1 << 40, 300).astype(np.uint64)
    direct[t.deep[::3]] = 1                                                   # the whole chain prints: codes far beyond S1
    direct[t.wide_kids[:6000]] = 7                                            # 6000 siblings tie on their clades
    direct[t.root2_nodes[::2]] = 2
    direct[1] = 3
    direct[0], direct[n] = 123_456, 1 << 40
    clade = tr.clade_sums(t.parent, direct, dep)
    want = tr.report(direct, t.parent, t.ranks, t.names, clade)
    got = hostio.format_report(direct, clade, t.parent, t.ranks, t.names)
    assert got == want, first_difference(got, want)
    # the report reaches what it is there for
    rows = [x.split("\t") for x in want.splitlines()]
    assert len(rows) > 100_000
    assert rows[0][3:] == ["U", "0", "unclassified"] and rows[-1][3:] == ["-", "4294967295", "(not in taxonomy)"]
    codes = Counter(r[3] for r in rows)
    assert max(int(c[1:]) for c in codes if re.fullmatch(r"S\d+", c)) >= 1000 and codes["-"] >= 3
    roots = [int(r[4]) for r in rows[1:-1] if not r[5].startswith(" ")]
    assert roots == [1, t.root2]                                              # two roots, by taxid
    assert max(len(r[5]) - len(r[5].lstrip(" ")) for r in rows) >= 2 * 2000   # (chains deeper than any recursion limit)
    tied = set(t.wide_kids[:6000][clade[t.wide_kids[:6000]] == 7].tolist())
    order = [int(r[4]) for r in rows[1:-1] if int(r[4]) in tied]
    assert len(order) >= 5000 and order == sorted(order)                      # ties by taxid, ascending
    assert any(ord(ch) > 127 for ch in want) and sum(" " in r[5].strip() for r in rows) > 1000
    assert sum(r[5].strip() == r[4] for r in rows[1:-1]) > 100                # (ids without a name print as their id)
    # no unclassified / not-in-taxonomy units: neither line; without names every taxon is its id
    direct[0] = direct[n] = clade[0] = clade[n] = 0
    got = hostio.format_report(direct, clade, t.parent, t.ranks, {})
    assert got == tr.report(direct, t.parent, t.ranks, {}, clade)
    assert "\tunclassified\n" not in got and "(not in taxonomy)" not in got


def test_confidence_fraction_64_bit_terms():
    top = 2 ** 64 - 1
    assert confidence_fraction(Fraction(1, top)) == (1, top)
    assert confidence_fraction(Fraction(top - 1, top)) == (top - 1, top)
    assert confidence_fraction(Fraction(top, top)) == (1, 1)
    assert confidence_fraction(Fraction(2 ** 64, 2 ** 65)) == (1, 2)                # (terms are reduced first)
    for bad in (Fraction(1, 2 ** 64), Fraction(1, 2 ** 64 + 3), Fraction(2 ** 64 + 1, 2 ** 64 + 3), Fraction(2 ** 70 - 1, 2 ** 70),
                "1/18446744073709551619"):
        with pytest.raises(ValueError):
            confidence_fraction(bad)
    stub = types.SimpleNamespace()                       # no library, no context: the value is refused first
    with pytest.raises(ValueError):
        Context.set_confidence(stub, Fraction(1, 2 ** 64 + 3))
