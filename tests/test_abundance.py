"""`bonsai abundance` (bns::estimate_abundance through hostio.estimate_abundance; no device) against tests/abundance_model.py, the
definition restated with fractions.Fraction.  Tolerances: abundance_model's docstring."""
from fractions import Fraction

import numpy as np
import pytest

import abundance_model as AM
from bonsai_amd import hostio

# two genera, four species, two strains under one species
PAIRS = [(1, 1), (10, 1), (20, 1), (101, 10), (102, 10), (201, 20), (202, 20), (1011, 101), (1012, 101)]
RANKS = {1: "no rank", 10: "genus", 20: "genus", 101: "species", 102: "species", 201: "species", 202: "species", 1011: "strain",
         1012: "no rank"}
NAMES = {101: "Aus bus", 202: "Cus dus", 10: "Aus"}
DIRECT = {0: 37, 1: 50, 10: 30, 20: 12, 101: 40, 102: 25, 201: 10, 202: 4, 1011: 20, 1012: 3, AM.NOT_IN_TAXONOMY: 2}
DISTRIB = {1: [(1011, 5, 100), (1012, 10, 100), (102, 10, 200), (201, 30, 300), (202, 60, 300)],
           10: [(1011, 50, 100), (102, 50, 200), (1012, 0, 100)],
           20: [(202, 100, 300)],                  # every genome of this line is dropped by -T: not distributed
           101: [(1011, 40, 100)]}                 # (a line of a taxon at the level: not used)


def par_of(pairs):
    return {c: (0 if p == c else p) for c, p in pairs}


def distrib_text(d):
    return "mapped_taxid\tgenome_taxids:kmers_mapped:total_genome_kmers\n" + "".join(
        "%d\t%s\n" % (t, " ".join("%d:%d:%d" % e for e in sorted(d[t]))) for t in sorted(d))


def report_text(direct, fields=6):
    """lines of the layout `classify -R` writes (the columns abundance does not read hold fillers)"""
    out = []
    for t in sorted(direct):
        name = "unclassified" if t == 0 else "(not in taxonomy)" if t == AM.NOT_IN_TAXONOMY else "  node %d" % t
        extra = {6: [], 7: ["77"], 9: ["77", "1234", "0.062399"]}[fields]
        out.append("\t".join(["%6.2f" % 1.0, str(direct[t] + 5), str(direct[t])] + extra + ["U" if t == 0 else "S1", str(t), name]) + "\n")
    return "".join(out)


def write_world(d, pairs, ranks, names=None, roots=()):
    with open(d / "nodes.dmp", "w") as f:
        for c, p in pairs:
            f.write("%d\t|\t%d\t|\t%s\t|\t\t|\n" % (c, 0 if c in roots else p, ranks[c]))
    if names:
        with open(d / "names.dmp", "w") as f:
            for t, nm in names.items():
                f.write("%d\t|\t%s\t|\t\t|\tscientific name\t|\n" % (t, nm))
                f.write("%d\t|\tsomething else\t|\t\t|\tsynonym\t|\n" % t)
    return str(d / "nodes.dmp"), (str(d / "names.dmp") if names else None)


def run(d, distrib, direct, nodes, names_path=None, fields=6, **kw):
    (d / "distrib.txt").write_text(distrib_text(distrib))
    (d / "report.txt").write_text(report_text(direct, fields))
    return hostio.estimate_abundance(d / "distrib.txt", d / "report.txt", nodes, names_path, **kw)


def test_hand_made_tree(tmp_path):
    nodes, names_path = write_world(tmp_path, PAIRS, RANKS, NAMES)
    par = par_of(PAIRS)
    text, totals = run(tmp_path, DISTRIB, DIRECT, nodes, names_path)
    rows, want = AM.estimate(DISTRIB, DIRECT, par, RANKS, "S", 10, NAMES)
    AM.check(text, totals, rows, want)
    # by hand: base 101 = 40 + 20 + 3 = 63, 102 = 25, 201 = 10; 202 = 4 < 10 is dropped: 4 reads discarded, and genus 20's only
    # genome belongs to it, so its 12 reads are not distributed
    assert [(r[1], r[3]) for r in rows] == [(101, 63), (102, 25), (201, 10)]
    assert want[:4] == [sum(DIRECT.values()), 39, 4, 12]
    # genus 10: weights 101: (50/100 + 0/100) 63 = 31.5, 102: (50/200) 25 = 6.25 -> 30 reads as 30 * 31.5 / 37.75 and 30 * 6.25 / 37.75
    # root 1: 101: (5/100 + 10/100) 63 = 9.45, 102: (10/200) 25 = 1.25, 201: (30/300) 10 = 1 -> 50 reads over 11.7
    w = Fraction(63 * 15, 100) + Fraction(25, 20) + 1
    assert rows[0][4] == 30 * Fraction(63, 2) / Fraction(151, 4) + 50 * Fraction(63 * 15, 100) / w
    assert rows[2][4] == 50 / w
    assert text.split("\n")[1].startswith("Aus bus\t101\tS\t63\t") and text.split("\n")[2].startswith("102\t102\tS\t25\t")
    # without names every taxon is named by its id; -T 0 keeps 202, which then takes genus 20's reads
    text, totals = run(tmp_path, DISTRIB, DIRECT, nodes, None, min_reads=0)
    rows, want = AM.estimate(DISTRIB, DIRECT, par, RANKS, "S", 0)
    AM.check(text, totals, rows, want)
    assert [r[1] for r in rows] == [101, 102, 201, 202] and rows[3][4] >= 12 and want[2] == 0 and want[3] == 0


def test_genus_level(tmp_path):
    nodes, _ = write_world(tmp_path, PAIRS, RANKS)
    text, totals = run(tmp_path, DISTRIB, DIRECT, nodes, level="G")
    rows, want = AM.estimate(DISTRIB, DIRECT, par_of(PAIRS), RANKS, "G", 10)
    AM.check(text, totals, rows, want)
    assert [(r[1], r[2], r[3]) for r in rows] == [(10, "G", 30 + 40 + 25 + 20 + 3), (20, "G", 12 + 10 + 4)]
    assert want[3] == 0 and rows[0][4] + rows[1][4] == 50              # only the root's reads are above the level


def test_report_field_counts(tmp_path):
    nodes, _ = write_world(tmp_path, PAIRS, RANKS)
    texts = [run(tmp_path, DISTRIB, DIRECT, nodes, fields=n) for n in (6, 7, 9)]
    assert texts[0] == texts[1] == texts[2]


def test_no_line_and_no_reads(tmp_path):
    nodes, _ = write_world(tmp_path, PAIRS, RANKS)
    distrib = {k: v for k, v in DISTRIB.items() if k != 10}           # genus 10 has reads and no line
    text, totals = run(tmp_path, distrib, DIRECT, nodes)
    rows, want = AM.estimate(distrib, DIRECT, par_of(PAIRS), RANKS, "S", 10)
    AM.check(text, totals, rows, want)
    assert want[3] == 30 + 12
    direct = {0: 5, AM.NOT_IN_TAXONOMY: 1, 1: 3}                      # nothing at the level: a header, nothing estimated
    text, totals = run(tmp_path, DISTRIB, direct, nodes)
    assert text == AM.HEADER and totals == {"all": 9.0, "unclassified": 6.0, "discarded": 0.0, "not_distributed": 3.0, "estimated": 0.0}
    text, totals = run(tmp_path, {}, {}, nodes)                        # empty inputs
    assert text == AM.HEADER and totals["all"] == 0.0


def random_forest(seed, n_nodes=200):
    rng = np.random.default_rng(seed)
    ids = [1] + sorted(rng.choice(np.arange(2, 5000), size=n_nodes - 1, replace=False).tolist())
    rng.shuffle(ids[1:])
    pairs, depth, roots = [(1, 1)], {1: 0}, {ids[1], ids[2]}
    for i, t in enumerate(ids[1:], 1):
        if t in roots:
            pairs.append((t, 0)); depth[t] = 0
            continue
        p = ids[int(rng.integers(0, i))]
        pairs.append((t, p)); depth[t] = depth[p] + 1
    by_depth = ["no rank", "phylum", "genus", "species"]
    ranks = {t: (by_depth[d] if d < 4 and rng.random() > 0.1 else "no rank") for t, d in depth.items()}
    direct = {int(t): int(rng.integers(0, 400)) for t in ids if rng.random() < 0.7}
    direct[0], direct[AM.NOT_IN_TAXONOMY] = 1234, 7
    direct[4999 + 3] = 11                                              # a taxid the taxonomy does not hold
    distrib = {}
    for t in ids:
        if rng.random() < 0.6:
            gs = rng.choice(ids, size=int(rng.integers(1, 12)), replace=False).tolist()
            distrib[int(t)] = [(int(g), int(rng.integers(0, 1001)), 1000 + int(g) % 7) for g in gs]
    return pairs, ranks, roots, direct, distrib


@pytest.mark.parametrize("level,min_reads", [("S", 60), ("G", 150), ("P", 0)])
def test_random_forest(tmp_path, level, min_reads):
    pairs, ranks, roots, direct, distrib = random_forest(77)
    nodes, _ = write_world(tmp_path, pairs, ranks, roots=roots)
    par = {c: (0 if (c in roots or c == 1) else p) for c, p in pairs}
    text, totals = run(tmp_path, distrib, direct, nodes, level=level, min_reads=min_reads)
    rows, want = AM.estimate(distrib, direct, par, ranks, level, min_reads)
    AM.check(text, totals, rows, want)
    assert len(rows) >= 5 and want[3] > 0 and any(r[4] > 0 for r in rows)
    if min_reads:
        assert want[2] > 0


def test_malformed_inputs(tmp_path):
    nodes, _ = write_world(tmp_path, PAIRS, RANKS)
    good_d, good_r = distrib_text(DISTRIB), report_text(DIRECT)

    def fails(d, r, *needles, **kw):
        (tmp_path / "d.txt").write_text(d)
        (tmp_path / "r.txt").write_text(r)
        with pytest.raises(hostio.HostIOError) as e:
            hostio.estimate_abundance(tmp_path / "d.txt", tmp_path / "r.txt", nodes, **kw)
        assert all(n in str(e.value) for n in needles), str(e.value)

    lines = good_d.split("\n")
    fails("taxid\tstuff\n" + "\n".join(lines[1:]), good_r, "distrib", "line 1")
    fails("\n".join(lines[:2] + ["10\t1011:5"] + lines[3:]), good_r, "distrib", "line 3")
    fails("\n".join(lines[:2] + ["10\t1011:5:0"] + lines[3:]), good_r, "distrib", "line 3")
    fails("\n".join(lines[:2] + ["10\t1011:7:5"] + lines[3:]), good_r, "distrib", "line 3")
    fails("\n".join(lines[:2] + ["x\t1011:5:9"] + lines[3:]), good_r, "distrib", "line 3")
    fails("\n".join(lines[:2] + ["", ""] + lines[3:]), good_r, "distrib", "line 3")
    fails(good_d + lines[1] + "\n", good_r, "distrib", "line %d" % len(lines))              # a taxid's second line
    rl = good_r.split("\n")
    fails(good_d, "\n".join(rl[:1] + ["\t".join(rl[1].split("\t")[1:])] + rl[2:]), "report", "line 2")      # five fields
    fails(good_d, "\n".join(rl[:2] + [rl[2] + "\tx\ty"] + rl[3:]), "report", "line 3")                      # eight
    f = rl[3].split("\t")
    fails(good_d, "\n".join(rl[:3] + ["\t".join(f[:2] + ["1e3"] + f[3:])] + rl[4:]), "report", "line 4")    # the direct count
    fails(good_d, "\n".join(rl[:3] + ["\t".join(f[:4] + ["ten"] + f[5:])] + rl[4:]), "report", "line 4")    # the taxid
    fails(good_d, good_r, "level", level="X")
    with pytest.raises(hostio.HostIOError):
        hostio.estimate_abundance(tmp_path / "absent.txt", tmp_path / "r.txt", nodes)
