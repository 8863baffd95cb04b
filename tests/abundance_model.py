"""`bonsai abundance` restated from its definition in DESIGN.md with fractions.Fraction: exact arithmetic, plain parent walks,
nothing shared with the host code.  Also the readers the tests need for the tool's inputs and output.  Test infrastructure only.

Tolerances (the only ones used): exact integer fields compare exactly; the tool's doubles agree with the exact value within relative
1e-9 -- every sum is of fewer than 2^20 non-negative terms and each operation has relative error 2^-53, so the total stays below
2^-33 -- with the printed precision on top: 5e-4 for the %.3f fields, 5e-7 for %.6f."""
from fractions import Fraction

LETTER = {"superkingdom": "D", "domain": "D", "kingdom": "K", "phylum": "P", "class": "C", "order": "O", "family": "F", "genus": "G",
          "species": "S"}
NOT_IN_TAXONOMY = 4294967295
HEADER = "name\ttaxonomy_id\ttaxonomy_lvl\tkraken_assigned_reads\tadded_reads\tnew_est_reads\tfraction_total_reads\n"
REL = 1e-9


def level_of(par, ranks, letter, t):
    """the first of t, parent(t), ... whose own rank maps to the letter; 0: none"""
    seen = set()
    while t and t in par and t not in seen:
        if LETTER.get(ranks.get(t, "no rank"), "") == letter:
            return t
        seen.add(t)
        t = par[t]
    return 0


def parse_distrib(text):
    """-> {called taxid: [(genome, here, all), ...]}"""
    lines = text.split("\n")
    assert lines[0] == "mapped_taxid\tgenome_taxids:kmers_mapped:total_genome_kmers" and lines[-1] == ""
    out = {}
    for line in lines[1:-1]:
        t, entries = line.split("\t")
        out[int(t)] = sorted(tuple(int(x) for x in e.split(":")) for e in entries.split(" "))
    return out


def parse_report(text):
    """a `classify -R` report (6, 7 or 9 fields, read from the right) -> {taxid: direct}"""
    direct = {}
    for line in text.split("\n")[:-1]:
        f = line.split("\t")
        assert len(f) in (6, 7, 9)
        direct[int(f[-2])] = int(f[2])
    return direct


def estimate(distrib, direct, par, ranks, level="S", min_reads=10, names=None):
    """distrib as parse_distrib gives it, direct {taxid: reads}, par {id: parent, 0 for a root}, ranks {id: rank}
    -> (rows [(name, taxid, level, base, added, new_est, fraction)] with Fractions, totals [all, unclassified, discarded,
    not distributed, sum of new_est])"""
    names = names or {}
    all_reads = sum(direct.values())
    unclassified = direct.get(0, 0) + direct.get(NOT_IN_TAXONOMY, 0)
    base, above = {}, []
    for t in sorted(direct):
        if t in (0, NOT_IN_TAXONOMY) or direct[t] == 0:
            continue
        s = level_of(par, ranks, level, t)
        if s:
            base[s] = base.get(s, 0) + direct[t]
        else:
            above.append(t)
    kept = {s for s, b in base.items() if b >= min_reads}
    discarded = sum(b for s, b in base.items() if s not in kept)
    added = {s: Fraction(0) for s in kept}
    not_distributed = 0
    for n in above:
        weight = {}
        for g, here, total in distrib.get(n, []):
            s = level_of(par, ranks, level, g)
            if s in kept:
                weight[s] = weight.get(s, Fraction(0)) + Fraction(here, total) * base[s]
        whole = sum(weight.values())
        if whole == 0:
            not_distributed += direct[n]
            continue
        for s, w in weight.items():
            added[s] += direct[n] * w / whole
    est = {s: base[s] + added[s] for s in kept}
    whole = sum(est.values())
    rows = [(names.get(s, str(s)), s, level, base[s], added[s], est[s], est[s] / whole if whole else Fraction(0)) for s in sorted(kept)]
    return rows, [all_reads, unclassified, discarded, not_distributed, whole]


def parse_output(text):
    assert text.startswith(HEADER) and text.endswith("\n")
    rows = []
    for line in text[len(HEADER):].split("\n")[:-1]:
        name, taxid, lvl, base, added, est, frac = line.split("\t")
        assert len(added.split(".")[1]) == 3 and len(est.split(".")[1]) == 3 and len(frac.split(".")[1]) == 6
        rows.append((name, int(taxid), lvl, int(base), float(added), float(est), float(frac)))
    return rows


def close(got, want, printed):
    return abs(got - float(want)) <= printed + REL * abs(float(want))


def check(text, totals, rows, want_totals):
    """the tool's table and totals against the model's, within the module's tolerances; and the accounting identity"""
    got = parse_output(text)
    assert [r[:4] for r in got] == [r[:4] for r in rows]                     # names, ids, level letters, integer reads: exact
    for g, w in zip(got, rows):
        assert close(g[4], w[4], 5e-4) and close(g[5], w[5], 5e-4) and close(g[6], w[6], 5e-7), (g, w)
    keys = ("all", "unclassified", "discarded", "not_distributed", "estimated")
    assert [totals[k] for k in keys[:4]] == [float(x) for x in want_totals[:4]]
    assert close(totals["estimated"], want_totals[4], 0.0)
    rest = totals["unclassified"] + totals["discarded"] + totals["not_distributed"] + totals["estimated"]
    assert abs(totals["all"] - rest) <= REL * totals["all"]
    assert want_totals[0] == sum(want_totals[1:])                            # (exactly, in the model)
