"""An NCBI-sized synthetic taxonomy and plain restatements of what the device tally, the clade sums, the confidence walk and the -R report
compute on it.  numpy and Python only; nothing is shared with the device code or with bns::format_report.

  make_taxonomy(seed)          parent array (TAX_ABSENT for ids that are not keys), ranks, names and the landmarks the tests aim at
  chain_ok / depths(parent)    which ids have a chain of keys up to a root (parent 0), and how many steps it takes
  bins(parent, taxa)           0 unclassified, t for a taxon whose chain reaches a root, n for anything else
  clade_sums(parent, direct)   subtree sums, level by level from the deepest level up (np.add.at), not through Euler intervals
  walker(...)                  the confidence walk of tests/confidence_ref.py, each hit's chain walked once: O(|H| * depth)
  report(direct, parent, ...)  the `-R` report, depth first with an explicit stack (chains of thousands of nodes)"""
import math
from collections import Counter
from fractions import Fraction

import numpy as np

TAX_ABSENT = 0xFFFFFFFF
LETTER = {"superkingdom": "D", "domain": "D", "kingdom": "K", "phylum": "P", "class": "C", "order": "O", "family": "F", "genus": "G",
          "species": "S"}
# the rank of each level of the main tree, NCBI-like; levels past the end are strains and unranked variants
LEVEL_RANKS = ["no rank", "superkingdom", "clade", "kingdom", "subkingdom", "phylum", "subphylum", "superclass", "class", "subclass",
               "infraclass", "superorder", "order", "suborder", "infraorder", "superfamily", "family", "subfamily", "tribe", "subtribe",
               "genus", "subgenus", "species group", "species subgroup", "species", "subspecies", "varietas", "forma", "strain", "isolate",
               "serotype", "serogroup", "biotype", "genotype", "morph", "pathogroup"]
MIXED = ["no rank", "clade", "strain"]
WORDS = ["alpha", "beta", "Gamma", "delta", "Escherichia", "coli", "K-12", "Bacillus", "sp.", "str.", "subsp.", "uncultured",
         "environmental", "samples", "été", "Ωmega", "β-strain", "Müller", "海洋", "café", "x"]


class Taxonomy:
    pass


def make_taxonomy(seed=0, n=3_500_000, n_keys=2_500_000, deep=2100, wide=100_000, n_root2=5000, n_broken=3000, levels=34):
    """an NCBI-like parent array of n ids (id n - 1 a key) with n_keys keys, shuffled over [1, n): a main tree under root 1 of `levels`
    levels below the root, one chain of `deep` nodes below a species, one genus with `wide` children, a second root (parent 0, unranked)
    with its own subtree, a subtree of n_broken nodes hung below an id that is not a key, ids that are not keys at all"""
    rng = np.random.default_rng(seed)
    n_main = n_keys - deep - wide - n_root2 - n_broken
    # level sizes grow geometrically (most nodes sit 25-35 levels down, as in NCBI), the parents of a level skewed towards a few nodes
    w = 1.5 ** np.arange(1, levels + 1)
    sizes = np.maximum(2, np.floor(w / w.sum() * (n_main - 1))).astype(np.int64)
    sizes[-1] += n_main - 1 - sizes.sum()
    lpar = [np.array([-1])]                                   # logical parent per logical node; node 0 is the root (id 1)
    lrank = [np.array([0])]                                   # index into LEVEL_RANKS, or -1 - index into MIXED
    lvl_start = [0]
    start = 1
    for lv, sz in enumerate(sizes):
        prev0, prevn = lvl_start[-1], len(lpar[-1])
        pick = np.floor(prevn * rng.random(sz) ** 2).astype(np.int64)          # skewed: low indices get many children
        lpar.append(prev0 + pick)
        r = np.full(sz, min(lv + 1, len(LEVEL_RANKS) - 1))
        mix = rng.random(sz) < 0.12
        r[mix] = -1 - rng.integers(0, len(MIXED), int(mix.sum()))
        lrank.append(r)
        lvl_start.append(start)
        start += sz
    main_total = start
    species_level = LEVEL_RANKS.index("species")
    genus_level = LEVEL_RANKS.index("genus")
    # the deep chain: below the first species-level node
    chain_top = lvl_start[species_level]
    dp = np.arange(main_total - 1, main_total - 1 + deep)
    dp[0] = chain_top
    lpar.append(dp)
    dr = -1 - (np.arange(deep) % len(MIXED))
    dr[deep // 2] = species_level                             # (one ranked node half way down: the step count starts again there)
    lrank.append(dr)
    deep_ids_l = np.arange(main_total, main_total + deep)
    start = main_total + deep
    # the wide genus: 100 k species
    wide_l = lvl_start[genus_level] + 1
    lpar.append(np.full(wide, wide_l))
    lrank.append(np.full(wide, species_level))
    wide_kids_l = np.arange(start, start + wide)
    start += wide
    # the second root and its subtree (ranks mixed: "-" codes above the first lettered node)
    root2_l = start
    p2 = np.empty(n_root2, np.int64)
    p2[0] = -1
    p2[1:] = root2_l + np.floor(np.arange(1, n_root2) * rng.random(n_root2 - 1)).astype(np.int64)
    lpar.append(p2)
    r2 = rng.integers(0, len(LEVEL_RANKS), n_root2)
    r2[0] = 0
    r2[rng.random(n_root2) < 0.4] = -1
    lrank.append(r2)
    root2_kids_l = np.arange(root2_l, root2_l + n_root2)
    start += n_root2
    # the broken subtree: its top hangs below an id that is not a key
    broken_l = start
    pb = np.empty(n_broken, np.int64)
    pb[0] = -2
    pb[1:] = broken_l + np.floor(np.arange(1, n_broken) * rng.random(n_broken - 1)).astype(np.int64)
    lpar.append(pb)
    lrank.append(rng.integers(0, len(LEVEL_RANKS), n_broken))
    start += n_broken
    assert start == n_keys
    lpar = np.concatenate(lpar)
    lrank = np.concatenate(lrank)
    # ids: root 1; the others shuffled over [2, n), n - 1 among them; one id left over is the broken subtree's missing parent
    pool = rng.choice(np.arange(2, n - 1, dtype=np.int64), size=n_keys - 1, replace=False)
    ids = np.empty(n_keys, np.int64)
    ids[0] = 1
    ids[1:] = rng.permutation(np.concatenate([pool[:-1], [n - 1]]))
    missing_parent = int(pool[-1])
    parent = np.full(n, TAX_ABSENT, np.uint32)
    pid = np.where(lpar >= 0, ids[np.maximum(lpar, 0)], np.where(lpar == -1, 0, missing_parent))
    parent[ids] = pid.astype(np.uint32)
    ranks = [""] * n
    rank_names = np.array(LEVEL_RANKS + MIXED[::-1], dtype=object)         # (-1 - i indexes MIXED from the end of this array)
    rank_of = rank_names[np.where(lrank >= 0, lrank, len(LEVEL_RANKS) + len(MIXED) + lrank)]
    rank_of[rank_of == "subkingdom"] = ""                                  # (a few keys without a rank: nodes.dmp lines without the field)
    for i, r in zip(ids.tolist(), rank_of.tolist()):
        ranks[i] = r
    # names: most keys, with spaces and some UTF-8
    named = ids[rng.random(n_keys) < 0.9]
    wsel = rng.integers(0, len(WORDS), size=(named.size, 2))
    names = {int(i): "%s %s %d" % (WORDS[a], WORDS[b], i) for i, (a, b) in zip(named.tolist(), wsel.tolist())}
    names[1] = "root"
    t = Taxonomy()
    t.n, t.parent, t.ranks, t.names = n, parent, ranks, names
    t.keys = np.sort(ids).astype(np.uint32)
    t.deep = ids[deep_ids_l].astype(np.uint32)                            # top to bottom
    t.deep_top = int(ids[chain_top])
    t.wide = int(ids[wide_l])
    t.wide_kids = ids[wide_kids_l].astype(np.uint32)
    t.root2 = int(ids[root2_l])
    t.root2_nodes = ids[root2_kids_l].astype(np.uint32)
    t.broken = ids[broken_l:broken_l + n_broken].astype(np.uint32)
    t.missing_parent = missing_parent
    is_key = parent != TAX_ABSENT
    t.non_keys = np.nonzero(~is_key)[0][1:].astype(np.uint32)            # (id 0 is no taxon)
    return t


def depths(parent):
    """steps from each id up to its root (parent 0); -1 where the chain leaves the keys (and for ids that are not keys)"""
    parent = np.asarray(parent, dtype=np.int64)
    n = parent.size
    d = np.full(n, -1, np.int64)
    ids = np.nonzero(parent != TAX_ABSENT)[0]
    ids = ids[ids != 0]
    cur = parent[ids]
    for step in range(n + 1):
        if not ids.size:
            return d
        done0 = cur == 0
        d[ids[done0]] = step
        live = ~done0 & (cur < n)
        live[live] = parent[cur[live]] != TAX_ABSENT
        ids, cur = ids[live], parent[cur[live]]
    raise ValueError("the parent array has a cycle")


def chain_ok(parent):
    return depths(parent) >= 0


def bins(parent, taxa, ok=None):
    """per unit: 0 for taxon 0, the taxon when its chain reaches a root, n otherwise"""
    n = len(parent)
    ok = chain_ok(parent) if ok is None else ok
    t = np.asarray(taxa, dtype=np.int64)
    inside = (t < n) & ok[np.minimum(t, n - 1)]
    return np.where(t == 0, 0, np.where(inside, t, n))


def clade_sums(parent, direct, dep=None):
    """clade[v] = direct[v] + the clades of v's children, for every v whose chain reaches a root (0 elsewhere); bins 0 and n as given"""
    parent = np.asarray(parent, dtype=np.int64)
    direct = np.asarray(direct, dtype=np.uint64)
    n = parent.size
    dep = depths(parent) if dep is None else dep
    off = dep < 0
    off[0] = False
    assert not direct[:n][off].any(), "counts at ids whose chain does not reach a root"
    clade = np.zeros(n + 1, np.uint64)
    clade[0], clade[n] = direct[0], direct[n]
    ok = np.nonzero(dep >= 0)[0]
    clade[ok] = direct[ok]
    order = ok[np.argsort(-dep[ok], kind="stable")]
    levels = np.split(order, np.nonzero(np.diff(dep[order]))[0] + 1)
    for lv in levels:
        if dep[lv[0]] == 0:
            break
        np.add.at(clade, parent[lv], clade[lv])
    return clade


# ---- the confidence walk

def up_chain(parent, t):
    """t, parent(t), ... up to the root; None when the chain leaves the keys"""
    n = len(parent)
    out = []
    while t != 0:
        if t >= n or parent[t] == TAX_ABSENT or len(out) > n:
            return None
        out.append(t)
        t = int(parent[t])
    return out


def walker(parent, taxon, missing, hits):
    """theta -> the walked taxon (tests/confidence_ref.py's walker): the clade counts along T's chain from one walk per distinct hit,
    up to the first node of that chain it meets"""
    taxon = int(taxon)
    n = len(parent)
    up = up_chain(parent, taxon) if taxon else None
    q = len(hits) + int(missing)
    counts = []
    if up:
        pos = {a: i for i, a in enumerate(up)}
        first = [0] * (len(up) + 1)
        for h, m in Counter(int(x) for x in hits).items():
            while h != 0 and h < n and h not in pos and parent[h] != TAX_ABSENT:
                h = int(parent[h])
            if h in pos:
                first[pos[h]] += m
        c = 0
        for i in range(len(up)):
            c += first[i]
            counts.append(c)

    def at(theta):
        theta = Fraction(theta)
        if theta == 0 or up is None:
            return taxon
        r = math.ceil(theta * q)
        if r == 0:
            return taxon
        for a, c in zip(up, counts):
            if c >= r:
                return a
        return 0
    at.counts = counts
    at.up = up
    at.q = q
    return at


# ---- the -R report

def _line(out, c, d, total, code, tid, depth, name):
    out.append("%6.2f\t%d\t%d\t%s\t%d\t%s%s\n" % (100.0 * c / total if total else 0.0, c, d, code, tid, "  " * depth, name))


def report(direct, parent, ranks=(), names=None, clade=None):
    """the -R report from direct[n + 1] (bins as above): an unclassified line, each root's clade depth first (children by clade
    descending, ties by taxid ascending; a rank without a letter takes the nearest lettered ancestor's and the steps from it, "-"
    without one; id 1 is "R"), a not-in-taxonomy line"""
    parent = np.asarray(parent, dtype=np.int64)
    n = parent.size
    names = names or {}
    clade = clade_sums(parent, direct) if clade is None else clade
    direct = np.asarray(direct, dtype=np.uint64)
    total = int(direct.sum(dtype=np.uint64))
    out = []
    if direct[0]:
        _line(out, int(direct[0]), int(direct[0]), total, "U", 0, 0, "unclassified")
    live = np.nonzero(clade[:n])[0]
    live = live[live != 0]
    lp = parent[live]
    roots = live[lp == 0]
    kid = live[(lp != 0) & (lp < n) & (lp != live)]
    cl = {v: int(c) for v, c in zip(kid.tolist(), clade[kid].tolist())}
    kids = {}
    for k, p in zip(kid.tolist(), parent[kid].tolist()):
        kids.setdefault(p, []).append(k)
    for grp in kids.values():
        grp.sort(key=lambda k: (-cl[k], k))
    nr = len(ranks)
    for r in roots.tolist():
        stack = [(r, 0, 0, "")]
        while stack:
            v, depth, steps, base = stack.pop()
            own = "R" if v == 1 else LETTER.get(ranks[v] if v < nr else "", "")
            if own:
                base, steps = own, 0
            elif base:
                steps += 1
            code = (base + (str(steps) if steps else "")) if base else "-"
            _line(out, int(clade[v]), int(direct[v]), total, code, v, depth, names.get(v, str(v)))
            for k in reversed(kids.get(v, ())):
                stack.append((k, depth + 1, steps, base))
    if direct[n]:
        _line(out, int(direct[n]), int(direct[n]), total, "-", TAX_ABSENT, 0, "(not in taxonomy)")
    return "".join(out)


def report_from_taxa(taxa, parent, ranks=(), names=None):
    n = len(parent)
    return report(np.bincount(bins(parent, taxa), minlength=n + 1).astype(np.uint64), parent, ranks, names)


# ---- the parent array as files

def write_dmps(tax, nodes_path, names_path):
    """nodes.dmp (the root as "1 | 1", the second root's parent 0) and names.dmp (a synonym next to each scientific name)"""
    with open(nodes_path, "w", encoding="utf-8") as f:
        f.write("".join("%d\t|\t%d\t|\t%s\t|\t\t|\n" % (i, 1 if i == 1 else int(tax.parent[i]), tax.ranks[i]) if tax.ranks[i] else
                        "%d\t|\t%d\t|\n" % (i, int(tax.parent[i])) for i in tax.keys.tolist()))
    with open(names_path, "w", encoding="utf-8") as f:
        f.write("".join("%d\t|\t%s\t|\t\t|\tscientific name\t|\n%d\t|\t%s x\t|\t\t|\tsynonym\t|\n" % (i, nm, i, nm)
                        for i, nm in tax.names.items()))
