"""The confidence threshold (bns_set_confidence, `bonsai classify -t`) restated from its definition in DESIGN.md: plain parent walks and
Fraction arithmetic, nothing shared with the device code.

  Q = |hits| + missing;  R = ceil(theta * Q);  clade(A) = the hits equal to A or below A;  the result is the first of T, parent(T), ...
  whose clade holds >= R hits, 0 when the walk passes a root (parent 0) first.  T stays when theta = 0, T = 0, or T is no node whose
  chain reaches a root."""
import math
from fractions import Fraction


def parent_map(pairs_or_parent):
    """(child, parent) pairs (a root's parent is itself or 0) or a parent array (TAX_ABSENT for ids that are not keys) -> {id: parent}"""
    if isinstance(pairs_or_parent, dict):
        return dict(pairs_or_parent)
    try:
        pairs = [(int(c), int(p)) for c, p in pairs_or_parent]
    except TypeError:
        return {i: int(p) for i, p in enumerate(pairs_or_parent) if i and int(p) != 0xFFFFFFFF}
    return {c: (0 if p == c else p) for c, p in pairs}


def chain(par, t):
    """t, parent(t), ... up to the root whose parent is 0; None when the chain leaves the keys (or loops)"""
    out, seen = [], set()
    while t != 0:
        if t not in par or t in seen:
            return None
        seen.add(t)
        out.append(t)
        t = par[t]
    return out


def required(theta, q):
    return math.ceil(Fraction(theta) * q)


def in_clade(par, a, h):
    """h == a, or a lies on h's parent chain"""
    seen = set()
    while h != 0 and h not in seen:
        if h == a:
            return True
        seen.add(h)
        if h not in par:
            return False
        h = par[h]
    return False


def clade_count(par, a, hits):
    return sum(1 for h in hits if in_clade(par, a, int(h)))


def walker(par, taxon, missing, hits):
    """theta -> the taxon the confidence threshold theta leaves for a unit classified at `taxon` with `missing` and `hits` (the clade
    counts along the chain are taken once)"""
    taxon = int(taxon)
    up = chain(par, taxon) if taxon else None
    q = len(hits) + int(missing)
    counts = [clade_count(par, a, [int(h) for h in hits]) for a in up] if up else []

    def at(theta):
        theta = Fraction(theta)
        if theta == 0 or up is None:
            return taxon
        r = required(theta, q)
        if r == 0:
            return taxon
        for a, c in zip(up, counts):
            if c >= r:
                return a
        return 0
    return at


def walk(par, theta, taxon, missing, hits):
    """the taxon the confidence threshold theta leaves for a unit classified at `taxon` with `missing` and `hits`"""
    return walker(par, taxon, missing, hits)(theta)


def boundaries(par, taxon, missing, hits):
    """the thetas c / Q at which this unit's answer changes (c = the clade counts along its chain): exact boundary cases"""
    up = chain(par, int(taxon))
    q = len(hits) + int(missing)
    if up is None or q == 0:
        return set()
    return {Fraction(clade_count(par, a, hits), q) for a in up}
