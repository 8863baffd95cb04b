"""The forms classify_kernel is compiled in, restated from the dispatch RULE (not from the C++), the matrix of cases that runs
every one of them, the read set those cases share, and a host restatement of the minimizer window (bucket_of / round_minhash,
bns_device.hpp) that says where in its window every k-mer of that read set has its minimum.  A helper module, not a conftest:
tests/test_classify_plan.py (CPU tier) holds it against the library's one statement of the rule, choose_form / choose_overflow_form
and the lists of forms in bonsai_amd/csrc/bns_classify_plan.hpp, on every point of image()'s domain;
tests/test_classify_forms_built.py (CPU tier) holds it against the built library, tests/test_gpu_classify_forms.py (GPU tier)
runs it against the oracle.

The rule.  A classify call launches ONE classify_kernel<SPACED, LAYOUT, KT, NM, SPAN, OVC, WIDE, PACKED>:
  * contiguous canonical seeds on the clustered table (layout 2) with k = 31 get k, the mates per unit (NM) and the minimizer
    window (SPAN = k - m) as compile-time constants, in every form: the cooperative overflow lookup (OVC), the 52-bit minimizer
    identity (WIDE), both, or packed input alone (packed input with OVC or WIDE is a generic form);
  * k = 21, 25, 27 and 32 get the same in the usual form only (per-lane overflow lookup, 32-bit identity, ASCII input);
  * everything else runs a generic kernel that reads k from its arguments -- KT = NM = 0, SPAN = 8 (unused), OVC = 0 -- one per
    (SPACED, LAYOUT, PACKED), and on the clustered table one more per PACKED for the wide identity.
Units with more than 128 distinct taxa go on to classify_overflow_kernel<SPACED, LAYOUT, WIDE, PACKED>, WIDE again only on the
clustered table with contiguous seeds.

A new instantiation gets into the matrix by (1) extending expected_form() with the rule that reaches it and (2) adding a case
to cases() whose expected form it is; the CPU-tier test fails until the set of compiled instantiations, the image of the rule
and the forms of the cases are one and the same set."""
import collections
import itertools

import numpy as np

import synth

M32 = 0xFFFFFFFF
CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = _i
    CODE[_c | 0x20] = _i

LAYOUT_KHASH, LAYOUT_BUCKET, LAYOUT_MINBUCKET = 0, 1, 2
DBG_PLACE_FAIL, DBG_OVC_OFF, DBG_OVC_ON = 0x100, 0x2000, 0x8000
LDS_CAP = 128                                            # distinct taxa per unit before the overflow kernel takes over

# ---- the minimizer window ---------------------------------------------------------------------------------------------
# window candidates, widest first: (span, floor).  m = k - span, but never below the floor, and m = k for k <= floor.
WINDOWS = ((15, 16), (11, 19), (8, 19))
SPANS = tuple(s for s, _ in WINDOWS)


def minimizer_len(k, span_asked):
    floor = dict(WINDOWS)[span_asked]
    return k if k <= floor else max(k - span_asked, floor)


def distinct_windows(k):
    """[(span asked, m)] with one entry per distinct m, the widest window first (the span asked for that is listed is the
    first that gives the m: for k = 25 the spans 11 and 8 both give m = 19)"""
    out = []
    for s in SPANS:
        m = minimizer_len(k, s)
        if all(m != m2 for _, m2 in out):
            out.append((s, m))
    return out


def kmer_buckets(seq, k, m, n_mb):
    """Home bucket of every k-mer of seq (None for one with a non-ACGT base): canonical m-mers, 32-bit identity."""
    codes = CODE[np.frombuffer(seq.tobytes(), dtype=np.uint8)]
    n = codes.size - k + 1
    if n <= 0:
        return []
    nm = codes.size - m + 1
    mh = []
    for i in range(nm):
        c = codes[i:i + m]
        if (c == 255).any():
            mh.append(None)
            continue
        fw = 0
        rc = 0
        for j, x in enumerate(c):
            fw = (fw << 2) | int(x)
            rc |= (3 - int(x)) << (2 * j)
        x = min(fw, rc)
        x = (x & M32) ^ (((x >> 32) << 13 | (x >> 32) >> 19) & M32) if m > 16 else x
        mh.append((x * 0x7FEB352D) & M32)
    out = []
    for j in range(n):
        win = mh[j:j + k - m + 1]
        if any(h is None for h in win):
            out.append(None)
            continue
        x = (min(win) * 0x9E3779B1) & M32
        x ^= x >> 15
        r = int("{:032b}".format(x)[::-1], 2)
        out.append((r * n_mb) >> 32)
    return out


INVALID = np.uint64(1) << np.uint64(32)                  # above every 32-bit hash: an m-mer with a non-ACGT base


def mmer_hashes(seq, m):
    """kmer_buckets' m-mer hashes for the whole of seq at once: uint64 array, INVALID where the m-mer holds a non-ACGT base"""
    codes = CODE[np.frombuffer(seq.tobytes(), dtype=np.uint8)]
    nm = codes.size - m + 1
    if nm <= 0:
        return np.zeros(0, dtype=np.uint64)
    bad = np.concatenate([[0], np.cumsum(codes == 255)])
    valid = (bad[m:] - bad[:-m]) == 0
    c = (codes & 3).astype(np.uint64)
    fw = np.zeros(nm, dtype=np.uint64)
    rc = np.zeros(nm, dtype=np.uint64)
    for j in range(m):
        x = c[j:j + nm]
        fw = (fw << np.uint64(2)) | x
        rc |= (np.uint64(3) - x) << np.uint64(2 * j)
    x = np.minimum(fw, rc)
    if m > 16:
        hi = x >> np.uint64(32)
        x = (x & np.uint64(M32)) ^ (((hi << np.uint64(13)) | (hi >> np.uint64(19))) & np.uint64(M32))
    h = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    return np.where(valid, h, INVALID)


def window_minima(seq, k, m):
    """(valid, pos, strict) per k-mer of seq: every base is A/C/G/T; the window position (0 .. k - m) of its smallest m-mer
    hash; no other entry of the window equals it"""
    h = mmer_hashes(seq, m)
    n = len(seq) - k + 1
    if n <= 0:
        return np.zeros(0, bool), np.zeros(0, np.int64), np.zeros(0, bool)
    win = np.lib.stride_tricks.sliding_window_view(h, k - m + 1)[:n]
    valid = (win < INVALID).all(axis=1)
    lo = win.min(axis=1)
    return valid, win.argmin(axis=1), (win == lo[:, None]).sum(axis=1) == 1


def window_coverage(reads, k, m):
    """Over the k-mers of `reads` that lie in one 2048-base chunk (round = k-mer // 64, lane = k-mer % 64): which window
    positions 0 .. span hold some valid k-mer's strict minimum, and which of the carried ring entries 0 .. span - 1 -- the
    previous round's tail, entry lane + position -- hold one in a round >= 1."""
    span = k - m
    at = np.zeros(span + 1, dtype=bool)
    carried = np.zeros(span, dtype=bool)
    for r in reads:
        if r.size > 2048 or r.size < k:
            continue
        valid, pos, strict = window_minima(r, k, m)
        ok = valid & strict
        at[np.unique(pos[ok])] = True
        j = np.arange(pos.size)
        ring = (j % 64) + pos
        sel = ok & (j >= 64) & (ring < span)
        carried[np.unique(ring[sel])] = True
    return at, carried


# ---- the dispatch rule -------------------------------------------------------------------------------------------------
FIXED_K_FULL = (31,)                                     # every form
FIXED_K_USUAL = (21, 25, 27, 32)                         # the usual form only
GENERIC_SPAN = 8                                         # the SPAN argument of a kernel that does not use it


def is_spaced(gaps):
    return gaps is not None and any(int(g) != 0 for g in gaps)


def expected_form(k, canon, gaps, layout, m_of_table, identity_bits, ovf_heavy, packed, paired):
    """(SPACED, LAYOUT, KT, NM, SPAN, OVC, WIDE, PACKED) of the classify_kernel a call must launch.  m_of_table and identity_bits
    are table_geometry()'s (0 off the clustered table); ovf_heavy: the cooperative overflow lookup is in force."""
    spaced = is_spaced(gaps)
    canon = bool(canon) and not spaced                   # a spaced seed is never canonicalised
    clustered = layout == LAYOUT_MINBUCKET and not spaced
    wide = clustered and identity_bits == 52
    ovc, packed = bool(ovf_heavy), bool(packed)
    if clustered and canon and k in FIXED_K_FULL + FIXED_K_USUAL:
        span = k - m_of_table
        if span not in [k - m for _, m in distinct_windows(k)]:
            raise ValueError("k = %d cannot have m = %d" % (k, m_of_table))
        nm = 2 if paired else 1
        if not (ovc or wide or packed):
            return (0, 2, k, nm, span, 0, 0, 0)
        if k in FIXED_K_FULL and not (packed and (ovc or wide)):
            return (0, 2, k, nm, span, int(ovc), int(wide), int(packed))
    return (int(spaced), layout, 0, 0, GENERIC_SPAN, 0, int(wide), int(packed))


def expected_overflow_form(gaps, layout, identity_bits, packed):
    """(SPACED, LAYOUT, WIDE, PACKED) of the classify_overflow_kernel that takes the units with more than LDS_CAP taxa"""
    spaced = is_spaced(gaps)
    wide = layout == LAYOUT_MINBUCKET and not spaced and identity_bits == 52
    return (int(spaced), layout, int(wide), int(bool(packed)))


def ovf_heavy(dbg, overflow_keys, n_keys):
    """the rule for the cooperative overflow lookup: forced on / off by the debug bits, else more than 1 key in 1000 lives in
    the overflow table"""
    if dbg & DBG_OVC_ON:
        return True
    if dbg & DBG_OVC_OFF:
        return False
    return overflow_keys * 1000 > n_keys


def image():
    """(set of classify_kernel forms, set of classify_overflow_kernel forms) over everything the API accepts: k = 1 .. 32,
    either strand rule, contiguous or spaced, the three layouts, every window the loader can build a table with, either
    identity where there is a window to carry it, either overflow lookup, ASCII or packed, single or paired"""
    kern, ovf = set(), set()
    for k, canon, spaced, layout in itertools.product(range(1, 33), (True, False), (False, True), (0, 1, 2)):
        if spaced and k < 2:
            continue                                     # (a 1-mer has no gaps)
        gaps = ([1] + [0] * (k - 2)) if spaced else None
        if layout == LAYOUT_MINBUCKET and not spaced:
            tables = [(m, bits) for _, m in distinct_windows(k) for bits in (32, 52) if bits == 32 or m < k]
        elif layout == LAYOUT_MINBUCKET:
            tables = [(k, 32)]                           # (a spaced seed's own minimizer; the form does not depend on it)
        else:
            tables = [(0, 0)]
        for (m, bits), heavy, packed, paired in itertools.product(tables, (False, True), (False, True), (False, True)):
            kern.add(expected_form(k, canon, gaps, layout, m, bits, heavy, packed, paired))
            ovf.add(expected_overflow_form(gaps, layout, bits, packed))
    return kern, ovf


# ---- the matrix --------------------------------------------------------------------------------------------------------
SPACED_GAPS = tuple([1] * 15 + [0] * 15)                 # k = 31, comb 46

Case = collections.namedtuple("Case", "k canon gaps layout span identity ovc packed paired world")
# span: the window asked for (0: none -- spaced seeds, the other layouts); identity: 32 / 52 asked for (0: not the clustered
# table); ovc: "on" = the cooperative overflow lookup forced, over a crowded table with real keys in its overflow table, None = the
# per-lane lookup forced (left alone the library turns cooperative once 1 key in 1000 lives in the overflow table, which groups of
# sixteen in buckets of ten reach on a roomy table too); world: "std" = synth.make_world, "many" = 700 taxa, units past LDS_CAP


def case_id(c):
    parts = ["k%d" % c.k]
    if c.gaps is not None:
        parts.append("spaced")
    if not c.canon and c.gaps is None:
        parts.append("noncanon")
    parts.append("span%d" % c.span if c.span else "layout%d" % c.layout)
    parts.append("paired" if c.paired else "single")
    if c.layout == LAYOUT_MINBUCKET and c.gaps is None:
        parts.append("wide" if c.identity == 52 else "narrow")
    if c.ovc:
        parts.append("ovc")
    parts.append("packed" if c.packed else "ascii")
    if c.world == "many":
        parts.append("manytaxa")
    return "-".join(parts)


def cases():
    out = []

    def add(k, span, identity=32, ovc=None, packed=False, canon=True, gaps=None, layout=2, world="std"):
        for paired in (False, True):
            out.append(Case(k, canon, gaps, layout, span, identity, ovc, packed, paired, world))

    # compile-time k, the usual form: every distinct window
    for k in FIXED_K_USUAL:
        for span, _ in distinct_windows(k):
            add(k, span)
    # k = 31: every window in every form
    for span in SPANS:
        add(31, span)
        add(31, span, ovc="on")
        add(31, span, identity=52)
        add(31, span, identity=52, ovc="on")
        add(31, span, packed=True)
    # forms that fall back from a compile-time k to a generic kernel (one window each, a different one per form)
    for k in FIXED_K_USUAL:
        w = distinct_windows(k)
        add(k, w[0][0], identity=52)
        add(k, w[1][0], ovc="on")
        add(k, w[-1][0], packed=True)
    add(31, 15, identity=52, packed=True)
    add(31, 11, ovc="on", packed=True)
    # the generic kernel over a partial window (the tail of its 16-entry window masked), and without the strand rule
    for k in (17, 20, 24, 28, 30):
        for span, _ in distinct_windows(k):
            add(k, span)
    add(25, 11, canon=False)
    add(31, 15, canon=False)
    # spaced seeds: every layout, ASCII and packed
    for layout in (0, 1, 2):
        for packed in (False, True):
            add(31, 0, identity=0, packed=packed, gaps=SPACED_GAPS, layout=layout)
    # classify_overflow_kernel in each of its instantiations: units with more than LDS_CAP distinct taxa
    for gaps in (None, SPACED_GAPS):
        for layout in (0, 1, 2):
            for packed in (False, True):
                add(31, 8 if (layout == 2 and gaps is None) else 0, identity=32 if (layout == 2 and gaps is None) else 0,
                    packed=packed, gaps=gaps, layout=layout, world="many")
    for packed in (False, True):
        add(31, 8, identity=52, packed=packed, world="many")
    return out


def case_dbg(c):
    return (DBG_OVC_ON | DBG_PLACE_FAIL) if c.ovc == "on" else DBG_OVC_OFF


def case_table(c):
    """(m, identity bits) table_geometry() must report for the case's table; (0, 0) off the clustered table, (None, 32) for a
    spaced seed on it (its minimizer is the loader's choice and no form depends on it)"""
    if c.layout != LAYOUT_MINBUCKET:
        return 0, 0
    if c.gaps is not None:
        return None, 32
    m = minimizer_len(c.k, c.span)
    return m, (52 if c.identity == 52 and m < c.k else 32)


def case_forms(c):
    """the forms the case is in the matrix for, without a device: (classify_kernel form, classify_overflow_kernel form)"""
    m, bits = case_table(c)
    return (expected_form(c.k, c.canon, c.gaps, c.layout, m if m is not None else c.k, bits, c.ovc == "on", c.packed, c.paired),
            expected_overflow_form(c.gaps, c.layout, bits, c.packed))


# ---- the worlds and the read set ------------------------------------------------------------------------------------------
_WORLDS = {}
MANY_LEAVES, MANY_SEG = 700, 60


def comb(k, gaps):
    return k + (sum(int(g) for g in gaps) if gaps is not None else 0)


def world(oracle, k, canon=True, gaps=None, kind="std"):
    key = (k, canon, gaps, kind)
    if key in _WORLDS:
        return _WORLDS[key]
    g = list(gaps) if gaps is not None else None
    if kind == "std":
        w = synth.make_world(oracle, seed=400 + k + (0 if canon else 50) + (100 if gaps else 0), k=k, genome_len=6000, gaps=g, canon=canon)
    else:
        # MANY_LEAVES leaves under ten inner nodes, one private segment each: a read of all segments holds 700 distinct taxa
        rng = np.random.default_rng(31)
        pairs = [(1, 1)] + [(10 + i, 1) for i in range(10)] + [(1000 + i, 10 + i % 10) for i in range(MANY_LEAVES)]
        w = synth.World()
        w.k, w.gaps, w.canon = k, g, canon
        w.tax = oracle.Taxonomy(pairs=pairs)
        w.parent = w.tax.parent
        w.table = oracle.Table()
        w.segs = [synth.rand_seq(rng, MANY_SEG) for _ in range(MANY_LEAVES)]
        for i, s in enumerate(w.segs):
            oracle.lca_map_add(w.table, w.tax, k, s.tobytes(), 1000 + i, gaps=g, canon=canon)
        w.flags, w.keys, w.vals = w.table.arrays()
        w.n_buckets = w.table.n_buckets
    _WORLDS[key] = w
    return w


NK = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193)
REPS = 4


def read_set(w, span):
    """The reads every case of one (world, window) classifies, singly and two by two.  c below is the comb (k for a contiguous
    seed): a read of n k-mers has n + c - 1 bases.
      * 1, 2, span, span + 1 and the counts around the round boundaries (64 k-mers a round) up to 193 k-mers, REPS times each:
        forward and reverse complement by turns, every third one in lower case, one base in 200 substituted;
      * 0, c - 1 and c bases; 2100 and 4200 bases (the ring restarts per 2048-base chunk), and their reverse complements;
      * an N at base 0, span - 1, span, the last base, and either side of k-mers 63 / 64;
      * homopolymer and dinucleotide reads, alone and inside genome sequence (window entries that tie);
      * random reads (k-mers the table does not hold);
      * thirty plain reads of 100 to 250 bases straight from the genomes: with them most units are classified whatever the seed
        (a seed that is not canonical finds no reverse complement, a spaced one loses 31 k-mers to one substitution)."""
    k, c = w.k, comb(w.k, w.gaps)
    rng = np.random.default_rng(1000 * k + 10 * span + (1 if w.gaps else 0))
    g = np.concatenate(list(w.genomes.values()))
    reads = []

    def cut(n_bases):
        st = int(rng.integers(0, g.size - n_bases))
        return g[st:st + n_bases].copy()

    nks = sorted(set(NK) | {x for x in (span, span + 1) if x >= 1})
    for rep in range(REPS):
        for nk in nks:
            r = synth.mutate(rng, cut(nk + c - 1), 0.005, 0.0)
            if rep % 2:
                r = synth.revcomp(r)
            if rep % 3 == 2:
                r = r | 0x20
            reads.append(r)
    reads += [g[:0].copy(), cut(c - 1), cut(c)]
    for n in (2100, 4200):
        r = cut(n)
        reads += [r, synth.revcomp(r)]
    n_at = {0, max(span - 1, 0), span, 62, 63, 64, 65, 63 + c - 1, 64 + c - 1}
    for pos in sorted(n_at) + [-1]:
        r = cut(130 + c - 1)
        r[pos] = ord("N")
        reads.append(r)
    low = [np.frombuffer(b"A" * 100, dtype=np.uint8), np.frombuffer(b"AC" * 70, dtype=np.uint8), np.frombuffer(b"t" * 90, dtype=np.uint8)]
    reads += [x.copy() for x in low]
    for x in low[:2]:
        r = cut(200)
        reads.append(np.concatenate([r[:90], x[:50], r[90:]]))
    reads += [synth.rand_seq(rng, 150) for _ in range(6)]
    reads += [cut(int(n)) for n in rng.integers(100, 251, size=30)]
    if len(reads) % 2:
        reads.append(cut(97))
    return [np.ascontiguousarray(r, dtype=np.uint8) for r in reads]


def many_taxa_reads(w):
    """Units with more than LDS_CAP distinct taxa (the 700 segments in a row, forwards and backwards; 300; 129: one past the
    cap), units at and below the cap, and a few reads with an N or of random sequence"""
    rng = np.random.default_rng(77)
    segs = w.segs
    every = np.concatenate(segs)
    reads = [every, np.concatenate(segs[:300]), segs[0].copy(), np.concatenate(segs[:5]), every[::-1].copy(), synth.revcomp(every)]
    reads += [np.concatenate(segs[a:a + n]) for a, n in ((0, 63), (3, 64), (5, 65), (7, 100), (11, 127), (13, 128), (17, 129), (400, 200))]
    for a in (20, 50):
        r = np.concatenate(segs[a:a + 140])
        r[int(rng.integers(0, r.size))] = ord("N")
        reads.append(r)
    reads += [synth.rand_seq(rng, 200), synth.rand_seq(rng, 90)]
    assert len(reads) % 2 == 0
    return [np.ascontiguousarray(r, dtype=np.uint8) for r in reads]
