"""The inputs of the device db build's edge tests: one seeded world generator, the table of build forms, and the expected
key -> LCA map of a (world, form) from the oracle.  A helper module, not a conftest: tests/test_build_cases.py (CPU tier) proves
with the oracle alone that a world holds what the GPU tests rely on, tests/test_gpu_build_edges.py (GPU tier) runs
bns_build_table_device over it, tools/fuzz_gpu_build.py soaks the same worlds with random forms.

The world.  A taxonomy of 400 nodes whose ids are drawn without order from [2, 5000) (children are often numbered below their
parents, as in NCBI), with a chain 30 deep; 260 sequences whose taxids are drawn from ALL nodes (internal ones included, several
sequences per taxid) and whose lengths come from
    {0, 10, c-1, c, c+1, w-1, w, w+1, 700, 2047, 2048, 2049, 3000, 4100}
for the comb c and the window w of the form: three of each, the rest from the five classes around and above the 2048-base chunk a
wavefront of build_kernel works in.  Of the long sequences (>= 2047 bases) most are slices of one of two 4100-base ancestors --
contigs of related genomes: thousands of keys that 50 to 100 sequences fold their taxid into -- some are slices of one of ten
genomes that a few sequences share (strains: an LCA of few), and the rest random (keys of one sequence).  On top of that: three 300-base repeats in 110 long sequences each (a mobile element: carriers meet at the root), a
fourth inside one deep subtree only, N runs of 1, 5 and 40 bases (some across a multiple of 32 and of 2048), lower-case
stretches, the IUPAC letters R / Y / K, A * 40 and T * 40 in two sequences each (key 0), one sequence of nothing but N.

The forms.  CASES names every build form: what build_kernel<SPACED, PASS> branches on (bns_kernels.hip) -- k, the seed, the
strand rule, the window and its score -- and nothing else."""
import collections

import numpy as np

import synth

SEED = 20240611                                          # the committed world

Case = collections.namedtuple("Case", "name k gaps w score canon")
# w: the window in bases; w == comb: unwindowed.  score: 0 lexicographic, 1 the path overloads' entropy, 2 the string overload's
# real entropy.  canon is what set_encoder is given (a spaced seed is never canonicalised, encoder.h:148-150).

G_HALF = tuple([1] * 15 + [0] * 15)                      # comb 46
G_TRIP = tuple([0, 2, 1] * 10)                           # comb 61
G_LONG = tuple([0] * 29 + [40])                          # comb 71: longer than the 64-base window of the run form
G_TWO = tuple([0] * 14 + [5] + [0] * 15)                 # comb 36, two runs: the run-by-run gather (more than 4 runs: compress network)

CASES = (
    Case("k31-canon", 31, None, 31, 0, True),
    Case("k31-forward", 31, None, 31, 0, False),
    Case("k32-canon", 32, None, 32, 0, True),
    Case("k21-canon", 21, None, 21, 0, True),
    Case("k11-canon", 11, None, 11, 0, True),
    Case("w50-lex-canon", 31, None, 50, 0, True),
    Case("w50-entropy-canon", 31, None, 50, 1, True),
    Case("w50-entropy-forward", 31, None, 50, 1, False),             # windows over the emitted stream, in LDS
    Case("w131-forward", 31, None, 31 + 100, 0, False),              # 101 k-mers a window: the queue image in win_scratch
    Case("w1031-canon", 31, None, 31 + 1000, 0, True),               # 15 rounds per 2048-base chunk
    Case("spaced-half", 31, G_HALF, 46, 0, True),                    # 16 runs: extract_spaced_runs through the compress network
    Case("spaced-triplets", 31, G_TRIP, 61, 0, True),                # 21 runs, the same
    Case("spaced-two-runs", 31, G_TWO, 36, 0, True),                 # 2 runs: extract_spaced_runs, gathered run by run
    Case("spaced-long-comb", 31, G_LONG, 71, 0, True),               # comb > 64: no runs, extract_spaced
    Case("spaced-half-w50-entropy", 31, G_HALF, 50, 1, True),
    Case("w50-real-entropy-canon", 31, None, 50, 2, True),           # the oracle has no lca_map for it: folded from its stream
)
BY_NAME = {c.name: c for c in CASES}
FOLD_TWICE = ("w50-entropy-canon", "w50-entropy-forward")          # supported by the oracle's lca_map AND folded: must agree


def is_spaced(case):
    return case.gaps is not None and any(int(g) for g in case.gaps)


def comb(case):
    return case.k + (sum(int(g) for g in case.gaps) if case.gaps is not None else 0)


def windowed(case):
    return case.w > comb(case)


def span(case):
    """bases a sequence needs before a position window emits"""
    return max(case.w, comb(case))


def emitted_stream(case):
    """for_each_uncanon_unspaced_windowed / the string overload: the windows run over the emitted k-mers (across N gaps), and a
    sequence that never fills one flushes one minimum (encoder.h:304-305)"""
    return windowed(case) and not is_spaced(case) and (not case.canon or case.score == 2)


def encoder_runs(k, gaps):
    """n_runs as bns_set_encoder leaves it: the runs of adjacent sampled bases of a spaced seed whose comb fits the 64-base window
    of extract_spaced_runs, 0 otherwise (then build_kernel gathers base by base, extract_spaced)"""
    if gaps is None or not any(int(g) for g in gaps):
        return 0
    pos = np.concatenate([[0], np.cumsum(np.asarray(gaps, dtype=np.int64) + 1)])
    if int(pos[-1]) + 1 > 64:
        return 0
    return 1 + int((np.diff(pos) != 1).sum())


def clean_stream_len(case, L):
    """values the reference's encoder emits for L bases of plain upper-case A/C/G/T (no N, no homopolymer run)"""
    c = comb(case)
    if not windowed(case):
        return max(0, L - c + 1)
    if emitted_stream(case):
        return 0 if L < c else max(1, L - case.w + 1)
    return max(0, L - case.w + 1)


# ---- the world -------------------------------------------------------------------------------------------------------------
N_NODES, CHAIN, DEEP_AT, N_TOP = 400, 30, 20, 6
LONG = (2047, 2048, 2049, 3000, 4100)
LONG_P = (0.1, 0.1, 0.1, 0.3, 0.4)
N_EXTRA = 218                                            # + 3 of each of the 14 classes = 260 sequences
REPEAT_LEN, REPEAT_IN = 300, 110
ANC_LEN, ANC_FRAC = 4100, 0.8
N_STRAINS, STRAIN_FRAC = 10, 0.85                         # of the long sequences that are no slice of an ancestor


def length_classes(c, w):
    return (0, 10, c - 1, c, c + 1, w - 1, w, w + 1, 700, 2047, 2048, 2049, 3000, 4100)


def make_taxonomy(rng):
    """[(child, parent)] with (1, 1) first, and {id: depth}.  ids[0 .. CHAIN) is a chain below the root, N_TOP more nodes are
    children of the root, 40 hang inside the subtree of the chain's node DEEP_AT, every other node below a random earlier one."""
    ids = [int(x) for x in rng.choice(np.arange(2, 5000), size=N_NODES - 1, replace=False)]
    parent = {1: 1}
    for i in range(CHAIN):
        parent[ids[i]] = ids[i - 1] if i else 1
    for i in range(CHAIN, CHAIN + N_TOP):
        parent[ids[i]] = 1
    deep = [ids[i] for i in range(DEEP_AT, CHAIN)]
    for i in range(CHAIN + N_TOP, CHAIN + N_TOP + 40):
        parent[ids[i]] = deep[int(rng.integers(len(deep)))]
        deep.append(ids[i])
    for i in range(CHAIN + N_TOP + 40, len(ids)):
        parent[ids[i]] = ids[int(rng.integers(i))]
    depth = {1: 0}
    for t in [1] + ids:                                  # (a parent is always placed before its children)
        depth[t] = 0 if t == 1 else depth[parent[t]] + 1
    return [(1, 1)] + [(t, parent[t]) for t in ids], depth, ids[DEEP_AT]


def ancestors_of(parent, t):
    out = [t]
    while t != 1:
        t = parent[t]
        out.append(t)
    return out


_WORLDS = {}


def make_edge_world(oracle, seed=SEED, c=31, w=31):
    """The world for a form of comb c and window w (w == c: unwindowed).  Returns a synth.World: .tax (oracle.Taxonomy), .pairs,
    .parent (the array load_taxonomy takes), .par / .depth (dicts), .seqs (list of bytes), .taxids (list), .cls (the length class of
    every sequence) and the bookkeeping the CPU tier checks: .clean (per class, one sequence of plain upper-case random A/C/G/T),
    .repeat_carriers (four lists of sequence indices), .deep_root, .poly (indices of the A * 40 / T * 40 carriers), .all_n, .masked
    (indices with an N or an IUPAC letter)."""
    key = (seed, c, w)
    if key in _WORLDS:
        return _WORLDS[key]
    rng = np.random.default_rng(seed)
    rng_short = np.random.default_rng([seed, 1])         # (so the long sequences are the same whatever c and w)
    wld = synth.World()
    wld.seed, wld.c, wld.w = seed, c, w
    wld.pairs, wld.depth, wld.deep_root = make_taxonomy(rng)
    wld.par = dict(wld.pairs)
    wld.tax = oracle.Taxonomy(pairs=wld.pairs)
    wld.parent = wld.tax.parent
    nodes = [t for t, _ in wld.pairs[1:]]
    in_deep = {t for t in nodes if wld.deep_root in ancestors_of(wld.par, t)}

    classes = length_classes(c, w)
    cls = [i for i in range(len(classes)) for _ in range(3)]
    cls += [len(classes) - len(LONG) + int(x) for x in rng.choice(len(LONG), size=N_EXTRA, p=LONG_P)]
    n = len(cls)
    taxids = [nodes[int(x)] for x in rng.integers(len(nodes), size=n)]
    anc = [synth.rand_seq(rng, ANC_LEN) for _ in range(2)]
    strains = [synth.rand_seq(rng, ANC_LEN) for _ in range(N_STRAINS)]
    repeats = [synth.rand_seq(rng, REPEAT_LEN) for _ in range(4)]
    clean = {}
    seqs = []
    for i in range(n):
        L = classes[cls[i]]
        if cls[i] not in clean:                          # the first of every class: plain random sequence
            clean[cls[i]] = i
            seqs.append(synth.rand_seq(rng if L >= 2047 else rng_short, L).copy())
        elif L >= 2047 and rng.random() < ANC_FRAC:      # a slice of an ancestor
            a = anc[int(rng.integers(2))]
            st = int(rng.integers(0, ANC_LEN - L + 1))
            seqs.append(a[st:st + L].copy())
        elif L >= 2047 and rng.random() < STRAIN_FRAC:   # a slice of a genome that two or three sequences share
            a = strains[int(rng.integers(N_STRAINS))]
            st = int(rng.integers(0, ANC_LEN - L + 1))
            seqs.append(a[st:st + L].copy())
        else:
            seqs.append(synth.rand_seq(rng if L >= 2047 else rng_short, L).copy())
    is_clean = set(clean.values())
    longs = [i for i in range(n) if len(seqs[i]) >= 2047 and i not in is_clean]

    def plant(i, what, at=None):
        s = seqs[i]
        at = int(rng.integers(0, s.size - len(what) + 1)) if at is None else at
        s[at:at + len(what)] = np.frombuffer(what, dtype=np.uint8) if isinstance(what, bytes) else what
        return at

    # repeats: three across the tree, one inside the deep subtree
    wld.repeat_carriers = []
    for r in range(3):
        who = sorted(int(x) for x in rng.choice(longs, size=REPEAT_IN, replace=False))
        for i in who:
            plant(i, repeats[r])
        wld.repeat_carriers.append(who)
    who = [i for i in longs if taxids[i] in in_deep]
    for i in who:
        plant(i, repeats[3])
    wld.repeat_carriers.append(who)
    # N runs, lower case, IUPAC letters
    for j, i in enumerate(longs):
        s = seqs[i]
        for run, p in ((1, 0.5), (5, 0.3), (40, 0.2)):
            if rng.random() < p:
                plant(i, b"N" * run)
        if j % 9 == 0 and s.size > 2100:                 # across the chunk boundary (and a multiple of 32)
            plant(i, b"N" * 40, at=2048 - 20)
        if j % 9 == 1:
            plant(i, b"N" * 5, at=32 * int(rng.integers(1, s.size // 32)) - 2)
        if j % 9 == 2 and s.size > 2100:
            plant(i, b"N", at=2048 - int(rng.integers(0, 2)))
        if rng.random() < 0.3:
            m = int(rng.integers(50, 400))
            at = int(rng.integers(0, s.size - m))
            s[at:at + m] |= 0x20
        if rng.random() < 0.1:
            for ch in rng.choice(np.frombuffer(b"RYK", dtype=np.uint8), size=int(rng.integers(1, 4))):
                s[int(rng.integers(0, s.size))] = ch
    # short sequences: the second of a class gets an N in the middle, the third is lower case
    seen = collections.Counter()
    for i in range(n):
        seen[cls[i]] += 1
        if len(seqs[i]) < 2047 and len(seqs[i]) > 0:
            if seen[cls[i]] == 2:
                seqs[i][len(seqs[i]) // 2] = ord("N")
            elif seen[cls[i]] == 3:
                seqs[i] |= 0x20
    # one sequence of nothing but N; A * 40 twice and T * 40 twice under four different taxids (planted last: nothing overwrites them)
    wld.all_n = longs[-1]
    seqs[wld.all_n][:] = ord("N")
    wld.poly = []
    for i in longs[:-1]:
        if taxids[i] not in [taxids[q] for q in wld.poly]:
            plant(i, (b"A" if len(wld.poly) < 2 else b"T") * 40)
            wld.poly.append(i)
        if len(wld.poly) == 4:
            break
    wld.seqs = [s.tobytes() for s in seqs]
    wld.taxids = taxids
    wld.cls = [classes[x] for x in cls]
    wld.clean = {classes[x]: i for x, i in clean.items()}
    valid = np.zeros(256, dtype=bool)
    valid[list(b"ACGTacgt")] = True
    wld.masked = [i for i in range(n) if not valid[seqs[i]].all()]
    _WORLDS[key] = wld
    return wld


def world_for(oracle, case, seed=SEED):
    return make_edge_world(oracle, seed, comb(case), case.w)


def unmasked(seq):
    """seq with an A for every base that is not A/C/G/T in either case: what a build that ignored the N mask would encode (an
    invalid base packs as code 0)"""
    a = np.frombuffer(seq, dtype=np.uint8).copy()
    valid = np.zeros(256, dtype=bool)
    valid[list(b"ACGTacgt")] = True
    a[~valid[a]] = ord("A")
    return a.tobytes()


# ---- the expected map --------------------------------------------------------------------------------------------------------
def stream(oracle, case, seq):
    """the oracle's own encode stream of one sequence in the case's form"""
    gaps = list(case.gaps) if case.gaps is not None else None
    if case.score == 2:
        return oracle.encode_windowed_entropy_str(seq, case.k, case.w, case.canon)
    if windowed(case):
        return oracle.encode_windowed(seq, case.k, case.w, case.score, gaps=gaps, canon=case.canon)
    return oracle.encode(seq, case.k, gaps=gaps, canon=case.canon, spaced_intended=True)


def oracle_supports(case):
    """bo_lca_map_add / bo_lca_map_add_windowed take the form (everything but the string overload's score)"""
    return case.score != 2


def folded_map(oracle, tax, case, seqs, taxids):
    """update_lca_map restated over the oracle's stream: first sighting stores the taxid, later ones lca(taxid, stored)"""
    d = {}
    for s, tx in zip(seqs, taxids):
        for key in np.unique(stream(oracle, case, s)).tolist():
            cur = d.get(key)
            d[key] = tx if cur is None or cur == tx else tax.lca(tx, cur)
    return d


def table_pairs(table):
    """(keys ascending, their values) of an oracle.Table"""
    f, k, v = table.arrays()
    i = np.arange(table.n_buckets)
    m = ((f[i >> 4] >> ((i & 15) << 1)) & 3) == 0
    order = np.argsort(k[m], kind="stable")
    return k[m][order], v[m][order]


def oracle_table(oracle, tax, case, seqs, taxids):
    """the oracle's sequential update_lca_map over (seqs, taxids) in the case's form; for the form it does not take, a table filled
    from the folded map"""
    t = oracle.Table()
    gaps = list(case.gaps) if case.gaps is not None else None
    if not oracle_supports(case):
        d = folded_map(oracle, tax, case, seqs, taxids)
        t.insert_many(np.fromiter(d.keys(), dtype=np.uint64, count=len(d)), np.fromiter(d.values(), dtype=np.uint32, count=len(d)))
        return t
    for s, tx in zip(seqs, taxids):
        if windowed(case):
            oracle.lca_map_add_windowed(t, tax, case.k, case.w, case.score, s, tx, gaps=gaps, canon=case.canon)
        else:
            oracle.lca_map_add(t, tax, case.k, s, tx, gaps=gaps, canon=case.canon)
    return t


_EXPECTED = {}


def expected(oracle, world, case):
    """(keys ascending uint64, values uint32, the oracle.Table that holds them), computed once per (world, case) and shared"""
    key = (world.seed, world.c, world.w, case.name)
    if key not in _EXPECTED:
        t = oracle_table(oracle, world.tax, case, world.seqs, world.taxids)
        k, v = table_pairs(t)
        k.setflags(write=False); v.setflags(write=False)
        _EXPECTED[key] = (k, v, t)
    return _EXPECTED[key]


def expected_map(oracle, world, case):
    """key -> value dict of the db the reference builds from the world in the case's form"""
    k, v, _ = expected(oracle, world, case)
    return dict(zip(k.tolist(), v.tolist()))


def buckets_for(n_keys):
    """the smallest power of two (>= 4) with n_keys < 0.77 * n_buckets"""
    nb = 4
    while not n_keys < 0.77 * nb:
        nb <<= 1
    return nb
