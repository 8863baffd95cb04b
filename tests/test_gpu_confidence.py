"""The confidence threshold on the device (bns_set_confidence: confidence_kernel behind every classify launch) and `bonsai classify -t`:
every unit's taxon against tests/confidence_ref.py applied to the oracle's (taxon, missing, hits) -- both hit sources (the caller's
stream, the context's own buffer), short, long and many-taxa units, every CLI input form, the report and the taxon file."""
import gzip
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import bonsai_amd
import confidence_ref as cr
import synth
from bonsai_amd import _lib
from test_gpu_cli import BIN, files  # noqa: F401  (the module's fixture)
from test_gpu_report import NAMES, RANKS, expected_report, fastq, rep  # noqa: F401  (rep: the module's fixture)

pytestmark = pytest.mark.gpu

THETAS = [Fraction(0), Fraction("0.05"), Fraction("0.1"), Fraction("0.25"), Fraction("0.5"), Fraction("0.75"), Fraction("0.9"), Fraction(1)]


def load_world(c, w):
    c.set_encoder(31, None, canonicalize=True)
    c.load_table(w.n_buckets, w.flags, w.keys, w.vals)
    c.load_taxonomy(w.parent)


def oracle_units(oracle, w, reads, paired):
    if paired:
        return [oracle.classify_seq(w.table, w.tax, 31, reads[2 * i].tobytes(), reads[2 * i + 1].tobytes()) for i in range(len(reads) // 2)]
    return [oracle.classify_seq(w.table, w.tax, 31, r.tobytes()) for r in reads]


def boundary_thetas(par, units, n_max=12, seed=0):
    b = set()
    for t, m, _, h in units:
        b |= cr.boundaries(par, t, m, h)
    b = sorted(x for x in b if 0 < x <= 1)
    rng = np.random.default_rng(seed)
    return [b[i] for i in sorted(rng.choice(len(b), size=min(n_max, len(b)), replace=False))] if b else []


def check_api(c, par, units, reads, paired, thetas, text=False):
    """every theta through classify / classify_packed with and without hits (and classify_text when asked): taxa as the restatement
    says, everything else as the oracle (= as at theta 0); -> the taxa of each theta"""
    bases, offsets = synth.concat(reads)
    words, bw, bm = bonsai_amd.pack_reads(bases, offsets)
    walkers = [cr.walker(par, t, m, h) for t, m, _, h in units]
    out = {}
    try:
        for th in thetas:
            c.set_confidence(th)
            want = np.array([f(th) for f in walkers], dtype=np.uint32)
            got = [c.classify(bases, offsets, paired=paired, want_hits=wh) for wh in (True, False)]
            got += [c.classify_packed(words, bw, bm, offsets, paired=paired, want_hits=wh) for wh in (True, False)]
            for g in got:
                bad = np.nonzero(g["taxon"] != want)[0]
                assert bad.size == 0, (th, paired, [(int(u), units[u][0], int(g["taxon"][u]), int(want[u])) for u in bad[:5]])
                assert g["missing"].tolist() == [u[1] for u in units] and g["ambig"].tolist() == [u[2] for u in units]
                assert g["n_hits"].tolist() == [u[3].size for u in units]
                if "hits" in g:
                    assert all(np.array_equal(a, u[3]) for a, u in zip(g["hits"], units))
            if text and not paired:
                assert np.array_equal(c.classify_text(fastq(reads), final=True)["taxon"], want), th
            out[th] = want
    finally:
        c.set_confidence(0)
    return out


@pytest.mark.parametrize("paired", [False, True])
def test_confidence_api_parity(gpu_ctx, oracle, small_world, paired):
    w, c = small_world, gpu_ctx
    load_world(c, w)
    par = cr.parent_map(w.parent)
    rng = np.random.default_rng(23 + paired)
    reads = synth.simulate_reads(rng, w.genomes, 600, var_len=True, sub_rate=0.02, n_rate=0.01, random_frac=0.15)
    units = oracle_units(oracle, w, reads, paired)
    # (terms beyond 2^31 take the device's 128-bit ceil: just below and just above one half)
    thetas = THETAS + boundary_thetas(par, units, seed=paired) + [Fraction(2 ** 61 - 1, 2 ** 62), Fraction(2 ** 62 + 1, 2 ** 63)]
    got = check_api(c, par, units, reads, paired, thetas, text=True)
    base = got[Fraction(0)]
    assert base.tolist() == [u[0] for u in units]
    changed = np.count_nonzero(got[Fraction("0.5")] != base)
    assert changed >= len(units) // 10, changed                       # (not vacuous: a good share walks up or drops out)
    assert np.count_nonzero((got[Fraction("0.5")] != base) & (got[Fraction("0.5")] != 0)) > 0      # some stop on the way up
    assert np.count_nonzero(got[Fraction(1)] == 0) > np.count_nonzero(base == 0)


def test_confidence_long_units(gpu_ctx, oracle):
    """10-kb reads and pairs: thousands of hits per unit, most of them past what the kernel keeps in registers"""
    w = synth.make_world(oracle, seed=17, k=31, genome_len=24000)
    c = gpu_ctx
    load_world(c, w)
    par = cr.parent_map(w.parent)
    rng = np.random.default_rng(29)
    reads = synth.simulate_reads(rng, w.genomes, 24, length=10000, sub_rate=0.004, n_rate=0.002, random_frac=0.0)
    for paired in (False, True):
        units = oracle_units(oracle, w, reads, paired)
        assert min(u[3].size for u in units) > 1000
        check_api(c, par, units, reads, paired, THETAS + boundary_thetas(par, units, seed=3 + paired))


def test_confidence_many_taxa(gpu_ctx, oracle):
    """test_gpu_parity's many-taxa world: units of 63..700 distinct taxa (register, LDS and overflow-kernel counters); the walk climbs
    leaf -> 10 + i -> 1 -> 0"""
    rng = np.random.default_rng(31)
    n_leaves = 700
    pairs = [(1, 1)] + [(10 + i, 1) for i in range(10)] + [(1000 + i, 10 + i % 10) for i in range(n_leaves)]
    tax = oracle.Taxonomy(pairs=pairs)
    table = oracle.Table()
    segs = []
    for i in range(n_leaves):
        s = synth.rand_seq(rng, 40)
        segs.append(s)
        oracle.lca_map_add(table, tax, 31, s.tobytes(), 1000 + i)
    w = synth.World()
    w.k, w.gaps, w.canon, w.tax, w.table = 31, None, True, tax, table
    w.flags, w.keys, w.vals = table.arrays()
    w.n_buckets, w.parent = table.n_buckets, tax.parent
    c = gpu_ctx
    load_world(c, w)
    par = cr.parent_map(w.parent)
    long_read = np.concatenate(segs)
    reads = [long_read, np.concatenate(segs[:300]), segs[0], np.concatenate(segs[:5]), long_read[::-1].copy()]
    reads += [np.concatenate(segs[a:a + n]) for a, n in ((0, 63), (3, 64), (5, 65), (7, 100), (11, 127), (13, 128), (17, 129))]
    # mostly one group (10 + 3) with a few others: the walk stops at the group, at the root, or drops out
    for n_other in (0, 2, 20, 200):
        reads.append(np.concatenate([segs[j] for j in range(3, n_leaves, 10)][:40] + segs[:n_other]))
    reads.append(np.concatenate([segs[3]] * 3 + [segs[13]] + [segs[0]]))
    units = oracle_units(oracle, w, reads, False)
    got = check_api(c, par, units, reads, False, THETAS + boundary_thetas(par, units, n_max=40))
    seen = set().union(*(set(v.tolist()) for v in got.values()))
    assert {0, 1, 13} <= seen and any(t >= 1000 for t in seen)


def test_confidence_off_means_off(gpu_ctx, oracle, small_world):
    w, c = small_world, gpu_ctx
    load_world(c, w)
    rng = np.random.default_rng(37)
    reads = synth.simulate_reads(rng, w.genomes, 300, var_len=True, sub_rate=0.02, n_rate=0.01)
    bases, offsets = synth.concat(reads)
    fresh = bonsai_amd.Context(0)
    try:
        with pytest.raises(bonsai_amd.BonsaiAmdError):
            fresh.set_confidence("0.5")                                  # no taxonomy yet
        fresh.set_confidence(0)                                          # (off needs none)
        load_world(fresh, w)
        L = _lib.load()
        for num, den in ((2, 1), (1, 0), (0, 0), (2 ** 64 - 1, 2 ** 64 - 2)):
            assert L.bns_set_confidence(fresh.h, num, den) == -1, (num, den)     # BNS_ERR_ARG
        with pytest.raises(ValueError):
            fresh.set_confidence(1.5)
        assert L.bns_set_confidence(fresh.h, 2 ** 64 - 1, 2 ** 64 - 1) == 0 and L.bns_set_confidence(fresh.h, 0, 5) == 0
        c.set_confidence(Fraction(1, 2))
        c.load_taxonomy(w.parent)                                        # (the setting survives a reload)
        on = c.classify(bases, offsets, want_hits=True)
        c.set_confidence(0)
        for wh in (True, False):
            a, b = c.classify(bases, offsets, want_hits=wh), fresh.classify(bases, offsets, want_hits=wh)
            for k in ("taxon", "missing", "ambig", "n_hits"):
                assert np.array_equal(a[k], b[k]), k
            if wh:
                assert all(np.array_equal(x, y) for x, y in zip(a["hits"], b["hits"]))
        assert np.count_nonzero(on["taxon"] != a["taxon"]) > 0
        # the largest terms (reduced on the way in): theta = 1 exactly
        assert L.bns_set_confidence(fresh.h, 2 ** 64 - 1, 2 ** 64 - 1) == 0
        exact = fresh.classify(bases, offsets)["taxon"]
        fresh.set_confidence(1)
        assert np.array_equal(exact, fresh.classify(bases, offsets)["taxon"])
    finally:
        c.set_confidence(0)
        fresh.close()


# ---- the CLI


@pytest.fixture(scope="module")
def conf(files, oracle):
    w, reads = files["w"], files["reads"]
    single = [oracle.classify_seq(w.table, w.tax, 31, r.tobytes()) for r in reads[:300]]
    pair = [oracle.classify_seq(w.table, w.tax, 31, reads[i].tobytes(), reads[300 + i].tobytes()) for i in range(300)]
    return {"par": cr.parent_map(w.parent), "single": single, "pair": pair}


def cli(args, env=None, stdin=None):
    p = subprocess.run([BIN, "classify"] + args, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300,
                       env=dict(os.environ, **(env or {})))
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout


def lines(oracle, conf, th, units, names, lens, emit_all=True):
    out = []
    for nm, l, (t, m, a, h) in zip(names, lens, units):
        wt = cr.walk(conf["par"], th, t, m, h)
        if wt or emit_all:
            out.append(oracle.kraken_line(nm, wt, l, m, a, h))
    return b"".join(out)


@pytest.mark.parametrize("th", ["0.1", "0.5", "0.9", "1"])
def test_cli_confidence_lines(oracle, files, conf, tmp_path, th):
    reads, db, nodes, r1 = files["reads"], files["db"], files["nodes"], files["r1"]
    T = Fraction(th)
    names = ["read%d" % i for i in range(300)]
    lens = [r.size for r in reads[:300]]
    want = lines(oracle, conf, T, conf["single"], names, lens)
    assert cli(["-t", th, "-a", db, nodes, r1]) == want
    assert cli(["-t", th, db, nodes, r1]) == lines(oracle, conf, T, conf["single"], names, lens, emit_all=False)
    text = open(r1, "rb").read()
    forms = {}
    bg = str(tmp_path / "r1.bgzf.gz"); synth.write_bgzf(bg, text, member_sizes=[5000, 700]); forms["bgzf"] = bg
    gz = str(tmp_path / "r1.gz")
    with gzip.open(gz, "wb") as f:
        f.write(text)
    forms["gzip"] = gz
    pk = str(tmp_path / "r1.bnsp")
    p = subprocess.run([BIN, "pack", "-o", pk, "-c", "20000", r1], stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    forms["bnsp"] = pk
    for tag, path in forms.items():
        assert cli(["-t", th, "-a", db, nodes, path]) == want, tag
    assert cli(["-t", th, "-a", "-c", "20000", db, nodes, r1], env={"BNS_TEXT_GPU": "0"}) == want
    assert cli(["-t", th, "-a", "-g", "0,0", "-c", "20000", db, nodes, r1]) == want
    assert cli(["-t", th, "-a", db, nodes, "/dev/stdin"], stdin=text) == want
    # FASTA, a pair
    assert cli(["-t", th, "-a", db, nodes, files["fa"]]) == lines(oracle, conf, T, conf["single"][:50], ["fa%d" % i for i in range(50)], lens[:50])
    assert cli(["-t", th, "-a", db, nodes, r1, files["r2"]]) == lines(oracle, conf, T, conf["pair"], names, lens)


def test_cli_confidence_taxa_report_fastq(oracle, files, conf, rep, tmp_path):  # noqa: F811
    db, r1 = files["db"], files["r1"]
    th = Fraction("0.5")
    walked = [cr.walk(conf["par"], th, t, m, h) for t, m, _, h in conf["single"]]
    assert sum(a != u[0] for a, u in zip(walked, conf["single"])) > 10
    for mode in (["-K"], ["-a"], ["-f", "-a"]):
        tb, rp = str(tmp_path / "t.bin"), str(tmp_path / "t.report")
        cli(["-t", "0.5", "-b", tb, "-R", rp, "-n", rep["names"]] + mode + [db, rep["nodes"], r1])
        assert np.fromfile(tb, dtype="<u4").tolist() == walked, mode
        assert open(rp).read() == expected_report(walked, ranks=RANKS, names=NAMES), mode
    # pairs, several contexts, the host parser: taxon file and report
    walked_pair = [cr.walk(conf["par"], th, t, m, h) for t, m, _, h in conf["pair"]]
    for extra, env in ((["-g", "0,0", "-c", "20000"], {}), (["-c", "20000"], {"BNS_TEXT_GPU": "0"})):
        tb, rp = str(tmp_path / "p.bin"), str(tmp_path / "p.report")
        cli(["-t", "0.5", "-K", "-b", tb, "-R", rp, "-n", rep["names"]] + extra + [db, rep["nodes"], r1, files["r2"]], env=env)
        assert np.fromfile(tb, dtype="<u4").tolist() == walked_pair, extra
        assert open(rp).read() == expected_report(walked_pair, ranks=RANKS, names=NAMES), extra
    # -f: the FASTQ records of a plain run, with the walked taxon (and C / U) in each header
    plain = cli(["-f", "-a", "-K", db, files["nodes"], r1]).split(b"\n")
    got = cli(["-t", "0.5", "-f", "-a", "-K", db, files["nodes"], r1]).split(b"\n")
    assert len(got) == len(plain) == 4 * 300 + 1
    for i in range(300):
        assert got[4 * i + 1:4 * i + 4] == plain[4 * i + 1:4 * i + 4]
        head, fields = got[4 * i].split(b" ", 1)[0], got[4 * i].split(b"\t")
        assert head == plain[4 * i].split(b" ", 1)[0]
        assert fields[0].endswith(b" " + (b"C" if walked[i] else b"U")) and int(fields[1]) == walked[i], i
        assert fields[2:] == plain[4 * i].split(b"\t")[2:]
    # -t 0 is no -t at all
    for mode in (["-a"], ["-K"], ["-f", "-a"]):
        tb0, tb1 = str(tmp_path / "z0.bin"), str(tmp_path / "z1.bin")
        assert cli(mode + ["-b", tb0, db, files["nodes"], r1]) == cli(mode + ["-t", "0", "-b", tb1, db, files["nodes"], r1])
        assert open(tb0, "rb").read() == open(tb1, "rb").read()
    assert cli(["-a", db, files["nodes"], r1]) == cli(["-a", "-t", "0.000", db, files["nodes"], r1])


@pytest.mark.parametrize("bad", ["1.5", "-0.1", "abc", "0.1234567891", "", ".", "0.5x", "2"])
def test_cli_confidence_errors(files, bad):
    p = subprocess.run([BIN, "classify", "-t", bad, files["db"], files["nodes"], files["r1"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=120)
    assert p.returncode != 0 and p.stdout == b"", bad
    assert b"-t" in p.stderr or b"Usage" in p.stderr
