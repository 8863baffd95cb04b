"""`bonsai build` streaming its genome files in batches, and `bonsai build -A old.db`: a db extended with new genomes alone.  The db's
map is the oracle's sequential build over all genomes either way, and the summary line of BNS_CLI_TIMING=1 says how it got there."""
import gzip
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bonsai_amd", "bin", "bonsai")
SUMMARY = re.compile(r"^build: (\d+) batches, (\d+) grows, (\d+) seeded keys, (\d+) keys in (\d+) buckets$", re.M)


@pytest.fixture(scope="module")
def genome_files(small_world, tmp_path_factory):
    """the genome files of test_cli_build_then_classify: two contigs each (the first in lines of 70), every second file gzip"""
    d = tmp_path_factory.mktemp("build_add")
    nodes = str(d / "nodes.dmp")
    synth.write_nodes_dmp(nodes)
    names = str(d / "nameidmap.txt")
    paths = []
    with open(names, "w") as nf:
        for i, (leaf, g) in enumerate(small_world.genomes.items()):
            acc = "NC_%06d.1" % i
            nf.write("%s\t%d\n" % (acc, leaf))
            s = g.tobytes()
            half = len(s) // 2
            body = (">%s contig one\n" % acc).encode() + b"\n".join(s[:half][j:j + 70] for j in range(0, half, 70)) + \
                   (b"\n>%s_2 contig two\n" % acc.encode()) + s[half:] + b"\n"
            p = str(d / ("g%d.fna%s" % (i, ".gz" if i % 2 else "")))
            with (gzip.open(p, "wb") if i % 2 else open(p, "wb")) as f:
                f.write(body)
            paths.append(p)
    return {"nodes": nodes, "names": names, "paths": paths}


_EXPECTED = {}


def expected_table(oracle, wld, w, score, canon):
    """the oracle's table over all six genomes, two contigs each (no k-mer spans the break); once per form"""
    key = (w, score, canon)
    if key not in _EXPECTED:
        t = oracle.Table()
        for leaf, g in wld.genomes.items():
            s = g.tobytes()
            for part in (s[:len(s) // 2], s[len(s) // 2:]):
                if w > 31:
                    oracle.lca_map_add_windowed(t, wld.tax, 31, w, score, part, leaf, canon=canon)
                else:
                    oracle.lca_map_add(t, wld.tax, 31, part, leaf, canon=canon)
        f, k, v = t.arrays()
        i = np.arange(t.n_buckets)
        m = ((f[i >> 4] >> ((i & 15) << 1)) & 3) == 0
        _EXPECTED[key] = (t, dict(zip(k[m].tolist(), v[m].tolist())))
    return _EXPECTED[key]


def db_map(d):
    i = np.arange(d["n_buckets"])
    m = ((d["flags"][i >> 4] >> ((i & 15) << 1)) & 3) == 0
    return dict(zip(d["keys"][m].tolist(), d["vals"][m].tolist()))


def build(gf, flags, out, paths, env=None):
    assert os.path.exists(BIN), "bonsai CLI not built (run __graft_entry__.build())"
    pr = subprocess.run([BIN, "build", "-T", gf["nodes"], "-M", gf["names"]] + flags + [out, "unused"] + paths, stderr=subprocess.PIPE,
                        timeout=300, env=dict(os.environ, BNS_CLI_TIMING="1", **(env or {})))
    err = pr.stderr.decode()
    assert pr.returncode == 0, err
    m = SUMMARY.search(err)
    assert m, err
    return dict(zip(("batches", "grows", "seeded", "keys", "buckets"), (int(x) for x in m.groups())))


def check_header(d, w):
    assert (d["k"], d["w"]) == (31, w) and d["gaps"].tolist() == [0] * 30
    assert d["upper_bound"] == int(d["n_buckets"] * 0.77 + 0.5) and d["size"] <= d["upper_bound"]
    assert d["n_buckets"] < 4 or int((d["n_buckets"] // 2) * 0.77 + 0.5) <= d["size"]      # as compact as khash grows it


@pytest.mark.parametrize("flags,w,score", [([], 31, 0), (["-w", "50", "-e"], 50, 1), (["-C", "-w", "50", "-e"], 50, 1)])
def test_cli_build_streamed(oracle, small_world, genome_files, tmp_path, flags, w, score):
    """batches of at most 5000 bases -- one 3000-base contig each --: the table starts at the first contig's size and grows"""
    from bonsai_amd import hostio
    wld, gf = small_world, genome_files
    canon = "-C" not in flags
    exp_t, exp = expected_table(oracle, wld, w, score, canon)
    out = str(tmp_path / "built.db")
    s = build(gf, ["-k", "31"] + flags, out, gf["paths"], env={"BNS_BUILD_BATCH": "5000"})
    print(s)
    assert s["batches"] >= 6 and s["grows"] >= 1 and s["seeded"] == 0
    d = hostio.read_db(out)
    check_header(d, w)
    assert (s["keys"], s["buckets"]) == (d["size"], d["n_buckets"])
    assert db_map(d) == exp
    # classify with the built file
    reads = synth.simulate_reads(np.random.default_rng(5), wld.genomes, 200)
    fq = str(tmp_path / "r.fq")
    with open(fq, "wb") as f:
        for j, r in enumerate(reads):
            f.write(b"@q%d\n%s\n+\n%s\n" % (j, r.tobytes(), b"I" * r.size))
    pr = subprocess.run([BIN, "classify", "-a"] + ([] if canon else ["-C"]) + [out, gf["nodes"], fq], stdout=subprocess.PIPE,
                        stderr=subprocess.PIPE, timeout=300)
    assert pr.returncode == 0, pr.stderr.decode()
    lines = []
    for j, r in enumerate(reads):
        t, mm, a, hits = oracle.classify_seq(exp_t, wld.tax, 31, r.tobytes(), canon=canon, spaced_intended=True)
        lines.append(oracle.kraken_line("q%d" % j, t, r.size, mm, a, hits))
    assert pr.stdout == b"".join(lines)


@pytest.mark.parametrize("flags,w,score", [([], 31, 0), (["-w", "50", "-e"], 50, 1)])
def test_cli_build_add(oracle, small_world, genome_files, tmp_path, flags, w, score):
    """genomes 0-2 into a.db, then -A a.db with genomes 3-5 alone: the db of all six, from a plain file, a gzip one, and in place"""
    from bonsai_amd import hostio
    wld, gf = small_world, genome_files
    _, exp = expected_table(oracle, wld, w, score, True)
    a_db = str(tmp_path / "a.db")
    build(gf, ["-k", "31"] + flags, a_db, gf["paths"][:3])
    n_a = hostio.read_db(a_db)["size"]
    plain = str(tmp_path / "all.db")
    build(gf, ["-k", "31"] + flags, plain, gf["paths"])
    assert db_map(hostio.read_db(plain)) == exp
    # k and w come from the file: -A with none of -k / -w (-e is not recorded: repeated)
    keep = [f for f in flags if f == "-e"]
    out = str(tmp_path / "out.db")
    s = build(gf, ["-A", a_db] + keep, out, gf["paths"][3:])
    d = hostio.read_db(out)
    check_header(d, w)
    assert s["seeded"] == n_a and (s["keys"], s["buckets"]) == (d["size"], d["n_buckets"])
    assert db_map(d) == exp
    # ... and with them given as they were
    s = build(gf, ["-A", a_db, "-k", "31"] + flags, out, gf["paths"][3:])
    assert s["seeded"] == n_a and db_map(hostio.read_db(out)) == exp
    # a gzip db (-z adds the suffix), extended into a gzip db
    build(gf, ["-k", "31", "-z"] + flags, a_db, gf["paths"][:3])
    out_gz = str(tmp_path / "out2.db.gz")
    s = build(gf, ["-A", a_db + ".gz"] + keep, out_gz, gf["paths"][3:])
    d = hostio.read_db(out_gz)
    check_header(d, w)
    assert s["seeded"] == n_a and db_map(d) == exp
    # in place: the output is the -A file itself
    same = str(tmp_path / "same.db")
    shutil.copy(a_db, same)
    s = build(gf, ["-A", same] + keep, same, gf["paths"][3:])
    d = hostio.read_db(same)
    check_header(d, w)
    assert s["seeded"] == n_a and db_map(d) == exp
    assert sorted(os.listdir(str(tmp_path))) == sorted(["a.db", "a.db.gz", "all.db", "out.db", "out2.db.gz", "same.db"])   # no temporary file left
