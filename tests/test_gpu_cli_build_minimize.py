"""`bonsai build -D`: a db of taxonomic-depth minimizers.  The files are streamed twice -- every k-mer scored, then every window's
deepest k-mer kept --; the db's map is the model's (tests/minimize_model.py), its header says w, and `bonsai classify` runs it as
any other db."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import minimize_model as mm
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bonsai_amd", "bin", "bonsai")
MINIMIZE = re.compile(r"^minimize: (\d+) batches, (\d+) grows, (\d+) scored keys, (\d+) lookups, (\d+) keys in (\d+) buckets$", re.M)


@pytest.fixture(scope="module")
def genome_files(small_world, tmp_path_factory):
    """the genome files of test_gpu_cli_build_add: two contigs each (the first in lines of 70), every second file gzip"""
    d = tmp_path_factory.mktemp("build_minimize")
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
    return {"nodes": nodes, "names": names, "paths": paths, "dir": str(d)}


_EXPECTED = {}


def expected(oracle, wld, w, canon):
    """the model's M over all six genomes, two contigs each: (dict, oracle.Table of it, number of scored keys); once per form"""
    key = (w, canon)
    if key not in _EXPECTED:
        seqs, taxids = [], []
        for leaf, g in wld.genomes.items():
            s = g.tobytes()
            seqs += [s[:len(s) // 2], s[len(s) // 2:]]
            taxids += [leaf, leaf]
        F = mm.full_map(oracle, wld.tax, seqs, taxids, 31, canon=canon)
        M = mm.select(F, mm.depths(wld.parent), seqs, 31, w, canon=canon)
        t = oracle.Table()
        ks, vs = mm.sorted_pairs(M)
        t.insert_many(ks, vs)
        _EXPECTED[key] = (M, t, len(F))
    return _EXPECTED[key]


def db_map(d):
    i = np.arange(d["n_buckets"])
    m = ((d["flags"][i >> 4] >> ((i & 15) << 1)) & 3) == 0
    return dict(zip(d["keys"][m].tolist(), d["vals"][m].tolist()))


def run_build(gf, flags, out, paths, env=None):
    assert os.path.exists(BIN), "bonsai CLI not built (run __graft_entry__.build())"
    return subprocess.run([BIN, "build", "-T", gf["nodes"], "-M", gf["names"]] + flags + [out, "unused"] + paths, stderr=subprocess.PIPE,
                          timeout=300, env=dict(os.environ, BNS_CLI_TIMING="1", **(env or {})))


@pytest.mark.parametrize("flags,env", [([], {}), ([], {"BNS_BUILD_BATCH": "5000"}), (["-C"], {"BNS_BUILD_BATCH": "5000"})])
def test_cli_build_taxdepth(oracle, small_world, genome_files, tmp_path, flags, env):
    from bonsai_amd import hostio
    wld, gf = small_world, genome_files
    canon = "-C" not in flags
    exp, exp_t, n_scored = expected(oracle, wld, 50, canon)
    out = str(tmp_path / "td.db")
    pr = run_build(gf, ["-k", "31", "-D", "-w", "50"] + flags, out, gf["paths"], env=env)
    err = pr.stderr.decode()
    assert pr.returncode == 0, err
    m = MINIMIZE.search(err)
    assert m, err
    s = dict(zip(("batches", "grows", "scored", "lookups", "keys", "buckets"), (int(x) for x in m.groups())))
    print(s)
    d = hostio.read_db(out)
    assert (d["k"], d["w"]) == (31, 50) and d["gaps"].tolist() == [0] * 30
    assert d["upper_bound"] == int(d["n_buckets"] * 0.77 + 0.5) and d["size"] <= d["upper_bound"]
    assert int((d["n_buckets"] // 2) * 0.77 + 0.5) < d["size"]                           # khash's own size
    assert db_map(d) == exp
    assert (s["scored"], s["keys"], s["buckets"]) == (n_scored, len(exp), d["n_buckets"])
    if env:
        assert s["batches"] >= 6 and s["grows"] >= 1                                      # one 3000-base contig a batch: M grows
    else:
        assert s["batches"] == 1
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
        t, miss, a, hits = oracle.classify_seq(exp_t, wld.tax, 31, r.tobytes(), canon=canon, spaced_intended=True)
        lines.append(oracle.kraken_line("q%d" % j, t, r.size, miss, a, hits))
    assert pr.stdout == b"".join(lines)


def test_cli_taxdepth_alone_is_every_kmer(oracle, small_world, genome_files, tmp_path):
    """-D without -w: w = the comb, a plain every-k-mer db"""
    from bonsai_amd import hostio
    exp, _, n_scored = expected(oracle, small_world, 31, True)
    out = str(tmp_path / "all.db")
    pr = run_build(genome_files, ["-k", "31", "-D"], out, genome_files["paths"])
    assert pr.returncode == 0, pr.stderr.decode()
    d = hostio.read_db(out)
    assert d["w"] == 31 and len(exp) == n_scored and db_map(d) == exp


def test_cli_taxdepth_refusals(small_world, genome_files, tmp_path):
    gf = genome_files
    out = str(tmp_path / "no.db")
    pr = run_build(gf, ["-k", "31", "-D", "-e", "-w", "50"], out, gf["paths"])
    assert pr.returncode != 0 and "-D and -e exclude each other" in pr.stderr.decode()
    old = str(tmp_path / "old.db")
    assert run_build(gf, ["-k", "31", "-w", "50"], old, gf["paths"][:2]).returncode == 0
    pr = run_build(gf, ["-D", "-A", old], out, gf["paths"][2:])
    assert pr.returncode != 0 and "-D and -A exclude each other" in pr.stderr.decode() and "does not hold" in pr.stderr.decode()
    fifo = str(tmp_path / "g.fifo")
    os.mkfifo(fifo)
    pr = run_build(gf, ["-k", "31", "-D", "-w", "50"], out, gf["paths"][:1] + [fifo])       # (refused before it is opened: no writer needed)
    assert pr.returncode != 0 and "is not a regular file" in pr.stderr.decode()
    assert not os.path.exists(out)


def test_cli_t_still_builds_the_entropy_db(oracle, small_world, genome_files, tmp_path):
    from bonsai_amd import hostio
    t = oracle.Table()
    for leaf, g in small_world.genomes.items():
        s = g.tobytes()
        for part in (s[:len(s) // 2], s[len(s) // 2:]):
            oracle.lca_map_add_windowed(t, small_world.tax, 31, 50, 1, part, leaf)
    f, k, v = t.arrays()
    i = np.arange(t.n_buckets)
    m = ((f[i >> 4] >> ((i & 15) << 1)) & 3) == 0
    out = str(tmp_path / "t.db")
    pr = run_build(genome_files, ["-k", "31", "-t", "-w", "50"], out, genome_files["paths"])
    assert pr.returncode == 0 and "[W] -t" in pr.stderr.decode() and "entropy-minimized" in pr.stderr.decode()
    assert not MINIMIZE.search(pr.stderr.decode())
    assert db_map(hostio.read_db(out)) == dict(zip(k[m].tolist(), v[m].tolist()))
