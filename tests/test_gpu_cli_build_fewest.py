"""`bonsai build -G`: a db of fewest-genome minimizers.  The files are streamed three times -- every k-mer scored, the genome files
that hold it counted, every window's rarest k-mer kept --; a genome is a FILE, so both contigs of one share an id.  The db's map is
the model's (tests/fewest_model.py), its header says w, and `bonsai classify` runs it as any other db."""
import os
import re
import subprocess

import numpy as np
import pytest

import fewest_model as fm
import minimize_model as mm
import synth
from test_gpu_cli_build_minimize import BIN, MINIMIZE, db_map, genome_files, run_build  # noqa: F401  (genome_files: the -D test's files)

pytestmark = pytest.mark.gpu
COUNT = re.compile(r"^count: (\d+) batches, (\d+) launches, (\d+) genomes, (\d+) lookups, largest count (\d+)$", re.M)

_EXPECTED = {}


def expected(oracle, wld, w, canon):
    """the model's M over the six genome files, two contigs each under one genome id: (dict, oracle.Table of it, F, n)"""
    key = (w, canon)
    if key not in _EXPECTED:
        seqs, taxids, ids = [], [], []
        for g, (leaf, a) in enumerate(wld.genomes.items()):
            s = a.tobytes()
            seqs += [s[:len(s) // 2], s[len(s) // 2:]]
            taxids += [leaf, leaf]
            ids += [g, g]
        F = mm.full_map(oracle, wld.tax, seqs, taxids, 31, canon=canon)
        n = fm.genome_counts(seqs, ids, 31, canon=canon)
        M = fm.select_fewest(F, n, seqs, 31, w, canon=canon)
        t = oracle.Table()
        ks, vs = mm.sorted_pairs(M)
        t.insert_many(ks, vs)
        _EXPECTED[key] = (M, t, F, n)
    return _EXPECTED[key]


@pytest.mark.parametrize("flags,env", [([], {}), ([], {"BNS_BUILD_BATCH": "5000"}), (["-C"], {"BNS_BUILD_BATCH": "5000"})])
def test_cli_build_fewest(oracle, small_world, genome_files, tmp_path, flags, env):
    from bonsai_amd import hostio
    wld, gf = small_world, genome_files
    canon = "-C" not in flags
    exp, exp_t, F, n = expected(oracle, wld, 50, canon)
    depth_map = mm.select(F, mm.depths(wld.parent), [s for g in wld.genomes.values() for s in (g.tobytes()[:g.size // 2], g.tobytes()[g.size // 2:])],
                          31, 50, canon=canon)
    assert set(depth_map) != set(exp)                    # (the -G db is not the -D db of these files)
    out = str(tmp_path / "fg.db")
    pr = run_build(gf, ["-k", "31", "-G", "-w", "50"] + flags, out, gf["paths"], env=env)
    err = pr.stderr.decode()
    assert pr.returncode == 0, err
    m, cm = MINIMIZE.search(err), COUNT.search(err)
    assert m and cm and cm.start() < m.start() and "[timing] count: add" in err, err
    s = dict(zip(("batches", "grows", "scored", "lookups", "keys", "buckets"), (int(x) for x in m.groups())))
    c = dict(zip(("batches", "launches", "genomes", "lookups", "largest"), (int(x) for x in cm.groups())))
    print(c, s)
    d = hostio.read_db(out)
    assert (d["k"], d["w"]) == (31, 50) and d["gaps"].tolist() == [0] * 30
    assert d["upper_bound"] == int(d["n_buckets"] * 0.77 + 0.5) and d["size"] <= d["upper_bound"]
    assert db_map(d) == exp
    assert (s["scored"], s["keys"], s["buckets"]) == (len(F), len(exp), d["n_buckets"])
    assert c["genomes"] == 6 and c["largest"] == max(n.values())
    if env:
        assert c["batches"] >= 6 and c["launches"] == c["batches"]       # one 3000-base contig a batch: every genome spans two
    else:
        assert c["batches"] == 1 and c["launches"] == 6
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


def test_cli_fewest_alone_is_every_kmer(oracle, small_world, genome_files, tmp_path):
    """-G without -w: w = the comb, a plain every-k-mer db"""
    from bonsai_amd import hostio
    exp, _, F, _ = expected(oracle, small_world, 31, True)
    out = str(tmp_path / "all.db")
    pr = run_build(genome_files, ["-k", "31", "-G"], out, genome_files["paths"])
    assert pr.returncode == 0, pr.stderr.decode()
    d = hostio.read_db(out)
    assert d["w"] == 31 and exp == F and db_map(d) == F


def test_cli_fewest_refusals(small_world, genome_files, tmp_path):
    gf = genome_files
    out = str(tmp_path / "no.db")
    pr = run_build(gf, ["-k", "31", "-G", "-e", "-w", "50"], out, gf["paths"])
    assert pr.returncode != 0 and "-G and -e exclude each other" in pr.stderr.decode()
    pr = run_build(gf, ["-k", "31", "-G", "-D", "-w", "50"], out, gf["paths"])
    assert pr.returncode != 0 and "-G and -D exclude each other" in pr.stderr.decode()
    old = str(tmp_path / "old.db")
    assert run_build(gf, ["-k", "31", "-w", "50"], old, gf["paths"][:2]).returncode == 0
    pr = run_build(gf, ["-G", "-A", old], out, gf["paths"][2:])
    assert pr.returncode != 0 and "-G and -A exclude each other" in pr.stderr.decode() and "holds neither" in pr.stderr.decode()
    fifo = str(tmp_path / "g.fifo")
    os.mkfifo(fifo)
    pr = run_build(gf, ["-k", "31", "-G", "-w", "50"], out, gf["paths"][:1] + [fifo])       # (refused before it is opened: no writer needed)
    assert pr.returncode != 0 and "three times" in pr.stderr.decode() and "is not a regular file" in pr.stderr.decode()
    assert not os.path.exists(out)
