"""`bonsai distrib`: the genome files through one window session on the device, and the file of per-genome window calls it writes,
against the text tests/windows_model.py writes from the oracle's calls of the explicitly cut windows."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import synth
import windows_model as WM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bonsai_amd", "bin", "bonsai")
L = 150


@pytest.fixture(scope="module")
def world_files(oracle, small_world, tmp_path_factory):
    """six FASTA files -- the first two with two records each (the first in lines of 70), the fourth gzip --, the name map, nodes.dmp,
    the db, and the text the model expects"""
    w = small_world
    d = tmp_path_factory.mktemp("distrib")
    nodes, names, db = str(d / "nodes.dmp"), str(d / "nameidmap.txt"), str(d / "w.db")
    synth.write_nodes_dmp(nodes)
    assert oracle.db_write(db, 31, 31, None, w.table) >= 0
    paths, records = [], []
    with open(names, "w") as nf:
        for i, (leaf, g) in enumerate(w.genomes.items()):
            g = synth.mutate(np.random.default_rng(100 + i), g, 0.01, 0.002)
            if i == 4:                                                          # a stretch the db has never seen: windows called 0
                g = np.concatenate([g, synth.rand_seq(np.random.default_rng(9), 400)])
            acc = "NC_%06d.1" % i
            nf.write("%s\t%d\n" % (acc, leaf))
            s = g.tobytes()
            if i < 2:
                half = 2500 + i
                body = (">%s contig one\n" % acc).encode() + b"\n".join(s[:half][j:j + 70] for j in range(0, half, 70)) + \
                       (b"\n>%s_2 contig two\n" % acc.encode()) + s[half:] + b"\n"
                records += [(leaf, g[:half]), (leaf, g[half:])]
            else:
                body = (">%s whole\n" % acc).encode() + s + b"\n"
                records.append((leaf, g))
            p = str(d / ("g%d.fna%s" % (i, ".gz" if i == 3 else "")))
            with (gzip.open(p, "wb") if i == 3 else open(p, "wb")) as f:
                f.write(body)
            paths.append(p)
    who, what = [], []
    for leaf, seq in records:
        c = WM.calls(oracle, w.table, w.tax, 31, seq, L)
        who.append(np.full(c.size, leaf, dtype=np.uint64)); what.append(c)
    pairs = WM.pairs_of(np.concatenate(who), np.concatenate(what))
    assert pairs[0].size > 4 and (pairs[1] == 0).any()                          # more pairs than `-P 4` holds; windows called 0
    return {"nodes": nodes, "names": names, "db": db, "paths": paths, "text": WM.distrib_text(*pairs)}


def distrib(wf, flags, out):
    assert os.path.exists(BIN), "bonsai CLI not built (run __graft_entry__.build())"
    return subprocess.run([BIN, "distrib", "-M", wf["names"], "-o", out] + flags + [wf["db"], wf["nodes"]] + wf["paths"],
                          stderr=subprocess.PIPE, timeout=120)


def test_the_file_is_the_models_whatever_the_batches(world_files, tmp_path):
    want = world_files["text"]
    assert want.count(b"\n") > 6 and want.startswith(b"mapped_taxid\tgenome_taxids:kmers_mapped:total_genome_kmers\n")
    for flags in ([], ["-B", "1"], ["-B", "7000"], ["-l", str(L), "-L", "khash"]):          # -B 1: a batch per sequence
        out = str(tmp_path / "distrib.txt")
        pr = distrib(world_files, flags, out)
        assert pr.returncode == 0, pr.stderr.decode()
        assert open(out, "rb").read() == want, flags


def test_paths_file(world_files, tmp_path):
    lst = str(tmp_path / "paths.txt")
    open(lst, "w").write("\n".join(world_files["paths"]) + "\n")
    out = str(tmp_path / "distrib.txt")
    pr = subprocess.run([BIN, "distrib", "-M", world_files["names"], "-F", lst, "-o", out, world_files["db"], world_files["nodes"]],
                        stderr=subprocess.PIPE, timeout=120)
    assert pr.returncode == 0, pr.stderr.decode()
    assert open(out, "rb").read() == world_files["text"]


def test_a_full_pair_table_is_an_error(world_files, tmp_path):
    out = str(tmp_path / "distrib.txt")
    pr = distrib(world_files, ["-P", "4"], out)
    assert pr.returncode != 0 and b"-P pairs" in pr.stderr, pr.stderr.decode()
    assert not os.path.exists(out)


def test_a_window_shorter_than_the_seed_is_refused(world_files, tmp_path):
    out = str(tmp_path / "distrib.txt")
    pr = distrib(world_files, ["-l", "20"], out)
    assert pr.returncode != 0 and b"-l 20" in pr.stderr, pr.stderr.decode()
    assert not os.path.exists(out)
