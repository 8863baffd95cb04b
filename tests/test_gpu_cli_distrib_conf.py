"""`bonsai distrib -t`: the window session with the threshold `classify -t` takes, against the model of tests/test_gpu_windows_conf.py
written out by windows_model.distrib_text; and the three commands end to end -- `classify -t -R`, `distrib -t -l`, `abundance` --
against tests/abundance_model.py run on the same two files.  No accuracy claim is asserted: nobody has measured one."""
import gzip
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import abundance_model as AM
import confidence_ref as cr
import synth
import windows_model as WM
from bonsai_amd import hostio
from test_gpu_cli_distrib import BIN, L, distrib, world_files  # noqa: F401  (world_files: the module's fixture)
from test_gpu_report import RANKS, fastq
from test_gpu_windows_conf import Model

pytestmark = pytest.mark.gpu


def fasta_records(path):
    text = (gzip.open(path, "rb") if path.endswith(".gz") else open(path, "rb")).read()
    recs = []
    for block in text.split(b">")[1:]:
        head, _, body = block.partition(b"\n")
        recs.append((head.split()[0].decode(), np.frombuffer(body.replace(b"\n", b""), dtype=np.uint8)))
    return recs


@pytest.fixture(scope="module")
def genome_records(world_files):
    """(taxid, sequence) of every record of the fixture's genome files: a file's records take the taxid of its first name"""
    taxid = dict(line.split("\t") for line in open(world_files["names"]).read().split("\n") if line)
    out = []
    for p in world_files["paths"]:
        recs = fasta_records(p)
        out += [(int(taxid[recs[0][0]]), seq) for _, seq in recs]
    return out


def model_text(oracle, w, records, theta):
    m = Model(oracle, w.table, w.tax, cr.parent_map(w.parent), [s for _, s in records], [t for t, _ in records], L)
    return WM.distrib_text(*m.at(theta)[1]), m


def test_the_threshold_reaches_the_session(oracle, small_world, world_files, genome_records, tmp_path):
    want, m = model_text(oracle, small_world, genome_records, Fraction(1, 4))
    assert WM.distrib_text(*m.at(0)[1]) == world_files["text"] and want != world_files["text"]
    out = str(tmp_path / "distrib.txt")
    for flags in (["-t", "0.25", "-l", str(L)], ["-t", "0.250", "-l", str(L), "-B", "1"], ["-t", ".25", "-B", "7000", "-L", "bucket"]):
        pr = distrib(world_files, flags, out)
        assert pr.returncode == 0, pr.stderr.decode()
        assert open(out, "rb").read() == want, flags
    for flags in (["-t", "0"], ["-t", "0.000", "-B", "7000"]):                              # no threshold: the file as it always was
        pr = distrib(world_files, flags, out)
        assert pr.returncode == 0, pr.stderr.decode()
        assert open(out, "rb").read() == world_files["text"], flags


@pytest.mark.parametrize("value", ["1.5", "0.1234567891", "-0.1", "x", "1.0000000001", ""])
def test_a_bad_threshold_is_refused(world_files, tmp_path, value):
    out = str(tmp_path / "distrib.txt")
    pr = distrib(world_files, ["-t", value], out)
    assert pr.returncode != 0 and b"Usage" in pr.stderr and not os.path.exists(out)


def test_classify_distrib_abundance(oracle, small_world, world_files, tmp_path):
    w = small_world
    nodes = str(tmp_path / "nodes.dmp")
    with open(nodes, "w") as f:
        for ch, p in synth.TAX_PAIRS:
            f.write("%d\t|\t%d\t|\t%s\t|\t\t|\n" % (ch, p, RANKS[ch]))
    reads = synth.simulate_reads(np.random.default_rng(77), w.genomes, 3000, length=L, sub_rate=0.02, random_frac=0.1)
    fq, report, dfile, out = (str(tmp_path / n) for n in ("reads.fq", "report.txt", "distrib.txt", "abundance.txt"))
    open(fq, "wb").write(fastq(reads))
    pr = subprocess.run([BIN, "classify", "-t", "0.1", "-R", report, "-o", os.devnull, world_files["db"], nodes, fq], stderr=subprocess.PIPE, timeout=120)
    assert pr.returncode == 0, pr.stderr.decode()
    wf = dict(world_files, nodes=nodes)
    pr = distrib(wf, ["-t", "0.1", "-l", str(L)], dfile)
    assert pr.returncode == 0, pr.stderr.decode()
    par = {c: (0 if c == p else p) for c, p in synth.TAX_PAIRS}
    direct, dist = AM.parse_report(open(report).read()), AM.parse_distrib(open(dfile).read())
    assert sum(direct.values()) == len(reads)
    for level, min_reads in (("S", 10), ("G", 10), ("S", 2000)):
        pr = subprocess.run([BIN, "abundance", "-l", level, "-T", str(min_reads), "-o", out, dfile, report, nodes], stderr=subprocess.PIPE, timeout=60)
        assert pr.returncode == 0, pr.stderr.decode()
        rows, want = AM.estimate(dist, direct, par, RANKS, level, min_reads)
        text, totals = hostio.estimate_abundance(dfile, report, nodes, level=level, min_reads=min_reads)
        assert open(out).read() == text
        AM.check(text, totals, rows, want)                                                  # the accounting identity is part of it
        # the five totals as the command prints them on stderr: four integers, the estimate with three decimals
        got = [line.rsplit(" ", 1)[1] for line in pr.stderr.decode().split("\n") if ": " in line]
        assert got == ["%d" % totals[k] for k in hostio.ABUNDANCE_TOTALS[:4]] + ["%.3f" % totals["estimated"]]
    rows, want = AM.estimate(dist, direct, par, RANKS, "S", 10)
    assert len(rows) >= 4 and any(r[4] > 0 for r in rows)                                   # reads above the species were distributed
    pr = subprocess.run([BIN, "abundance", dfile, report], stderr=subprocess.PIPE, timeout=60)
    assert pr.returncode != 0 and b"Usage" in pr.stderr
    pr = subprocess.run([BIN, "abundance", "-l", "X", dfile, report, nodes], stderr=subprocess.PIPE, timeout=60)
    assert pr.returncode != 0 and b"Usage" in pr.stderr
