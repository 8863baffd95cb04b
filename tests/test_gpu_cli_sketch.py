"""`bonsai classify -R <path> -u`: the taxon report with the distinct k-mer column, against one restated here -- test_gpu_report.py's
expected_report from the oracle's per-read taxa, and the column from the numpy model's sketches (tests/sketch_model.py) merged up
the synthetic taxonomy."""
import gzip
import os
import subprocess

import pytest

import sketch_model as SM
import synth
from test_gpu_cli import BIN, files  # noqa: F401  (the module's fixture)
from test_gpu_report import NAMES, RANKS, expected_report, rep  # noqa: F401  (rep: the module's fixture)

pytestmark = pytest.mark.gpu


def classify(opts, inputs, files, rep, report, env=None, ok=True):
    p = subprocess.run([BIN, "classify", "-K"] + (["-R", report, "-n", rep["names"]] if report else []) + opts + [files["db"], rep["nodes"]] + inputs,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=dict(os.environ, **(env or {})))
    if ok:
        assert p.returncode == 0, p.stderr.decode()
    return p


def expected_distinct_report(oracle, w, taxa, reads):
    seven = expected_report(taxa, ranks=RANKS, names=NAMES)
    bins, regs = SM.sketches(oracle, w.table, w.parent, reads, 31)
    n = w.parent.size
    assert bins.size > 6 and bins[-1] < n
    return SM.add_column(seven, SM.clade_estimates(bins, regs, synth.TAX_PAIRS), n), seven


def test_report_with_distinct_kmers(oracle, files, rep, tmp_path):
    w, reads = files["w"], files["reads"]
    want1, seven1 = expected_distinct_report(oracle, w, rep["tax1"], reads[:300])
    want2, _ = expected_distinct_report(oracle, w, rep["tax_pair"], reads)
    # the column is there, a clade's value is not the sum of its children's (shared k-mers count once) and never below a child's
    col = {int(f[5]): int(f[3]) for f in (ln.split("\t") for ln in want1.splitlines())}
    assert col[0] == 0 and col[1] >= col[2] >= col[11] >= col[101] >= col[1001] > 100
    text = open(files["r1"], "rb").read()
    gz = str(tmp_path / "r1.gz")
    with gzip.open(gz, "wb") as f:
        f.write(text)
    bg = str(tmp_path / "r1.bgzf.gz"); synth.write_bgzf(bg, text, member_sizes=[5000, 700])
    r = str(tmp_path / "out.report")
    for tag, inputs, opts, want in (("plain", [files["r1"]], [], want1), ("gzip", [gz], [], want1), ("bgzf", [bg], [], want1),
                                    ("pair", [files["r1"], files["r2"]], [], want2), ("two contexts", [files["r1"]], ["-g", "0,0", "-c", "5000"], want1),
                                    ("small chunks", [files["r1"]], ["-c", "5000"], want1)):
        for env in ({}, {"BNS_TEXT_GPU": "0"}):
            p = classify(["-u"] + opts, inputs, files, rep, r, env=env)
            assert open(r).read() == want, (tag, env)
            assert "got no sketch" not in p.stderr.decode()
    # without -u: today's report
    classify([], [files["r1"]], files, rep, r)
    assert open(r).read() == seven1


def test_u_needs_the_report(files, rep):
    p = classify(["-u"], [files["r1"]], files, rep, None, ok=False)
    assert p.returncode != 0 and b"-u" in p.stderr and b"-R" in p.stderr
    assert b"Successfully completed" not in p.stderr


def test_dropped_bins_are_reported(oracle, files, rep, tmp_path):
    w, reads = files["w"], files["reads"]
    r = str(tmp_path / "few.report")
    p = classify(["-u", "-U", "2"], [files["r1"]], files, rep, r)
    bins, regs = SM.sketches(oracle, w.table, w.parent, reads[:300], 31)
    assert ("[W] -u: %d taxon bins got no sketch" % (bins.size - 2)) in p.stderr.decode()
    # one launch: the two smallest bins have their sketches, so the column is what they alone give
    want = SM.add_column(expected_report(rep["tax1"], ranks=RANKS, names=NAMES), SM.clade_estimates(bins[:2], regs[:2], synth.TAX_PAIRS), w.parent.size)
    assert open(r).read() == want
    for bad in ("0", "x", "1048577"):
        q = classify(["-u", "-U", bad], [files["r1"]], files, rep, r, ok=False)
        assert q.returncode != 0 and b"-U" in q.stderr
