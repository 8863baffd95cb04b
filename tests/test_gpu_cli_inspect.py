"""`bonsai inspect` (the db's keys per taxon, counted on the device from the loaded table) and `bonsai classify -R r -u -d` (the clade's
db key count and the coverage behind the distinct k-mer column), against the numpy model of tests/inspect_model.py."""
import subprocess

import numpy as np
import pytest

import inspect_model
import synth
from test_gpu_cli import BIN, files  # noqa: F401  (the module's fixture)
from test_gpu_report import NAMES, RANKS, expected_report, rep  # noqa: F401  (rep: the module's fixture)

pytestmark = pytest.mark.gpu


def present_vals(w):
    return w.vals[inspect_model.present_mask(w.flags, w.n_buckets)]


def inspect(args, ok=True):
    p = subprocess.run([BIN, "inspect"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    if ok:
        assert p.returncode == 0, p.stderr.decode()
    return p


def split_comments(text):
    lines = text.splitlines(True)
    head = [ln for ln in lines if ln.startswith("# ")]
    assert lines[:len(head)] == head                                    # the comment lines come first
    return dict(ln[2:].rstrip("\n").split("\t") for ln in head), "".join(lines[len(head):])


@pytest.mark.parametrize("layout", ["minbucket", "bucket", "khash"])
def test_inspect(files, rep, tmp_path, layout):
    w = files["w"]
    vals = present_vals(w)
    want = expected_report(vals.tolist(), ranks=RANKS, names=NAMES)
    p = inspect(["-L", layout, "-n", rep["names"], files["db"], rep["nodes"]])
    head, body = split_comments(p.stdout.decode())
    assert body == want
    assert head["k"] == "31" and head["keys"] == str(vals.size) and head["layout"] == layout
    assert set(head) == {"k", "keys", "layout", "buckets", "window", "overflow keys"}
    assert int(head["buckets"]) > 0 and int(head["overflow keys"]) == 0
    assert (int(head["window"]) in (8, 11, 15)) == (layout == "minbucket")
    if layout == "minbucket":                                           # -o, -g, and the default layout; names left out
        out = str(tmp_path / "inspect.txt")
        q = inspect(["-g", "0", "-o", out, files["db"], rep["nodes"]])
        assert q.stdout == b""
        head2, body2 = split_comments(open(out).read())
        assert head2 == head and body2 == expected_report(vals.tolist(), ranks=RANKS)


def test_inspect_usage():
    p = inspect(["only_one_argument"], ok=False)
    assert p.returncode != 0 and b"Usage" in p.stderr and b"inspect" in p.stderr
    p = inspect(["-L", "nonsense", "a", "b"], ok=False)
    assert p.returncode != 0 and b"Usage" in p.stderr


def classify(opts, files, rep, report):
    return subprocess.run([BIN, "classify", "-K", "-R", report, "-n", rep["names"]] + opts + [files["db"], rep["nodes"], files["r1"]],
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_classify_db_keys_and_coverage(files, rep, tmp_path):
    w = files["w"]
    _, clade = inspect_model.model(w.flags, w.keys, w.vals, w.parent)
    ru, rd, rg = (str(tmp_path / x) for x in ("u.report", "d.report", "g.report"))
    p = classify(["-u"], files, rep, ru)
    assert p.returncode == 0, p.stderr.decode()
    p = classify(["-u", "-d"], files, rep, rd)
    assert p.returncode == 0, p.stderr.decode()
    base, got = open(ru).read(), open(rd).read()
    rows = [ln.split("\t") for ln in got.splitlines(True)]
    assert len(rows) > 8 and all(len(f) == 9 for f in rows)
    assert "".join("\t".join(f[:4] + f[6:]) for f in rows) == base      # the two columns cut out: the -u report, byte for byte
    n = w.parent.size
    for f in rows:
        distinct, keys, taxid = int(f[3]), int(f[4]), int(f[7])
        if f[6] == "U":
            assert (f[4], f[5]) == ("0", "0.000000")
            continue
        assert keys == int(clade[n if taxid == 0xFFFFFFFF else taxid]), f
        assert keys > 0 and f[5] == "%.6f" % (distinct / keys), f
    assert any(f[6] == "U" for f in rows) and any(int(f[7]) == 1001 for f in rows)
    # two contexts hold the same table twice: the db column is context 0's, not the sum
    p = classify(["-u", "-d", "-g", "0,0", "-c", "5000"], files, rep, rg)
    assert p.returncode == 0, p.stderr.decode()
    assert open(rg).read() == got


def test_d_needs_the_distinct_column(files, rep, tmp_path):
    r = str(tmp_path / "no.report")
    p = classify(["-d"], files, rep, r)
    assert p.returncode != 0 and b"-d" in p.stderr and b"-u" in p.stderr and b"Usage" in p.stderr
    assert b"Successfully completed" not in p.stderr
    p = subprocess.run([BIN, "classify", "-K", "-u", "-d", files["db"], rep["nodes"], files["r1"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=300)
    assert p.returncode != 0 and b"-R" in p.stderr


def test_build_then_inspect(rep, tmp_path):
    """two small genomes built on the device, then inspected: the totals are the built db's key count"""
    from bonsai_amd import hostio
    rng = np.random.default_rng(12)
    seqs = {"NC_A.1": (1001, synth.rand_seq(rng, 33).tobytes()), "NC_B.1": (1002, synth.rand_seq(rng, 400).tobytes())}
    names = str(tmp_path / "nameidmap.txt")
    paths = []
    with open(names, "w") as nf:
        for acc, (tx, s) in seqs.items():
            nf.write("%s\t%d\n" % (acc, tx))
            p = str(tmp_path / (acc + ".fna"))
            open(p, "wb").write(b">" + acc.encode() + b"\n" + s + b"\n")
            paths.append(p)
    db = str(tmp_path / "two.db")
    pr = subprocess.run([BIN, "build", "-k", "31", "-T", rep["nodes"], "-M", names, db, "unused"] + paths, stderr=subprocess.PIPE, timeout=300)
    assert pr.returncode == 0, pr.stderr.decode()
    d = hostio.read_db(db)
    assert d["size"] == 3 + 370
    head, body = split_comments(inspect([db, rep["nodes"]]).stdout.decode())
    assert head["keys"] == str(d["size"])
    rows = {int(f[4]): f for f in (ln.split("\t") for ln in body.splitlines())}
    assert int(rows[1][1]) == d["size"] and rows[1][0] == "100.00"
    assert int(rows[1001][2]) == 3 and int(rows[1002][2]) == 370
    pres = inspect_model.present_mask(d["flags"], d["n_buckets"])
    assert body == expected_report(d["vals"][pres].tolist(), ranks=RANKS)
