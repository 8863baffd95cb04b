"""`bonsai classify -M`: every input form and several contexts against tests/hit_groups_ref.py -- the -b taxa, the Kraken lines (host
formatter and BNS_LINES_GPU=1 byte for byte), the -R report -- over a thinned db (minimizers of 50-base windows), where -M 3 moves a
good share of the units."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import hit_groups_ref as HG
import synth
from test_gpu_cli import BIN
from test_gpu_report import NAMES, RANKS, expected_report

pytestmark = pytest.mark.gpu

N = 3


@pytest.fixture(scope="module")
def hg(oracle, small_world, tmp_path_factory):
    d = tmp_path_factory.mktemp("hit_groups")
    w = HG.thinned_world(oracle, small_world)
    f = {"w": w, "db": str(d / "bns.db"), "nodes": str(d / "nodes.dmp"), "names": str(d / "names.dmp"), "r1": str(d / "r1.fq"),
         "r2": str(d / "r2.fq.gz")}
    oracle.db_write(f["db"], 31, 50, None, w.table, spacing_width=1)
    with open(f["nodes"], "w") as fh:
        for ch, p in synth.TAX_PAIRS:
            fh.write("%d\t|\t%d\t|\t%s\t|\t\t|\n" % (ch, p, RANKS[ch]))
    with open(f["names"], "w") as fh:
        for t, nm in NAMES.items():
            fh.write("%d\t|\t%s\t|\t\t|\tscientific name\t|\n" % (t, nm))
    reads = HG.parity_reads(small_world, False)
    with open(f["r1"], "wb") as fh:
        for i, r in enumerate(reads[:300]):
            fh.write(b"@read%d/1 some comment\n%s\n+\n%s\n" % (i, r.tobytes(), b"I" * r.size))
    with gzip.open(f["r2"], "wb") as fh:
        for i, r in enumerate(reads[300:]):
            fh.write(b"@read%d/2\n%s\n+\n%s\n" % (i, r.tobytes(), b"I" * r.size))
    f["lens"] = [r.size for r in reads[:300]]
    f["names_of"] = ["read%d" % i for i in range(300)]
    for tag, rs, paired in (("single", reads[:300], False), ("pair", [x for i in range(300) for x in (reads[i], reads[300 + i])], True)):
        units = HG.oracle_units(oracle, w, rs, paired)
        g, _ = HG.groups_of(oracle, w.table, rs, paired, 31)
        base = np.array([u[0] for u in units], dtype=np.uint32)
        f[tag] = {"units": units, "base": base, "g": g, "taxa": HG.apply(base, g, N)}
        changed = np.count_nonzero(f[tag]["taxa"] != base)
        assert changed >= 15 and np.count_nonzero(f[tag]["taxa"]) >= 100, (tag, changed)     # (-M 3 moves units, and leaves units)
    text = open(f["r1"], "rb").read()
    f["bgzf"] = str(d / "r1.bgzf.gz"); synth.write_bgzf(f["bgzf"], text, member_sizes=[5000, 700])
    f["gzip"] = str(d / "r1.gz")
    with gzip.open(f["gzip"], "wb") as fh:
        fh.write(text)
    f["bnsp"] = str(d / "r1.bnsp")
    p = subprocess.run([BIN, "pack", "-o", f["bnsp"], "-c", "20000", f["r1"]], stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    return f


def cli(args, env=None, ok=True):
    e = dict(os.environ)
    e.pop("BNS_LINES_GPU", None)
    e.update({k: str(v) for k, v in (env or {}).items()})
    p = subprocess.run([BIN, "classify"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=e)
    if ok:
        assert p.returncode == 0, p.stderr.decode()
    return p


def lines(oracle, hg, tag, taxa, emit_all=True):
    out = []
    for nm, l, (_, m, a, h), t in zip(hg["names_of"], hg["lens"], hg[tag]["units"], taxa):
        if t or emit_all:
            out.append(oracle.kraken_line(nm, int(t), l, m, a, h))
    return b"".join(out)


def check_run(oracle, hg, tmp_path, tag, opts, inputs, env=None, what=""):
    """-M 3 -a with -b and -R: the taxon file, the lines and the report as the model says; -> stderr"""
    tb, rp = str(tmp_path / "t.bin"), str(tmp_path / "t.report")
    p = cli(["-M", str(N), "-a", "-b", tb, "-R", rp, "-n", hg["names"]] + opts + [hg["db"], hg["nodes"]] + inputs, env=env)
    taxa = hg[tag]["taxa"]
    assert np.fromfile(tb, dtype="<u4").tolist() == taxa.tolist(), what
    assert p.stdout == lines(oracle, hg, tag, taxa), what
    assert open(rp).read() == expected_report(taxa.tolist(), ranks=RANKS, names=NAMES), what
    n_c = int(np.count_nonzero(taxa))
    assert ("Classified %d, unclassified %d" % (n_c, taxa.size - n_c)).encode() in p.stderr, what
    return p.stderr


FORMS = {"plain": ("single", [], ["r1"], {}), "bgzf": ("single", [], ["bgzf"], {}), "gzip": ("single", [], ["gzip"], {}),
         "container": ("single", [], ["bnsp"], {}), "host-parser": ("single", ["-c", "20000"], ["r1"], {"BNS_TEXT_GPU": 0}),
         "two-contexts": ("single", ["-g", "0,0", "-c", "20000"], ["r1"], {}), "pair": ("pair", [], ["r1", "r2"], {}),
         "pair-host-parser": ("pair", ["-c", "20000"], ["r1", "r2"], {"BNS_TEXT_GPU": 0}),
         "pair-two-contexts": ("pair", ["-g", "0,0", "-c", "20000"], ["r1", "r2"], {})}


@pytest.mark.parametrize("form", list(FORMS))
def test_cli_input_forms(oracle, hg, tmp_path, form):
    tag, opts, inputs, env = FORMS[form]
    for mode in (0, 1):                                                  # the host formatter, the lines assembled on the device
        check_run(oracle, hg, tmp_path, tag, opts, [hg[x] for x in inputs], env=dict(env, BNS_LINES_GPU=mode), what=(form, mode))


def test_cli_outputs_that_follow_the_taxon(oracle, hg, tmp_path):
    taxa = hg["single"]["taxa"]
    # without -a only the units -M leaves classified are printed
    assert cli(["-M", str(N), hg["db"], hg["nodes"], hg["r1"]]).stdout == lines(oracle, hg, "single", taxa, emit_all=False)
    # -f: the FASTQ records of a plain run, with the new taxon (and C / U) in each header
    plain = cli(["-f", "-a", "-K", hg["db"], hg["nodes"], hg["r1"]]).stdout.split(b"\n")
    got = cli(["-M", str(N), "-f", "-a", "-K", hg["db"], hg["nodes"], hg["r1"]]).stdout.split(b"\n")
    assert len(got) == len(plain) == 4 * 300 + 1
    for i in range(300):
        assert got[4 * i + 1:4 * i + 4] == plain[4 * i + 1:4 * i + 4]
        fields = got[4 * i].split(b"\t")
        assert fields[0].endswith(b" " + (b"C" if taxa[i] else b"U")) and int(fields[1]) == taxa[i], i
        assert fields[2:] == plain[4 * i].split(b"\t")[2:]
    # with -t in front of it
    import confidence_ref as CR
    from fractions import Fraction
    par = CR.parent_map(hg["w"].parent)
    units = hg["single"]["units"]
    g = hg["single"]["g"]
    walked = np.array([CR.walk(par, Fraction(1, 10), t, m, h.tolist()) for t, m, _, h in units], dtype=np.uint32)
    want = HG.apply(walked, g, N)
    tb = str(tmp_path / "c.bin")
    assert cli(["-t", "0.1", "-M", str(N), "-a", "-b", tb, hg["db"], hg["nodes"], hg["r1"]]).stdout == lines(oracle, hg, "single", want)
    assert np.fromfile(tb, dtype="<u4").tolist() == want.tolist()


def test_cli_zero_is_off(hg, tmp_path):
    for mode in (["-a"], ["-K"], ["-f", "-a"]):
        tb0, tb1 = str(tmp_path / "z0.bin"), str(tmp_path / "z1.bin")
        a = cli(mode + ["-b", tb0, hg["db"], hg["nodes"], hg["r1"]])
        b = cli(mode + ["-M", "0", "-b", tb1, hg["db"], hg["nodes"], hg["r1"]])
        assert a.stdout == b.stdout and open(tb0, "rb").read() == open(tb1, "rb").read(), mode
        assert np.fromfile(tb0, dtype="<u4").tolist() == hg["single"]["base"].tolist()
    # and 1 changes nothing
    assert cli(["-a", "-M", "1", hg["db"], hg["nodes"], hg["r1"]]).stdout == cli(["-a", hg["db"], hg["nodes"], hg["r1"]]).stdout


@pytest.mark.parametrize("bad", ["65", "x", "", "-1", "3.5", "3x", "100000000000"])
def test_cli_errors(hg, bad):
    p = cli(["-M", bad, hg["db"], hg["nodes"], hg["r1"]], ok=False)
    assert p.returncode != 0 and p.stdout == b"", bad
    assert b"-M" in p.stderr, p.stderr.decode()
