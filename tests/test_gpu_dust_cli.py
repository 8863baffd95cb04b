"""`bonsai classify -m` and `bonsai build -m`: every input form of the CLI with low-complexity masking on gives, byte for byte, the
output of the run without -m on the file whose masked bases are replaced by 'N' (tests/dust_ref.py); -f still prints the original
bases; a db built with -m is the db of the substituted genomes."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import build_cases as bc
from test_gpu_cli_build_add import db_map
import dust_world as DW
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bonsai_amd", "bin", "bonsai")
LEVEL = str(DW.T)


def fastq(names, reads):
    return b"".join(b"@%s\n%s\n+\n%s\n" % (n, r.tobytes(), b"I" * r.size) for n, r in zip(names, reads))


@pytest.fixture(scope="module")
def files(oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("dust_cli")
    w = DW.make_world(oracle, seed=61)
    f = {"w": w, "dir": d, "db": str(d / "bns.db"), "nodes": str(d / "nodes.dmp")}
    oracle.db_write(f["db"], 31, 31, None, w.table, spacing_width=1)
    synth.write_nodes_dmp(f["nodes"])
    reads = synth.simulate_reads(np.random.default_rng(7), w.genomes, 800, n_rate=0.002, lower_rate=0.01)
    reads[9] = reads[9][:0]; reads[10] = reads[10][:20]
    sub, masks = DW.substituted(reads)
    assert sum(int(m.any()) for m in masks) * 5 >= len(reads)
    f["reads"], f["sub"] = reads, sub
    half = len(reads) // 2
    for tag, rs in (("x", reads), ("s", sub)):
        one = fastq([b"r%d" % i for i in range(len(rs))], rs)
        m1 = fastq([b"p%d/1" % i for i in range(half)], rs[:half])
        m2 = fastq([b"p%d/2" % i for i in range(half)], rs[half:])
        for name, data in (("one.fq", one), ("m1.fq", m1), ("m2.fq", m2)):
            with open(str(d / (tag + "_" + name)), "wb") as fh:
                fh.write(data)
        synth.write_bgzf(str(d / (tag + "_bgzf.fq.gz")), one, block=20000)
        with gzip.open(str(d / (tag + "_plain.fq.gz")), "wb") as fh:
            fh.write(one)
        pk = str(d / (tag + "_reads.bnsp"))
        p = subprocess.run([BIN, "pack", "-o", pk, "-c", "20000", str(d / (tag + "_one.fq"))], stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, p.stderr.decode()
    return f


def classify(files, flags, inputs, tag):
    """-> (stdout, -b bytes, -R text)"""
    d = files["dir"]
    tb, rp = str(d / ("taxa_%s.bin" % tag)), str(d / ("report_%s.txt" % tag))
    p = subprocess.run([BIN, "classify"] + flags + ["-b", tb, "-R", rp, files["db"], files["nodes"]] + inputs, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode()
    with open(tb, "rb") as a, open(rp, "rb") as b:
        return p.stdout, a.read(), b.read()


FORMS = {"fastq": ["one.fq"], "pair": ["m1.fq", "m2.fq"], "bgzf": ["bgzf.fq.gz"], "gz": ["plain.fq.gz"], "container": ["reads.bnsp"]}


@pytest.mark.parametrize("form", list(FORMS))
def test_classify_m(files, form):
    d = files["dir"]
    on = classify(files, ["-a", "-m", LEVEL], [str(d / ("x_" + n)) for n in FORMS[form]], "on")
    off = classify(files, ["-a"], [str(d / ("s_" + n)) for n in FORMS[form]], "off")
    plain = classify(files, ["-a"], [str(d / ("x_" + n)) for n in FORMS[form]], "plain")
    n_units = len(files["reads"]) // (2 if form == "pair" else 1)
    assert on[0].count(b"\n") == n_units and len(on[1]) == 4 * n_units
    assert on[0] == off[0], "stdout"
    assert on[1] == off[1], "-b"
    assert on[2] == off[2], "-R"
    lo, lp = on[0].split(b"\n"), plain[0].split(b"\n")
    assert sum(a != b for a, b in zip(lo, lp)) * 5 >= n_units      # the mask changes a fifth of the lines at least


@pytest.fixture(scope="module")
def fastq_on(files):
    return classify(files, ["-a", "-m", LEVEL], [str(files["dir"] / "x_one.fq")], "ref")


def test_classify_m_two_contexts_on_one_device(files, fastq_on):
    """-g 0,0: the setting reaches every context; small chunks dealt to both"""
    x = [str(files["dir"] / "x_one.fq")]
    two = classify(files, ["-a", "-m", LEVEL, "-g", "0,0", "-c", "9000"], x, "two")
    assert two == classify(files, ["-a", "-m", LEVEL, "-g", "0", "-c", "9000"], x, "one")
    assert two == fastq_on


def test_classify_m_host_parser(files, fastq_on):
    """what the host parser reads reaches the device as a packed image: masked there as well"""
    d = files["dir"]
    p = subprocess.run([BIN, "classify", "-a", "-m", LEVEL, files["db"], files["nodes"], str(d / "x_one.fq")], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300, env=dict(os.environ, BNS_TEXT_GPU="0"))
    assert p.returncode == 0 and p.stdout == fastq_on[0]


def test_classify_m_fastq_output_prints_the_original_bases(files):
    d = files["dir"]
    on = classify(files, ["-a", "-f", "-K", "-m", LEVEL], [str(d / "x_one.fq")], "f_on")[0].split(b"\n")
    off = classify(files, ["-a", "-f", "-K"], [str(d / "s_one.fq")], "f_off")[0].split(b"\n")
    assert len(on) == len(off) == 4 * len(files["reads"]) + 1
    assert on[0::4] == off[0::4]                                  # the classification fields
    assert on[1::4] == [r.tobytes() for r in files["reads"]]      # ... over the bases as they were read
    assert off[1::4] == [r.tobytes() for r in files["sub"]]


@pytest.mark.parametrize("flags", [[], ["-w", "50", "-e"], ["-w", "50", "-D"]], ids=["every-kmer", "w50-entropy", "w50-taxdepth"])
def test_build_m(files, tmp_path, flags):
    from bonsai_amd import hostio
    w = files["w"]
    names = str(tmp_path / "nameidmap.txt")
    paths = {"x": [], "s": []}
    seqs = list(w.genomes.values())
    sub, _ = DW.substituted(seqs)
    with open(names, "w") as nf:
        for i, leaf in enumerate(w.genomes):
            nf.write("NC_%06d.1\t%d\n" % (i, leaf))
            for tag, g in (("x", seqs[i]), ("s", sub[i])):
                p = str(tmp_path / ("%s%d.fna" % (tag, i)))
                with open(p, "wb") as fh:
                    fh.write(b">NC_%06d.1 genome\n%s\n" % (i, g.tobytes()))
                paths[tag].append(p)

    def build(extra, which, out):
        pr = subprocess.run([BIN, "build", "-k", "31", "-T", files["nodes"], "-M", names] + flags + extra + [out, "unused"] + paths[which],
                            stderr=subprocess.PIPE, timeout=300)
        assert pr.returncode == 0, pr.stderr.decode()
        return hostio.read_db(out)
    on = build(["-m", LEVEL], "x", str(tmp_path / "on.db"))
    off = build([], "s", str(tmp_path / "off.db"))
    plain = build([], "x", str(tmp_path / "plain.db"))
    for k in ("k", "w", "n_buckets", "n_occupied", "size", "upper_bound"):
        assert on[k] == off[k], k
    assert db_map(on) == db_map(off)                              # (where a key sits in the arrays is the order of arrival's to decide)
    assert 0 < on["size"] < plain["size"]
    if not flags:
        t = bc.table_pairs(_oracle_table(files, sub))
        i = np.arange(on["n_buckets"])
        m = ((on["flags"][i >> 4] >> ((i & 15) << 1)) & 3) == 0
        order = np.argsort(on["keys"][m], kind="stable")
        assert np.array_equal(on["keys"][m][order], t[0]) and np.array_equal(on["vals"][m][order], t[1])


def _oracle_table(files, sub):
    import oracle_lib as O
    w = files["w"]
    t = O.Table()
    for leaf, g in zip(w.genomes, sub):
        O.lca_map_add(t, w.tax, 31, g.tobytes(), leaf)
    return t


def test_build_m_extends_a_db(files, tmp_path):
    """-A -m: the added genomes are masked; with a masked old db the result is the masked build over all genomes"""
    from bonsai_amd import hostio
    w = files["w"]
    names = str(tmp_path / "nameidmap.txt")
    paths = []
    with open(names, "w") as nf:
        for i, (leaf, g) in enumerate(w.genomes.items()):
            nf.write("NC_%06d.1\t%d\n" % (i, leaf))
            p = str(tmp_path / ("g%d.fna" % i))
            with open(p, "wb") as fh:
                fh.write(b">NC_%06d.1 genome\n%s\n" % (i, g.tobytes()))
            paths.append(p)

    def build(extra, which, out):
        pr = subprocess.run([BIN, "build", "-T", files["nodes"], "-M", names, "-m", LEVEL] + extra + [out, "unused"] + which, stderr=subprocess.PIPE, timeout=300)
        assert pr.returncode == 0, pr.stderr.decode()
        return hostio.read_db(out)
    whole = build(["-k", "31"], paths, str(tmp_path / "whole.db"))
    build(["-k", "31"], paths[:3], str(tmp_path / "first.db"))
    both = build(["-A", str(tmp_path / "first.db")], paths[3:], str(tmp_path / "both.db"))
    assert whole["size"] == both["size"] and whole["n_buckets"] == both["n_buckets"]
    assert db_map(whole) == db_map(both)


def test_usage_errors(files, tmp_path):
    d = files["dir"]
    for bad in ("0", "1001", "20x", "-3", ""):
        p = subprocess.run([BIN, "classify", "-m", bad, files["db"], files["nodes"], str(d / "x_one.fq")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode != 0 and b"-m: the low-complexity level must be an integer in [1, 1000]" in p.stderr, (bad, p.stderr)
        p = subprocess.run([BIN, "build", "-m", bad, "-T", files["nodes"], "-M", "none", str(tmp_path / "o.db"), "unused", "none.fna"], stderr=subprocess.PIPE, timeout=60)
        assert p.returncode != 0 and b"-m: the low-complexity level must be an integer in [1, 1000]" in p.stderr, (bad, p.stderr)
    p = subprocess.run([BIN, "pack", "-m", "20", "-o", str(tmp_path / "o.bnsp"), str(d / "x_one.fq")], stderr=subprocess.PIPE, timeout=60)
    assert p.returncode != 0 and b"Usage" in p.stderr and b"no -m" in p.stderr and not os.path.exists(str(tmp_path / "o.bnsp"))
    p = subprocess.run([BIN, "distrib", "-m", "20", "-M", "none", files["db"], files["nodes"], "none.fna"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode != 0 and b"Usage" in p.stderr and b"no -m" in p.stderr
