"""`bonsai classify -Q <q>`: stdout, the taxon file (-b) and the report (-R) byte for byte those of the run WITHOUT -Q on the same file
with every base of low quality replaced by 'N' (tests/minq_lib.py) -- for every way the text reaches the kernels (plain, a pair, BGZF,
a BGZF pair, one gzip stream, the device's own Kraken lines, two contexts on one device) and for the host parser (BNS_TEXT_GPU=0, a
stretch the device hands back, -f); `bonsai pack -Q`; and what is refused."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import minq_lib as M
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bonsai_amd", "bin", "bonsai")
Q = 20


def run(cmd, args, ok=True, **env):
    e = dict(os.environ, BNS_CLI_TIMING="1")
    e.update({k: str(v) for k, v in env.items()})
    p = subprocess.run([BIN, cmd] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=e)
    if ok:
        assert p.returncode == 0, p.stderr.decode()
    return p.stdout, p.stderr.decode(), p.returncode


def write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


@pytest.fixture(scope="module")
def files(oracle, small_world, tmp_path_factory):
    d = tmp_path_factory.mktemp("cliq")
    w = small_world
    db = str(d / "bns.db")
    oracle.db_write(db, 31, 31, None, w.table, spacing_width=1)
    nodes = str(d / "nodes.dmp")
    synth.write_nodes_dmp(nodes)
    rng = np.random.default_rng(41)
    n = 1500
    r1 = synth.simulate_reads(rng, w.genomes, n, var_len=True, n_rate=0.002)
    r2 = synth.simulate_reads(rng, w.genomes, n, var_len=True)
    q1 = [M.illumina_qual(rng, r.size) for r in r1]
    q2 = [M.illumina_qual(rng, r.size) if i % 4 else None for i, r in enumerate(r2)]        # (every fourth second mate: FASTA)
    for i in range(0, n, 7):                                       # quality lines that start like a header or a '+' line
        q1[i] = b"@>+"[i % 3:i % 3 + 1] + q1[i][1:]
    d1 = M.fastq_text([b"read%d/1 a comment" % i for i in range(n)], r1, q1)
    d2 = M.fastq_text([b"read%d/2" % i for i in range(n)], r2, q2, wrap_seq=80, wrap_qual=61)
    f = {"db": db, "nodes": nodes, "n": n, "d1": d1, "d2": d2}
    for tag, doc in (("1", d1), ("2", d2)):
        sub, recs = M.substituted_text(doc, Q)
        assert len(recs) == n and sub != doc
        f["r" + tag] = write(d / ("r%s.fq" % tag), doc)
        f["s" + tag] = write(d / ("s%s.fq" % tag), sub)
        for kind in ("r", "s"):
            text = doc if kind == "r" else sub
            bg = str(d / ("%s%s.bgzf.fq.gz" % (kind, tag)))
            synth.write_bgzf(bg, text, member_sizes=[65280, 30000, 1000])
            f[kind + tag + "_bgzf"] = bg
            f[kind + tag + "_gz"] = write(d / ("%s%s.fq.gz" % (kind, tag)), gzip.compress(text, 6))
    return f


def outputs(files, tmp_path, tag, flags, inputs, **env):
    """stdout, the -b file and the -R file of one run"""
    b, r = str(tmp_path / (tag + ".bin")), str(tmp_path / (tag + ".report"))
    out, err, _ = run("classify", ["-a", "-b", b, "-R", r] + flags + [files["db"], files["nodes"]] + inputs, **env)
    return out, open(b, "rb").read(), open(r, "rb").read(), err


FORMS = {
    "plain": (["1"], "", {}, "text on the device"),
    "pair": (["1", "2"], "", {}, None),
    "bgzf": (["1"], "_bgzf", {"BNS_BGZF_BATCH_MEMBERS": 3}, "BGZF text on the device"),
    "bgzf_pair": (["1", "2"], "_bgzf", {"BNS_BGZF_BATCH_MEMBERS": 3}, None),
    "gzip": (["1"], "_gz", {}, "gzip text on the device"),
    "host_parser": (["1"], "", {"BNS_TEXT_GPU": 0}, None),
    "host_parser_pair": (["1", "2"], "", {"BNS_TEXT_GPU": 0}, None),
    "device_lines": (["1"], "", {"BNS_LINES_GPU": 1}, "text on the device"),
    "device_lines_blocks": (["1"], "", {"BNS_LINES_GPU": 1, "BNS_TEXT_BLOCK_BYTES": 20000}, "text on the device"),
    "two_contexts": (["1"], "", {"BNS_TEXT_BLOCK_BYTES": 20000}, "text on the device"),
    "two_contexts_pair": (["1", "2"], "", {}, None),
}


@pytest.mark.parametrize("form", sorted(FORMS))
def test_q_equals_the_substituted_file(files, tmp_path, form):
    which, suffix, env, says = FORMS[form]
    flags = ["-g", "0,0"] if form.startswith("two_contexts") else []
    got = outputs(files, tmp_path, "q", ["-Q", str(Q)] + flags, [files["r" + t + suffix] for t in which], **env)
    exp = outputs(files, tmp_path, "s", flags, [files["s" + t + suffix] for t in which], **env)
    plain = outputs(files, tmp_path, "p", flags, [files["r" + t + suffix] for t in which], **env)
    assert got[0] == exp[0], "stdout"
    assert got[1] == exp[1] and len(got[1]) == 4 * files["n"], "-b"
    assert got[2] == exp[2] and got[2], "-R"
    if says:
        assert says in got[3] and "host parser takes the rest" not in got[3], got[3]
    # it bites: a tenth of the lines differ from the run without -Q, and a tenth of the units are still classified
    a, b = got[0].split(b"\n"), plain[0].split(b"\n")
    assert len(a) == len(b) == files["n"] + 1
    assert sum(1 for x, y in zip(a, b) if x != y) * 10 >= files["n"]
    assert np.count_nonzero(np.frombuffer(got[1], dtype=np.uint32)) * 10 >= files["n"]


def test_device_and_host_parser_meet_at_a_record_boundary(files, tmp_path):
    """an irregular stretch in the middle of a file: the device takes what is in front, the host parser the rest -- both mask alike"""
    d1 = files["d1"]
    cut = d1.index(b"@read700/1")
    doc = d1[:cut] + b"stray text between records\n" + d1[cut:]
    sub, recs = M.substituted_text(d1, Q)
    scut = sub.index(b"@read700/1")
    p, s = write(tmp_path / "mid.fq", doc), write(tmp_path / "mid_sub.fq", sub[:scut] + b"stray text between records\n" + sub[scut:])
    for block in (20000, 1 << 22):
        got = outputs(files, tmp_path, "q", ["-Q", str(Q)], [p], BNS_TEXT_BLOCK_BYTES=block)
        exp = outputs(files, tmp_path, "s", [], [s], BNS_TEXT_BLOCK_BYTES=block)
        host = outputs(files, tmp_path, "h", ["-Q", str(Q)], [p], BNS_TEXT_GPU=0)
        assert "text on the device" in got[3] and "host parser takes the rest" in got[3], got[3]
        assert got[:3] == exp[:3] and got[:3] == host[:3]
        assert got[0].count(b"\n") == files["n"]


def test_fastq_style_output_keeps_the_original_bases(files, tmp_path):
    """-f prints the ORIGINAL bases and qualities; only the classification carried in the record reflects the mask: the substituted
    file's output with the original sequence lines put back"""
    for which in (["1"], ["1", "2"]):
        got, _, _ = run("classify", ["-a", "-f", "-K", "-Q", str(Q), files["db"], files["nodes"]] + [files["r" + t] for t in which])
        sub, _, _ = run("classify", ["-a", "-f", "-K", files["db"], files["nodes"]] + [files["s" + t] for t in which])
        plain, _, _ = run("classify", ["-a", "-f", "-K", files["db"], files["nodes"]] + [files["r" + t] for t in which])
        g, s, p = got.split(b"\n"), sub.split(b"\n"), plain.split(b"\n")
        assert len(g) == len(s) == len(p) >= 4 * files["n"] * len(which)
        # (the two runs print the same lines but for the classification in the header lines and the bases: a line of the unmasked run
        # that is a read's sequence goes back in)
        bases = {r[2] for t in which for r in M.records(files["d" + t])}
        exp = [y if y in bases else x for x, y in zip(s, p)]
        n_back = sum(1 for x, y in zip(s, p) if y in bases and x != y)
        assert n_back * 2 >= files["n"]
        assert g == exp
        assert g != p and g != s


def test_pack_with_q_then_classify(files, tmp_path):
    """`bonsai pack -Q` masks while packing (the container holds flags, not qualities): classifying it equals `classify -Q` on the text"""
    for which in (["1"], ["1", "2"]):
        cont = str(tmp_path / ("c%d.bnsp" % len(which)))
        run("pack", ["-o", cont, "-Q", str(Q)] + [files["r" + t] for t in which])
        got = outputs(files, tmp_path, "c", [], [cont])
        exp = outputs(files, tmp_path, "q", ["-Q", str(Q)], [files["r" + t] for t in which])
        assert got[:3] == exp[:3]
        unmasked = str(tmp_path / ("u%d.bnsp" % len(which)))
        run("pack", ["-o", unmasked] + [files["r" + t] for t in which])
        assert open(unmasked, "rb").read() != open(cont, "rb").read()
        # -Q on a container: it holds no qualities
        out, err, rc = run("classify", ["-a", "-Q", str(Q), files["db"], files["nodes"], unmasked], ok=False)
        assert rc != 0 and out == b"" and "read container does not hold" in err and "-Q" in err, err


@pytest.mark.parametrize("arg", ["94", "x", "-1", "2.5", "", "20q", "1000000000000"])
def test_q_outside_its_range_is_refused(files, arg):
    for cmd, args in (("classify", [files["db"], files["nodes"], files["r1"]]), ("pack", ["-o", os.devnull, files["r1"]])):
        out, err, rc = run(cmd, ["-Q", arg] + args, ok=False)
        assert rc != 0 and out == b"" and "-Q: the minimum base quality must be an integer in [0, 93]" in err, (cmd, arg, err)


def test_q_zero_and_the_top_of_the_range(files, tmp_path):
    """-Q 0 is the run without -Q; -Q 93 masks every base of every record that has quality"""
    plain = outputs(files, tmp_path, "p", [], [files["r1"]])
    zero = outputs(files, tmp_path, "z", ["-Q", "0"], [files["r1"]])
    assert plain[:3] == zero[:3]
    top = outputs(files, tmp_path, "t", ["-Q", "93"], [files["r1"]])
    assert not np.frombuffer(top[1], dtype=np.uint32).any()
