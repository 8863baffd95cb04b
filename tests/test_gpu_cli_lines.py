"""`bonsai classify` with the Kraken lines assembled on the device (BNS_LINES_GPU=1: bns_classify_text with out->lines, the writer
writes the bytes that come back) against the host formatter (BNS_LINES_GPU=0): stdout, the -b file, the -R report and the tally on
stderr byte for byte, for every input form whose text the device parses -- plain FASTQ, wrapped FASTA, a pair of files, BGZF, a pair of
BGZF files, one gzip stream, a pair of gzip files -- with and without -a, with -t, with many blocks and several contexts, and with a
tail that goes back to the host parser.  The BNS_CLI_TIMING line says which formatter ran."""
import gzip
import os
import re
import subprocess

import pytest

import synth
from test_gpu_cli import BIN, files  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

GZ = {"BNS_GZ_CHUNK_KB": 4, "BNS_GZ_RATIO_CAP": 400}           # (small texts: chunks of a few KB keep the stream on the device)


def cli(args, **env):
    e = dict(os.environ, BNS_CLI_TIMING="1")
    e.pop("BNS_LINES_GPU", None)
    e.update({k: str(v) for k, v in env.items()})
    p = subprocess.run([BIN, "classify"] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=e)
    assert p.returncode == 0, p.stderr.decode()
    return p.stdout, p.stderr.decode()


def tally_of(err):
    return [l for l in err.splitlines() if "lassified" in l and "timing" not in l]


@pytest.fixture(scope="module")
def inputs(files, tmp_path_factory):
    d = tmp_path_factory.mktemp("clilines")
    reads = files["reads"]

    def fq(tag, rs, mate):
        return b"".join(b"@%s%d_%d/%d c\n%s\n+\n%s\n" % (tag, rep, i, mate, r.tobytes(), (b"@>+I" * r.size)[:r.size]) for rep in range(6) for i, r in enumerate(rs))

    one = fq(b"m", reads[:300], 1)
    two = fq(b"m", reads[300:600], 2)
    fa = b"".join(b">fa%d_%d\n" % (rep, i) + b"\n".join(r.tobytes()[j:j + 60] for j in range(0, r.size, 60)) + b"\n" for rep in range(4) for i, r in enumerate(reads[:300]))
    p = {}
    for name, data in (("fq", one), ("fq2", two), ("fa", fa)):
        p[name] = str(d / (name + (".fa" if name == "fa" else ".fq")))
        open(p[name], "wb").write(data)
    for name, data in (("bgzf", one), ("bgzf2", two)):
        p[name] = str(d / (name + ".fq.gz"))
        synth.write_bgzf(p[name], data)
    for name, data, level in (("gz", one, 6), ("gz2", two, 9)):
        p[name] = str(d / (name + "_stream.fq.gz"))
        open(p[name], "wb").write(gzip.compress(data, compresslevel=level))
    return p


# (files, the words of the pipeline's timing line, environment that keeps small inputs on the path and cuts them into many jobs)
FORMS = {
    "fastq": (["fq"], "text on the device:", {"BNS_TEXT_BLOCK_BYTES": 50000}),
    "fasta": (["fa"], "text on the device:", {}),
    "pair": (["fq", "fq2"], "pair of files, text on the device", {"BNS_TEXT_BLOCK_BYTES": 60000}),
    "bgzf": (["bgzf"], "BGZF text on the device", {"BNS_BGZF_BATCH_MEMBERS": 3}),
    "bgzf_pair": (["bgzf", "bgzf2"], "pair of BGZF files", {"BNS_BGZF_BATCH_MEMBERS": 3}),
    "gz": (["gz"], "gzip text on the device", GZ),
    "gz_pair": (["gz", "gz2"], "pair of gzip files, text on the device", GZ),
}


def both(args, paths, words, env, tmp_path, tag, with_files=False):
    """the same run with device lines and with host lines -> its stdout; everything observable must be the same"""
    got = {}
    for mode in ("1", "0"):
        extra = []
        if with_files:
            extra = ["-b", str(tmp_path / ("%s_b%s.bin" % (tag, mode))), "-R", str(tmp_path / ("%s_r%s.txt" % (tag, mode)))]
        out, err = cli(args + extra + paths, BNS_LINES_GPU=mode, **env)
        line = [l for l in err.splitlines() if "[timing]" in l and words in l]
        assert len(line) == 1 and "host parser takes the rest" not in line[0], err
        if "-K" in args:
            assert "no Kraken lines" in line[0]
        elif mode == "1":
            m = re.search(r"lines: device formatter \((\d+) bytes from the device in (\d+) jobs, 0 jobs formatted on the host\)", line[0])
            assert m and int(m.group(1)) == len(out) and int(m.group(2)) >= 1, line[0]
        else:
            assert "lines: host formatter (0 bytes from the device in 0 jobs" in line[0], line[0]
        got[mode] = (out, tally_of(err))
        if with_files:
            got[mode] += (open(extra[1], "rb").read(), open(extra[3], "rb").read())
            assert len(got[mode][2]) > 0 and len(got[mode][3]) > 0
    assert got["1"] == got["0"], tag
    return got["1"][0]


@pytest.mark.parametrize("form", list(FORMS))
def test_device_lines_equal_host_lines(files, inputs, form, tmp_path):
    names, words, env = FORMS[form]
    paths = [inputs[n] for n in names]
    base = [files["db"], files["nodes"]]
    n_units = 1200 if form == "fasta" else 1800
    out_all = both(["-a"] + base, paths, words, env, tmp_path, form + "_a")
    assert out_all.count(b"\n") == n_units
    out_cls = both(base, paths, words, env, tmp_path, form + "_c")
    assert 0 < out_cls.count(b"\n") < n_units                     # (-a off: the unclassified units take no bytes)
    out_t = both(["-a", "-t", "0.3"] + base, paths, words, env, tmp_path, form + "_t")
    assert out_t.count(b"\n") == n_units and out_t != out_all     # (the threshold rewrote taxa: 'C' / 'U' and the taxon field follow)
    both(["-a"] + base, paths, words, env, tmp_path, form + "_files", with_files=True)
    both(["-t", "0.3"] + base, paths, words, env, tmp_path, form + "_tfiles", with_files=True)
    assert both(["-K"] + base, paths, words, env, tmp_path, form + "_K", with_files=True) == b""
    # one job for the whole input
    assert both(["-a"] + base, paths, words, {k: v for k, v in env.items() if k in GZ}, tmp_path, form + "_one") == out_all


@pytest.mark.parametrize("form,env", [("fastq", {"BNS_TEXT_BLOCK_BYTES": 3000}), ("fastq", {"BNS_TEXT_BLOCK_BYTES": 700}), ("pair", {"BNS_TEXT_BLOCK_BYTES": 5000}),
                                      ("bgzf", {"BNS_BGZF_BATCH_MEMBERS": 1}), ("bgzf_pair", {"BNS_BGZF_BATCH_MEMBERS": 1})])
@pytest.mark.parametrize("devices", ["0", "0,0,0"])
def test_many_blocks_and_contexts(files, inputs, form, env, devices, tmp_path):
    names, words, _ = FORMS[form]
    paths = [inputs[n] for n in names]
    host, _ = cli(["-a", files["db"], files["nodes"]] + paths, BNS_LINES_GPU=0)
    out = both(["-a", "-g", devices, files["db"], files["nodes"]], paths, words, env, tmp_path, "%s_%s" % (form, devices))
    assert out == host and out.count(b"\n") == 1800


def test_tail_that_goes_back_to_the_host_parser(files, tmp_path):
    """device lines for the head, the host parser's (and its formatter's) lines for the tail, in order"""
    reads = files["reads"]
    good = b"".join(b"@g%d\n%s\n+\n%s\n" % (i, r.tobytes(), b"I" * r.size) for i, r in enumerate(reads[:200]))
    tail = b"stray text\n" + b"".join(b"@s%d\n%s\n+\n%s\n" % (i, r.tobytes(), b"I" * r.size) for i, r in enumerate(reads[200:260]))
    p = str(tmp_path / "stray.fq")
    open(p, "wb").write(good + tail + good)
    ref, _ = cli(["-a", files["db"], files["nodes"], p], BNS_TEXT_GPU=0)
    assert ref.count(b"\n") == 460
    for block in (5000, 1 << 22):
        for mode in ("1", "0"):
            out, err = cli(["-a", files["db"], files["nodes"], p], BNS_TEXT_BLOCK_BYTES=block, BNS_LINES_GPU=mode)
            line = [l for l in err.splitlines() if "[timing]" in l and "text on the device:" in l]
            assert len(line) == 1 and "host parser takes the rest" in line[0], err
            m = re.search(r"lines: (\w+) formatter \((\d+) bytes from the device", line[0])
            assert m and m.group(1) == ("device" if mode == "1" else "host"), line[0]
            if mode == "1":
                # (one block for the whole file: the parse finds the stray text and takes nothing of the block -- all of it is the host parser's)
                assert (0 if block > len(good) else 1) <= int(m.group(2)) < len(out) and out.startswith(ref[:int(m.group(2))])
            assert out == ref, (block, mode)
