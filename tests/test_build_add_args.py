"""`bonsai build -A old.db`: k, w and the spacing come from the file, and a -k, -w or -S that disagrees is an error named before any
device is opened -- so it is the same error on a machine without a GPU (CPU tier)."""
import os
import subprocess

import numpy as np
import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bonsai_amd", "bin", "bonsai")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from bonsai_amd import hostio
    d = tmp_path_factory.mktemp("add_args")
    db = str(d / "old.db")
    # k = 31, w = 50, contiguous; an empty khash of 4 buckets
    hostio.write_db(db, 31, 50, None, [4, 0, 0, 3], np.full(1, 0xAAAAAAAA, dtype=np.uint32), np.zeros(4, dtype=np.uint64),
                    np.zeros(4, dtype=np.uint32))
    got = hostio.read_db(db)
    assert (got["k"], got["w"], got["n_buckets"]) == (31, 50, 4)
    nodes = str(d / "nodes.dmp")
    synth.write_nodes_dmp(nodes)
    names = str(d / "nameidmap.txt")
    with open(names, "w") as f:
        f.write("NC_1.1\t%d\n" % synth.TAX_PAIRS[-1][0])
    fa = str(d / "g.fna")
    with open(fa, "wb") as f:
        f.write(b">NC_1.1 one\n" + synth.rand_seq(np.random.default_rng(1), 200).tobytes() + b"\n")
    return {"db": db, "nodes": nodes, "names": names, "fa": fa, "out": str(d / "out.db")}


def build(files, flags):
    assert os.path.exists(BIN), "bonsai CLI not built (run __graft_entry__.build())"
    return subprocess.run([BIN, "build", "-A", files["db"], "-T", files["nodes"], "-M", files["names"]] + flags +
                          [files["out"], "unused", files["fa"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("flags,named", [(["-k", "21"], ("21", "31")), (["-w", "40"], ("40", "50")),
                                         (["-k", "31", "-w", "40", "-e"], ("40", "50")),
                                         (["-S", "1x15,0x15"], ("1x15,0x15", "0,0,0"))])
def test_add_mismatch_is_refused_before_the_device(files, flags, named):
    pr = build(files, flags)
    err = pr.stderr.decode()
    assert pr.returncode != 0, err
    line = [l for l in err.splitlines() if l.startswith("[E]")]
    assert len(line) == 1 and "disagrees" in line[0] and "old.db" in line[0], err
    assert all(n in line[0] for n in named), err
    assert "GPU" not in err and "bns_create" not in err                     # (nothing was asked of a device)
    assert not os.path.exists(files["out"])


def test_add_missing_db_is_an_error(files, tmp_path):
    pr = subprocess.run([BIN, "build", "-A", str(tmp_path / "nope.db"), "-T", files["nodes"], "-M", files["names"], files["out"], "unused",
                         files["fa"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert pr.returncode != 0 and b"[E]" in pr.stderr
    assert not os.path.exists(files["out"])


def test_usage_names_the_new_flags():
    pr = subprocess.run([BIN, "build", "-h", "x", "y", "z"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    err = pr.stderr.decode()
    assert pr.returncode != 0 and "-A:" in err and "-B:" in err and "repeat them" in err
