"""CPU tier: the two columns `bonsai classify -R -u -d` puts behind the distinct k-mer column (the clade's key count in the db and
distinct / db keys), through libbns_host's formatter, and the model of bns_table_tally (tests/inspect_model.py) on hand-made tables."""
import os
import subprocess

import numpy as np
import pytest

import inspect_model
import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hostio():
    from bonsai_amd.build import build_device_library
    build_device_library()
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bonsai_amd", "csrc", "host")], check=True)
    from bonsai_amd import hostio
    return hostio


@pytest.fixture(scope="module")
def world(hostio, tmp_path_factory):
    """synth's taxonomy, a tally with every kind of line, and sketches of a few bins"""
    d = tmp_path_factory.mktemp("inspect_report")
    nodes = str(d / "nodes.dmp")
    synth.write_nodes_dmp(nodes)
    parent = hostio.read_nodes_dmp(nodes)
    n = parent.size
    direct = np.zeros(n + 1, np.uint64)
    for t, c in {0: 9, 1: 1, 11: 2, 101: 3, 1001: 40, 1002: 5, 1004: 7, 2001: 11, 2002: 4, n: 6}.items():
        direct[t] = c
    clade = inspect_model.clade_sums(direct, parent)
    rng = np.random.default_rng(4)
    bins = np.array([11, 1001, 1002, 1004, 2001, n], dtype=np.uint32)
    regs = np.zeros((bins.size, 4096), np.uint8)
    regs[0, :5] = 1                                            # a handful of k-mers
    regs[1] = rng.integers(0, 6, 4096)                         # thousands
    regs[2, 100:130] = 2
    regs[3] = rng.integers(0, 3, 4096)
    regs[4, ::7] = 1
    regs[5, 7:19] = 3                                          # bin n has a sketch of its own
    return {"parent": parent, "n": n, "direct": direct, "clade": clade, "bins": bins, "regs": regs}


def with_columns(text_u, db_keys, n):
    """the -u text with "%d\\t%.6f" of (db keys, printed distinct count / db keys) behind the distinct column of every line"""
    out = []
    for line in text_u.splitlines(True):
        f = line.split("\t")
        taxid, distinct = int(f[5]), int(f[3])
        if f[4] == "U":
            db = 0
            assert distinct == 0
        else:
            db = int(db_keys[n if taxid == 0xFFFFFFFF else taxid])
        out.append("\t".join(f[:4] + ["%d\t%.6f" % (db, distinct / db if db else 0.0)] + f[4:]))
    return "".join(out)


def test_null_column_pointer_is_the_u_text(hostio, world):
    w = world
    base = hostio.format_report(w["direct"], w["clade"], w["parent"], [], {}, w["bins"], w["regs"])
    assert base.count("\n") > 8 and all(len(ln.split("\t")) == 7 for ln in base.splitlines())
    L = hostio.lib()
    import ctypes as C
    out, ob = C.c_void_p(), C.c_uint64()
    d, c, p = (np.ascontiguousarray(x) for x in (w["direct"], w["clade"], w["parent"]))
    rc = L.bnsh_format_report_coverage(d.ctypes.data, c.ctypes.data, w["n"], p.ctypes.data, None, 0, None, None, 0,
                                       w["bins"].ctypes.data, w["regs"].ctypes.data, w["bins"].size, None, C.byref(out), C.byref(ob))
    assert rc == 0
    got = C.string_at(out.value, ob.value).decode()
    L.bnsh_free(out)
    assert got == base


def test_db_key_and_coverage_columns(hostio, world):
    w, n = world, world["n"]
    base = hostio.format_report(w["direct"], w["clade"], w["parent"], [], {}, w["bins"], w["regs"])
    distinct = {int(ln.split("\t")[5]): int(ln.split("\t")[3]) for ln in base.splitlines()}
    assert distinct[1001] > 1000 and 0 < distinct[11] and distinct[4294967295] > 0
    db = np.zeros(n + 1, np.uint64)
    db[1] = 10 ** 12                                           # a large clade: coverage near 0
    db[2] = 3 * distinct[1001]
    db[11] = db[101] = distinct[101]                           # exactly 1
    db[1001] = distinct[1001] - 100                            # an estimate above the key count: coverage above 1, not clamped
    db[1002] = 0                                               # distinct k-mers, no keys: 0.000000
    db[1004] = 7
    db[3] = db[21] = db[201] = 123456789
    db[2001] = 3
    db[n] = 5                                                  # the "(not in taxonomy)" line
    db[0] = 77                                                 # (bin 0 of the db: never printed, the unclassified line has no k-mers)
    got = hostio.format_report(w["direct"], w["clade"], w["parent"], [], {}, w["bins"], w["regs"], db_keys=db)
    want = with_columns(base, db, n)
    assert got == want
    lines = {ln.split("\t")[7]: ln.split("\t") for ln in got.splitlines()}
    assert all(len(f) == 9 for f in lines.values())
    assert lines["0"][4:6] == ["0", "0.000000"] and lines["0"][6] == "U"
    assert lines["1002"][4:6] == ["0", "0.000000"] and int(lines["1002"][3]) > 0
    assert float(lines["1001"][5]) > 1.0
    assert lines["101"][5] == "1.000000"
    assert lines["4294967295"][4] == "5" and lines["4294967295"][5] == "%.6f" % (distinct[4294967295] / 5)
    # ranks and names do not move the columns
    named = hostio.format_report(w["direct"], w["clade"], w["parent"], ["", "no rank", "phylum"], {1: "root", 1001: "Strain x"},
                                 w["bins"], w["regs"], db_keys=db)
    base_named = hostio.format_report(w["direct"], w["clade"], w["parent"], ["", "no rank", "phylum"], {1: "root", 1001: "Strain x"},
                                      w["bins"], w["regs"])
    assert named == with_columns(base_named, db, n)
    with pytest.raises(ValueError):
        hostio.format_report(w["direct"], w["clade"], w["parent"], [], {}, w["bins"], w["regs"], db_keys=db[:-1])
    with pytest.raises(ValueError):                                # the columns follow the distinct one: not without sketches
        hostio.format_report(w["direct"], w["clade"], w["parent"], [], {}, db_keys=db)


def test_model_on_a_hand_made_table():
    """the expectation itself: flag pairs, bins and subtree sums on a table small enough to count by hand"""
    parent = np.full(2003, 0xFFFFFFFF, np.uint32)
    for c, p in synth.TAX_PAIRS:
        parent[c] = 0 if c == 1 else p
    parent[1500] = 1400                                        # a key under an id that is not one: a broken chain
    nb = 32
    flags = np.full(2, 0xAAAAAAAA, np.uint32)                  # all empty
    keys = np.zeros(nb, np.uint64)
    vals = np.zeros(nb, np.uint32)
    put = {0: (0, 1001), 3: (~0 & 0xFFFFFFFFFFFFFFFF, 1001), 5: (17, 101), 16: (18, 0), 17: (19, 7777), 20: (20, 1500), 21: (21, 0xFFFFFFFF),
           22: (22, 5), 31: (23, 2)}
    for i, (k, v) in put.items():
        keys[i], vals[i] = k, v
        flags[i >> 4] &= ~np.uint32(3 << ((i & 15) << 1))
    keys[7], vals[7] = 99, 1002                                # deleted: does not count
    flags[0] = (flags[0] & ~np.uint32(3 << 14)) | np.uint32(1 << 14)
    direct, clade = inspect_model.model(flags, keys, vals, parent)
    n = 2003
    assert direct.sum() == len(put)
    assert direct[1001] == 2 and direct[101] == 1 and direct[2] == 1 and direct[0] == 1 and direct[n] == 4 and direct[1002] == 0
    assert clade[1] == 4 and clade[2] == 4 and clade[11] == 3 and clade[101] == 3 and clade[1001] == 2 and clade[3] == 0
    assert clade[0] == 1 and clade[n] == 4 and clade[1500] == 0
