"""CPU tier: the taxon report of `bonsai classify -R` (bns::format_report, the nodes.dmp rank reader and the names.dmp reader in
libbns_host), on a hand-written taxonomy whose report is written out below byte for byte."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (taxid, parent, rank, scientific name or None)
NODES = [
    (1, 1, "no rank", "root"),
    (131567, 1, "no rank", "cellular organisms"),
    (2, 131567, "superkingdom", "Bacteria"),
    (1224, 2, "phylum", "Pseudomonadota"),
    (1117, 2, "phylum", "Cyanobacteriota"),
    (1236, 1224, "class", "Gammaproteobacteria"),
    (999, 1236, "no rank", "Enterobacterales group"),
    (91347, 999, "order", "Enterobacterales"),
    (543, 91347, "family", "Enterobacteriaceae"),
    (620, 543, "genus", "Shigella"),
    (561, 543, "genus", "Escherichia"),
    (564, 561, "species", "Escherichia fergusonii"),
    (562, 561, "species", "Escherichia coli"),
    (83333, 562, "strain", "Escherichia coli K-12"),
    (10239, 0, "superkingdom", None),
    (12000, 10239, "species", "Example virus"),
]
DIRECT = {1: 2, 2: 3, 1117: 1, 1236: 1, 561: 4, 562: 5, 83333: 2, 564: 7, 10239: 1, 12000: 6}
UNCLASSIFIED, NOT_IN_TAX = 10, 3
CLADE = {1: 25, 131567: 23, 2: 23, 1224: 19, 1117: 1, 1236: 19, 999: 18, 91347: 18, 543: 18, 561: 18, 562: 7, 83333: 2,
         564: 7, 10239: 7, 12000: 6}

# 45 units in all.  The two species tie at 7 (562 before 564), Shigella counts nothing, 1117 has the smaller taxid but the smaller clade.
EXPECTED = (
    " 22.22\t10\t10\tU\t0\tunclassified\n"
    " 55.56\t25\t2\tR\t1\troot\n"
    " 51.11\t23\t0\tR1\t131567\t  cellular organisms\n"
    " 51.11\t23\t3\tD\t2\t    Bacteria\n"
    " 42.22\t19\t0\tP\t1224\t      Pseudomonadota\n"
    " 42.22\t19\t1\tC\t1236\t        Gammaproteobacteria\n"
    " 40.00\t18\t0\tC1\t999\t          Enterobacterales group\n"
    " 40.00\t18\t0\tO\t91347\t            Enterobacterales\n"
    " 40.00\t18\t0\tF\t543\t              Enterobacteriaceae\n"
    " 40.00\t18\t4\tG\t561\t                Escherichia\n"
    " 15.56\t7\t5\tS\t562\t                  Escherichia coli\n"
    "  4.44\t2\t2\tS1\t83333\t                    Escherichia coli K-12\n"
    " 15.56\t7\t7\tS\t564\t                  Escherichia fergusonii\n"
    "  2.22\t1\t1\tP\t1117\t      Cyanobacteriota\n"
    " 15.56\t7\t1\tD\t10239\t10239\n"
    " 13.33\t6\t6\tS\t12000\t  Example virus\n"
    "  6.67\t3\t3\t-\t4294967295\t(not in taxonomy)\n"
)


@pytest.fixture(scope="module")
def hostio():
    from bonsai_amd.build import build_device_library
    build_device_library()
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bonsai_amd", "csrc", "host")], check=True)
    from bonsai_amd import hostio
    return hostio


def write_dmps(d):
    nodes, names = str(d / "nodes.dmp"), str(d / "names.dmp")
    with open(nodes, "w") as f:
        for t, p, r, _ in NODES:
            f.write("%d\t|\t%d\t|\t%s\t|\t\t|\n" % (t, p, r))
    with open(names, "w") as f:
        for t, _, _, nm in NODES:
            if nm is not None:
                f.write("%d\t|\t%s\t|\t\t|\tscientific name\t|\n" % (t, nm))
        f.write("562\t|\tBacillus coli\t|\t\t|\tsynonym\t|\n")
        f.write("10239\t|\tViruses\t|\t\t|\tgenbank common name\t|\n")
    return nodes, names


def test_report_hand_written_taxonomy(hostio, tmp_path):
    nodes, names = write_dmps(tmp_path)
    parent = hostio.read_nodes_dmp(nodes)
    n = parent.size
    assert n == 131568
    direct = np.zeros(n + 1, np.uint64)
    clade = np.zeros(n + 1, np.uint64)
    for t, c in DIRECT.items():
        direct[t] = c
    for t, c in CLADE.items():
        clade[t] = c
    direct[0] = clade[0] = UNCLASSIFIED
    direct[n] = clade[n] = NOT_IN_TAX
    got = hostio.format_report(direct, clade, parent, hostio.read_node_ranks(nodes), hostio.read_scientific_names(names))
    assert got == EXPECTED
    # without names every taxon is its id; nothing counted, nothing printed
    plain = hostio.format_report(direct, clade, parent, hostio.read_node_ranks(nodes), {})
    assert plain.splitlines()[2] == " 51.11\t23\t0\tR1\t131567\t  131567"
    assert plain.splitlines()[0].endswith("\tunclassified") and plain.splitlines()[-1].endswith("\t(not in taxonomy)")
    assert hostio.format_report(np.zeros(n + 1), np.zeros(n + 1), parent, [], {}) == ""
    # no unclassified / not-in-taxonomy units: neither line
    direct[0] = clade[0] = direct[n] = clade[n] = 0
    lines = hostio.format_report(direct, clade, parent, hostio.read_node_ranks(nodes), {}).splitlines()
    assert lines[0].startswith(" 78.12\t25\t2\tR\t1\t") and lines[-1].endswith("\t  12000")


def test_rank_reader(hostio, tmp_path):
    p = tmp_path / "nodes.dmp"
    p.write_text("#comment\n\n1\t|\t1\t|\tno rank\t|\t\t|\n3\t|\t1\t|\tgenus\t|\n7\t|\t3\t|\n8\t|\t3\n"
                 "9\t|\t3\t|\tspecies\r\n5\t|\t3\t|\tspecies\t|\n5\t|\t3\t|\tsubspecies\t|\n")
    r = hostio.read_node_ranks(str(p))
    assert len(r) == 10
    assert r[1] == "no rank" and r[3] == "genus" and r[9] == "species" and r[5] == "subspecies"   # (later lines win)
    assert r[7] == "no rank" and r[8] == "no rank"            # lines without a rank field
    assert r[0] == "" and r[2] == "" and r[4] == "" and r[6] == ""   # ids without a line
    with pytest.raises(hostio.HostIOError):
        hostio.read_node_ranks(str(tmp_path / "missing.dmp"))


def test_names_reader(hostio, tmp_path):
    _, names = write_dmps(tmp_path)
    got = hostio.read_scientific_names(names)
    assert got == {t: nm for t, _, _, nm in NODES if nm is not None}
    assert 10239 not in got and got[562] == "Escherichia coli"
    with pytest.raises(hostio.HostIOError):
        hostio.read_scientific_names(str(tmp_path / "missing.dmp"))
