"""The text of `bonsai distrib` through the host C API (bns::format_distrib: no device), on hand-made pairs; the ABI version; and the
Python binding's copies of the window session's constants against the device source."""
import os
import re

import numpy as np

import windows_model as WM
from bonsai_amd import _lib, hostio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "mapped_taxid\tgenome_taxids:kmers_mapped:total_genome_kmers\n"


def fmt(pairs, path=None):
    s, t, n = (np.array([p[i] for p in pairs], dtype=d) for i, d in enumerate((np.uint32, np.uint32, np.uint64)))
    return hostio.format_distrib(s, t, n, path=path)


def test_ordering_totals_and_the_omitted_zero_line():
    # (genome taxid, called, windows), ascending as bns_windows_read returns them
    pairs = [(7, 0, 5), (7, 1, 10), (7, 7, 100), (7, 4000000000, 2), (9, 1, 3), (9, 9, 40), (12, 0, 8), (1000, 7, 1), (1000, 1000, 50)]
    want = (HEADER +
            "1\t7:10:117 9:3:43\n"
            "7\t7:100:117 1000:1:51\n"
            "9\t9:40:43\n"
            "1000\t1000:50:51\n"
            "4000000000\t7:2:117\n")
    assert fmt(pairs) == want                      # no line for 0; the totals count the windows called 0; genome 12 (all 0) is nowhere
    assert fmt(pairs[::-1]) == want                # the order of the lines is the text's own, not the input's
    assert fmt(pairs) == WM.distrib_text(*(np.array([p[i] for p in pairs], dtype=np.uint64) for i in range(3))).decode()


def test_counts_beyond_32_bits_and_equal_pairs():
    assert fmt([(3, 5, 1 << 40), (3, 5, 2), (3, 0, 1)]) == HEADER + "5\t3:%d:%d\n" % ((1 << 40) + 2, (1 << 40) + 3)


def test_empty_input_is_the_header_alone(tmp_path):
    assert fmt([]) == HEADER
    p = tmp_path / "empty.txt"
    assert fmt([], path=p) == HEADER and p.read_bytes() == HEADER.encode()


def test_written_to_a_path(tmp_path):
    p = tmp_path / "d.txt"
    text = fmt([(2, 2, 4), (2, 3, 1)], path=p)
    assert text == HEADER + "2\t2:4:5\n3\t2:1:5\n" and p.read_bytes() == text.encode()


def test_abi_version_and_signatures():
    lib = _lib.load()
    assert lib.bns_version() >= 110
    for name in ("bns_windows_begin", "bns_windows_add", "bns_windows_read", "bns_windows_end"):
        assert name in lib._bns_signatures and hasattr(lib, name)


def test_python_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "bonsai_amd", "csrc", "bns_windows.hpp")).read()
    assert int(re.search(r"constexpr u32 WIN_TILE = (\d+);", src).group(1)) == _lib.WINDOWS_TILE
    assert int(re.search(r"constexpr u32 WIN_FAST_TAXA = (\d+);", src).group(1)) == _lib.WINDOWS_FAST_TAXA
    assert int(re.search(r"constexpr u32 WIN_LDS_LIST_MAX = (\d+);", src).group(1)) == _lib.WINDOWS_LDS_LIST
