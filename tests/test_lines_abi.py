"""bns_text_out / bns_text_info as ctypes sees them (bonsai_amd/_lib.py) against the header (include/bonsai_amd.h): sizes and the offset of
every field from a C snippet built with the host compiler; the fields of version 107 (the Kraken lines made on the device) sit behind
every older field, whose offsets are those of version 106 -- a caller that zero-initialises the structs keeps its behaviour."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from bonsai_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# version 106 (LP64): what callers built against the older header rely on
OLD_OUT = {"taxon": 0, "missing": 8, "ambig": 16, "n_hits": 24, "run_start": 32, "n_runs": 40, "seq_len": 48, "rec_pos": 56, "name_off": 64,
           "names": 72, "names_cap": 80, "run_tax": 88, "run_len": 96, "runs_cap": 104, "words": 112, "nmask": 120}
OLD_INFO = {"n_records": 0, "consumed": 8, "total_bases": 24, "names_bytes": 32, "n_runs_total": 40, "run_tax": 48, "run_len": 56, "status": 64,
            "why": 68, "n_slices": 72, "n_launches": 76, "ms_parse": 80, "ms_classify": 88}
NEW_OUT = ["lines", "lines_cap", "line_off", "lines_flags"]
NEW_INFO = ["lines_bytes", "ms_lines"]


def header_layout(tmp_path):
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "g++", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no host compiler")
    fields = {"bns_text_out": [n for n, _ in _lib.TextOut._fields_], "bns_text_info": [n for n, _ in _lib.TextInfo._fields_]}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "bonsai_amd.h"', 'int main(void) {']
    for st, names in fields.items():
        src.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (st, st))
        for n in names:
            src.append('    printf("%s %s %%zu\\n", offsetof(%s, %s));' % (st, n, st, n))
    src += ['    printf("BNS_LINES_ALL value %u\\n", (unsigned)BNS_LINES_ALL);', '    return 0;', '}']
    c_file = tmp_path / "layout.c"
    c_file.write_text("\n".join(src) + "\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-x", "c", "-I", os.path.join(ROOT, "include"), str(c_file), "-o", str(exe)], check=True, timeout=120)
    out = {}
    for line in subprocess.run([str(exe)], stdout=subprocess.PIPE, check=True, timeout=60).stdout.decode().splitlines():
        st, name, val = line.split()
        out.setdefault(st, {})[name] = int(val)
    return out


def test_text_structs_match_the_header(tmp_path):
    lay = header_layout(tmp_path)
    for st, cls in (("bns_text_out", _lib.TextOut), ("bns_text_info", _lib.TextInfo)):
        assert C.sizeof(cls) == lay[st].pop("sizeof"), st
        assert {n: getattr(cls, n).offset for n, _ in cls._fields_} == lay[st], st
    assert lay["BNS_LINES_ALL"]["value"] == _lib.LINES_ALL == 1


def test_new_fields_sit_behind_the_old_ones(tmp_path):
    for cls, old, new in ((_lib.TextOut, OLD_OUT, NEW_OUT), (_lib.TextInfo, OLD_INFO, NEW_INFO)):
        names = [n for n, _ in cls._fields_]
        assert names == list(old) + new                                    # same order, the new ones appended
        assert {n: getattr(cls, n).offset for n in old} == old             # nothing moved
        end_old = max(getattr(cls, n).offset + getattr(cls, n).size for n in old)
        assert all(getattr(cls, n).offset >= end_old for n in new)
    lay = header_layout(tmp_path)
    assert {n: lay["bns_text_out"][n] for n in OLD_OUT} == OLD_OUT and {n: lay["bns_text_info"][n] for n in OLD_INFO} == OLD_INFO
