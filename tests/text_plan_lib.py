"""bonsai_amd/csrc/bns_text_plan.hpp on the host, for the tests: tests/helpers/text_plan_harness.cpp compiled into a small
library once per process, and a text call's decisions as plain Python calls."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG = 0, -1                                          # include/bonsai_amd.h
DBG_SLICE_8K, DBG_BATCH_TINY = 0x4000, 0x40
STREAM_FIELDS = ("rel", "end", "j0", "n", "piece")
BYTES_FIELDS = ("ls0", "line_off0", "cand0", "ls1", "line_off1", "cand1", "seq_len", "name_off", "pos64", "names", "offsets", "words",
                "nmask", "info", "out", "lines_off", "lines_state", "hits", "runs0", "runs1", "runs2", "runs3")
FIELDS = tuple("s%d_%s" % (s, f) for s in range(2) for f in STREAM_FIELDS) + (
    "n_slices", "pieces_forced", "range_cap", "window", "cap_lines", "cap_rec", "batch_reads", "batch_bases", "batch_names",
    "slice_reads_cap", "slice_bases_cap", "carry_reads", "carry_bases", "carry_names", "cap_reads", "cap_bases", "cap_names",
    "st_tiles", "st_groups", "st_cand", "st_recs", "off_lines", "off_groups", "off_compact", "off_offsets", "info_bytes") + \
    tuple("bytes_" + f for f in BYTES_FIELDS)
assert len(FIELDS) == 58
_LIB = None
_DIR = None


def lib():
    global _LIB, _DIR
    if _LIB is None:
        _DIR = tempfile.TemporaryDirectory(prefix="bns_text_plan_")
        so = os.path.join(_DIR.name, "libtextplan.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror",
                        os.path.join(ROOT, "tests", "helpers", "text_plan_harness.cpp"), "-o", so], check=True)
        L = C.CDLL(so)
        u32, u64, i32, i64 = C.c_uint32, C.c_uint64, C.c_int, C.c_longlong
        for name, res, args in (
                ("text_constants", None, [C.c_void_p]),
                ("text_piece", u64, [i32, i64, u64]),
                ("text_tile0", u32, [u32]),
                ("text_n_tiles", u32, [u32, u32]),
                ("text_plan", i32, [C.c_void_p, C.c_void_p, C.c_char_p]),
                ("text_up_to", u32, [u32, u32, u32, u32, u64, u32]),
                ("text_piece_of", u32, [u32, u32, u32])):
            getattr(L, name).restype = res
            getattr(L, name).argtypes = args
        _LIB = L
    return _LIB


def constants():
    w = np.zeros(8, dtype=np.uint64)
    lib().text_constants(w.ctypes.data)
    return dict(zip(("TILE", "REC_BLOCK", "MAX_PIECES", "sizeof_CallInfo", "CALL_INFO_BYTES", "sizeof_StreamInfo", "DBG_SLICE_8K", "DBG_BATCH_TINY"),
                    (int(x) for x in w)))


def piece_bytes(dbg, piece_mb, nbytes):
    return int(lib().text_piece(dbg, piece_mb, nbytes))


def tile0(lo):
    return int(lib().text_tile0(lo))


def n_tiles(lo, hi):
    return int(lib().text_n_tiles(lo, hi))


def plan(sizes, rel=(0, 0), upload_piece=(0, 0), on_device=False, parse_only=False, want_runs=False, want_lines=False, want_words=False,
         dbg=0, piece_mb=0, batch_reads=0):
    """plan_text -> (code, {field: value}, message); sizes: the text bytes of one stream or of two"""
    sizes, rel, upload_piece = list(sizes), list(rel), list(upload_piece)
    a = np.array([len(sizes)] + (sizes + [0])[:2] + (rel + [0])[:2] + (upload_piece + [0])[:2] +
                 [int(on_device), int(parse_only), int(want_runs), int(want_lines), int(want_words), dbg, piece_mb, batch_reads], dtype=np.int64)
    out, msg = np.zeros(58, dtype=np.uint64), C.create_string_buffer(128)
    rc = lib().text_plan(a.ctypes.data, out.ctypes.data, msg)
    return rc, dict(zip(FIELDS, (int(x) for x in out))), msg.value.decode()


def up_to(p, s, k):
    """TextPlan::up_to of stream s of a plan() result"""
    return int(lib().text_up_to(*(p["s%d_%s" % (s, f)] for f in STREAM_FIELDS), k))


def piece_of(p, s, k):
    return int(lib().text_piece_of(p["s%d_j0" % s], p["s%d_n" % s], k))
