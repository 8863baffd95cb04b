"""bonsai_amd/csrc/bns_table_plan.hpp on the host, for the tests: tests/helpers/table_plan_harness.cpp compiled into a small
library once per process, and the table load's decisions as plain Python calls."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_NOMEM, ERR_TABLE = 0, -1, -3, -7            # include/bonsai_amd.h
DBG_PLAIN_FILL, DBG_GROUP_FILL, DBG_PLACE_FAIL, DBG_SPACED_NOCLUSTER, DBG_STREAM_LOAD = 0x10, 0x20, 0x100, 0x200, 0x1000
DBG_SPACED_M_SHIFT = 24
_LIB = None
_DIR = None


def lib():
    global _LIB, _DIR
    if _LIB is None:
        _DIR = tempfile.TemporaryDirectory(prefix="bns_plan_")
        so = os.path.join(_DIR.name, "libplan.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror",
                        os.path.join(ROOT, "tests", "helpers", "table_plan_harness.cpp"), "-o", so], check=True)
        L = C.CDLL(so)
        u32, u64, i32, dbl = C.c_uint32, C.c_uint64, C.c_int, C.c_double
        for name, res, args in (
                ("plan_constants", dbl, [C.c_void_p]),
                ("plan_minimizer_len", u32, [u32, u32, u32]),
                ("plan_size_minbucket", i32, [u64, u64, u64, u32, C.POINTER(u64), C.c_char_p]),
                ("plan_size_bucket", i32, [u64, u64, u32, C.POINTER(u32), C.c_char_p]),
                ("plan_list_spaced", u32, [u32, u64, u32, u32, i32, C.c_void_p]),
                ("plan_list_contiguous", u32, [u32, u32, i32, C.c_void_p]),
                ("plan_pick_of", u32, [u32, C.c_void_p, i32, C.c_void_p, C.POINTER(dbl)]),
                ("plan_fill", i32, [u32, dbl, u64, u64, i32, i32]),
                ("plan_ovf_slots", u64, [u64, u64, i32]),
                ("plan_sample", u32, [u64]),
                ("plan_stream", i32, [u64, u64, i32])):
            getattr(L, name).restype = res
            getattr(L, name).argtypes = args
        _LIB = L
    return _LIB


def constants():
    w = np.zeros(9, dtype=np.uint32)
    load = lib().plan_constants(w.ctypes.data)
    return {"MINB_CAP": int(w[0]), "MINB_MAX_CHAIN": int(w[1]), "PLAN_MAX_CANDS": int(w[2]),
            "MIN_CANDS": [(int(w[3 + 2 * i]), int(w[4 + 2 * i])) for i in range(3)], "MINB_TARGET_LOAD": load}


def minimizer_len(k, span, floor):
    return lib().plan_minimizer_len(k, span, floor)


def size_minbucket(n_present, free_b, n_buckets_req=0, slots_log2_req=0):
    """-> (code, home buckets or None, message)"""
    n, msg = C.c_uint64(0), C.create_string_buffer(128)
    rc = lib().plan_size_minbucket(n_present, free_b, n_buckets_req, slots_log2_req, C.byref(n), msg)
    return rc, (n.value if rc == OK else None), msg.value.decode()


def size_bucket(n_buckets, free_b, slots_log2_req=0):
    """-> (code, log2 of the table's 16-byte slots or None, message)"""
    lg, msg = C.c_uint32(0), C.create_string_buffer(128)
    rc = lib().plan_size_bucket(n_buckets, free_b, slots_log2_req, C.byref(lg), msg)
    return rc, (lg.value if rc == OK else None), msg.value.decode()


def _rows(n, out):
    return [dict(zip(("m", "len", "shift", "canon", "wide", "span"), (int(x) for x in out[6 * i:6 * i + 6]))) for i in range(n)]


def cands_spaced(k, n_present, run_len, run_shift=0, dbg=0):
    out = np.zeros(36, dtype=np.uint32)
    return _rows(lib().plan_list_spaced(k, n_present, run_len, run_shift, dbg, out.ctypes.data), out)


def cands_contiguous(k, min_span_req=0, wide_req=-1):
    out = np.zeros(36, dtype=np.uint32)
    return _rows(lib().plan_list_contiguous(k, min_span_req, wide_req, out.ctypes.data), out)


def pick(wide, counters, spaced=False):
    """wide: the candidates' identity flags in trial order; counters: (sampled, spilled, chain exhausted) per candidate
    -> (index of the winner, its miss share)"""
    w = np.ascontiguousarray(wide, dtype=np.uint32)
    tr = np.ascontiguousarray(counters, dtype=np.uint64).reshape(-1)
    assert tr.size == 3 * w.size
    miss = C.c_double(-1.0)
    i = lib().plan_pick_of(w.size, w.ctypes.data, int(spaced), tr.ctypes.data, C.byref(miss))
    return i, miss.value


def group_fill(n_cands, trial_miss, n_present, n_mb, fill_req=-1, dbg=0):
    return bool(lib().plan_fill(n_cands, trial_miss, n_present, n_mb, fill_req, dbg))


def overflow_slots(n_ovf_keys, n_alloc, dbg=0):
    return lib().plan_ovf_slots(n_ovf_keys, n_alloc, dbg)


def trial_sample(n_mb):
    return lib().plan_sample(n_mb)


def stream_load(n_buckets, free_b, dbg=0):
    return bool(lib().plan_stream(n_buckets, free_b, dbg))
