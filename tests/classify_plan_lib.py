"""bonsai_amd/csrc/bns_classify_plan.hpp on the host, for the tests: tests/helpers/classify_plan_harness.cpp compiled into a small
library once per process, and the classify launch's decisions as plain Python calls."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
_DIR = None


def lib():
    global _LIB, _DIR
    if _LIB is None:
        _DIR = tempfile.TemporaryDirectory(prefix="bns_cplan_")
        so = os.path.join(_DIR.name, "libcplan.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror",
                        os.path.join(ROOT, "tests", "helpers", "classify_plan_harness.cpp"), "-o", so], check=True)
        L = C.CDLL(so)
        u32, u64, i32 = C.c_uint32, C.c_uint64, C.c_int
        for name, res, args in (
                ("cplan_constants", None, [C.c_void_p]),
                ("cplan_choose", None, [u32, u32, i32, i32, i32, i32, i32, i32, i32, C.c_void_p]),
                ("cplan_choose_overflow", None, [i32, i32, i32, i32, C.c_void_p]),
                ("cplan_forms", i32, [C.c_void_p, i32]),
                ("cplan_overflow_forms", i32, [C.c_void_p, i32]),
                ("cplan_ovf_heavy", i32, [i32, u64, u64]),
                ("cplan_max_unit_kmers", u64, [i32, u32, u32]),
                ("cplan_can_overflow", i32, [i32, u32, u32]),
                ("cplan_too_many_units", i32, [u64]),
                ("cplan_win_scratch", u64, [i32, i32, i32, u32, u32, C.c_uint])):
            getattr(L, name).restype = res
            getattr(L, name).argtypes = args
        _LIB = L
    return _LIB


def constants():
    w = np.zeros(4, dtype=np.uint64)
    lib().cplan_constants(w.ctypes.data)
    return {"LDS_CAP": int(w[0]), "DBG_OVC_OFF": int(w[1]), "DBG_OVC_ON": int(w[2]), "MAX_CLASSIFY_UNITS": int(w[3])}


def choose_form(k, m, canon, spaced, layout, table_wide, heavy, packed, nmates):
    """-> (SPACED, LAYOUT, KT, NM, SPAN, OVC, WIDE, PACKED)"""
    out = np.full(8, -1, dtype=np.int32)
    lib().cplan_choose(k, m, int(canon), int(spaced), layout, int(table_wide), int(heavy), int(packed), nmates, out.ctypes.data)
    return tuple(int(x) for x in out)


def choose_overflow_form(spaced, layout, table_wide, packed):
    """-> (SPACED, LAYOUT, WIDE, PACKED)"""
    out = np.full(4, -1, dtype=np.int32)
    lib().cplan_choose_overflow(int(spaced), layout, int(table_wide), int(packed), out.ctypes.data)
    return tuple(int(x) for x in out)


def _rows(fn, width):
    n = fn(None, 0)
    out = np.full(n * width, -1, dtype=np.int32)
    assert fn(out.ctypes.data, n) == n
    return [tuple(int(x) for x in out[width * i:width * (i + 1)]) for i in range(n)]


def forms():
    """the header's list of classify_kernel forms, in its order"""
    return _rows(lib().cplan_forms, 8)


def overflow_forms():
    return _rows(lib().cplan_overflow_forms, 4)


def ovf_heavy(dbg, n_ovf_keys, n_keys):
    return bool(lib().cplan_ovf_heavy(dbg, n_ovf_keys, n_keys))


def max_unit_kmers(nmates, max_read_len, c):
    return lib().cplan_max_unit_kmers(nmates, max_read_len, c)


def can_overflow(nmates, max_read_len, c):
    return bool(lib().cplan_can_overflow(nmates, max_read_len, c))


def too_many_units(n_units):
    return bool(lib().cplan_too_many_units(n_units))


def win_scratch_bytes(spaced, canon, score, win, c, grid):
    return lib().cplan_win_scratch(int(spaced), int(canon), score, win, c, grid)
