"""bonsai_amd/csrc/bns_claims.hpp on the host, for the tests: tests/helpers/claim_schedule_harness.cpp compiled into a small
library once per process, and the list of claims of a launch as the launcher and the kernel compute it."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = 31                                 # classify_chunk(1) == classify_chunk(2), bns_kernels.hpp
_LIB = None
_DIR = None


def lib():
    global _LIB, _DIR
    if _LIB is None:
        _DIR = tempfile.TemporaryDirectory(prefix="bns_claims_")
        so = os.path.join(_DIR.name, "libclaims.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror",
                        os.path.join(ROOT, "tests", "helpers", "claim_schedule_harness.cpp"), "-o", so], check=True)
        L = C.CDLL(so)
        u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
        L.claims_geometry.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, u32p, u32p, u32p]
        L.claims_geometry.restype = None
        L.claims_list.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, u64p]
        L.claims_list.restype = C.c_uint64
        L.claims_verify.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        L.claims_verify.restype = C.c_int
        _LIB = L
    return _LIB


def geometry(n, blocks):
    """-> (chunk, grid, first unit of the dynamic claims) for a batch of n units on `blocks` resident workgroups"""
    chunk, grid, dyn = C.c_uint32(), C.c_uint32(), C.c_uint32()
    lib().claims_geometry(n, blocks, FULL, C.byref(chunk), C.byref(grid), C.byref(dyn))
    return chunk.value, grid.value, dyn.value


def claims(n, blocks):
    """-> (base[], cnt[], number of static claims): the static claims by wavefront, then the dynamic ones by index"""
    cap = n // FULL + 4 * blocks + 64
    base = np.zeros(cap, dtype=np.uint32)
    cnt = np.zeros(cap, dtype=np.uint32)
    ns = C.c_uint64()
    k = lib().claims_list(n, blocks, FULL, base.ctypes.data, cnt.ctypes.data, cap, C.byref(ns))
    assert k <= cap
    return base[:k].astype(np.int64), cnt[:k].astype(np.int64), int(ns.value)


def stagger_total(waves):
    """units of the staggered static claims (1 + w mod 31 each) of `waves` wavefronts"""
    q, r = divmod(waves, FULL)
    return q * (FULL * (FULL + 1) // 2) + r * (r + 1) // 2
