#!/usr/bin/env python
"""What the minimum base quality costs on the text path: bns_classify_text on FASTQ text in page-locked host memory (the default path of
`bonsai classify`: the text travels in 64 MiB pieces while the pieces in front are parsed, packed and classified), with
  (a) q = 0 on this tree's library against the same call on ANOTHER build of the library (--parent-lib: the commit in front of the
      feature, whose pack_text_kernel the q = 0 instantiation is meant to be), and
  (b) q = 20 against q = 0 on this tree's library
-- the legs interleaved round by round in ONE process (both libraries loaded side by side, a context each on device 0), medians and
ranges of the call's wall time, reads/s, and the device time of the parse kernels (count .. pack, HIP events) per slice.
usage: minq_bench.py [n_reads (6000000)] [--parent-lib path/to/libbonsai_amd.so] [--rounds 7] [--q 20]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

vp, u32p, u64p = C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)


class Lib:
    """the few entry points the measurement needs, from any build of the library (one that predates bns_set_min_base_quality included)"""
    def __init__(self, path, world):
        from bonsai_amd import _lib
        self.path = path
        L = self.L = C.CDLL(path)
        L.bns_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.bns_destroy.argtypes = [vp]; L.bns_destroy.restype = None
        L.bns_set_encoder.argtypes = [vp, C.c_uint32, vp, C.c_int, C.c_int]
        L.bns_load_table.argtypes = [vp, C.c_uint64, u32p, u64p, u32p, C.c_int]
        L.bns_load_taxonomy.argtypes = [vp, u32p, C.c_uint32]
        L.bns_set_timing.argtypes = [vp, C.c_int]
        L.bns_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        L.bns_classify_text.argtypes = [vp, C.POINTER(vp), u64p, C.c_int, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(_lib.TextOut), C.POINTER(_lib.TextInfo)]
        L.bns_last_error.argtypes = [vp]; L.bns_last_error.restype = C.c_char_p
        self.version = L.bns_version()
        self.h = vp()
        self.chk(L.bns_create(0, C.byref(self.h)), "bns_create")
        w = world
        self.chk(L.bns_set_encoder(self.h, 31, None, 1, 1), "bns_set_encoder")
        self.chk(L.bns_load_table(self.h, w.n_buckets, w.flags.ctypes.data_as(u32p), w.keys.ctypes.data_as(u64p), w.vals.ctypes.data_as(u32p), 2), "bns_load_table")
        par = np.ascontiguousarray(w.parent, dtype=np.uint32)
        self.chk(L.bns_load_taxonomy(self.h, par.ctypes.data_as(u32p), par.size), "bns_load_taxonomy")
        self.chk(L.bns_set_timing(self.h, 1), "bns_set_timing")

    def chk(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s (%s): %d %s" % (what, self.path, rc, (self.L.bns_last_error(self.h) or b"").decode()))

    def set_q(self, q):
        if q or hasattr(self.L, "bns_set_min_base_quality"):
            self.L.bns_set_min_base_quality.argtypes = [vp, C.c_uint32]
            self.chk(self.L.bns_set_min_base_quality(self.h, q), "bns_set_min_base_quality")

    def pinned(self, nbytes, dtype):
        p = vp()
        self.chk(self.L.bns_host_alloc(self.h, nbytes, C.byref(p)), "bns_host_alloc")
        return p, np.frombuffer((C.c_uint8 * nbytes).from_address(p.value), dtype=dtype)


def make_text(lib, world, n, rng):
    """"@r<9 digits>\\n" + 150 bases + "\\n+\\n" + 150 quality bytes + "\\n" = 316 bytes per record (tools/text_bench.py's text), in page-locked
    memory; quality: Phred 30 .. 40 with 2 % of the bases at Phred 2 .. 15 (rows drawn from 65536 patterns)"""
    g = np.concatenate(list(world.genomes.values()))
    p, text = lib.pinned(316 * n + 64, np.uint8)
    rec = text[:316 * n].reshape(n, 316)
    pat = rng.integers(33 + 30, 33 + 41, size=(65536, 150)).astype(np.uint8)
    low = rng.random(pat.shape) < 0.02
    pat[low] = rng.integers(33 + 2, 33 + 16, size=int(low.sum())).astype(np.uint8)
    step = 1 << 20
    for a in range(0, n, step):                                      # (in parts: the index arrays of 6 M reads at once are 7 GB)
        b = min(n, a + step)
        r = rec[a:b]
        idx = np.arange(a, b)
        r[:, 0] = ord("@"); r[:, 1] = ord("r")
        for d in range(9):
            r[:, 2 + d] = ord("0") + (idx // 10 ** (8 - d)) % 10
        r[:, 11] = 10
        st = rng.integers(0, g.size - 150, size=b - a)
        r[:, 12:162] = g[st[:, None] + np.arange(150)[None, :]]
        r[:, 162] = 10; r[:, 163] = ord("+"); r[:, 164] = 10
        r[:, 165:315] = pat[rng.integers(0, 65536, size=b - a)]
        r[:, 315] = 10
    return p, text, 316 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_reads", nargs="?", type=int, default=6_000_000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--q", type=int, default=20)
    a = ap.parse_args()
    from bonsai_amd import _lib
    import oracle_lib as O
    import synth
    n = a.n_reads
    w = synth.make_world(O, seed=3, k=31, genome_len=20000)
    new = Lib(_lib.SO, w)
    parent = Lib(os.path.abspath(a.parent_lib), w) if a.parent_lib else None
    p_text, text, nbytes = make_text(new, w, n, np.random.default_rng(1))
    cap = n + 16
    taxon = {l: l.pinned(4 * cap, np.uint32) for l in (new, parent) if l}
    ptrs = (vp * 1)(p_text)
    sizes = np.array([nbytes], dtype=np.uint64)

    def call(lib, q):
        lib.set_q(q)
        o = _lib.TextOut()
        o.taxon = taxon[lib][0].value
        info = _lib.TextInfo()
        t0 = time.perf_counter()
        rc = lib.L.bns_classify_text(lib.h, ptrs, sizes.ctypes.data_as(u64p), 1, 0xFFFFFFFFFFFFFFFF, _lib.TEXT_FINAL | _lib.TEXT_TRIM_READNO, cap, C.byref(o), C.byref(info))
        dt = time.perf_counter() - t0
        lib.chk(rc, "bns_classify_text")
        assert info.status == 0 and info.n_records == n, (info.status, info.why, info.n_records)
        return {"call_s": dt, "ms_parse": float(info.ms_parse), "n_slices": int(info.n_slices), "ms_classify": float(info.ms_classify)}

    legs = {"new_q0": (new, 0), "new_q%d" % a.q: (new, a.q)}
    if parent:
        legs = dict({"parent_q0": (parent, 0)}, **legs)
    for name, (lib, q) in legs.items():                              # (the first call of a context sizes its workspaces)
        call(lib, q)
    runs = {name: [] for name in legs}
    for _ in range(a.rounds):
        for name, (lib, q) in legs.items():
            runs[name].append(call(lib, q))
    # the masked call did mask, the unmasked calls agree
    call(new, 0); t0 = taxon[new][1][:n].copy()
    call(new, a.q); tq = taxon[new][1][:n].copy()
    same_as_parent = None
    if parent:
        call(parent, 0)
        same_as_parent = bool(np.array_equal(taxon[parent][1][:n], t0))
    new.set_q(0)

    def summary(rs):
        cs = sorted(r["call_s"] for r in rs)
        us = sorted(1e3 * r["ms_parse"] / r["n_slices"] for r in rs)
        return {"call_s": {"median": statistics.median(cs), "min": cs[0], "max": cs[-1]},
                "reads_per_s": {"median": n / statistics.median(cs), "min": n / cs[-1], "max": n / cs[0]},
                "parse_us_per_slice": {"median": statistics.median(us), "min": us[0], "max": us[-1]},
                "n_slices": rs[0]["n_slices"], "ms_classify_median": statistics.median(r["ms_classify"] for r in rs)}
    out = {"entry": "bns_classify_text, FASTQ text in page-locked memory", "reads": n, "text_bytes": nbytes, "rounds": a.rounds, "q": a.q,
           "slice_bytes": 64 << 20, "versions": {"new": new.version, "parent": parent.version if parent else None},
           "legs": {name: summary(rs) for name, rs in runs.items()},
           "units_whose_taxon_the_mask_changes": int(np.count_nonzero(t0 != tq)), "classified_q0": int(np.count_nonzero(t0)), "classified_q": int(np.count_nonzero(tq)),
           "parent_q0_equals_new_q0": same_as_parent}
    if parent:
        out["a_new_q0_median_not_above_parents_slowest"] = out["legs"]["new_q0"]["call_s"]["median"] <= out["legs"]["parent_q0"]["call_s"]["max"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
