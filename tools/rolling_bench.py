#!/usr/bin/env python
"""The hash feeders over long reads (10 kb synthetic reads; self-consistency only, F10): RollingHasher<u64>,
RollingHasher<u128> and ntHash (Encoder::for_each_hash), the same shape each.  Kernel time from rocprofv3 --kernel-trace --stats
around this script, end-to-end time printed here (dominated by the 8 or 16 B/base copy back).
usage: rolling_bench.py [reads]"""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import bonsai_amd, oracle_lib as O
n, L = (int(sys.argv[1]) if len(sys.argv) > 1 else 20000), 10000
rng = np.random.default_rng(5)
bases = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n * L)
bases[rng.integers(0, n * L, size=n * L // 1000)] = ord("N")
offsets = np.arange(n + 1, dtype=np.uint64) * L
first = bases[:L].tobytes()
ctx = bonsai_amd.Context(0)


def leg(what, run, expect):
    run(bases[:L * 10], offsets[:11])
    t0 = time.perf_counter()
    out = run(bases, offsets)
    dt = time.perf_counter() - t0
    assert np.array_equal(out[0], expect)
    print("%s: %d x %d bp, %.2f s end to end (%.1f M bases/s), %d values" % (what, n, L, dt, n * L / dt / 1e6, sum(a.shape[0] for a in out)))


for k, canon, w in ((21, True, 0), (31, False, 0), (21, True, 50)):
    leg("u64  k %d canon %d w %d" % (k, canon, w), lambda b, o: ctx.rolling_hash(b, o, k, canon, w=w), O.rolling_hash(first, k, canon, w=w))
    leg("u128 k %d canon %d w %d" % (k, canon, w), lambda b, o: ctx.rolling_hash128(b, o, k, canon, w=w), O.rolling_hash128(first, k, canon, w=w))
for k, canon in ((21, True), (31, False)):
    leg("ntHash k %d canon %d" % (k, canon), lambda b, o: ctx.for_each_hash(b, o, k=k, canon=int(canon)), O.for_each_hash(first, k, canon))
