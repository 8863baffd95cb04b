#!/usr/bin/env python
"""What one walk of the loaded table (bns_table_tally: the db's keys per taxon) costs: inspect_bench.py DIR [calls] [--no-model].
DIR holds bns.db + nodes.dmp as `bench.py --save-db DIR` writes them (the benchmark db: 2.25e8 keys, a 34.5 GB clustered table).
Loads the db as classify does, then times `calls` walks of each form alternately -- the upper 64 bytes of every 128-byte bucket, and
whole lines (bns_debug_set 0x80) -- with a host clock around the call (which ends in a stream synchronise and includes the scratch
allocation, the clade sums and the copies back); kernel times come from running this under `rocprofv3 --kernel-trace --stats`.  Unless
--no-model, the numpy model of tests/inspect_model.py then counts the same khash arrays on the host, chunk by chunk, confined to 16
of the process's CPUs, and the two results are compared.  One JSON line."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import bonsai_amd
from bonsai_amd import hostio
import inspect_model as M

args = [a for a in sys.argv[1:] if not a.startswith("--")]
d = args[0]
calls = int(args[1]) if len(args) > 1 else 5
db = hostio.read_db(os.path.join(d, "bns.db"))
parent = hostio.read_nodes_dmp(os.path.join(d, "nodes.dmp"))
n = parent.size
ctx = bonsai_amd.Context(0)
ctx.set_encoder(db["k"], None, canonicalize=True)
ctx.load_table(db["n_buckets"], db["flags"], db["keys"], db["vals"])
ctx.load_taxonomy(parent)
info, geo = ctx.table_info(), ctx.table_geometry()
direct, clade = ctx.table_tally()                                      # (first call: code object load)
wall = {"upper_half": [], "whole_lines": []}
for _ in range(calls):
    for name, bits in (("upper_half", 0), ("whole_lines", 0x80)):
        ctx.debug_set(bits)
        t0 = time.perf_counter()
        dd, cc = ctx.table_tally()
        wall[name].append(round((time.perf_counter() - t0) * 1e3, 3))
        assert np.array_equal(dd, direct) and np.array_equal(cc, clade)
ctx.debug_set(0)
rec = {"n_keys": info["n_keys"], "table_bytes": info["device_bytes"], "buckets": geo["buckets"], "window": geo["span"],
       "overflow_keys": geo["overflow_keys"], "taxonomy_n": int(n), "bins_with_keys": int(np.count_nonzero(direct)),
       "sum_direct": int(direct.sum()), "call_wall_ms": wall}
if "--no-model" not in sys.argv:
    os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:16])
    t0 = time.perf_counter()
    want = np.zeros(n + 1, dtype=np.uint64)
    CH = 1 << 24
    for o in range(0, db["n_buckets"], CH):
        cn = min(CH, db["n_buckets"] - o)
        pres = M.present_mask(db["flags"][o >> 4:(o + cn + 15) >> 4], cn)
        want += np.bincount(M.tally_bins(db["vals"][o:o + cn][pres], parent), minlength=n + 1).astype(np.uint64)
    want_clade = M.clade_sums(want, parent)
    rec["numpy_model_wall_s"] = round(time.perf_counter() - t0, 3)
    rec["cpus"] = len(os.sched_getaffinity(0))
    rec["equal_to_model"] = bool(np.array_equal(want, direct) and np.array_equal(want_clade, clade))
print(json.dumps(rec), flush=True)
ctx.close()
