"""Why does the two-round probe (probe_minbucket2) take a later pass?  On a -DBNS_COUNT_FETCHES build g_fetch_count[5..7] count
the later passes by cause: run leaders ranked beyond the stage, lanes that walk on down their chains, both.  bench.py reads the
counters once at the end of its timed loop (bns_debug_fetch_count reads and clears all eight) and reports slots 0..4 only; this
runs bench.py in-process and taps that one call for the rest.
usage (GPU box):  BONSAI_AMD_LIB=$PWD/bonsai_amd/lib/libbonsai_amd_count.so python tools/pass_causes.py [bench.py arguments]
(default arguments: --no-cpu --no-probe --no-text --no-inflate --steps 4 --warmup 1)"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import bonsai_amd  # noqa: E402

args = sys.argv[1:] or ["--no-cpu", "--no-probe", "--no-text", "--no-inflate", "--steps", "4", "--warmup", "1"]
sys.argv = ["bench.py"] + args
L = bonsai_amd.load()
if not hasattr(L, "bns_debug_fetch_count"):
    sys.exit("pass_causes.py: the library was not built with -DBNS_COUNT_FETCHES")
real = L.bns_debug_fetch_count
real.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
seen = []


def tap(h, out8):
    rc = real(h, out8)
    seen.append([int(x) for x in out8])
    return rc


L.bns_debug_fetch_count = tap
a = bench.parse()
rc = bench.main()
if len(seen) != 1:                                       # (the tap stands or falls with bench.py reading the counters once, through this library object)
    sys.exit("pass_causes.py: bench.py read the counters %d times, not once: the figures below would not cover the whole run" % len(seen))
c = seen[-1]
reads = float(a.reads) * (a.steps + a.warmup) / (2 if a.paired else 1)
print("per unit: %.3f bucket fetches in %.4f probe passes; later passes of the two-round probe: %.4f for runs beyond the stage, "
      "%.4f for chain walks, %.4f for both (%.4f in all); lanes sent to the overflow table %.5f"
      % (c[0] / reads, c[1] / reads, c[5] / reads, c[6] / reads, c[7] / reads, (c[5] + c[6] + c[7]) / reads, c[2] / reads))
sys.exit(rc or 0)
