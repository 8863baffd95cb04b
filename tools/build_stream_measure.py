#!/usr/bin/env python3
"""Times `bonsai build -k31 -w50 -e` over the set of tools/build_stream_set.py: wall time, peak resident set (the ru_maxrss that wait4
reports for the child, what `/usr/bin/time -v` prints as "Maximum resident set size") and the stderr lines of BNS_CLI_TIMING=1.

    python tools/build_stream_measure.py BONSAI_BINARY SETDIR RUNS [more build flags, e.g. -B 200000]"""
import os
import subprocess
import sys
import time


def main():
    binary, setdir, runs = sys.argv[1], sys.argv[2], int(sys.argv[3])
    extra = sys.argv[4:]
    out = os.path.join(setdir, "measure.db")
    cmd = [binary, "build", "-k", "31", "-w", "50", "-e", "-T", os.path.join(setdir, "nodes.dmp"), "-M", os.path.join(setdir, "nameidmap.txt"),
           "-F", os.path.join(setdir, "paths.txt")] + extra + [out, "unused"]
    print("$ BNS_CLI_TIMING=1 " + " ".join(cmd))
    walls, rss = [], []
    for r in range(runs):
        t0 = time.time()
        p = subprocess.Popen(cmd, stderr=subprocess.PIPE, env=dict(os.environ, BNS_CLI_TIMING="1"))
        err = p.stderr.read().decode()
        _, status, ru = os.wait4(p.pid, 0)
        wall = time.time() - t0
        p.returncode = os.waitstatus_to_exitcode(status)
        keep = [l for l in err.splitlines() if l.startswith(("build:", "[timing]", "Wrote", "[E]"))]
        print("run %d: wall %.2f s, peak RSS %.0f MiB, exit %d, db %d bytes | %s" % (r, wall, ru.ru_maxrss / 1024.0, p.returncode,
              os.path.getsize(out) if os.path.exists(out) else -1, " | ".join(keep)))
        sys.stdout.flush()
        if p.returncode != 0:
            sys.exit(1)
        walls.append(wall); rss.append(ru.ru_maxrss / 1024.0)
    print("wall: min %.2f  median %.2f  max %.2f s; peak RSS: median %.0f MiB" % (min(walls), sorted(walls)[len(walls) // 2], max(walls),
          sorted(rss)[len(rss) // 2]))


if __name__ == "__main__":
    main()
