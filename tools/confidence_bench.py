#!/usr/bin/env python
"""What `bonsai classify -t` (the confidence threshold, walked on the device) costs: confidence_bench.py [n_reads] [dir] [pairs] [theta].
The FASTQ of tools/make_fastq.py against its db; runs with and without -t alternate in two modes -- `-K -b` (no Kraken lines: the
classify kernel writes the hit stream into the context's own buffer for the walk) and Kraken lines to /dev/null (the walk reads the
stream the lines are made of) -- and the medians of the process_dataset stage are compared.  One JSON line per run, then a summary
line per mode."""
import json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
n = int(sys.argv[1]) if len(sys.argv) > 1 else 16_000_000
d = sys.argv[2] if len(sys.argv) > 2 else "/tmp/confbench"
pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
theta = sys.argv[4] if len(sys.argv) > 4 else "0.1"
os.makedirs(d, exist_ok=True)
fq = os.path.join(d, "r.fq")
subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_fastq.py"), str(n), fq], check=True)
BIN = os.path.join(ROOT, "bonsai_amd", "bin", "bonsai")
MODES = {"K": ["-K", "-b", os.path.join(d, "tax.bin")], "lines": []}


def run(mode, with_t):
    args = [BIN, "classify", "-p", "4"] + MODES[mode] + (["-t", theta] if with_t else [])
    p = subprocess.run(args + [os.path.join(d, "bns.db"), os.path.join(d, "nodes.dmp"), fq], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                       env=dict(os.environ, BNS_CLI_TIMING="1"), timeout=900)
    err = p.stderr.decode()
    if p.returncode != 0:
        sys.exit("bonsai classify failed:\n" + err)
    rec = {"mode": mode, "t": theta if with_t else None}
    for l in err.splitlines():
        if l.startswith("[timing] process_dataset"):
            rec["process_dataset_s"] = float(l.split()[2])
        if l.startswith("Classified"):
            rec["classified"] = int(l.split()[1].rstrip(","))
    print(json.dumps(rec), flush=True)
    return rec


for mode in MODES:
    run(mode, False)                                              # (page cache, first-touch of the db)
    recs = []
    for _ in range(pairs):
        recs.append(run(mode, False))
        recs.append(run(mode, True))
    p0 = statistics.median(r["process_dataset_s"] for r in recs if r["t"] is None)
    p1 = statistics.median(r["process_dataset_s"] for r in recs if r["t"] is not None)
    print(json.dumps({"mode": mode, "n_reads": n, "pairs": pairs, "t": theta, "median_process_dataset_s": [p0, p1],
                      "process_dataset_overhead_pct": round(100 * (p1 - p0) / p0, 2),
                      "classified": [recs[0]["classified"], recs[1]["classified"]]}), flush=True)
