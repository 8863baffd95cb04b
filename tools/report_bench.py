#!/usr/bin/env python
"""What `bonsai classify -R` (the taxon report, tallied on the device) costs on top of a -K run: report_bench.py [n_reads] [dir] [pairs].
The FASTQ of tools/make_fastq.py against its db; runs with and without -R alternate, the medians of wall time and of the process_dataset
stage are compared.  One JSON line per run, then a summary line."""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
n = int(sys.argv[1]) if len(sys.argv) > 1 else 16_000_000
d = sys.argv[2] if len(sys.argv) > 2 else "/tmp/reportbench"
pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
os.makedirs(d, exist_ok=True)
fq = os.path.join(d, "r.fq")
subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_fastq.py"), str(n), fq], check=True)
BIN = os.path.join(ROOT, "bonsai_amd", "bin", "bonsai")


def run(with_report):
    args = [BIN, "classify", "-K", "-p", "4", "-b", os.path.join(d, "tax.bin")]
    if with_report:
        args += ["-R", os.path.join(d, "report.txt")]
    t0 = time.time()
    p = subprocess.run(args + [os.path.join(d, "bns.db"), os.path.join(d, "nodes.dmp"), fq], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE,
                       env=dict(os.environ, BNS_CLI_TIMING="1"), timeout=600)
    wall = time.time() - t0
    err = p.stderr.decode()
    if p.returncode != 0:
        sys.exit("bonsai classify failed:\n" + err)
    stage = {}
    for l in err.splitlines():
        if l.startswith("[timing] process_dataset"):
            stage["process_dataset_s"] = float(l.split()[2])
        if l.startswith("[timing] report"):
            stage["report_s"] = float(l.split()[2])
    rec = dict(report=with_report, wall_s=round(wall, 4), mreads_per_s=round(n / wall / 1e6, 2), **stage)
    print(json.dumps(rec), flush=True)
    return rec


run(False)                                                         # (page cache, first-touch of the db)
recs = []
for _ in range(pairs):
    recs.append(run(False))
    recs.append(run(True))
tot = sum(int(l.split("\t")[1]) for l in open(os.path.join(d, "report.txt")) if l.split("\t")[4] in ("0", "1", "4294967295"))
w0 = statistics.median(r["wall_s"] for r in recs if not r["report"])
w1 = statistics.median(r["wall_s"] for r in recs if r["report"])
p0 = statistics.median(r["process_dataset_s"] for r in recs if not r["report"])
p1 = statistics.median(r["process_dataset_s"] for r in recs if r["report"])
print(json.dumps({"n_reads": n, "pairs": pairs, "units_in_report": tot, "median_wall_s": [w0, w1], "wall_overhead_pct": round(100 * (w1 - w0) / w0, 2),
                  "median_process_dataset_s": [p0, p1], "process_dataset_overhead_pct": round(100 * (p1 - p0) / p0, 2),
                  "median_report_s": statistics.median(r.get("report_s", 0.0) for r in recs if r["report"])}))
