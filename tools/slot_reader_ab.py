#!/usr/bin/env python
"""SlotReader A/B: the bonsai of a checkout of the parent commit (built beside this tree) against this tree's, alternating, on the inputs
of slot_reader_ab_make.py N M.  slot_reader_ab.py PAIRS N M PARENT_BONSAI OUT [workloads] -> the table in OUT (profiles/slot_reader_ab.txt).
Every run under its own time limit; the first failure ends the script."""
import hashlib, os, re, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS, N, M = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
ONLY = sys.argv[6].split(",") if len(sys.argv) > 6 else None     # workloads by name (default: all)
D = "/tmp/slotab"
BIN = {"parent": sys.argv[4], "new": ROOT + "/bonsai_amd/bin/bonsai"}
out = open(sys.argv[5], "w")
def say(s=""):
    print(s, flush=True); out.write(s + "\n"); out.flush()

F = r"([0-9.]+)"
# workload: (reads, mode args, inputs, the [timing] line of its pipeline, {figure: regex})
WORK = {
    "plain -K": (N, ["-K", "-p", "4"], ["r.fq"], "text on the device:", {"pread": "pread " + F, "page-lock": "page-lock " + F, "callers waited for blocks": "callers waited " + F}),
    "plain lines": (N, ["-p", "4"], ["r.fq"], "text on the device:", {"pread": "pread " + F, "page-lock": "page-lock " + F, "callers waited for blocks": "callers waited " + F}),
    "paired lines": (N, ["-p", "4"], ["r_1.fq", "r_2.fq"], "pair of files, text on the device:", {"pread": "pread " + F, "waited for blocks": "waited " + F + " s for blocks"}),
    "paired -K": (N, ["-K", "-p", "4"], ["r_1.fq", "r_2.fq"], "pair of files, text on the device:", {"pread": "pread " + F, "waited for blocks": "waited " + F + " s for blocks"}),
    "BGZF -K": (M, ["-K", "-p", "4"], ["r.fq.bgz.gz"], "BGZF text on the device:", {"pread": "pread " + F, "page-lock": "page-lock " + F, "walker waited for bytes": "walker for bytes " + F, "classify waited for text": "classify for text " + F}),
    "gzip -K": (M, ["-K", "-p", "4"], ["r.fq.gz"], "gzip text on the device:", {"pread": "pread " + F, "page-lock": "page-lock " + F, "caller waited for bytes": "caller for bytes " + F, "classify waited for text": "classify for text " + F}),
}

def md5(path):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()

def run(which, name, hash_out=True):
    n, args, inputs, tag, figs = WORK[name]
    cmd = [BIN[which], "classify", "-a"] + args + ["-b", D + "/tax.bin", "-o", D + "/out.txt", D + "/bns.db", D + "/nodes.dmp"] + [D + "/" + i for i in inputs]
    t0 = time.time()
    p = subprocess.run(cmd, stderr=subprocess.PIPE, env=dict(os.environ, BNS_CLI_TIMING="1"), timeout=180)
    dt = time.time() - t0
    err = p.stderr.decode()
    if p.returncode != 0:
        say("FAILED rc %d: %s\n%s" % (p.returncode, " ".join(cmd), err[-3000:]))
        sys.exit(1)
    tl = [l for l in err.splitlines() if l.startswith("[timing]")]
    su = 0.0
    for l in tl:
        if "start-up" in l:
            su = float(l.split(")")[1].split()[0])
    line = [l for l in tl if tag in l]
    if len(line) != 1:
        say("no single '%s' line: the input did not take its device route\n%s" % (tag, err[-3000:]))
        sys.exit(1)
    pd = [float(l.split()[2]) for l in tl if l.startswith("[timing] process_dataset")][0]
    r = {"wall": dt, "wall - start-up": dt - su, "process_dataset": pd, "launch and exit": dt - su - pd}
    for k, rx in figs.items():
        r[k] = float(re.search(rx, line[0]).group(1))
    r["handed back"] = "host parser takes the rest" in line[0]
    r["tax"] = md5(D + "/tax.bin"); r["out"] = md5(D + "/out.txt") if hash_out else "%d bytes" % os.path.getsize(D + "/out.txt")
    return r, line[0], cmd

say("SlotReader A/B: parent commit against this tree, alternating, %d pairs per plain workload and %d per compressed one (their runs are short and fall into two groups ~0.1 s apart), one MI355X" % (PAIRS, 2 * PAIRS + 1))
say("inputs: tools/cli_bench.py's records (314 bytes each), N = %d reads plain and as two halves, the first M = %d reads as BGZF (synth.write_bgzf, level 1) and gzip (level 1)" % (N, M))
for f in ("r.fq", "r_1.fq", "r_2.fq", "r.fq.bgz.gz", "r.fq.gz"):
    say("  %-12s %d bytes" % (f, os.path.getsize(D + "/" + f)))
for f in ("r.fq", "r_1.fq", "r_2.fq", "r.fq.bgz.gz", "r.fq.gz"):      # (page cache)
    subprocess.run(["cat", D + "/" + f], stdout=subprocess.DEVNULL, check=True)
verdicts = []
for name in (ONLY or WORK):
    res = {"parent": [], "new": []}
    say("\n== " + name)
    for i in range((PAIRS if "lines" in name or "plain" in name or "paired" in name else 2 * PAIRS + 1) + 1):                                  # (pair 0 warms up and is not counted)
        for which in ("parent", "new"):
            r, line, cmd = run(which, name, hash_out=(i == 0 or "lines" not in name))      # (GBs of Kraken lines: hashed in the warm-up pair, their size compared in the others)
            if i == 1 and "lines" in name: res["ids"] = {w: (t, r["out"], h) for w, (t, o, h) in res["ids"].items()}
            if i == 0:
                if which == "parent": say("   " + " ".join(cmd[1:]).replace(D + "/", ""))
                say("   [%s, warm-up] %s" % (which, line[:700]))
                res.setdefault("ids", {})[which] = (r["tax"], r["out"], r["handed back"])
                if which == "new":
                    if res["ids"]["new"] != res["ids"]["parent"]: say("OUTPUT DIFFERS in the warm-up pair of " + name); sys.exit(1)
                    res["hash"] = r["out"]
                continue
            res[which].append(r)
            if (r["tax"], r["out"], r["handed back"]) != res["ids"]["parent"]:
                say("OUTPUT DIFFERS: %s run %d of %s" % (which, i, name)); sys.exit(1)
    say("   -b taxon file and -o output identical in all %d runs (md5 %s / %s)%s" % (2 * len(res["new"]) + 2, res["ids"]["parent"][0][:12], res["hash"][:12] + (", " + res["ids"]["parent"][1] if "lines" in name else ""), "; HANDED BACK" if res["ids"]["parent"][2] else ""))
    keys = [k for k in res["parent"][0] if k not in ("tax", "out", "handed back")]
    for k in keys:
        a = [r[k] for r in res["parent"]]; b = [r[k] for r in res["new"]]
        inside = min(a) <= statistics.median(b) <= max(a)
        say("   %-26s parent %s  median %.3f [%.3f, %.3f] | new %s  median %.3f [%.3f, %.3f]%s"
            % (k, " ".join("%.3f" % x for x in a), statistics.median(a), min(a), max(a), " ".join("%.3f" % x for x in b), statistics.median(b), min(b), max(b),
               "" if k not in ("wall - start-up", "process_dataset") else ("  -> new median inside parent's spread" if inside else "  -> new median OUTSIDE parent's spread")))
        if k == "wall - start-up":
            verdicts.append((name, inside, statistics.median(a), statistics.median(b), min(a), max(a)))
say("\n== wall time without start-up, new median against the parent's min-max")
for name, inside, ma, mb, lo, hi in verdicts:
    say("   %-14s parent median %.3f [%.3f, %.3f], new median %.3f: %s" % (name, ma, lo, hi, mb, "inside" if inside else "OUTSIDE"))
