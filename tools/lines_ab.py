#!/usr/bin/env python
"""A/B of `bonsai classify` with Kraken lines: another build of the CLI (--other: the parent commit's bonsai binary, built beside this
checkout) against this one with BNS_LINES_GPU=1 and =0, and the -K (no lines) mode of both, on the workloads of the round-6 review
(profiles/r06_cli_realdb.txt, profiles/r06_gz.txt), restated:

  plain   bench.py's benchmark-size db and --reads of its reads as FASTQ (bench.py --save-db / --save-reads), the file --copies times
          over;  `bonsai classify -a -p 6 -o /dev/null` and the same with -K
  gz      --gz-reads of those reads as ONE gzip member (zlib level 6); with lines and with -K

Every input is read once in front of the timing (page cache); the legs are interleaved run by run; every run is a process of its own
under a time limit, and the first one that fails ends the script.  Per run: wall time around the process and the time inside
process_dataset (BNS_CLI_TIMING).  Every run is printed, then median / min / max per leg.
usage: lines_ab.py --other PATH/bonsai [--work DIR] [--reads N] [--copies C] [--gz-reads N] [--runs R] [--out FILE]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = os.path.join(ROOT, "bonsai_amd", "bin", "bonsai")


def one_run(binary, args, env, limit):
    e = dict(os.environ, BNS_CLI_TIMING="1")
    e.pop("BNS_LINES_GPU", None)
    e.update(env)
    t0 = time.perf_counter()
    p = subprocess.run([binary, "classify"] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=limit, env=e)
    wall = time.perf_counter() - t0
    err = p.stderr.decode(errors="replace")
    if p.returncode != 0:
        sys.exit("run failed (rc %d): %s %s\n%s" % (p.returncode, binary, " ".join(args), err[-2000:]))
    m = re.search(r"process_dataset[^\n]*?([0-9]+\.[0-9]+) s", err)
    note = re.search(r"lines: [^\n;]*|no Kraken lines", err)
    return {"wall_s": wall, "process_dataset_s": float(m.group(1)) if m else None, "formatter": note.group(0) if note else "(parent build)"}


def deflate_piece(chunk):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    return co.compress(chunk) + co.flush(zlib.Z_FULL_FLUSH)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="the other build's bonsai binary (the parent commit's)")
    ap.add_argument("--work", default="/tmp/lines_ab")
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--copies", type=int, default=12)
    ap.add_argument("--gz-reads", type=int, default=32_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per run")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.makedirs(a.work, exist_ok=True)
    d = a.work
    subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--save-db", d, "--save-reads", str(a.reads), "--steps", "2", "--warmup", "1",
                    "--no-cpu", "--no-probe", "--no-text", "--no-inflate"], check=True, timeout=900, stdout=subprocess.DEVNULL)
    db, nodes, fq = os.path.join(d, "bns.db"), os.path.join(d, "nodes.dmp"), os.path.join(d, "reads.fq")
    data = open(fq, "rb").read()
    rec = len(data) // a.reads
    long_fq = os.path.join(d, "long.fq")
    with open(long_fq, "wb") as f:
        for _ in range(a.copies):
            f.write(data)
    gz = os.path.join(d, "stream.fq.gz")
    # ONE gzip member (a header, one deflate stream, one trailer).  The 10 M-read text is deflated once, in 16 processes: every piece ends
    # in a full flush (byte-aligned, dictionary reset), so the pieces -- and the whole text over again -- concatenate to one valid stream
    from multiprocessing import Pool
    step = (a.reads // 16 + 1) * rec
    with Pool(16) as pool:
        parts = pool.map(deflate_piece, [data[i:i + step] for i in range(0, len(data), step)])
    body = b"".join(parts)
    with open(gz, "wb") as f:
        f.write(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff")
        crc, size, left = 0, 0, a.gz_reads
        while left >= a.reads:
            f.write(body); crc = zlib.crc32(data, crc); size += len(data); left -= a.reads
        if left:
            f.write(deflate_piece(data[:left * rec])); crc = zlib.crc32(data[:left * rec], crc); size += left * rec
        f.write(b"\x03\x00")                                        # (the final block: empty, fixed codes)
        f.write((crc & 0xFFFFFFFF).to_bytes(4, "little") + (size & 0xFFFFFFFF).to_bytes(4, "little"))
    del data
    for p in (db, long_fq, gz):                                      # once through the page cache
        with open(p, "rb") as f:
            while f.read(1 << 26):
                pass
    n_plain, n_gz = a.reads * a.copies, a.gz_reads
    base = ["-p", "6", "-o", "/dev/null"]
    legs = []
    for wl, path, n in (("plain", long_fq, n_plain), ("gz", gz, n_gz)):
        tail = [db, nodes, path]
        legs += [(wl, n, "parent lines", a.other, ["-a"] + base + tail, {}),
                 (wl, n, "new lines on the device", NEW, ["-a"] + base + tail, {"BNS_LINES_GPU": "1"}),
                 (wl, n, "new lines on the host", NEW, ["-a"] + base + tail, {"BNS_LINES_GPU": "0"}),
                 (wl, n, "parent -K", a.other, ["-a", "-K"] + base + tail, {}),
                 (wl, n, "new -K", NEW, ["-a", "-K"] + base + tail, {})]
    res = {(l[0], l[2]): [] for l in legs}
    lines = ["workloads: plain = %d reads of %d bytes (%.1f GB), gz = %d reads in one gzip member (%.2f GB); %d runs per leg, interleaved"
             % (n_plain, rec, os.path.getsize(long_fq) / 1e9, n_gz, os.path.getsize(gz) / 1e9, a.runs)]
    for r in range(a.runs + 1):                                      # (run 0 warms every leg up and is not counted)
        for wl, n, name, binary, args, env in legs:
            x = one_run(binary, args, env, a.limit)
            if r:
                res[(wl, name)].append(x)
            lines.append("%-5s %-24s run %d%s: process_dataset %s s, wall %.3f s  [%s]" % (wl, name, r, " (warm-up)" if not r else "",
                         "%.3f" % x["process_dataset_s"] if x["process_dataset_s"] is not None else "?", x["wall_s"], x["formatter"]))
            print(lines[-1], flush=True)
    lines.append("")
    for wl, n, name, *_ in legs:
        xs = res[(wl, name)]
        for key in ("process_dataset_s", "wall_s"):
            v = [x[key] for x in xs if x[key] is not None]
            if v:
                lines.append("%-5s %-24s %-18s median %.3f  min %.3f  max %.3f   (%.1f M reads/s at the median)" % (wl, name, key, statistics.median(v), min(v), max(v), n / statistics.median(v) / 1e6))
    print("\n".join(lines[-(2 * len(legs) + 1):]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    print(json.dumps({"%s / %s" % k: v for k, v in res.items()})[:200])


if __name__ == "__main__":
    main()
