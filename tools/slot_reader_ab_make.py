#!/usr/bin/env python
"""Inputs for the SlotReader A/B: the file of tools/cli_bench.py (150 bp, 314 bytes per record) with N reads, its halves as a pair, and the
first M reads as BGZF (tests/synth.write_bgzf, level 1, written in four parts side by side) and as one gzip stream (Python's gzip,
level 1).  Chunks of STEP reads are made side by side, each from its own seed.  slot_reader_ab_make.py N M"""
import gzip, os, sys, time
import multiprocessing as mp
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O, synth
N, M = int(sys.argv[1]), int(sys.argv[2])
D = "/tmp/slotab"; os.makedirs(D, exist_ok=True)
t0 = time.time()
w = synth.make_world(O, seed=3, k=31, genome_len=50000)
O.db_write(D + "/bns.db", 31, 31, None, w.table)
synth.write_nodes_dmp(D + "/nodes.dmp")
g = np.concatenate(list(w.genomes.values()))
STEP = int(os.environ.get("SLOTAB_STEP", 1_000_000))
assert N % (2 * STEP) == 0 and M % (4 * STEP) == 0 and M <= N // 2

def chunk(a):
    rng = np.random.default_rng([1, a])
    st = rng.integers(0, g.size - 150, size=STEP)
    rec = np.empty((STEP, 314), dtype=np.uint8)
    rec[:, 0] = ord("@"); rec[:, 1] = ord("r")
    idx = (np.arange(STEP) + a) % 10_000_000
    for j in range(7):
        rec[:, 8 - j] = ord("0") + (idx // 10 ** j) % 10
    rec[:, 9] = 10
    rec[:, 10:160] = g[st[:, None] + np.arange(150)[None, :]]
    rec[:, 160] = 10; rec[:, 161] = ord("+"); rec[:, 162] = 10
    rec[:, 163:313] = ord("I"); rec[:, 313] = 10
    b = rec.tobytes()
    for path, off in ((D + "/r.fq", a), (D + ("/r_1.fq" if a < N // 2 else "/r_2.fq"), a % (N // 2))):
        fd = os.open(path, os.O_WRONLY)
        os.pwrite(fd, b, off * 314)
        os.close(fd)
    return a

def make_gz(_):
    with open(D + "/r.fq", "rb") as src, gzip.open(D + "/r.fq.gz", "wb", compresslevel=1) as f:
        left = M * 314
        while left:
            b = src.read(min(left, 64 << 20)); f.write(b); left -= len(b)
    return "gzip: %.1f s, %d bytes" % (time.time() - t0, os.path.getsize(D + "/r.fq.gz"))

def make_bgzf_part(i):
    with open(D + "/r.fq", "rb") as src:
        src.seek(i * (M // 4) * 314)
        data = src.read((M // 4) * 314)
    synth.write_bgzf(D + "/bgz.%d" % i, data, level=1)
    return "bgzf part %d: %.1f s" % (i, time.time() - t0)

def work(job):
    return job[0](job[1])

for p, n in (("/r.fq", N), ("/r_1.fq", N // 2), ("/r_2.fq", N // 2)):
    with open(D + p, "wb") as f:
        f.truncate(n * 314)
with mp.get_context("fork").Pool(12) as pool:
    for a in pool.imap_unordered(chunk, range(0, N, STEP)):
        print("plain: chunk at %d, %.1f s" % (a, time.time() - t0), flush=True)
    for line in pool.imap_unordered(work, [(make_gz, 0)] + [(make_bgzf_part, i) for i in range(4)]):
        print(line, flush=True)
EOF_MEMBER = 28                                                 # (write_bgzf ends every file with the empty member: kept behind the last part only)
with open(D + "/r.fq.bgz.gz", "wb") as f:
    for i in range(4):
        b = open(D + "/bgz.%d" % i, "rb").read()
        f.write(b if i == 3 else b[:-EOF_MEMBER])
        os.remove(D + "/bgz.%d" % i)
print("done: %.1f s" % (time.time() - t0), flush=True)
os.system("df -h /tmp | tail -1; ls -l " + D)
