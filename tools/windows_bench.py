#!/usr/bin/env python
"""Window session against the expanded path, in one process, alternating.

A `-w 50 -e` db of seeded synthetic genomes (bench.py's recipe: make_taxonomy, make_pool) is built and loaded on the device.  Then,
REPEATS times in turn:
  session   one bns_windows_add at L = 150 over ALL genomes (d_taxon taken), between two device events -> windows/s;
  expanded  bns_classify_batch_device -- the code of the parent commit, the yardstick -- on the windows of the first SLICE genomes, every
            window copied out as a read of its own (>= 4 M reads of 150 bases), between two events, scaled to windows/s.
The bar: the session's windows/s is at least the expanded path's in every repeat.  The calls of the slice's windows are compared as
well (they must be equal), and a last, timed session (bns_set_timing) gives the split over the session's three stages.

  python tools/windows_bench.py [--genomes 64] [--genome-len 2621440] [--slice 2] [--repeats 5] [--out profiles/windows_ab.txt]
  python tools/windows_bench.py --session-only      (what a kernel trace is taken of: warm-up and three session runs, nothing else)
"""
import argparse
import os
import statistics
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                  # the genome recipe
import bonsai_amd                             # after torch: shares torch's HIP runtime

L, K = 150, 31


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=64)
    ap.add_argument("--genome-len", type=int, default=2_621_440)
    ap.add_argument("--slice", type=int, default=2, help="genomes whose windows are expanded into reads (2 x 2.6 Mb: 5.2 M windows)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--log2-buckets", type=int, default=25)
    ap.add_argument("--db-window", type=int, default=50)
    ap.add_argument("--session-only", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else None

    def say(s=""):
        print(s, flush=True)
        if out:
            out.write(s + "\n"); out.flush()

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    tstream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(tstream)
    stream = tstream.cuda_stream
    ctx = bonsai_amd.Context(0)
    ctx.set_encoder(K, None, canonicalize=True)
    NG, G = a.genomes, a.genome_len
    parent, leaves = bench.make_taxonomy(NG)
    ctx.load_taxonomy(parent)
    nb = 1 << a.log2_buckets
    flags = torch.empty(max(1, nb >> 4), dtype=torch.int32, device=dev)
    keys = torch.empty(nb, dtype=torch.int64, device=dev)
    vals = torch.empty(nb, dtype=torch.int32, device=dev)
    pool = bench.codes_to_ascii(bench.make_pool(NG, G, dev, seed=7))
    pool = torch.cat([pool, torch.full((8,), ord("N"), dtype=torch.uint8, device=dev)])      # readable tail
    g_off = torch.arange(NG + 1, device=dev, dtype=torch.int64) * G
    taxid = torch.from_numpy(leaves.astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    if a.db_window > K:
        ctx.set_window(a.db_window, bonsai_amd.SCORE_ENTROPY_PATH)
    hdr = ctx.build_table_device(pool.data_ptr(), g_off.data_ptr(), NG, NG * G, taxid.data_ptr(), nb, flags.data_ptr(), keys.data_ptr(),
                                 vals.data_ptr(), stream)
    ctx.set_window(0, bonsai_amd.SCORE_LEX)
    ctx.load_table_device(nb, flags.data_ptr(), keys.data_ptr(), vals.data_ptr(), bonsai_amd.LAYOUT_MINBUCKET, stream)
    torch.cuda.synchronize()
    del flags, keys, vals
    n_windows = NG * (G - L + 1)
    say("windows_bench: %d genomes x %d bases, db -w %d -e: %d keys; L = %d: %d windows" % (NG, G, a.db_window, int(hdr[2]), L, n_windows))

    d_taxon = torch.empty(NG * G, dtype=torch.int32, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(tstream)
        fn()
        e1.record(tstream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def session(taxon=True):
        ctx.windows_add(pool.data_ptr(), g_off.data_ptr(), NG, NG * G, taxid.data_ptr(), d_taxon.data_ptr() if taxon else None, stream)

    ctx.windows_begin(L, 1 << 20)
    timed(session)                                                        # warm-up: the workspace is allocated here
    if a.session_only:
        for _ in range(3):
            say("session %.3f ms" % timed(session))
        ctx.windows_end()
        return 0

    # the expanded slice: window p of genome g -> read g * (G - L + 1) + p
    S, W1 = a.slice, G - L + 1
    n_exp = S * W1
    assert n_exp >= 4_000_000 or S == NG, "the slice is a toy: fewer than 4 M windows"
    exp = torch.empty((n_exp, L), dtype=torch.uint8, device=dev)
    idx = torch.arange(L, device=dev, dtype=torch.int64)[None, :]
    for g in range(S):
        for p0 in range(0, W1, 1 << 20):
            p1 = min(W1, p0 + (1 << 20))
            exp[g * W1 + p0:g * W1 + p1] = pool[(g * G + torch.arange(p0, p1, device=dev, dtype=torch.int64))[:, None] + idx]
    exp = torch.cat([exp.reshape(-1), torch.full((8,), ord("N"), dtype=torch.uint8, device=dev)])
    e_off = torch.arange(n_exp + 1, device=dev, dtype=torch.int64) * L
    e_taxon = torch.empty(n_exp, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def expanded():
        ctx.classify_device(exp.data_ptr(), e_off.data_ptr(), n_exp, n_exp * L, L, False, e_taxon.data_ptr(), stream=stream)

    timed(expanded)                                                       # warm-up
    timed(session)
    got = d_taxon.reshape(NG, G)[:S, :W1].reshape(-1)
    n_diff = int((got != e_taxon).sum().item())
    tail = d_taxon.reshape(NG, G)[:, W1:]
    say("calls of the %d expanded windows that differ between the two paths: %d; bases that start no window and are not 0xFFFFFFFF: %d"
        % (n_exp, n_diff, int((tail != -1).sum().item())))

    rs, re_ = [], []
    for r in range(a.repeats):
        ms_s = timed(session)
        ms_e = timed(expanded)
        rs.append(n_windows / ms_s * 1e3); re_.append(n_exp / ms_e * 1e3)
        say("repeat %d: session %9.3f ms = %8.1f M windows/s | expanded slice %9.3f ms = %8.1f M windows/s | ratio %.2f"
            % (r, ms_s, rs[-1] / 1e6, ms_e, re_[-1] / 1e6, rs[-1] / re_[-1]))
    ms_none = timed(lambda: session(taxon=False))
    say("session without d_taxon: %.3f ms = %.1f M windows/s" % (ms_none, n_windows / ms_none * 1e3 / 1e6))
    seq, called, count, dropped = ctx.windows(reset=True)
    say("pairs: %d, dropped %d, windows counted %d of %d per add" % (seq.size, dropped, int(count.sum()), n_windows))
    ctx.windows_end()

    ctx.set_timing(True)                                                  # the split: a session of its own, its adds wait for the device
    ctx.windows_begin(L, 1 << 20)
    session(); ctx.windows_timing()
    for _ in range(3):
        session()
    ms, n_adds = ctx.windows_timing()
    ctx.windows_end()
    ctx.set_timing(False)
    say("per add (mean of %d): pack + clears %.3f ms, lookup pass %.3f ms, vote pass %.3f ms" %
        (n_adds, ms["pack_ms"] / n_adds, ms["lookup_ms"] / n_adds, ms["vote_ms"] / n_adds))

    def spread(v):
        return "median %.1f, min %.1f, max %.1f M windows/s" % (statistics.median(v) / 1e6, min(v) / 1e6, max(v) / 1e6)
    say("session:  " + spread(rs))
    say("expanded: " + spread(re_))
    ok = all(s >= e for s, e in zip(rs, re_)) and n_diff == 0
    say("bar (session >= expanded in every repeat, equal calls): %s" % ("met" if ok else "MISSED"))
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
