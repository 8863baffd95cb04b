#!/usr/bin/env python
"""Vote-stage time of the window session with and without a threshold of its own, on the input of profiles/windows_ab.txt.

The db and genomes of tools/windows_bench.py (bench.py's recipe: 64 genomes x 2.6 Mb, a `-w 50 -e` db, L = 150).  One timed session
(bns_set_timing: events around the three stages of every add) of --adds adds after a warm-up; per add the milliseconds of the vote
stage, which holds the confidence walk.  One process measures one library: run it from the parent commit's tree and from this one in
turn (--confidence 0) to see that the form without a threshold is the code it was, then with --confidence 0.1 for the new work.

  python tools/windows_conf_bench.py [--confidence 0.1] [--adds 10] [--tag new] [--out profiles/windows_conf.txt]
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
    ap.add_argument("--log2-buckets", type=int, default=25)
    ap.add_argument("--db-window", type=int, default=50)
    ap.add_argument("--confidence", default="0")
    ap.add_argument("--adds", type=int, default=10)
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
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
    ctx.build_table_device(pool.data_ptr(), g_off.data_ptr(), NG, NG * G, taxid.data_ptr(), nb, flags.data_ptr(), keys.data_ptr(),
                           vals.data_ptr(), stream)
    ctx.set_window(0, bonsai_amd.SCORE_LEX)
    ctx.load_table_device(nb, flags.data_ptr(), keys.data_ptr(), vals.data_ptr(), bonsai_amd.LAYOUT_MINBUCKET, stream)
    torch.cuda.synchronize()
    del flags, keys, vals
    d_taxon = torch.empty(NG * G, dtype=torch.int32, device=dev)

    ctx.set_timing(True)
    if a.confidence == "0":
        ctx.windows_begin(L, 1 << 20)                                     # (the call every tree has)
    else:
        ctx.windows_begin(L, 1 << 20, confidence=a.confidence)
    vote, lookup = [], []
    for i in range(a.adds + 1):                                           # the first add allocates the workspace: not counted
        ctx.windows_add(pool.data_ptr(), g_off.data_ptr(), NG, NG * G, taxid.data_ptr(), d_taxon.data_ptr(), stream)
        ms, _ = ctx.windows_timing()
        if i:
            vote.append(ms["vote_ms"]); lookup.append(ms["lookup_ms"])
    seq, called, count, dropped = ctx.windows(reset=True)
    n_zero = int(count[called == 0].sum()) // (a.adds + 1)
    ctx.windows_end()
    ctx.set_timing(False)
    line = "%-8s theta %-4s vote ms per add: %s | median %.3f [%.3f, %.3f] | lookup median %.3f | windows called 0: %d of %d" % (
        a.tag, a.confidence, " ".join("%.3f" % v for v in vote), statistics.median(vote), min(vote), max(vote), statistics.median(lookup),
        n_zero, NG * (G - L + 1))
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
