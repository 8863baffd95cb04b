#!/usr/bin/env python3
"""What the minimum number of hit groups (bns_set_min_hit_groups, `classify -M`) costs, on bench.py's synthetic world at a size of
one's choosing: one batch of 150-bp reads against the device-built `-w 50 -e` db, classified with the filter off, with N = 2 and
N = 5, and -- the yardstick -- with the sketches on, whose sketch_kernel does the same walk of every unit without an early exit.
Milliseconds per call by stream events; the share of units that walk at all (a taxon and at least N hits) and the share the filter
zeroes.  Run it under `rocprofv3 --kernel-trace --stats` for the kernels' own durations.  Prints one JSON line.

usage: hit_groups_bench.py [--genomes 1024] [--genome-len 2621440] [--reads 10000000] [--genome-model uniform|repeats] [--rounds 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=1024)
    ap.add_argument("--genome-len", type=int, default=2_621_440)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome-model", choices=["uniform", "repeats"], default="uniform")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    import bench
    import bonsai_amd
    dev = torch.device("cuda:0")
    NG, G, L, n = a.genomes, a.genome_len, 150, a.reads
    parent, leaves = bench.make_taxonomy(NG)
    pool = bench.make_pool(NG, G, dev, seed=7)
    info = bench.add_repeats(pool, NG, G, seed=11) if a.genome_model == "repeats" else {"model": "uniform"}
    reads = bench.gen_reads(pool, n, L, NG, G, dev, seed=3)
    reads = torch.cat([reads, torch.zeros(16, dtype=torch.uint8, device=dev)])
    genomes = torch.cat([bench.codes_to_ascii(pool), torch.zeros(16, dtype=torch.uint8, device=dev)])
    del pool
    g_off = torch.arange(NG + 1, dtype=torch.int64, device=dev) * G
    r_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * L
    d_tax = torch.from_numpy(leaves.astype(np.int32)).to(dev)
    ctx = bonsai_amd.Context(0)
    ctx.set_encoder(31, None, canonicalize=True)
    ctx.load_taxonomy(parent)
    ctx.set_window(50, bonsai_amd.SCORE_ENTROPY_PATH)
    ctx.build_begin(NG * G // 8)
    try:
        ctx.build_add(genomes.data_ptr(), g_off.data_ptr(), NG, NG * G, d_tax.data_ptr())
        hdr, flags, keys, vals = ctx.build_finish()
    finally:
        ctx.build_end()
    ctx.set_window(31, bonsai_amd.SCORE_LEX)
    del genomes
    ctx.load_table(int(hdr[0]), flags, keys, vals)
    out = {"genomes": NG, "genome_len": G, "genome_model": info, "reads": n, "read_len": L, "keys": int(hdr[2])}
    taxon = torch.zeros(n, dtype=torch.int32, device=dev)
    n_hits = torch.zeros(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()                                 # (a stream of the caller's: the events bracket what the call enqueues on it)

    def classify(n_min, sketch=False):
        ctx.set_min_hit_groups(n_min)
        ctx.sketch_enable(65536 if sketch else 0)
        ms = []
        for _ in range(a.rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            ctx.classify_device(reads.data_ptr(), r_off.data_ptr(), n, n * L, L, False, taxon.data_ptr(), None, None, n_hits.data_ptr(), stream=stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        ctx.sketch_enable(0)
        return sorted(ms[1:]), taxon.clone()

    out["off_ms"], t_off = classify(0)
    hits = n_hits.clone()
    out["classified_off"] = float((t_off != 0).float().mean())
    out["mean_hits_of_classified"] = float(hits[t_off != 0].float().mean())
    for n_min in (2, 5):
        ms, t_on = classify(n_min)
        out["n%d" % n_min] = {"ms": ms, "units_that_walk": float(((t_off != 0) & (hits >= n_min)).float().mean()),
                              "units_settled_by_hit_count": float(((t_off != 0) & (hits < n_min)).float().mean()),
                              "units_zeroed": float(((t_off != 0) & (t_on == 0)).float().mean()),
                              "classified": float((t_on != 0).float().mean())}
        assert bool(((t_on == t_off) | (t_on == 0)).all())
    out["sketch_ms"], _ = classify(0, sketch=True)
    ctx.set_min_hit_groups(0)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
