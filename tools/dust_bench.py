#!/usr/bin/env python3
"""What low-complexity masking (bns_set_dust, `classify -m` / `build -m`) costs and does, on bench.py's synthetic world at a size of
one's choosing: the device build of a `-w 50 -e` db with and without the mask (seconds inside bns_build_add, keys), one batch of
150-bp reads classified with the mask off and on (milliseconds per call by stream events: the on call adds pack_kernel,
dust_mark_kernel and dust_apply_kernel and runs classify_kernel in its packed form), and the share of reads whose call changes.
Prints one JSON line.  Descriptive: no accuracy claim.

usage: dust_bench.py [--genomes 128] [--genome-len 1048576] [--reads 10000000] [--genome-model repeats|uniform] [--level 20] [--rounds 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=128)
    ap.add_argument("--genome-len", type=int, default=1 << 20)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genome-model", choices=["uniform", "repeats"], default="repeats")
    ap.add_argument("--level", type=int, default=20)
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
    out = {"genomes": NG, "genome_len": G, "genome_model": info, "reads": n, "read_len": L, "window": 64, "level": a.level}

    def build(level):
        ctx.set_window(50, bonsai_amd.SCORE_ENTROPY_PATH)
        ctx.set_dust(64 if level else 0, level)
        ctx.build_begin(NG * G // 8)
        try:
            ctx.build_add(genomes.data_ptr(), g_off.data_ptr(), NG, NG * G, d_tax.data_ptr())
            st = ctx.build_stats(timing=True)
            hdr, flags, keys, vals = ctx.build_finish()
        finally:
            ctx.build_end()
        ctx.set_window(31, bonsai_amd.SCORE_LEX)
        return {"keys": int(hdr[2]), "add_s": st["add_s"], "grows": st["grows"]}, (int(hdr[0]), flags, keys, vals)

    build(0)                                                     # (warm-up: code objects, workspace)
    out["build_off"], db_off = build(0)
    out["build_on"], db_on = build(a.level)
    taxon = torch.zeros(n, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()                                 # (a stream of the caller's: the events bracket what the call enqueues on it)

    def classify(level):
        ctx.set_dust(64 if level else 0, level)
        ms = []
        for _ in range(a.rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            ctx.classify_device(reads.data_ptr(), r_off.data_ptr(), n, n * L, L, False, taxon.data_ptr(), stream=stream.cuda_stream)
            e1.record(stream)
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return sorted(ms[1:]), taxon.clone(), ctx.last_classify_form()["kernel"]

    ctx.load_table(*db_off)
    out["classify_off_ms"], t_off, out["form_off"] = classify(0)
    out["classify_on_ms"], t_on, out["form_on"] = classify(a.level)
    out["calls_changed_same_db"] = float((t_off != t_on).float().mean())
    ctx.load_table(*db_on)
    _, t_both, _ = classify(a.level)
    out["calls_changed_masked_db_and_reads"] = float((t_off != t_both).float().mean())
    out["classified_off"], out["classified_masked_db_and_reads"] = float((t_off != 0).float().mean()), float((t_both != 0).float().mean())
    ctx.set_dust(0)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
