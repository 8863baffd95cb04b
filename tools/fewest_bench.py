#!/usr/bin/env python
"""The three scored builds on the benchmark's genomes, through the library: what profiles/fewest.txt reports.

bench.py's generator, read-only (make_taxonomy, make_pool seed 7): NG genomes of G bases as ONE batch of device arrays, k 31
canonical, w 50.  Times are the library's own clocks (wall seconds inside bns_build_add / bns_build_count_add /
bns_build_minimize_add, each of which ends in a stream synchronise: the "add" of the CLI's [timing] lines).

  --what depth   ROUNDS times: build_begin, build_add (pass A), build_minimize_begin(50), build_minimize_add (pass B).  Uses nothing
                 a library before bns_build_count_* lacks: --root OTHER_TREE runs the same rounds on another checkout's package.
  --what all     the -e, -D and -G builds (passes A, C, B), the keys of each db, classify_device ms per 10 M of the benchmark's reads
                 against each db, the share of reads the -G db calls differently from the -D db, and the count pass on the same bases
                 cut into many small genomes (a launch each) and into few large ones.

  python tools/fewest_bench.py --what depth [--rounds 3] [--root DIR]
  python tools/fewest_bench.py --what all [--genomes 1024] [--genome-len 2621440] [--reads 10000000]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

K, W = 31, 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=["depth", "all"], default="depth")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose bonsai_amd and bench are imported")
    ap.add_argument("--genomes", type=int, default=1024)
    ap.add_argument("--genome-len", type=int, default=2_621_440)
    ap.add_argument("--log2-f", type=int, default=32, help="buckets of the table of all k-mers")
    ap.add_argument("--log2-m", type=int, default=30, help="buckets M and the -e table start with")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--small-genomes", type=int, default=20000)
    ap.add_argument("--small-len", type=int, default=5000)
    ap.add_argument("--large-genomes", type=int, default=40)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import bench                                  # the genome recipe
    import bonsai_amd                             # after torch: shares torch's HIP runtime

    def say(s=""):
        print(s, flush=True)

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    ctx = bonsai_amd.Context(0)
    ctx.set_encoder(K, None, canonicalize=True)
    NG, G = a.genomes, a.genome_len
    parent, leaves = bench.make_taxonomy(NG)
    ctx.load_taxonomy(parent)
    pool_codes = bench.make_pool(NG, G, dev, seed=7)
    pool = torch.cat([bench.codes_to_ascii(pool_codes), torch.full((8,), ord("N"), dtype=torch.uint8, device=dev)])      # readable tail
    g_off = torch.arange(NG + 1, device=dev, dtype=torch.int64) * G
    taxid = torch.from_numpy(leaves.astype(np.int32)).to(dev)
    torch.cuda.synchronize()
    say("fewest_bench --what %s: %s, library version %d; %d genomes x %d bases, k %d, w %d" %
        (a.what, os.path.abspath(a.root), ctx.L.bns_version(), NG, G, K, W))
    args = (pool.data_ptr(), g_off.data_ptr(), NG, NG * G)

    def pass_a():
        ctx.build_begin(1 << a.log2_f)
        ctx.build_add(*args, taxid.data_ptr())
        return ctx.build_stats(timing=True)

    def pass_b(score):
        if score == "depth":
            ctx.build_minimize_begin(W, 1 << a.log2_m)
        else:
            ctx.build_minimize_begin(W, 1 << a.log2_m, score=score)
        ctx.build_minimize_add(*args)
        return ctx.build_minimize_stats()

    def finish(export):
        """-> (keys, table arrays or None); the session is ended"""
        if export:
            hdr, flags, keys, vals = ctx.build_finish()
            ctx.build_end()
            return int(hdr[2]), (int(hdr[0]), flags, keys, vals)
        hdr = np.zeros(4, dtype=np.uint64)
        ctx._chk(ctx.L.bns_build_finish(ctx.h, hdr.ctypes.data_as(ctx.L.bns_build_finish.argtypes[1])), "bns_build_finish")
        ctx.build_end()
        return int(hdr[2]), None

    if a.what == "depth":
        secs = []
        for r in range(a.rounds):
            sa = pass_a()
            sm = pass_b("depth")
            n_keys, _ = finish(False)
            secs.append(sm["add_s"])
            say("round %d: pass A add %.3f s, minimize: add %.3f s (%d lookups, %.2f G/s), %d scored keys, %d keys in M, %d grows" %
                (r, sa["add_s"], sm["add_s"], sm["lookups"], sm["lookups"] / sm["add_s"] / 1e9, sm["scored_keys"], n_keys, sm["grows"]))
        say("minimize: add over %d rounds: median %.3f s, min %.3f s, max %.3f s" % (a.rounds, statistics.median(secs), min(secs), max(secs)))
        ctx.close()
        return 0

    # ---- the three builds
    dbs = {}
    ctx.set_window(W, bonsai_amd.SCORE_ENTROPY_PATH)
    ctx.build_begin(1 << a.log2_m)
    ctx.build_add(*args, taxid.data_ptr())
    se = ctx.build_stats(timing=True)
    n_e, dbs["-e"] = finish(True)
    ctx.set_window(0, bonsai_amd.SCORE_LEX)
    say("-e: add %.3f s (%d grows); %d keys" % (se["add_s"], se["grows"], n_e))
    sa = pass_a()
    sm = pass_b("depth")
    n_d, dbs["-D"] = finish(True)
    say("-D: pass A %.3f s, pass B %.3f s (%d lookups, %.2f G/s); F %d keys, M %d keys" %
        (sa["add_s"], sm["add_s"], sm["lookups"], sm["lookups"] / sm["add_s"] / 1e9, sm["scored_keys"], n_d))
    ids = np.arange(NG, dtype=np.uint32)
    sa = pass_a()
    t0 = time.perf_counter()
    ctx.build_count_begin()
    t_begin = time.perf_counter() - t0
    ctx.build_count_add(*args, ids)
    sc = ctx.build_count_stats()
    sm = pass_b("fewest")
    n_g, dbs["-G"] = finish(True)
    say("-G: pass A %.3f s, count_begin %.3f s, pass C %.3f s (%d launches, %d lookups, %.2f G/s, largest count %d), pass B %.3f s (%.2f G lookups/s); M %d keys" %
        (sa["add_s"], t_begin, sc["add_s"], sc["launches"], sc["lookups"], sc["lookups"] / sc["add_s"] / 1e9, sc["largest"], sm["add_s"],
         sm["lookups"] / sm["add_s"] / 1e9, n_g))

    # ---- classify against each db
    n, L = a.reads, 150
    bases, offsets, total, _ = bench.make_batch(pool_codes, n, L, NG, G, dev, 0, 0, False, None)
    bases = torch.cat([bases, torch.full((8,), ord("N"), dtype=torch.uint8, device=dev)])
    outs = [torch.zeros(n, dtype=torch.int32, device=dev)]
    called = {}
    for name, (nb, flags, keys, vals) in dbs.items():
        ctx.load_table(nb, flags, keys, vals, layout=bonsai_amd.LAYOUT_MINBUCKET)
        ms = []
        for i in range(13):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.classify_device(bases.data_ptr(), offsets.data_ptr(), n, total, L, False, *(o.data_ptr() for o in outs))
            ctx.sync()
            if i >= 3:
                ms.append((time.perf_counter() - t0) * 1e3)
        called[name] = outs[0].clone()
        say("classify against the %s db: ms per %d reads min %.3f median %.3f max %.3f; classified %d" %
            (name, n, min(ms), statistics.median(ms), max(ms), int((called[name] != 0).sum().item())))
    say("reads the -G db calls differently from the -D db: %d of %d (%.4f %%); from the -e db: %d" %
        (int((called["-G"] != called["-D"]).sum().item()), n, 100.0 * float((called["-G"] != called["-D"]).float().mean().item()),
         int((called["-G"] != called["-e"]).sum().item())))
    del dbs, called

    # ---- the count pass on small genomes: the same bases as many launches and as few
    bases_n = a.small_genomes * a.small_len
    assert bases_n % a.large_genomes == 0 and bases_n <= NG * G
    for n_seq in (a.large_genomes, a.small_genomes):
        seq_len = bases_n // n_seq
        off = torch.arange(n_seq + 1, device=dev, dtype=torch.int64) * seq_len
        l_off = torch.arange(a.large_genomes + 1, device=dev, dtype=torch.int64) * (bases_n // a.large_genomes)
        l_tx = torch.from_numpy(leaves[np.arange(a.large_genomes) * NG // a.large_genomes].astype(np.int32)).to(dev)
        torch.cuda.synchronize()
        ctx.build_begin(1 << 28)
        ctx.build_add(pool.data_ptr(), l_off.data_ptr(), a.large_genomes, bases_n, l_tx.data_ptr())     # F: every k-mer of the bases
        ctx.build_count_begin()
        ctx.build_count_add(pool.data_ptr(), off.data_ptr(), n_seq, bases_n, np.arange(n_seq, dtype=np.uint32))
        sc = ctx.build_count_stats()
        ctx.build_end()
        say("count pass, %d bases as %d genomes of %d: %.4f s, %d launches (%.1f us a launch), %d lookups, %.2f G lookups/s" %
            (bases_n, n_seq, seq_len, sc["add_s"], sc["launches"], sc["add_s"] / sc["launches"] * 1e6, sc["lookups"], sc["lookups"] / sc["add_s"] / 1e9))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
