"""The distinct k-mer sketches (bns_sketch_enable / bns_sketch_read, `bonsai classify -R -u`) restated in numpy from DESIGN.md's
"Defined behaviour": fmix64, the registers, the estimate, tally_bin, the clade merge and the eight-column report.  Keys come from the
oracle's encoder and values from the oracle's table: nothing here calls the code under test.  Test infrastructure only."""
import math
from collections import defaultdict

import numpy as np

M = 4096
ABSENT = 0xFFFFFFFF
U = np.uint64


def fmix64(x):
    x = np.ascontiguousarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U(33); x *= U(0xff51afd7ed558ccd)
        x ^= x >> U(33); x *= U(0xc4ceb9fe1a85ec53)
        x ^= x >> U(33)
    return x


def clz64(w):
    """leading zeros of each non-zero uint64"""
    w = w.copy()
    n = np.zeros(w.size, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        small = w < (U(1) << U(64 - s))
        n[small] += s
        w[small] <<= U(s)
    return n


def registers(keys):
    """the 4096 register bytes of a set (any multiset) of uint64 keys"""
    reg = np.zeros(M, dtype=np.uint8)
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    if keys.size == 0:
        return reg
    h = fmix64(keys)
    j = (h >> U(52)).astype(np.int64)
    w = h << U(12)
    rho = np.where(w == 0, 53, clz64(w) + 1).astype(np.uint8)
    np.maximum.at(reg, j, rho)
    return reg


def estimate(reg):
    """floor(E + 0.5) in IEEE doubles; the sum of 2^-reg runs rank by rank from 0 upwards, as bns::hll_estimate's does"""
    cnt = np.bincount(np.asarray(reg, dtype=np.int64), minlength=64)
    if cnt[0] == M:
        return 0
    s = 0.0
    for r in range(64):
        s += float(cnt[r]) * math.ldexp(1.0, -r)
    e = 0.7213 / (1.0 + 1.079 / M) * M * M / s
    if e <= 2.5 * M and cnt[0]:
        e = M * math.log(M / float(cnt[0]))
    return int(math.floor(e + 0.5))


def chain_ok(parent):
    """ok[t]: t is a key of the parent array whose chain reaches a root with parent 0 (NODE_CHAIN_OK)"""
    parent = np.asarray(parent, dtype=np.uint32)
    n = parent.size
    ok = np.zeros(n, dtype=bool)
    for t in range(1, n):
        if parent[t] == ABSENT:
            continue
        v, steps = t, 0
        while steps <= n:
            p = int(parent[v])
            if p == 0:
                ok[t] = True
                break
            if p == ABSENT or p >= n or parent[p] == ABSENT:
                break
            v = p; steps += 1
    return ok


def bins_of(vals, parent, ok=None):
    """tally_bin of table values"""
    n = len(parent)
    ok = chain_ok(parent) if ok is None else ok
    vals = np.asarray(vals, dtype=np.int64)
    inside = (vals > 0) & (vals < n)
    good = np.zeros(vals.size, dtype=bool)
    good[inside] = ok[vals[inside]]
    return np.where(vals == 0, 0, np.where(good, vals, n)).astype(np.int64)


def keys_by_bin(oracle, table, parent, reads, k, gaps=None, canon=True, spaced_intended=False):
    """{bin: uint64 keys (with repeats)} over the reads' k-mers that the table holds"""
    ks = [oracle.encode(bytes(r.tobytes() if hasattr(r, "tobytes") else r), k, gaps=gaps, canon=canon, spaced_intended=spaced_intended)
          for r in reads]
    keys = np.concatenate(ks) if ks else np.zeros(0, np.uint64)
    if keys.size == 0:
        return {}
    vals, found = table.get_batch(keys)
    keys, vals = keys[found != 0], vals[found != 0]
    b = bins_of(vals, parent)
    return {int(x): keys[b == x] for x in np.unique(b)}


def sketches(oracle, table, parent, reads, k, **kw):
    """(bins ascending uint32[s], registers uint8[s, 4096]) as bns_sketch_read returns them when every bin got a sketch"""
    kb = keys_by_bin(oracle, table, parent, reads, k, **kw)
    bins = np.array(sorted(kb), dtype=np.uint32)
    regs = np.stack([registers(kb[int(b)]) for b in bins]) if bins.size else np.zeros((0, M), np.uint8)
    return bins, regs


def clade_estimates(bins, regs, pairs):
    """{node: estimate of the register-wise maximum over the sketched bins in its subtree} for the nodes of (child, parent) pairs;
    key n (any bin that is no chain-ok node of the pairs) is not merged anywhere"""
    par = {c: (0 if c == 1 else p) for c, p in pairs}
    kids = defaultdict(list)
    for c, p in par.items():
        if p != 0:
            kids[p].append(c)
    own = {int(b): regs[i] for i, b in enumerate(bins)}
    out = {}

    def merged(v):
        r = own.get(v, np.zeros(M, np.uint8)).copy()
        for ch in kids[v]:
            r = np.maximum(r, merged(ch))
        out[v] = estimate(r)
        return r

    for root in (c for c, p in par.items() if p == 0):
        merged(root)
    return out


def add_column(report7, distinct, n):
    """the seven-column report text with the distinct column put in after the direct count: distinct[taxid] for a node's line, 0 on
    the unclassified line, distinct[n] on the (not in taxonomy) line"""
    out = []
    for line in report7.splitlines():
        f = line.split("\t")
        tid = int(f[4])
        d = 0 if f[3] == "U" else (distinct.get(n, 0) if tid == 4294967295 else distinct.get(tid, 0))
        out.append("\t".join(f[:3] + [str(d)] + f[3:]) + "\n")
    return "".join(out)
