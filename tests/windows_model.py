"""The window session's model: every window of L bases is cut out as a read of its own and classified by the CPU oracle
(oracle.classify_batch), one unpaired read per window.  Returns what bns_windows_add writes (the d_taxon image) and what
bns_windows_read reports (the pairs, counted with numpy.unique), and writes the text `bonsai distrib` writes.  Test
infrastructure only."""
import numpy as np

NONE = 0xFFFFFFFF


def n_windows(n, L):
    return max(0, n - L + 1)


def calls(oracle, table, tax, k, seq, L, gaps=None, canon=True, spaced_intended=False, nthreads=16):
    """the oracle's taxon of every window of one sequence (uint32[max(0, n - L + 1)])"""
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    nw = n_windows(seq.size, L)
    if nw == 0:
        return np.zeros(0, dtype=np.uint32)
    cut = np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(seq, L)).reshape(-1)
    offsets = np.arange(nw + 1, dtype=np.uint64) * np.uint64(L)
    res = oracle.classify_batch(table, tax, k, cut, offsets, gaps=gaps, canon=canon, spaced_intended=spaced_intended, nthreads=nthreads)
    return res["taxon"].astype(np.uint32)


def pairs_of(seq_taxids, called):
    """(seq_taxid, called, count) ascending by (seq_taxid, called) from one entry per window"""
    key = (np.asarray(seq_taxids, dtype=np.uint64) << np.uint64(32)) | np.asarray(called, dtype=np.uint64)
    u, n = np.unique(key, return_counts=True)
    return (u >> np.uint64(32)).astype(np.uint32), (u & np.uint64(0xFFFFFFFF)).astype(np.uint32), n.astype(np.uint64)


def windows(oracle, table, tax, k, bases, offsets, taxids, L, **kw):
    """-> (image uint32[total_bases], (seq_taxid, called, count))"""
    offsets = np.asarray(offsets, dtype=np.uint64)
    total = int(offsets[-1])
    image = np.full(total, NONE, dtype=np.uint32)
    who, what = [], []
    for s in range(offsets.size - 1):
        o, e = int(offsets[s]), int(offsets[s + 1])
        c = calls(oracle, table, tax, k, bases[o:e], L, **kw)
        image[o:o + c.size] = c
        who.append(np.full(c.size, int(taxids[s]), dtype=np.uint64))
        what.append(c)
    who = np.concatenate(who) if who else np.zeros(0, np.uint64)
    what = np.concatenate(what) if what else np.zeros(0, np.uint32)
    return image, pairs_of(who, what)


def merge_pairs(*parts):
    """the pairs of several adds: counts of equal pairs added up"""
    key = np.concatenate([(p[0].astype(np.uint64) << np.uint64(32)) | p[1].astype(np.uint64) for p in parts])
    cnt = np.concatenate([p[2] for p in parts])
    u, inv = np.unique(key, return_inverse=True)
    out = np.zeros(u.size, dtype=np.uint64)
    np.add.at(out, inv, cnt)
    return (u >> np.uint64(32)).astype(np.uint32), (u & np.uint64(0xFFFFFFFF)).astype(np.uint32), out


def distrib_text(seq_taxid, called, count):
    """the file of `bonsai distrib`: a line per called taxon != 0, ascending; entries genome:windows called here:all windows of the
    genome (those called 0 included), ascending by genome taxid"""
    total = {}
    for g, n in zip(seq_taxid.tolist(), count.tolist()):
        total[g] = total.get(g, 0) + n
    lines = {}
    for g, t, n in zip(seq_taxid.tolist(), called.tolist(), count.tolist()):
        if t:
            lines.setdefault(t, []).append((g, n))
    out = ["mapped_taxid\tgenome_taxids:kmers_mapped:total_genome_kmers\n"]
    for t in sorted(lines):
        out.append("%d\t%s\n" % (t, " ".join("%d:%d:%d" % (g, n, total[g]) for g, n in sorted(lines[t]))))
    return "".join(out).encode()
