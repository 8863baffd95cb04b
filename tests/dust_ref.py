"""Reference for low-complexity masking (bns_set_dust; DESIGN.md "Defined behaviour"): symmetric DUST with window W and level T.

    brute_mask       straight from the definition: every interval of every run, every sub-interval, integer cross-products
    recurrence_mask  the recurrence M(i, j) = max(S(i, j), M(i + 1, j), M(i, j - 1)), vectorised over the start triplets (long inputs)
    batch_masks      recurrence_mask of a list of sequences in one pass
    substitute       the sequence with its masked bases replaced by 'N'
    gen_seq / gen_batch   the generator the tests use: random stretches mixed with homopolymers and short tandem repeats

A helper, not a test.  Sequences are bytes; masks are numpy bool arrays of the sequence's length."""
import numpy as np

PARAMS = [(64, 20), (16, 20), (8, 10), (33, 40), (64, 10)]

_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c | 0x20] = _i                                 # the packed image folds case: acgt are valid bases


def _runs(seq):
    """(start, end) of every maximal run of valid bases"""
    code = _CODE[np.frombuffer(bytes(seq), dtype=np.uint8)]
    ok = np.concatenate(([0], (code != 255).astype(np.int8), [0]))
    d = np.diff(ok)
    return code, list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def _triplets(code):
    c = code.astype(np.int64)
    return c[:-2] * 16 + c[1:-1] * 4 + c[2:]


def brute_mask(seq, W=64, T=20):
    code, runs = _runs(seq)
    mask = np.zeros(len(seq), dtype=bool)
    lmax = W - 2
    for r0, r1 in runs:
        if r1 - r0 < 4:
            continue
        tr = _triplets(code[r0:r1])
        nt = tr.size
        num = np.zeros((nt, lmax + 1), dtype=np.int64)    # num[i, l]: sum c (c - 1) / 2 of the l triplets from i on; the score is num / (l - 1)
        for i in range(nt):
            for l in range(2, min(lmax, nt - i) + 1):
                c = np.bincount(tr[i:i + l], minlength=64)
                num[i, l] = int((c * (c - 1) // 2).sum())
        for i in range(nt):
            for l in range(2, min(lmax, nt - i) + 1):
                n0, d0 = int(num[i, l]), l - 1
                if 10 * n0 <= T * d0:
                    continue
                a = np.arange(l)[:, None]                 # sub-interval: a triplets in, m long, a + m <= l
                m = np.arange(2, l + 1)[None, :]
                inside = a + m <= l
                sub = num[i:i + l, 2:l + 1]
                if np.any((sub * d0 > n0 * (m - 1)) & inside):
                    continue                              # a sub-interval scores strictly higher
                mask[r0 + i:r0 + i + l + 2] = True
    return mask


def recurrence_mask(seq, W=64, T=20):
    """all runs of the sequence at once: entry i is the start triplet at base i, active at length l while l valid triplets follow it"""
    n = len(seq)
    if n < 4:
        return np.zeros(n, dtype=bool)
    code = _CODE[np.frombuffer(bytes(seq), dtype=np.uint8)]
    ok = code != 255
    tv = ok[:-2] & ok[1:-1] & ok[2:]
    tr = np.where(tv, _triplets(np.where(ok, code, 0)), 0).astype(np.int64)
    nt = tr.size
    # valid triplets in a row from i on, capped at W - 2
    lmax = W - 2
    run = np.zeros(nt + 1, dtype=np.int32)
    stop = np.flatnonzero(~tv)
    nxt = np.full(nt, nt, dtype=np.int64)
    if stop.size:
        pos = np.searchsorted(stop, np.arange(nt), side="left")
        nxt = np.where(pos < stop.size, stop[np.minimum(pos, stop.size - 1)], nt)
    run[:nt] = np.minimum(nxt - np.arange(nt), lmax)
    cnt = np.zeros((nt, 64), dtype=np.uint8)
    on = np.flatnonzero(run[:nt] >= 1)
    cnt[on, tr[on]] = 1
    num = np.zeros(nt, dtype=np.int64)
    mn = np.zeros(nt + 1, dtype=np.int64); md = np.ones(nt + 1, dtype=np.int64)     # M of length l - 1 per start, as mn / md
    best = np.zeros(nt, dtype=np.int64)
    for l in range(2, lmax + 1):
        i = np.flatnonzero(run[:nt] >= l)
        if not i.size:
            break
        t = tr[i + l - 1]
        num[i] += cnt[i, t]
        cnt[i, t] += 1
        den = l - 1
        on_, od = mn[i], md[i]                            # M(i, j - 1)
        rn, rd = mn[i + 1], md[i + 1]                     # M(i + 1, j): start i + 1 was active at l - 1 when i is at l
        right = rn * od > on_ * rd
        pn = np.where(right, rn, on_); pd = np.where(right, rd, od)
        ni = num[i]
        ge = ni * pd >= pn * den
        best[i[ge & (10 * ni > T * den)]] = l
        mn[i] = np.where(ge, ni, pn)
        md[i] = np.where(ge, den, pd)
    cover = np.zeros(n + 1, dtype=np.int64)
    s = np.flatnonzero(best)
    np.add.at(cover, s, 1)
    np.add.at(cover, s + best[s] + 2, -1)
    return np.cumsum(cover)[:n] > 0


def batch_masks(seqs, W=64, T=20):
    """recurrence_mask of every sequence of a list, in one pass (an 'N' between two sequences ends every run)"""
    joined = b"N".join(bytes(s) for s in seqs)
    m = recurrence_mask(joined, W, T)
    out, at = [], 0
    for s in seqs:
        out.append(m[at:at + len(s)].copy())
        at += len(s) + 1
    return out


def substitute(seq, mask):
    b = np.frombuffer(bytes(seq), dtype=np.uint8).copy()
    b[np.asarray(mask, dtype=bool)] = ord("N")
    return b.tobytes()


def gen_seq(rng, length):
    """segments with probability 0.5 / 0.2 / 0.3: 5-40 random bases | one base 5-40 times | a random unit of 2-6 bases 3-12 times"""
    parts, n = [], 0
    while n < length:
        u = rng.random()
        if u < 0.5:
            seg = rng.integers(0, 4, size=int(rng.integers(5, 41)))
        elif u < 0.7:
            seg = np.full(int(rng.integers(5, 41)), int(rng.integers(0, 4)))
        else:
            seg = np.tile(rng.integers(0, 4, size=int(rng.integers(2, 7))), int(rng.integers(3, 13)))
        parts.append(seg); n += seg.size
    if not parts:
        return b""
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.concatenate(parts)[:length]].tobytes()


def gen_batch(rng, lengths):
    return [gen_seq(rng, int(n)) for n in lengths]


def masked_share(seqs, W, T):
    tot = sum(len(s) for s in seqs)
    return sum(int(m.sum()) for m in batch_masks(seqs, W, T)) / max(1, tot)
