"""A DEFLATE writer for tests, from RFC 1951 alone: streams that are legal and that zlib's encoder never writes (codes of 11 to 15
bits on frequent symbols, distances up to 32768, length 258 as symbol 284 + 31, dense runs of matches, rare header and block shapes),
and illegal ones with a known answer.  zlib's INFLATER is the witness of every stream made here (tests/test_deflate_craft.py).

A token is an int (a literal), bytes (a run of literals), a 4-tuple (length symbol, extra, distance symbol, extra) -- the caller
chooses the symbols, so 258 can be 285 or 284 + 31 -- or ("raw", value, nbits): bits as they are.  A distance symbol of None writes
the length alone (the illegal streams go on with raw bits)."""
import collections
import functools
import struct
import zlib

import numpy as np

# RFC 1951 3.2.5: length symbols 257..285 and distance symbols 0..29
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
# 3.2.7: the order in which the code-length code's lengths are sent
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
# 3.2.6
FIXED_LL = {s: (8 if s < 144 else 9 if s < 256 else 7 if s < 280 else 8) for s in range(288)}
FIXED_D = {s: 5 for s in range(32)}          # (30 and 31 have codes that no stream may use)
LL_DIRECT, D_DIRECT = 10, 9                  # the decoders' direct tables: longer codes take their other paths
WINDOW = 32768
BGZF_TEXT = 65280


def _rev(v, k):
    return int(format(v, "0%db" % k)[::-1], 2) if k else 0


def kraft(lens):
    """sum of 2^-l over the code, in units of 2^-15"""
    return sum(32768 >> l for l in lens.values() if l)


def canonical(lens):
    """{symbol: length} -> {symbol: (code as it goes into an LSB-first stream, length)} (3.2.2).  An over-subscribed assignment gets
    codes too (they wrap): an illegal header is all such a stream is read for."""
    count = collections.Counter(l for l in lens.values() if l)
    code, nxt = 0, {}
    for l in range(1, 16):
        code = (code + count.get(l - 1, 0)) << 1
        nxt[l] = code
    out = {}
    for s in sorted(lens):
        l = lens[s]
        if l:
            out[s] = (_rev(nxt[l] & ((1 << l) - 1), l), l)
            nxt[l] += 1
    return out


def complete(lens, spare):
    """complete a partial assignment to a Kraft sum of exactly 1 (maximum length 15) with symbols from `spare`: one code for every set
    bit of what is missing, the longest on the first spare symbols"""
    lens = dict(lens)
    missing = 32768 - kraft(lens)
    assert missing >= 0, "over-subscribed"
    spare = [s for s in spare if not lens.get(s)]
    for l in range(15, 0, -1):
        if missing & (32768 >> l):
            assert spare, "no symbol left to complete the code with"
            lens[spare.pop(0)] = l
    return lens


def flat(symbols):
    """a complete code over `symbols`, all lengths k or k - 1 (one symbol: the one-bit code alone, which only a distance code may be)"""
    symbols = sorted(set(symbols))
    n = len(symbols)
    if n == 1:
        return {symbols[0]: 1}
    k = (n - 1).bit_length()
    short = (1 << k) - n
    return {s: (k - 1 if i < short else k) for i, s in enumerate(symbols)}


def ladder(symbols):
    """lengths 1, 2, ... 14, 15, 15 over exactly sixteen symbols, in their order"""
    assert len(symbols) == 16 and len(set(symbols)) == 16
    return {s: min(i + 1, 15) for i, s in enumerate(symbols)}


def len_sym(length, alt258=False):
    """(length symbol, extra) of a match length; alt258: 258 as 284 + 31"""
    if length == 258:
        return (284, 31) if alt258 else (285, 0)
    i = max(j for j in range(28) if LEN_BASE[j] <= length)
    assert length - LEN_BASE[i] < (1 << LEN_EXTRA[i])
    return 257 + i, length - LEN_BASE[i]


def dist_sym(dist):
    i = max(j for j in range(30) if DIST_BASE[j] <= dist)
    assert 0 <= dist - DIST_BASE[i] < (1 << DIST_EXTRA[i])
    return i, dist - DIST_BASE[i]


def match(length, dist, alt258=False):
    return len_sym(length, alt258) + dist_sym(dist)


def token_len(t):
    return LEN_BASE[t[0] - 257] + t[1]


def token_dist(t):
    return DIST_BASE[t[2]] + t[3]


def expand(tokens, out=None):
    """the simulator: the text a token list stands for (appended to `out`)"""
    out = bytearray() if out is None else out
    for t in tokens:
        if type(t) is int:
            out.append(t)
        elif type(t) is bytes:
            out += t
        elif t[0] != "raw":
            n, d = token_len(t), token_dist(t)
            assert 1 <= d <= len(out), "a match reaching in front of the text"
            if d >= n:
                out += out[len(out) - d:len(out) - d + n]
            else:
                out += (bytes(out[-d:]) * (n // d + 1))[:n]
    return out


def used_symbols(tokens):
    ll, d = {256}, set()
    for t in tokens:
        if type(t) is int:
            ll.add(t)
        elif type(t) is bytes:
            ll.update(t)
        elif t[0] != "raw":
            ll.add(t[0])
            if t[2] is not None:
                d.add(t[2])
    return ll, d


def auto_rle(seq):
    """a plan for Writer.dynamic's `rle`: greedy runs over the concatenated lengths (a run does not know where the literal/length
    lengths end, so it crosses into the distance lengths whenever the values allow)"""
    plan, i, n = [], 0, len(seq)
    while i < n:
        j = i
        while j < n and seq[j] == seq[i]:
            j += 1
        run = j - i
        if seq[i] == 0 and run >= 3:
            r = min(run, 138)
            plan.append((18 if r >= 11 else 17, r))
            i += r
        elif seq[i] != 0 and run >= 4:
            plan.append(1)
            r = min(run - 1, 6)
            plan.append((16, r))
            i += 1 + r
        else:
            plan.append(1)
            i += 1
    return plan


class Writer:
    """bits LSB first.  Fields are collected (value, width <= 16) and packed at the end by numpy; Huffman codes are kept bit-reversed,
    so a symbol is one field."""

    def __init__(self):
        self._chunks, self._v, self._k = [], [], []
        self.nbits = 0
        self.census = collections.Counter()

    def put(self, v, k):
        assert 0 <= k <= 16 and 0 <= v < (1 << k)
        if k:
            self._v.append(v)
            self._k.append(k)
            self.nbits += k

    def _seal(self):
        if self._v:
            self._chunks.append((np.array(self._v, dtype=np.uint64), np.array(self._k, dtype=np.int64)))
            self._v, self._k = [], []

    def put_arrays(self, vals, widths):
        self._seal()
        self._chunks.append((np.asarray(vals, dtype=np.uint64), np.asarray(widths, dtype=np.int64)))
        self.nbits += int(self._chunks[-1][1].sum())

    def align(self):
        self.put(0, -self.nbits & 7)

    def getvalue(self):
        self._seal()
        nbytes = (self.nbits + 7) // 8
        if not self._chunks:
            return b""
        vals = np.concatenate([c[0] for c in self._chunks])
        widths = np.concatenate([c[1] for c in self._chunks])
        start = np.cumsum(widths) - widths
        sh = vals << (start & 7).astype(np.uint64)                 # at most 16 + 7 bits: three bytes
        at = start >> 3
        acc = np.zeros(nbytes + 3, dtype=np.float64)               # (fields own disjoint bits: a byte's sum is its OR, exact in a double)
        for b in range(3):
            acc += np.bincount(at + b, weights=((sh >> np.uint64(8 * b)) & np.uint64(255)).astype(np.float64), minlength=nbytes + 3)
        return acc[:nbytes].astype(np.uint8).tobytes()

    # ---- blocks -------------------------------------------------------------------------------------------------------------------
    def stored(self, data, final=False):
        assert len(data) <= 65535
        self.put(int(final), 1)
        self.put(0, 2)
        self.census["stored_behind_bit:%d" % (self.nbits & 7)] += 1
        self.align()
        self.put(len(data), 16)
        self.put(len(data) ^ 0xFFFF, 16)
        if data:
            self.put_arrays(np.frombuffer(bytes(data), dtype=np.uint8), np.full(len(data), 8))
        self.census["stored"] += 1

    def fixed(self, tokens, final=False, eob=True):
        self.put(int(final), 1)
        self.put(1, 2)
        self._tokens(tokens, canonical(FIXED_LL), canonical(FIXED_D), eob)
        self.census["fixed"] += 1

    def dynamic(self, tokens, ll_lens, d_lens, final=False, rle=None, hlit=None, hdist=None, cl_lens=None, eob=True, check=True):
        """rle: None (every length plainly), "auto", or a plan: an int n for "the next n lengths plainly", (16 | 17 | 18, count) for a
        repeat that covers the next `count` lengths of literal/length and distance lengths taken together.  hlit / hdist / cl_lens and
        check=False are for illegal headers: nothing is verified then."""
        nll = hlit if hlit is not None else max([257] + [s + 1 for s, l in ll_lens.items() if l])
        nd = hdist if hdist is not None else max([1] + [s + 1 for s, l in d_lens.items() if l])
        seq = [ll_lens.get(i, 0) for i in range(nll)] + [d_lens.get(i, 0) for i in range(nd)]
        if check:
            assert nll <= 286 and nd <= 30 and ll_lens.get(256) and kraft(ll_lens) == 32768, "literal/length code"
            assert kraft(d_lens) == 32768 or sorted(l for l in d_lens.values() if l) in ([], [1]), "distance code"
        plan = [len(seq)] if rle is None else auto_rle(seq) if rle == "auto" else rle
        ops, i = [], 0                                                # (code-length symbol, extra value, extra bits)
        for p in plan:
            if type(p) is int:
                ops += [(l, 0, 0) for l in seq[i:i + p]]
                i += p
                continue
            sym, cnt = p
            lo, hi, xb = {16: (3, 6, 2), 17: (3, 10, 3), 18: (11, 138, 7)}[sym]
            if check:
                assert lo <= cnt <= hi and i + cnt <= len(seq) and (i > 0 or sym != 16)
                assert all(l == (seq[i - 1] if sym == 16 else 0) for l in seq[i:i + cnt]), "the repeat does not say what the lengths are"
                if i < nll < i + cnt:
                    self.census["repeat_across_boundary"] += 1
            ops.append((sym, cnt - lo, xb))
            i += cnt
        assert not check or i == len(seq)
        if cl_lens is None:
            used = sorted({o[0] for o in ops})
            if len(used) == 1:                                        # (zlib wants the code-length code complete: a second one-bit code)
                used.append(0 if used[0] else 1)
            cl_lens = flat(used)
        assert max(cl_lens.values()) <= 7
        hclen = max([4] + [j + 1 for j, s in enumerate(CL_ORDER) if cl_lens.get(s)])
        self.put(int(final), 1)
        self.put(2, 2)
        self.put(nll - 257, 5)
        self.put(nd - 1, 5)
        self.put(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.put(cl_lens.get(s, 0), 3)
        clc = canonical(cl_lens)
        for sym, xv, xb in ops:
            self.put(*clc[sym])
            self.put(xv, xb)
        self._tokens(tokens, canonical(ll_lens), canonical(d_lens), eob)
        self.census["dynamic"] += 1
        self.census["hlit:%d" % nll] += 1
        self.census["hdist:%d" % nd] += 1
        self.census["dist_codes:%d" % sum(1 for l in d_lens.values() if l)] += 1
        self.census["ll_codes:%d" % sum(1 for l in ll_lens.values() if l)] += 1

    def _tokens(self, tokens, llc, dc, eob):
        cs, put = self.census, self.put
        llv = np.zeros(288, dtype=np.uint64)
        llw = np.zeros(288, dtype=np.int64)
        for s, (c, l) in llc.items():
            llv[s], llw[s] = c, l
        lv, lw = [int(x) for x in llv[:256]], [int(x) for x in llw[:256]]
        any_deep = max(lw) > LL_DIRECT
        n_sym = run = 0
        for t in tokens:
            if type(t) is int or type(t) is bytes:
                run = 0
            if type(t) is int:
                c, l = llc[t]
                put(c, l)
                cs["ll_deep"] += l > LL_DIRECT
                n_sym += 1
            elif type(t) is bytes:
                if len(t) < 512:                                      # (short runs: list appends; long ones: arrays)
                    ws = [lw[b] for b in t]
                    assert all(ws), "a literal without a code"
                    self._v.extend([lv[b] for b in t])
                    self._k.extend(ws)
                    self.nbits += sum(ws)
                    if any_deep:
                        cs["ll_deep"] += sum(x > LL_DIRECT for x in ws)
                else:
                    a = np.frombuffer(t, dtype=np.uint8)
                    w = llw[a]
                    assert w.all(), "a literal without a code"
                    self.put_arrays(llv[a], w)
                    cs["ll_deep"] += int((w > LL_DIRECT).sum())
                n_sym += len(t)
            elif t[0] == "raw":
                put(t[1], t[2])
            else:
                ls, lx, ds, dx = t
                c, l = llc[ls]
                put(c, l)
                put(lx, LEN_EXTRA[ls - 257])
                cs["ll_deep"] += l > LL_DIRECT
                cs["len:%d" % (LEN_BASE[ls - 257] + lx)] += 1
                cs["lsym:%d" % ls] += 1
                if LEN_BASE[ls - 257] + lx == 258:
                    cs["len258_sym%d" % ls] += 1
                n_sym += 1
                if ds is None:
                    continue
                c, l = dc[ds]
                put(c, l)
                put(dx, DIST_EXTRA[ds])
                d = DIST_BASE[ds] + dx
                cs["matches"] += 1
                cs["d_deep"] += l > D_DIRECT
                cs["dist_gt_32506"] += d > 32506
                cs["dist_32768"] += d == 32768
                cs["dist_900_1300"] += 900 <= d <= 1300
                cs["dist_lt_len"] += d < LEN_BASE[ls - 257] + lx
                run += 1
                cs["longest_run_of_matches"] = max(cs["longest_run_of_matches"], run)
                if dx == 0:
                    cs["dsym:%d:zeros" % ds] += 1
                if dx == (1 << DIST_EXTRA[ds]) - 1:
                    cs["dsym:%d:ones" % ds] += 1
        if eob:
            c, l = llc[256]
            put(c, l)
            cs["ll_deep"] += l > LL_DIRECT
            cs["eob_deep"] += l > LL_DIRECT
        if n_sym == 0:
            cs["empty_blocks"] += 1
        if n_sym == 1:
            cs["one_symbol_blocks"] += 1


# ---- wrappers -------------------------------------------------------------------------------------------------------------------------
def gzip_member(raw, text, name=None):
    """RFC 1952: header (with FNAME when `name`), the stream, CRC-32, ISIZE"""
    head = b"\x1f\x8b\x08" + (b"\x08" if name else b"\x00") + b"\0\0\0\0\x00\xff" + (name + b"\0" if name else b"")
    return head + raw + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text) & 0xFFFFFFFF)


def bgzf_member(raw, text):
    """a BGZF member (SAM specification 4.1): the extra field BC with BSIZE = the member's size - 1"""
    total = 18 + len(raw) + 8
    assert total <= 65536 and len(text) <= 65536, "too large for a BGZF member"
    head = b"\x1f\x8b\x08\x04\0\0\0\0\x00\xff" + struct.pack("<HBBHH", 6, 66, 67, 2, total - 1)
    return head + raw + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text))


BGZF_EOF = bgzf_member(b"\x03\x00", b"")


# ---- token sources --------------------------------------------------------------------------------------------------------------------
def random_tokens(rng, n_bytes, ll_syms, d_syms, start=0, p_match=0.5, run=(1, 1), opener=False, alt258=True):
    """tokens for exactly n_bytes of text behind `start` bytes already there: symbols drawn evenly from ll_syms (literals and length
    symbols; end-of-block is not a token) and d_syms, every distance <= the bytes so far.  run: literals come in runs of this many.
    opener (True, or the length symbol to use): the first token is a match at distance min(position, 32768), and the one behind it
    copies the same bytes again."""
    import random
    r = random.Random(int(rng.integers(1 << 62)))                  # (scalar draws: many times faster than the generator's)
    lits = bytes(sorted(s for s in ll_syms if s < 256))
    lsyms = [s for s in ll_syms if s > 256]
    d_syms = sorted(d_syms)
    assert lits
    pos, end, toks = start, start + n_bytes, []

    def pick(top):                                                  # all zeros and all ones are as likely as all the rest
        q = r.randrange(4)
        return 0 if q == 0 else top if q == 1 else r.randrange(top + 1)

    def try_match():
        nonlocal pos
        ls = r.choice(lsyms)
        lx = pick((1 << LEN_EXTRA[ls - 257]) - 1)
        if ls == 284 and lx == 31 and not alt258:
            lx = 30
        n = LEN_BASE[ls - 257] + lx
        ok = [d for d in d_syms if DIST_BASE[d] <= pos]
        if not ok or pos + n > end:
            return False
        ds = r.choice(ok)
        dx = pick(min((1 << DIST_EXTRA[ds]) - 1, pos - DIST_BASE[ds]))
        toks.append((ls, lx, ds, dx))
        pos += n
        return True

    if opener and lsyms and pos:
        far = min(pos, WINDOW)
        ds, dx = dist_sym(far)
        if ds in d_syms:
            ls = lsyms[0] if opener is True else opener
            n = LEN_BASE[ls - 257]
            if pos + 2 * n <= end:
                toks.append((ls, 0, ds, dx))
                pos += n
                near = [d for d in d_syms if DIST_BASE[d] <= n]       # overlapping: what the opener brought is copied again
                if near:
                    toks.append((ls, 0, max(near), 0))
                    pos += n
    while pos < end:
        if lsyms and r.random() < p_match and try_match():
            continue
        k = min(r.randint(run[0], run[1]), end - pos)
        toks.append(bytes(r.choices(lits, k=k)) if k > 1 else r.choice(lits))
        pos += k
    return toks


def text_tokens(text, lo, hi, rng, ll_ok=None, d_ok=None, p_match=0.6, opener=False, alt258=True):
    """tokens for text[lo:hi] with matches taken from real earlier occurrences (bytes.rfind inside the 32 KiB window): the decoded text
    is the text.  ll_ok / d_ok: the only length / distance symbols there are codes for.  opener: the first token is a match at the
    largest distance at which the window holds the next three bytes (32768 where the text repeats itself there)."""
    fits = None
    if ll_ok is not None:                                           # the longest length <= n that the allowed symbols can say
        can = {LEN_BASE[s - 257] + x for s in ll_ok if s > 256 for x in range(1 << LEN_EXTRA[s - 257])}
        fits = [max([c for c in can if c <= n], default=0) for n in range(259)]
    toks, p, lit0, first = [], lo, lo, opener
    while p < hi:
        m = None
        if p > 0 and hi - p >= 3 and (first or rng.random() < p_match):
            w0, found = max(0, p - WINDOW), None
            if first:
                q = text.find(text[p:p + 3], w0, p + 2)
                if q >= 0:
                    n, top = 3, min(258, hi - p)
                    while n < top and text[q + n] == text[p + n]:
                        n += 1
                    found = (n, q)
            else:
                for n in (int(rng.integers(3, 259)), 9, 4, 3):
                    n = min(n, hi - p)
                    q = text.rfind(text[p:p + n], w0, p + n - 1)
                    if q >= 0:
                        found = (n, q)
                        break
            if found:
                n, q = found
                n = fits[n] if fits else n
                ds, dx = dist_sym(p - q)
                if n >= 3 and (d_ok is None or ds in d_ok):
                    ls, lx = len_sym(n, alt258 and bool(rng.integers(2)))
                    if ll_ok is not None and ls not in ll_ok:
                        ls, lx = len_sym(n, not (ls == 284))
                    m = (ls, lx, ds, dx)
        first = False
        if m is None:
            p += 1
            continue
        if p > lit0:
            toks.append(text[lit0:p])
        toks.append(m)
        p += token_len(m)
        lit0 = p
    if hi > lit0:
        toks.append(text[lit0:hi])
    return toks


def fastq_periodic(rng, n_records, period=128):
    """FASTQ of 256-byte records whose sequence and quality lines repeat `period` records (32768 bytes at 128) back under another
    name: a match at distance 32768 is there for every position inside them"""
    base = []
    for i in range(period):
        s = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 121))
        q = bytes(rng.integers(35, 75, 121).astype(np.uint8))
        base.append(s + b"\n+\n" + q + b"\n")
    return b"".join(b"@r%07d\n" % i + base[i % period] for i in range(n_records))


# the sixteen symbols of the deep codes, shortest code first: lengths 1..14, 15, 15 ("fwd") and the same ladder turned round ("rev":
# the end-of-block symbol changes places with the first literal, so that it stays deep).  The 11- to 15-bit codes -- the last six of a
# list -- are in both a literal or two, length symbols with extra bits, and the end of the block; 284 is there for 258 as 284 + 31.
DEEP_LL = {"fwd": [65, 269, 67, 277, 71, 284, 10, 84, 260, 285, 48, 270, 278, 283, 43, 256],
           "rev": [65, 43, 283, 278, 270, 48, 285, 260, 84, 10, 284, 71, 277, 67, 269, 256]}
DEEP_D = {"fwd": [0, 1, 2, 3, 5, 8, 10, 12, 15, 17, 19, 21, 24, 26, 28, 29],
          "rev": [29, 28, 26, 24, 21, 19, 17, 15, 12, 10, 8, 5, 3, 2, 1, 0]}


def deep_lens(ll, d):
    """(literal/length lengths, distance lengths): 1..14, 15, 15 in orientation ll / d"""
    return ladder(DEEP_LL[ll]), ladder(DEEP_D[d])


def deep_over(symbols, short):
    """a complete code over `symbols` (more than sixteen, as real text needs): the eight of `short` get 1..8 bits, all the others share
    the last 2^-8 of the code space -- 11 bits and more for up to 128 of them"""
    rest = flat([s for s in symbols if s not in short])
    assert len(short) == 8 and max(rest.values()) <= 7
    lens = {s: 8 + l for s, l in rest.items()}
    lens.update({s: i + 1 for i, s in enumerate(short)})
    assert kraft(lens) == 32768
    return lens


def auto_block(w, tokens, final=False, rle="auto", spare_ll=range(286), extra_d=()):
    """a dynamic block over exactly the symbols the tokens use (plus extra_d), flat codes"""
    ll, d = used_symbols(tokens)
    d |= set(extra_d)
    ll_lens = flat(ll) if len(ll) > 1 else complete(flat(ll), [s for s in spare_ll if s not in ll])
    w.dynamic(tokens, ll_lens, flat(d) if d else {}, final, rle=rle)


# ---- the catalogue --------------------------------------------------------------------------------------------------------------------
def _case(build):
    w, pre = Writer(), bytearray()
    build(w, pre)
    return bytes(pre), w.getvalue(), w.census


def _build_catalogue():
    cases = []

    def add(name, fn):
        text, raw, cs = _case(fn)
        cases.append((name, text, raw, cs))

    def emit(w, text, tokens, kind="auto", final=False, **kw):
        expand(tokens, text)
        if kind == "auto":
            auto_block(w, tokens, final, **kw)
        elif kind == "fixed":
            w.fixed(tokens, final)
        else:
            w.dynamic(tokens, kind[0], kind[1], final, **kw)

    # deep codes: lengths 1..14,15,15 on both codes, both orientations, two blocks, random tokens over all sixteen symbols each
    for lo in ("fwd", "rev"):
        for do in ("fwd", "rev"):
            def deep(w, text, lo=lo, do=do):
                rng = np.random.default_rng([1, lo == "rev", do == "rev"])
                ll, d = deep_lens(lo, do)
                syms = [s for s in ll if s != 256]
                emit(w, text, random_tokens(rng, 30000, syms, list(d), p_match=0.3), (ll, d))
                emit(w, text, random_tokens(rng, 35280, syms, list(d), start=30000, p_match=0.3, opener=True), (ll, d), final=True, rle="auto")
            add("deep/ll_%s/d_%s" % (lo, do), deep)

    rngs = np.random.default_rng(2)
    noise = bytes(rngs.integers(0, 256, 65280).astype(np.uint8))

    def every_length(w, text):
        toks = [noise[:300]]
        for n in range(3, 259):
            toks.append(match(n, 1 + (n * 7) % 290))
            toks.append(noise[n])
        toks += [match(258, 77, alt258=True), match(258, 300, alt258=True)]
        emit(w, text, toks, final=True)
    add("every_length", every_length)

    def every_distance(w, text):
        toks = [noise[:32768], match(3, 32768), match(258, 32768, alt258=True), noise[0]]      # at 32768 exactly, then later
        for ds in range(30):
            for dx in (0, (1 << DIST_EXTRA[ds]) - 1):
                toks += [(257 + (ds + dx) % 20, 0, ds, dx), noise[ds]]
        toks += [match(5, 32768), match(9, 32767), match(17, 32507)]
        emit(w, text, toks, final=True)
    add("every_distance", every_distance)

    def reaches_byte_0(w, text):
        toks = []
        for k in (1, 2, 5, 70, 700, 3000):                         # each match's distance is the output position itself: it starts at byte 0
            toks.append(noise[k:2 * k])
            toks.append(match(3 + k % 250, len(expand(toks))))
        emit(w, text, toks, final=True)
    add("distance_is_position", reaches_byte_0)

    def overlapping(w, text):
        toks = [noise[:100], match(258, 1)]
        for d in (1, 2, 3, 63, 64, 65):
            for n in (d + 1, d + 2, 2 * d + 1, 130, 258):
                toks += [noise[d:d + 3], match(max(3, n), d)]
        emit(w, text, toks)
        emit(w, text, [match(258, 1), match(258, 1, alt258=True), match(200, 2), noise[5], match(258, 1)], "fixed", final=True)
    add("overlapping", overlapping)

    def straddle(w, text):
        rng = np.random.default_rng(3)
        toks = [noise[:1310]]
        for i in range(260):                                        # source partly in text already written, partly in the staged batch
            toks.append(match(int(rng.integers(3, 259)), int(rng.integers(900, 1301))))
            if i % 3 == 0:
                toks.append(noise[i])
        emit(w, text, toks, final=True)
    add("straddle_900_1300", straddle)

    for n, name in ((3, "dense_len3"), (258, "dense_len258")):
        def dense(w, text, n=n):
            ls = len_sym(n)[0]
            ll = {ls: 1, 97: 2, 256: 3, 98: 3}
            emit(w, text, [b"ab" * 40], (ll, {0: 1}))
            emit(w, text, [(ls, 0, 1, 0)] * 90 + [97] + [(ls, 0, 0, 0)] * 75, (ll, {0: 1, 1: 1}))     # one-bit length and distance codes
            emit(w, text, [(ls, 0, 0, 0)] * 71, (ll, {0: 1}), final=True)
        add(name, dense)

    def short_literals(w, text):
        rng = np.random.default_rng(4)
        ll = {65: 1, 67: 2, 71: 3, 84: 4, 10: 5, 256: 5}
        lits = bytes(rng.choice(np.frombuffer(b"AAAAAAAACCCCGGT\n", dtype=np.uint8), 6000))
        emit(w, text, [lits], (ll, {}), final=True)
    add("short_literals", short_literals)

    # header shapes
    def one_dist_code(w, text):
        emit(w, text, [noise[:50], match(10, 20), noise[3], match(30, 20), match(3, 20)], final=True)
    add("header/one_distance_code", one_dist_code)

    def no_dist_code(w, text):
        emit(w, text, [noise[:500]], final=True)
    add("header/no_distance_code", no_dist_code)

    def thirty_dist_codes(w, text):
        toks = [noise[:40], match(4, 5), noise[:10]]
        emit(w, text, toks, final=True, extra_d=range(30))
    add("header/30_distance_codes", thirty_dist_codes)

    def all_286(w, text):
        toks = [noise[:2000]] + [bytes(range(256))] + [match(LEN_BASE[i], 100 + i) for i in range(29)]
        emit(w, text, toks, (flat(range(286)), flat(range(30))), rle=None)
        emit(w, text, toks, (flat(range(286)), flat(range(30))), final=True, rle="auto")
    add("header/286_codes", all_286)

    def two_symbols(w, text):
        emit(w, text, [b"x" * 777], ({120: 1, 256: 1}, {}), final=True, rle="auto")
    add("header/two_symbol_code", two_symbols)

    def across(w, text):
        # the literal/length lengths end 8 8 8 and the distance lengths begin 8 8 8: one 16 covers the last two and the first three
        ll = complete({s: 8 for s in list(range(200)) + [256, 283, 284, 285]}, range(200, 256))
        d = complete({0: 8, 1: 8, 2: 8}, range(3, 30))
        seq = [ll.get(i, 0) for i in range(286)]
        nd = max(d) + 1
        assert seq[282:] == [0, 8, 8, 8]
        emit(w, text, [bytes(range(200)), match(258, 3), match(258, 2, alt258=True), match(227, 1)], (ll, d),
             rle=auto_rle(seq[:283]) + [1, (16, 5), nd - 3])
        # zeros across it: 28 unused length symbols and 4 unused distance symbols in one 18
        ll = flat(list(range(250)) + [256, 257])
        d = flat([4, 5])
        seq = [ll.get(i, 0) for i in range(258)]
        emit(w, text, [bytes(range(250)), (257, 0, 4, 1), (257, 0, 5, 0)], (ll, d), hlit=286, rle=auto_rle(seq) + [(18, 32), 2])
        # an 18 with 138 zeros
        ll = flat(list(range(100)) + [256, 257])
        d = {0: 1, 29: 1}
        emit(w, text, [bytes(range(100)), (257, 0, 0, 0)], (ll, d), final=True,
             rle=auto_rle([ll[i] for i in range(100)]) + [(18, 138), (18, 18), 2, 1, (18, 28), 1])
    add("header/repeat_across_boundary", across)

    # block shapes
    def empties(w, text):
        emit(w, text, [noise[:30]], "fixed")
        emit(w, text, [], "fixed")
        emit(w, text, [], ({256: 1, 0: 1}, {}))
        emit(w, text, [noise[30:60], match(5, 60)])
        emit(w, text, [], "fixed")
        w.stored(b"")
        emit(w, text, [], ({256: 1, 0: 1}, {}), rle="auto")
        emit(w, text, [match(40, 33)], "fixed", final=True)
    add("blocks/empty", empties)

    def hundred(w, text):
        for i in range(100):
            t = [noise[i]] if i % 7 else [match(3 + i, 1)]
            if i == 0:
                t = [noise[0]]
            emit(w, text, t, "fixed" if i % 2 else "auto", final=i == 99)
    add("blocks/100_one_symbol", hundred)

    def stored0(w, text):
        w.stored(b"")
        emit(w, text, [b"after nothing"], "fixed")
        w.stored(b"", final=True)
    add("blocks/stored_0", stored0)

    def stored_max(w, text):
        text += noise + noise[:255]
        w.stored(bytes(text), final=True)
    add("blocks/stored_65535", stored_max)

    def alignments(w, text):
        for b in range(8):                                          # 3 + 8a + 9b + 7 bits: the stored block starts at every bit of a byte
            lits = bytes([65] * 3 + [200] * b)
            emit(w, text, [lits], "fixed")
            assert w.nbits % 8 == (2 + b) % 8
            data = noise[100 * b:100 * b + 37 + b]
            text += data
            w.stored(data)
        for b in range(8):                                          # ... and so does an empty one
            emit(w, text, [bytes([66] * 2 + [201] * b)], "fixed")
            w.stored(b"")
        emit(w, text, [match(20, 45)], "fixed", final=True)
    add("blocks/stored_at_8_alignments", alignments)

    for kind in ("stored", "fixed", "dynamic"):
        def last(w, text, kind=kind):
            emit(w, text, [b"ACGTACGT", match(8, 8)])
            if kind == "stored":
                text += b"the end"
                w.stored(b"the end", final=True)
            else:
                emit(w, text, [b"the end", match(7, 7)], "fixed" if kind == "fixed" else "auto", final=True)
        add("blocks/last_%s" % kind, last)

    def from_stored(w, text):
        text += noise[:40000]
        w.stored(noise[:40000])
        rng = np.random.default_rng(6)
        toks = []
        for i in range(300):                                        # matches out of the stored bytes, from next door to 32768 back
            toks.append(match(int(rng.integers(3, 259)), int(rng.choice([1, 40, 999, 20000, 32768, int(rng.integers(1, 32769))]))))
            if len(expand(toks, bytearray(text))) > 64000:
                toks.pop()
                break
        emit(w, text, toks, final=True)
    add("blocks/dynamic_copies_from_stored", from_stored)

    def fixed_all(w, text):
        toks = [noise[:256], bytes(range(256))]
        for i in range(29):
            toks.append((257 + i, (1 << LEN_EXTRA[i]) - 1 if i % 2 else 0, i % 9, 0))
        emit(w, text, toks, "fixed")
        toks = [noise[:32768 - len(text)]]
        for ds in range(30):
            toks += [(257 + ds % 29, 0, ds, 0), (285 - ds % 29, 0, ds, (1 << DIST_EXTRA[ds]) - 1)]
        toks += [match(258, 32768, alt258=True), match(258, 1)]
        emit(w, text, toks, "fixed", final=True)
    add("fixed/every_symbol", fixed_all)

    def holds_gz(w, text):
        # a stored block that carries a real DEFLATE stream: genuine block headers that are no boundaries of THIS stream
        rng = np.random.default_rng(8)
        inner = b"".join(b"@i%d\n" % i + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 100)) + b"\n+\n" + b"I" * 100 + b"\n" for i in range(700))
        co = zlib.compressobj(6, zlib.DEFLATED, 31, 8)
        gz = co.compress(inner) + co.flush()
        assert len(gz) < 60000
        emit(w, text, [b">outer\n"], "fixed")
        text += gz
        w.stored(gz)
        emit(w, text, [match(100, 5000), b"\n"], final=True)
    add("blocks/stored_holds_gz", holds_gz)
    return cases


@functools.lru_cache(maxsize=None)
def _catalogue():
    return tuple(_build_catalogue())


def catalogue():
    """named cases (name, text, raw stream); every text but blocks/stored_65535's is at most 65280 bytes: a BGZF member's"""
    return [(n, t, r) for n, t, r, _ in _catalogue()]


def catalogue_census():
    """{name: what the writer counted while it wrote the case}"""
    return {n: c for n, _, _, c in _catalogue()}


# ---- illegal streams with a known answer ------------------------------------------------------------------------------------------------
def illegal():
    """(name, raw stream, the decoders' status): crafted, not damaged; zlib refuses each"""
    out = []

    def add(name, status, fn):
        w = Writer()
        fn(w)
        w.put(0, 7)
        out.append((name, w.getvalue() + b"\0" * 4, status))

    okll = {97: 1, 256: 2, 257: 2}

    def t3(w):
        w.fixed([b"ab"])
        w.put(1, 1); w.put(3, 2)
    add("block type 3", 1, t3)

    def nlen(w):
        w.put(1, 1); w.put(0, 2); w.align(); w.put(5, 16); w.put(5 ^ 0xFFFE, 16)
        w.put_arrays(np.frombuffer(b"hello", dtype=np.uint8), np.full(5, 8))
    add("stored NLEN wrong", 2, nlen)
    add("over-subscribed literal/length code", 3, lambda w: w.dynamic([97], {97: 1, 98: 1, 256: 1}, {}, True, check=False))
    add("over-subscribed distance code", 3, lambda w: w.dynamic([97], okll, {0: 1, 1: 1, 2: 1}, True, check=False))
    add("over-subscribed code-length code", 3, lambda w: w.dynamic([97], okll, {}, True, cl_lens={0: 1, 1: 1, 2: 2}, check=False))
    add("repeat 16 as the first length", 3, lambda w: w.dynamic([], okll, {}, True, rle=[(16, 3), 255], check=False))
    add("repeat running past HLIT + HDIST", 3, lambda w: w.dynamic([], okll, {}, True, rle=[258 - 10, (18, 138)], check=False))
    add("no end-of-block code", 3, lambda w: w.dynamic([97, 98], {97: 1, 98: 1}, {}, True, eob=False, check=False))
    add("HLIT of 287", 3, lambda w: w.dynamic([97], okll, {}, True, hlit=287, check=False))
    add("HDIST of 31", 3, lambda w: w.dynamic([97], okll, {}, True, hdist=31, check=False))
    fll, fd = canonical(FIXED_LL), canonical(FIXED_D)
    add("literal/length symbol 286 in a fixed block", 4, lambda w: w.fixed([b"abc", ("raw",) + fll[286]], True))
    add("distance symbol 30 in a fixed block", 4, lambda w: w.fixed([b"abc", (257, 0, None, None), ("raw",) + fd[30]], True))
    add("bits that are no code of an incomplete distance code", 4,
        lambda w: w.dynamic([97, 97, 97, (257, 0, 0, 0), (257, 0, None, None), ("raw", 1, 1)], okll, {0: 1}, True))
    add("a match in a block whose distance code is empty", 4,
        lambda w: w.dynamic([97, 97, 97, (257, 0, None, None), ("raw", 0, 1)], okll, {}, True))
    add("distance one more than the output position", 5, lambda w: w.fixed([b"abc", match(3, 3), match(3, 7)], True))
    return out


# ---- whole files of parseable text ------------------------------------------------------------------------------------------------------
def craft_stream(text, rng, block=(6000, 20000), deep=False, opener=False, stored_every=0, stored=(1, 700), p_match=0.5):
    """one raw stream that inflates to `text` (text-driven tokens).  block: the blocks' sizes in bytes of text.  deep: codes with
    11 bits and more on most symbols (deep_over: the frequent ones in every other block, the rare ones in the rest).  opener: every
    block opens with a match at the largest distance the position allows.  stored_every: every n-th block is followed by a stored one
    of `stored` bytes, which starts wherever the block in front ended in its byte."""
    w, p, k = Writer(), 0, 0
    while True:
        q = min(len(text), p + int(rng.integers(block[0], block[1] + 1)))
        toks = text_tokens(text, p, q, rng, p_match=p_match, opener=opener)
        p = q
        if stored_every and k % stored_every == stored_every - 1 and p < len(text):
            n = min(len(text) - p, int(rng.integers(stored[0], stored[1] + 1)))
            if deep:
                _deep_block(w, toks, k, False)
            else:
                auto_block(w, toks, False, extra_d=(0, 1))
            w.stored(text[p:p + n], final=p + n == len(text))
            p += n
            if p == len(text):
                break
        else:
            final = p == len(text)
            if deep:
                _deep_block(w, toks, k, final)
            else:
                auto_block(w, toks, final, extra_d=(0, 1))         # (two distance codes at the least: a complete code, a header that can be found)
            if final:
                break
        k += 1
    return w.getvalue(), w.census


def _deep_block(w, toks, k, final):
    ll, _ = used_symbols(toks)
    ll |= set(range(257, 286))
    lits = sorted(s for s in ll if s < 256)
    if k % 2:
        short_ll, short_d = lits[:3] + [256, 285, 284, 283, 282], list(range(29, 21, -1))     # the frequent symbols are the deep ones
    else:
        freq = [s for s in (65, 67, 71, 84, 10) if s in lits][:5]
        short_ll = (freq + [s for s in lits if s not in freq])[:6] + [257, 258]
        short_d = list(range(8))
    w.dynamic(toks, deep_over(ll, short_ll), deep_over(range(30), short_d), final, rle="auto" if k % 3 else None)


def random_stream(rng, n_text, codes, block=(20000, 40000), opener=False, p_match=0.1, run=(1, 8), between=None):
    """one raw stream of about n_text bytes of text from the random source, a dynamic block per `block` bytes; codes(k) -> the
    (literal/length, distance) lengths of block k; between(k, text) -> bytes for a stored block behind block k, or None"""
    w, text, k = Writer(), bytearray(), 0
    while len(text) < n_text:
        ll, d = codes(k)
        n = int(rng.integers(block[0], block[1] + 1))
        toks = random_tokens(rng, n, [s for s in ll if s != 256], list(d), start=len(text), p_match=p_match, run=run, opener=opener)
        expand(toks, text)
        data = between(k, text) if between else None
        final = len(text) >= n_text
        w.dynamic(toks, ll, d, final and not data, rle="auto" if k % 2 else None)
        if data:
            for a in range(0, len(data), 65535):
                text += data[a:a + 65535]
                w.stored(data[a:a + 65535], final and a + 65535 >= len(data))
        k += 1
    return bytes(text), w.getvalue(), w.census


def _fastq(rng, n):
    return b"".join(b"@q%d\n" % i + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 150)) + b"\n+\n" + bytes(rng.integers(35, 75, 150).astype(np.uint8)) + b"\n"
                    for i in range(n))


STREAM_CASES = ("deep", "openers", "one_distance_code", "stored_between", "stored_holds_gz", "gzip_0_of_gzip_6", "members")


@functools.lru_cache(maxsize=None)
def stream_case(name):
    """(text, gzip file, census or None): a gzip file of 1 to 2 MB of text for the one-stream decoder (bns_inflate_stream_device), blocks
    of at most 40000 bytes of text (a chunk of 4 KiB has room for 66560 symbols), literal-heavy (under 8:1)"""
    import gzip
    rng = np.random.default_rng([77, STREAM_CASES.index(name)])
    lits = list(b"ACGTNacgtn0123\n@")
    plain = flat(lits + [256, 257, 258, 260, 265, 270, 284, 285]), flat(range(30))
    if name == "deep":
        # deep codes, both orientations in turn, on complete distance codes: headers the search accepts
        text, raw, cs = random_stream(rng, 1200000, lambda k: deep_lens("fwd" if k % 2 else "rev", "rev" if k % 4 < 2 else "fwd"))
    elif name == "openers":
        # every block opens with a match at distance 32768 (the first: as far as the text goes): 258 bytes, which the next match copies again
        text, raw, cs = random_stream(rng, 1200000, lambda k: plain, block=(9000, 30000), opener=285)
    elif name == "one_distance_code":
        # a header the search does not accept
        text, raw, cs = random_stream(rng, 1000000, lambda k: (plain[0], {10 + k % 12: 1}), block=(9000, 30000))
    elif name == "stored_between":
        # stored blocks wherever the dynamic block in front ends in its byte
        text, raw, cs = random_stream(rng, 1000000, lambda k: plain, block=(3000, 12000),
                                      between=lambda k, t: bytes(rng.integers(0, 256, int(rng.integers(0, 3000))).astype(np.uint8)))
    elif name == "stored_holds_gz":
        # stored blocks that carry a real .gz: block headers that are no boundaries of this stream
        inner = gzip.compress(_fastq(rng, 4000), 6)
        text, raw, cs = random_stream(rng, len(inner) * 5 // 3, lambda k: plain, block=(20000, 40000), between=lambda k, t: inner[k * 60001:(k + 1) * 60001])
    elif name == "gzip_0_of_gzip_6":
        inner = gzip.compress(_fastq(rng, 8000), 6)
        return inner, gzip.compress(inner, 0), None
    else:
        # two crafted members and an empty one between them
        a, ra, _ = random_stream(rng, 500000, lambda k: deep_lens("rev", "fwd"))
        b, rb, _ = random_stream(rng, 500000, lambda k: plain, opener=285)
        return a + b, gzip_member(ra, a) + gzip_member(b"\x03\x00", b"", name=b"empty") + gzip_member(rb, b), None
    return text, gzip_member(raw, text), cs
