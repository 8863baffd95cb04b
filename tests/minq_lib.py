"""Helpers of the minimum-base-quality tests (bns_set_min_base_quality, bns_pack_reads_qual_ptrs, `bonsai classify -Q`).

The truth of every one of them: classifying with threshold q equals classifying, WITHOUT the feature, the same records with every
base of low quality replaced by 'N'.  So this file parses text with tests/kseq_py.py (kseq_read restated byte by byte), substitutes,
and writes the records out again as plain four-line FASTQ (FASTA for records without quality) for the existing q = 0 path -- which
the existing tests hold to the oracle.  Test infrastructure only."""
import numpy as np

import kseq_py

CODE = np.full(256, 255, dtype=np.uint8)
for _c, _v in zip(b"ACGTacgt", (0, 1, 2, 3, 0, 1, 2, 3)):
    CODE[_c] = _v


def mask(seq, qual, q):
    """seq with 'N' wherever the unsigned quality byte is below 33 + q; a record without quality (qual empty) is untouched"""
    if not q or not qual:
        return bytes(seq)
    assert len(qual) == len(seq)
    s = np.frombuffer(bytes(seq), dtype=np.uint8).copy()
    s[np.frombuffer(bytes(qual), dtype=np.uint8) < 33 + q] = ord("N")
    return s.tobytes()


def records(doc, trim=False):
    """[(name, comment, seq, qual, header offset)] as kseq_read yields them, up to its first error"""
    return kseq_py.read_until_error(doc, trim=trim)[0]


def plain_text(recs, q):
    """the records, masked by q, as plain text: '@name comment / seq / + / qual' (a record without quality: '>name comment / seq').
    Checked here: kseq_read reads exactly the masked records back from it."""
    out = []
    for r in recs:
        name, comment, seq, qual = r[0], r[1], r[2], r[3]
        hdr = name + (b" " + comment if comment else b"")
        s = mask(seq, qual, q)
        # (kseq_read drops one trailing '\r' of a line it appends to a longer string: a string that ends in one is written with two)
        s, qual = (x + b"\r" if len(x) > 1 and x.endswith(b"\r") else x for x in (s, qual))
        out.append(b"@" + hdr + b"\n" + s + b"\n+\n" + qual + b"\n" if qual else b">" + hdr + b"\n" + s + b"\n")
    text = b"".join(out)
    back = records(text)
    assert [(b[0], b[2]) for b in back] == [(r[0], mask(r[2], r[3], q)) for r in recs], "the substituted text does not read back"
    return text


def substituted_text(doc, q, n=None):
    """doc's first n records (all of them by default) with low-quality bases replaced by 'N', as plain text -> (text, records)"""
    recs = records(doc)
    if n is not None:
        recs = recs[:n]
    return plain_text(recs, q), recs


def norm(seq):
    """what the packed image says of a sequence: ACGT in upper case, 'N' for everything else"""
    s = np.frombuffer(bytes(seq), dtype=np.uint8)
    c = CODE[s]
    return np.where(c < 4, np.frombuffer(b"ACGT", dtype=np.uint8)[c & 3], ord("N")).astype(np.uint8).tobytes()


def unpack(words, nmask, seq_len):
    """packed image (dense flags) -> list of byte strings over ACGT with 'N' for flagged bases; also checks that a flagged base's
    code bits are 0"""
    out = []
    off = 0
    for r, L in enumerate(int(x) for x in seq_len):
        wb = (off >> 5) + r
        i = np.arange(L)
        w = words[wb + (i >> 5)].astype(np.uint64)
        m = nmask[wb + (i >> 5)].astype(np.uint64)
        code = ((w >> (62 - 2 * (i & 31)).astype(np.uint64)) & np.uint64(3)).astype(np.int64)
        bad = ((m >> (31 - (i & 31)).astype(np.uint64)) & np.uint64(1)).astype(bool)
        assert not np.any(code[bad]), "a flagged base with code bits"
        out.append(np.where(bad, ord("N"), np.frombuffer(b"ACGT", dtype=np.uint8)[code]).astype(np.uint8).tobytes())
        off += L
    return out


def read_words(arr, seq_len):
    """the entries of a packed image's word (or flag word) array that belong to reads: read r's (L + 31) / 32 words from word
    (offset >> 5) + r on.  The slack word between two reads, and behind the last one, is not part of the image: the device packer
    never writes it, so it holds whatever the buffer held before"""
    seq_len = np.asarray(seq_len, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(seq_len)[:-1]]) if seq_len.size else np.zeros(0, np.int64)
    wb = (off >> 5) + np.arange(seq_len.size)
    nw = (seq_len + 31) >> 5
    idx = np.concatenate([np.arange(b, b + n) for b, n in zip(wb, nw)]) if seq_len.size else np.zeros(0, np.int64)
    return np.asarray(arr)[idx.astype(np.int64)]


def dense_flags(n_words, bad_word, bad_mask):
    d = np.zeros(n_words, dtype=np.uint32)
    d[bad_word.astype(np.int64)] = bad_mask
    return d


# ---- text --------------------------------------------------------------------------------------------------------------------------
ALPHA = np.frombuffer(b"ACGTACGTACGTACGTNacgtnRYK", dtype=np.uint8)
LOW_BYTES = np.frombuffer(b" \t\x01\x1e", dtype=np.uint8)       # quality bytes below 33 that a line may hold ('\r' at a line end would be stripped)
LENGTHS = (0, 1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 150)


def rand_qual(rng, n, low=0.03):
    """quality bytes over the whole printable range (33 .. 126), a few below 33"""
    q = rng.integers(33, 127, size=n).astype(np.uint8)
    m = rng.random(n) < low
    q[m] = LOW_BYTES[rng.integers(0, LOW_BYTES.size, size=int(m.sum()))]
    return q


def wrap(b, w):
    return [b[i:i + w] for i in range(0, len(b), w)] if b else [b""]


def make_qdoc(rng, n_records, crlf=False, final_newline=True, fasta=0.2, headerish=0.3):
    """regular FASTA / FASTQ text whose sequence and quality are wrapped INDEPENDENTLY (one line or several each), quality lines that
    start with '@', '>' or '+', empty sequences, blank lines between records, FASTA mixed in"""
    nl = b"\r\n" if crlf else b"\n"
    out = []
    for i in range(n_records):
        L = int(LENGTHS[rng.integers(0, len(LENGTHS))]) if rng.random() < 0.4 else int(rng.integers(0, 400))
        seq = ALPHA[rng.integers(0, ALPHA.size, size=L)].tobytes()
        name = b"q%d" % i if rng.random() < 0.9 else b""
        if rng.random() < fasta:
            lines = [b">" + name + (b" fasta record" if rng.random() < 0.5 else b"")]
            lines += wrap(seq, int(rng.integers(1, 90))) if rng.random() < 0.5 else [seq]
        else:
            lines = [b"@" + name + (b"\tc" if rng.random() < 0.3 else b"")]
            lines += wrap(seq, int(rng.integers(1, 90))) if rng.random() < 0.5 else [seq]
            lines.append(b"+" + (name if rng.random() < 0.2 else b""))
            q = rand_qual(rng, L)
            ql = wrap(q.tobytes(), int(rng.integers(1, max(2, L)))) if rng.random() < 0.5 and L > 1 else [q.tobytes()]
            ql = [bytearray(x) for x in ql]
            for x in ql:                                     # lines that look like a header or a '+' line
                if x and rng.random() < headerish:
                    x[0] = b"@>+"[int(rng.integers(0, 3))]
            lines += [bytes(x) for x in ql]
        if rng.random() < 0.1:
            lines.append(b"")
        out.append(nl.join(lines) + nl)
    doc = b"".join(out)
    # (CRLF text that ends in an empty line keeps its end: cut there, an empty FASTQ record would lose its quality line while its
    # sequence keeps a lone '\r' -- kseq_read's error -2)
    if not final_newline and doc.endswith(nl) and not (crlf and doc.endswith(nl + nl)):
        doc = doc[:-len(nl)]
    return doc


def illumina_qual(rng, n, low=0.02):
    """mostly high scores (Phred 30 .. 40) with sparse low bases (Phred 2 .. 15)"""
    q = rng.integers(33 + 30, 33 + 41, size=n).astype(np.uint8)
    m = rng.random(n) < low
    q[m] = rng.integers(33 + 2, 33 + 16, size=int(m.sum())).astype(np.uint8)
    return q.tobytes()


def fastq_text(names, reads, quals, eol=b"\n", wrap_seq=0, wrap_qual=0):
    """reads (uint8 arrays or bytes) and their quality strings (None: a FASTA record) as text"""
    out = []
    for nm, r, q in zip(names, reads, quals):
        s = r.tobytes() if hasattr(r, "tobytes") else bytes(r)
        body = eol.join(wrap(s, wrap_seq)) if wrap_seq else s
        if q is None:
            out.append(b">" + nm + eol + body + eol)
        else:
            out.append(b"@" + nm + eol + body + eol + b"+" + eol + (eol.join(wrap(q, wrap_qual)) if wrap_qual else q) + eol)
    return b"".join(out)


def rle(hits):
    """the hit stream as runs of equal consecutive taxa: (taxa, lengths)"""
    hits = np.asarray(hits, dtype=np.uint32)
    if not hits.size:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    cut = np.flatnonzero(np.concatenate([[True], hits[1:] != hits[:-1]]))
    return hits[cut], np.diff(np.concatenate([cut, [hits.size]])).astype(np.uint32)
