"""Minimum base quality on the host (no GPU): bns_pack_reads_qual_ptrs against bns_pack_reads on the same reads with 'N' in place of
every base whose quality byte is below 33 + q -- words, bad words and masks equal; q = 0 and reads without quality reproduce
bns_pack_reads_ptrs; the ABI; and the host reader's records (CRLF text, quality wrapped differently from the sequence) through the
new packer against tests/kseq_py.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bonsai_amd
from bonsai_amd import _lib, hostio
from bonsai_amd._lib import u32p, u64p, vp
import kseq_py
import minq_lib as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def batch(rng, n, low=0.05, no_qual=0.1):
    """reads of every length that matters (word edges, not a multiple of 4), bases of every kind, quality over the whole byte range"""
    seqs, quals = [], []
    for i in range(n):
        L = int(M.LENGTHS[i % len(M.LENGTHS)]) if i % 3 else int(rng.integers(0, 310))
        seqs.append(M.ALPHA[rng.integers(0, M.ALPHA.size, size=L)].tobytes())
        if rng.random() < no_qual:
            quals.append(None)
            continue
        q = rng.integers(0, 256, size=L).astype(np.uint8) if i % 5 == 0 else M.rand_qual(rng, L, low)
        quals.append(q.tobytes())
    return seqs, quals


def edge_batch():
    """masked bases exactly at word edges: bases 0, 31, 32, 63, 64 and the last one, of reads of 33, 64, 65, 150 and 151 bases"""
    seqs, quals = [], []
    for L in (33, 64, 65, 150, 151):
        for at in (0, 31, 32, 63, 64, L - 1):
            if at >= L:
                continue
            q = bytearray(b"I" * L)
            q[at] = ord("#")
            seqs.append((b"ACGT" * 40)[:L]); quals.append(bytes(q))
    return seqs, quals


def expected(seqs, quals, q, threads=1):
    sub = [M.mask(s, ql or b"", q) for s, ql in zip(seqs, quals)]
    bases, offsets = bonsai_amd.concat_reads(sub)
    return bonsai_amd.pack_reads(bases, offsets, threads=threads) + (offsets,)


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("q", [1, 20, 41, 93])
def test_packer_equals_pack_reads_on_the_substituted_batch(q, threads):
    rng = np.random.default_rng(1000 + q)
    seqs, quals = batch(rng, 9000 if threads > 1 else 1500)     # (several threads: the packer takes one per 4096 reads)
    e_seqs, e_quals = edge_batch()
    seqs, quals = e_seqs + seqs, e_quals + quals
    got = bonsai_amd.pack_reads_qual(seqs, quals, q, threads=threads)
    exp = expected(seqs, quals, q)
    for g, e, what in zip(got, exp, ("words", "bad_word", "bad_mask", "offsets")):
        assert np.array_equal(g, e), (what, q, threads)
    # it bites, and not everywhere
    plain = expected(seqs, quals, 0)
    assert not np.array_equal(plain[0], exp[0]) and exp[1].size > plain[1].size
    lens = {len(s) for s in seqs}
    assert {0, 1, 31, 32, 33, 64, 150} <= lens and any(n % 4 for n in lens)
    # the image read back: every masked base flagged, its code bits 0 (unpack checks them)
    seq_len = np.diff(exp[3].astype(np.int64))
    un = M.unpack(got[0], M.dense_flags(got[0].size, got[1], got[2]), seq_len[:200])
    assert un == [M.norm(M.mask(s, ql or b"", q)) for s, ql in zip(seqs[:200], quals[:200])]


def test_edge_bases_are_masked_one_by_one():
    seqs, quals = edge_batch()
    got = bonsai_amd.pack_reads_qual(seqs, quals, 20)
    seq_len = [len(s) for s in seqs]
    un = M.unpack(got[0], M.dense_flags(got[0].size, got[1], got[2]), seq_len)
    for s, ql, u in zip(seqs, quals, un):
        assert u.count(b"N") == 1 and u.index(b"N") == ql.index(b"#"), (len(s), ql.index(b"#"))


def ptrs_call(seqs, threads=1):
    """bns_pack_reads_ptrs itself"""
    L = _lib.load()
    n = len(seqs)
    sp = (C.c_char_p * max(1, n))(*seqs)
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    words = np.zeros(int(L.bns_packed_words(int(lens.sum()), n)), dtype=np.uint64)
    bw = np.zeros(words.size + 1, dtype=np.uint64); bm = np.zeros(words.size + 1, dtype=np.uint32); nb = C.c_uint64()
    rc = L.bns_pack_reads_ptrs(C.cast(sp, vp), lens.ctypes.data_as(u32p), n, offsets.ctypes.data_as(u64p), words.ctypes.data_as(u64p),
                               bw.ctypes.data_as(u64p), bm.ctypes.data_as(u32p), bw.size, C.cast(C.byref(nb), u64p), threads)
    assert rc == 0
    return words, bw[:nb.value].copy(), bm[:nb.value].copy(), offsets


@pytest.mark.parametrize("threads", [1, 3])
def test_q0_and_no_quality_reproduce_pack_reads_ptrs(threads):
    rng = np.random.default_rng(5)
    seqs, quals = batch(rng, 9000)
    exp = ptrs_call(seqs, threads)
    for args in ((quals, 0), (None, 0), (None, 20), ([None] * len(seqs), 20), ([None] * len(seqs), 93)):
        got = bonsai_amd.pack_reads_qual(seqs, args[0], args[1], threads=threads)
        for g, e, what in zip(got, exp, ("words", "bad_word", "bad_mask", "offsets")):
            assert np.array_equal(g, e), (what, args[1], args[0] is None)
    # no read at all
    got = bonsai_amd.pack_reads_qual([], [], 20)
    assert got[0].size == 1 and got[1].size == 0 and got[3].tolist() == [0]


def test_abi():
    L = _lib.load()
    assert L.bns_version() >= 108
    for name in ("bns_set_min_base_quality", "bns_pack_reads_qual_ptrs"):
        assert name in L._bns_signatures and getattr(L, name) is not None
    text = open(os.path.join(ROOT, "include", "bonsai_amd.h")).read()
    assert "int bns_set_min_base_quality(bns_ctx *ctx, uint32_t q);" in text and "int bns_pack_reads_qual_ptrs(" in text
    # the library exports them
    so = os.path.join(ROOT, "bonsai_amd", "lib", "libbonsai_amd.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert " T bns_set_min_base_quality" in syms and " T bns_pack_reads_qual_ptrs" in syms
    # a threshold beyond Phred 93 is refused, whatever else is given; so is a call without a context
    with pytest.raises(bonsai_amd.BonsaiAmdError):
        bonsai_amd.pack_reads_qual([b"ACGT"], [b"IIII"], 94)
    with pytest.raises(bonsai_amd.BonsaiAmdError):
        bonsai_amd.pack_reads_qual([b"ACGT"], None, 94)
    assert bonsai_amd.pack_reads_qual([b"ACGT"], [b"IIII"], 93)[1].size == 1
    assert L.bns_set_min_base_quality(None, 20) != 0
    with pytest.raises(ValueError):
        bonsai_amd.pack_reads_qual([b"ACGT"], [b"III"], 20)


@pytest.mark.parametrize("crlf", [False, True])
def test_host_reader_and_packer(tmp_path, crlf):
    """the host parser's records (libbns_host: what `bonsai classify` falls back to) carry the quality as kseq_read yields it -- lines
    joined, '\\r' dropped -- so the packer masks the bases the definition names: against tests/kseq_py.py on text whose sequence and
    quality are wrapped independently"""
    rng = np.random.default_rng(31 + crlf)
    n_fastq = 0
    for it in range(6):
        doc = M.make_qdoc(rng, 150, crlf=crlf, final_newline=bool(it % 2))
        assert kseq_py.reads_cleanly(doc)
        p = str(tmp_path / ("d%d.fq" % it))
        open(p, "wb").write(doc)
        got, _ = hostio.read_fastx(p, block_bytes=(0, 4096)[it % 2])
        truth = M.records(doc, trim=True)
        assert [(g[0], g[2], g[3]) for g in got] == [(t[0], t[2], t[3]) for t in truth]
        seqs = [g[2] for g in got]
        quals = [g[3] if g[3] else None for g in got]
        n_fastq += sum(1 for x in quals if x)
        for q in (1, 20, 41, 93):
            w, bw, bm, off = bonsai_amd.pack_reads_qual(seqs, quals, q)
            un = M.unpack(w, M.dense_flags(w.size, bw, bm), [len(s) for s in seqs])
            assert un == [M.norm(M.mask(t[2], t[3], q)) for t in truth], (it, q)
    assert n_fastq > 300
