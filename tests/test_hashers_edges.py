"""The hash feeders at the edges of their wavefront scan and of their window queue: RollingHasher<u64 | u128> with and without a
window (bns_rolling_hash_windowed_batch, bns_rolling_hash128_windowed_batch) and Encoder::for_each_hash (bns_for_each_hash_batch).

All three kernels write a run's first value apart from the scan and then take 64 positions per step, carrying lane 63's value into
the next step: runs of exactly 1, 2, 64, 65, 66, 128, 129 and 130 values sit on either side of zero, one and two carries.  An N
directly behind the run and a second run behind that reach the restart rule (k + 1 characters after the N) and, on the canonical
path, the exit of encoder.h:714.  k = 64 / 128 and their neighbours are where a rotation count reduces to 0.  The window kernels
take 64 windows per step, and a stream shorter than its window takes a branch of its own; a window whose minimum is all ones emits
nothing unless the stream is shorter than the window.

Expected values come from the oracle; the CPU half holds the oracle on the same inputs to the Python restatements of
test_nthash.py, so that they do not rest on the oracle alone."""
import numpy as np
import pytest

import synth
from test_nthash import as_ints, py_for_each_hash, py_rolling128, py_rolling128_both, py_window128

VALUES = (1, 2, 64, 65, 66, 128, 129, 130)             # values the first run gives
K64 = (1, 31, 64, 65)
K128 = K64 + (127, 128, 129)
WS = (2, 64, 65)                                       # window lengths in values (w - k + 1)
WIN_K = 3
ONES = 0xFFFFFFFFFFFFFFFF
ONES_N = (1, 3, 4, 5, 70)
ONES_W = (0, 2, 5)


def tables64():
    rng = np.random.default_rng(41)
    return (rng.integers(0, 1 << 63, size=256, dtype=np.uint64) * np.uint64(2) + np.uint64(1), rng.integers(0, 1 << 63, size=256, dtype=np.uint64))


def tables128():
    """full tables: hi != 0 (the default 128-bit tables keep the low word only)"""
    rng = np.random.default_rng(42)
    return (rng.integers(0, 1 << 63, size=512, dtype=np.uint64) * np.uint64(2) + np.uint64(1), rng.integers(1, 1 << 63, size=512, dtype=np.uint64))


def table_nt(oracle):
    return oracle.nthash_tables([int(x) for x in np.random.default_rng(43).integers(1, 1 << 63, size=4)])


def scan_cases(k, nthash):
    """(sequence, values it gives): a clean run of k + v - 1 bases, an N, a second run.  Rolling restarts k + 1 characters behind the
    N, so a second run of t bases gives t - 2k + 1 values: 2k - 1 (none: one base short; the canonical path leaves at encoder.h:714),
    2k (one) and 2k + 3.  ntHash starts again right behind the N and gives t - k + 1 values, but none when the run's first window ends
    with the string: t = k (none), k + 1, k + 3."""
    rng = np.random.default_rng(1000 * k + nthash)
    out = []
    for v in VALUES:
        for t in ((k, k + 1, k + 3) if nthash else (2 * k - 1, 2 * k, 2 * k + 3)):
            s = synth.rand_seq(rng, k + v - 1).tobytes() + b"N" + synth.rand_seq(rng, t).tobytes()
            tail = (t - k + 1 if t > k else 0) if nthash else max(0, t - 2 * k + 1)
            out.append((s, v + tail))
    return out


def window_cases(ws, canon):
    """clean sequences whose stream has ws - 1, ws, ws + 1, ws + 63, ws + 64 and ws + 65 entries.  The canonical path queues two entries
    a position, so its streams are even: an odd count is replaced by its two even neighbours."""
    rng = np.random.default_rng(2000 + ws)
    entries = []
    for e in (ws - 1, ws, ws + 1, ws + 63, ws + 64, ws + 65):
        entries += [e] if not (canon and e % 2) else [e - 1, e + 1]
    per = 2 if canon else 1
    return [(synth.rand_seq(rng, e // per + WIN_K - 1).tobytes(), e) for e in sorted(set(entries)) if e]


def batch(seqs):
    return synth.concat([np.frombuffer(s, dtype=np.uint8) for s in seqs])


def ones_tables(n):
    return (np.full(n, ONES, dtype=np.uint64), np.full(n, ONES, dtype=np.uint64))


# ---------------------------------------------------------------- CPU tier: the oracle against the Python restatements

def test_scan_edges_nthash_restatement(oracle):
    T = table_nt(oracle)
    for k in K64:
        for s, n in scan_cases(k, True):
            for canon in (False, True):
                got = oracle.for_each_hash(s, k, canon, T)
                assert got.size == n, (k, len(s))
                assert np.array_equal(got, py_for_each_hash(s, k, canon, T)), (k, canon, len(s))


def test_scan_edges_u128_restatement(oracle):
    tf, tr = tables128()
    for k in K128:
        for s, n in scan_cases(k, False):
            for canon in (False, True):
                got = oracle.rolling_hash128(s, k, canon, (tf, tr))
                assert got.shape[0] == n, (k, len(s))
                assert as_ints(got) == py_rolling128(s, k, canon, tf, tr), (k, canon, len(s))


def test_scan_edges_u64_counts(oracle):
    """no Python restatement of the 64-bit hasher: the shapes give the number of values they are built for"""
    for k in K64:
        for s, n in scan_cases(k, False):
            for canon in (False, True):
                assert oracle.rolling_hash(s, k, canon, tables64()).size == n, (k, canon, len(s))


def test_window_edges_u128_restatement(oracle):
    tf, tr = tables128()
    for ws in WS:
        w = ws + WIN_K - 1
        for canon in (False, True):
            for s, e in window_cases(ws, canon):
                stream = py_rolling128_both(s, WIN_K, tf, tr) if canon else py_rolling128(s, WIN_K, False, tf, tr)
                assert len(stream) == e, (ws, canon, len(s))
                assert as_ints(oracle.rolling_hash128(s, WIN_K, canon, (tf, tr), w=w)) == py_window128(stream, ws), (ws, canon, e)


def test_all_ones_restatement(oracle):
    t64, t128 = ones_tables(256), ones_tables(512)
    # an all-ones minimum is dropped when the stream fills a window and kept when it does not
    assert oracle.rolling_hash(b"AAAA", 1, False, t64, w=5).tolist() == [ONES]
    assert oracle.rolling_hash128(b"AAAA", 1, False, t128, w=5).tolist() == [[ONES, ONES]]
    assert oracle.rolling_hash(b"AAAAA", 1, False, t64, w=5).size == 0
    assert oracle.rolling_hash128(b"AAAAA", 1, False, t128, w=5).shape[0] == 0
    assert oracle.rolling_hash(b"AAAA", 1, True, t64, w=5).size == 0          # 8 queued entries >= ws
    for n in ONES_N:
        s = b"A" * n
        for w in ONES_W:
            for canon in (False, True):
                stream = py_rolling128_both(s, 1, *t128) if canon else py_rolling128(s, 1, False, *t128)
                assert stream == [(1 << 128) - 1] * (n * (2 if canon else 1))
                got = as_ints(oracle.rolling_hash128(s, 1, canon, t128, w=w))
                if w > 1:
                    assert got == py_window128(stream, w), (n, w, canon)
                else:
                    assert got == py_rolling128(s, 1, canon, *t128), (n, w, canon)


# ---------------------------------------------------------------- GPU tier: the entry points against the oracle

@pytest.mark.gpu
@pytest.mark.parametrize("canon", (False, True))
def test_scan_edges_u64_gpu(gpu_ctx, oracle, canon):
    tabs = tables64()
    for k in K64:
        cases = scan_cases(k, False)
        got = gpu_ctx.rolling_hash(*batch([s for s, _ in cases]), k, canon, tabs)
        for (s, n), g in zip(cases, got):
            assert g.size == n, (k, len(s))
            assert np.array_equal(g, oracle.rolling_hash(s, k, canon, tabs)), (k, canon, len(s))


@pytest.mark.gpu
@pytest.mark.parametrize("canon", (False, True))
def test_scan_edges_u128_gpu(gpu_ctx, oracle, canon):
    tabs = tables128()
    for k in K128:
        cases = scan_cases(k, False)
        got = gpu_ctx.rolling_hash128(*batch([s for s, _ in cases]), k, canon, tabs)
        for (s, n), g in zip(cases, got):
            assert g.shape == (n, 2), (k, len(s))
            assert np.array_equal(g, oracle.rolling_hash128(s, k, canon, tabs)), (k, canon, len(s))


@pytest.mark.gpu
@pytest.mark.parametrize("canon", (0, 1))
def test_scan_edges_nthash_gpu(gpu_ctx, oracle, canon):
    T = table_nt(oracle)
    for k in K64:
        cases = scan_cases(k, True)
        got = gpu_ctx.for_each_hash(*batch([s for s, _ in cases]), k=k, canon=canon, table=T)
        for (s, n), g in zip(cases, got):
            assert g.size == n, (k, len(s))
            assert np.array_equal(g, oracle.for_each_hash(s, k, bool(canon), T)), (k, canon, len(s))


@pytest.mark.gpu
@pytest.mark.parametrize("canon", (False, True))
def test_window_edges_gpu(gpu_ctx, oracle, canon):
    t64, t128 = tables64(), tables128()
    for ws in WS:
        w = ws + WIN_K - 1
        cases = window_cases(ws, canon)
        bases, offsets = batch([s for s, _ in cases])
        got64 = gpu_ctx.rolling_hash(bases, offsets, WIN_K, canon, t64, w=w)
        got128 = gpu_ctx.rolling_hash128(bases, offsets, WIN_K, canon, t128, w=w)
        for (s, e), g64, g128 in zip(cases, got64, got128):
            assert oracle.rolling_hash(s, WIN_K, canon, t64).size * (2 if canon else 1) == e
            exp64, exp128 = oracle.rolling_hash(s, WIN_K, canon, t64, w=w), oracle.rolling_hash128(s, WIN_K, canon, t128, w=w)
            assert exp64.size == exp128.shape[0] == max(1, e - ws + 1)        # (random values: none is all ones)
            assert np.array_equal(g64, exp64), (ws, canon, e)
            assert np.array_equal(g128, exp128), (ws, canon, e)


@pytest.mark.gpu
def test_all_ones_gpu(gpu_ctx, oracle):
    t64, t128 = ones_tables(256), ones_tables(512)
    seqs = [b"A" * n for n in ONES_N]
    bases, offsets = batch(seqs)
    for w in ONES_W:
        for canon in (False, True):
            got64 = gpu_ctx.rolling_hash(bases, offsets, 1, canon, t64, w=w)
            got128 = gpu_ctx.rolling_hash128(bases, offsets, 1, canon, t128, w=w)
            for s, g64, g128 in zip(seqs, got64, got128):
                assert np.array_equal(g64, oracle.rolling_hash(s, 1, canon, t64, w=w)), (len(s), w, canon)
                assert np.array_equal(g128, oracle.rolling_hash128(s, 1, canon, t128, w=w)), (len(s), w, canon)
    four, five = batch([b"AAAA"]), batch([b"AAAAA"])
    assert gpu_ctx.rolling_hash(*four, 1, False, t64, w=5)[0].tolist() == [ONES]
    assert gpu_ctx.rolling_hash128(*four, 1, False, t128, w=5)[0].tolist() == [[ONES, ONES]]
    assert gpu_ctx.rolling_hash(*five, 1, False, t64, w=5)[0].size == 0
    assert gpu_ctx.rolling_hash128(*five, 1, False, t128, w=5)[0].shape[0] == 0
    assert gpu_ctx.rolling_hash(*four, 1, True, t64, w=5)[0].size == 0
