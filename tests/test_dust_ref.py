"""The reference of low-complexity masking (tests/dust_ref.py) against itself: the brute-force reading of the definition, the
recurrence the kernel rests on, and the locality that lets a long sequence be cut into pieces.  No GPU."""
import numpy as np
import pytest

import dust_ref as D


def _with_ns(rng, seq):
    s = bytearray(seq)
    for _ in range(int(rng.integers(0, 3))):
        s[int(rng.integers(0, len(s)))] = ord("N")
    return bytes(s)


@pytest.fixture(scope="module")
def generated():
    """30 sequences of 3-130 bases per (W, T), 150 in all; every other one with 0-2 N's"""
    rng = np.random.default_rng(20)
    out = {}
    for p in D.PARAMS:
        seqs = D.gen_batch(rng, rng.integers(3, 131, size=30))
        out[p] = [_with_ns(rng, s) if i & 1 else s for i, s in enumerate(seqs)]
    return out


@pytest.mark.parametrize("W,T", D.PARAMS)
def test_brute_force_equals_recurrence(generated, W, T):
    seqs = generated[(W, T)]
    assert len(seqs) * len(D.PARAMS) >= 150
    batch = D.batch_masks(seqs, W, T)
    for s, bm in zip(seqs, batch):
        want = D.brute_mask(s, W, T)
        assert np.array_equal(D.recurrence_mask(s, W, T), want), (W, T, s)
        assert np.array_equal(bm, want), (W, T, s)


@pytest.mark.parametrize("W,T", D.PARAMS)
def test_generator_is_not_degenerate(generated, W, T):
    share = D.masked_share(generated[(W, T)], W, T)
    print("masked share at (%d, %d): %.3f" % (W, T, share))
    assert 0.10 <= share <= 0.70


@pytest.mark.parametrize("W,T", D.PARAMS)
def test_locality_pieces_with_halo(W, T):
    rng = np.random.default_rng(W * 1000 + T)
    seq = bytearray(D.gen_seq(rng, 5000))
    for at in (700, 2047, 2048, 3500):
        seq[at] = ord("N")
    seq = bytes(seq)
    whole = D.recurrence_mask(seq, W, T)
    share = whole.mean()
    assert 0.10 <= share <= 0.70
    halo = W - 1
    for a in range(0, len(seq), 256):
        b = min(a + 256, len(seq))
        lo, hi = max(0, a - halo), min(len(seq), b + halo)
        piece = D.recurrence_mask(seq[lo:hi], W, T)
        assert np.array_equal(piece[a - lo:b - lo], whole[a:b]), (W, T, a)


def test_homopolymer_threshold_at_64_20():
    # l equal triplets score l (l - 1) / 2 / (l - 1) = l / 2; 10 l / 2 > 20 needs l >= 5 triplets = 7 bases (score 10 / 4 = 2.5 > 2), and
    # the whole run is then one perfect interval
    first = next(n for n in range(4, 40) if D.brute_mask(b"A" * n, 64, 20).any())
    assert first == 7
    for base in b"ACGT":
        assert not D.brute_mask(bytes([base]) * (first - 1), 64, 20).any()
        assert D.brute_mask(bytes([base]) * first, 64, 20).all()
        assert not D.recurrence_mask(bytes([base]) * (first - 1), 64, 20).any()
        assert D.recurrence_mask(bytes([base]) * first, 64, 20).all()
    # inside random flanks that repeat no triplet of their own: exactly the run
    flank_l, flank_r = b"CGTCAGT", b"CTGACGC"
    s = flank_l + b"A" * first + flank_r
    m = D.brute_mask(s, 64, 20)
    assert m[len(flank_l):len(flank_l) + first].all()
    assert np.array_equal(m, D.recurrence_mask(s, 64, 20))


def _de_bruijn_4_3():
    """every triplet over ACGT exactly once: 64 + 2 bases"""
    k, n = 4, 3
    a = [0] * (k * n)
    seq = []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    seq = seq + seq[:2]
    return bytes(b"ACGT"[x] for x in seq)


@pytest.mark.parametrize("W,T", D.PARAMS + [(64, 1)])
def test_no_repeated_triplet_is_never_masked(W, T):
    s = _de_bruijn_4_3()
    tr = {s[i:i + 3] for i in range(len(s) - 2)}
    assert len(s) == 66 and len(tr) == 64
    assert not D.brute_mask(s, W, T).any()
    assert not D.recurrence_mask(s, W, T).any()


def test_short_sequences_and_case():
    for n in range(0, 4):
        assert D.recurrence_mask(b"A" * n).size == n and not D.recurrence_mask(b"A" * n).any()
        assert not D.brute_mask(b"A" * n).any()
    # lower case is a valid base in the packed image and does not end a run; any other byte does
    assert D.recurrence_mask(b"AAAaAAAA").all()
    assert not D.recurrence_mask(b"AAAAXAAAA").any()
    assert D.substitute(b"ACGTACGT", np.array([0, 1, 1, 0, 0, 0, 0, 1], dtype=bool)) == b"ANNTACGN"
