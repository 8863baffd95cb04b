"""The confidence threshold's definition (tests/confidence_ref.py) against answers worked out by hand on synth.TAX_PAIRS, and the Python
binding's conversion of a threshold into num / den.  No GPU: tests/test_gpu_confidence.py holds the device against the same restatement."""
import math
import types
from fractions import Fraction

import pytest

import confidence_ref as cr
import synth
from bonsai_amd.context import Context, confidence_fraction

PAR = cr.parent_map(synth.TAX_PAIRS)


def test_parent_map_and_chain():
    assert PAR[1] == 0 and PAR[2001] == 201
    assert cr.chain(PAR, 1001) == [1001, 101, 11, 2, 1]
    assert cr.chain(PAR, 1500) is None and cr.chain(PAR, 0xFFFFFFFF) is None
    broken = cr.parent_map([(c, p) for c, p in synth.TAX_PAIRS if c != 201])
    assert cr.chain(broken, 2001) is None
    # a parent array (as bns_load_taxonomy takes it) gives the same map
    n = max(c for c, _ in synth.TAX_PAIRS) + 1
    arr = [0xFFFFFFFF] * n
    for c, p in synth.TAX_PAIRS:
        arr[c] = 0 if c == 1 else p
    assert cr.parent_map(arr) == PAR


def test_clade_exactly_r_passes():
    hits = [1001] * 3 + [2001] * 7                      # Q = 10
    assert cr.walk(PAR, Fraction(3, 10), 1001, 0, hits) == 1001      # R = 3, clade(1001) = 3
    assert cr.walk(PAR, Fraction(31, 100), 1001, 0, hits) == 1       # R = 4: 101, 11 and 2 hold 3 too; the root holds 10


def test_walk_stops_midway():
    hits = [1001] * 2 + [1002] * 3                      # Q = 10 with 5 missing
    assert cr.walk(PAR, Fraction(1, 2), 1001, 5, hits) == 101
    assert cr.walk(PAR, Fraction(1, 5), 1001, 5, hits) == 1001


def test_theta_zero_is_the_identity():
    for t in (0, 1, 1001, 2002, 1500, 0xFFFFFFFF):
        assert cr.walk(PAR, 0, t, 5, [2001]) == t


def test_theta_one_with_a_missing_kmer_gives_zero():
    assert cr.walk(PAR, 1, 1001, 1, [1001] * 10) == 0
    assert cr.walk(PAR, 1, 1001, 0, [1001] * 10) == 1001


def test_taxon_outside_the_taxonomy_is_unchanged():
    for t in (1500, 7777, 0xFFFFFFFF):
        assert cr.walk(PAR, Fraction(1, 2), t, 0, [1001] * 4) == t
    broken = cr.parent_map([(c, p) for c, p in synth.TAX_PAIRS if c != 201])
    assert cr.walk(broken, 1, 2001, 50, [1001]) == 2001
    assert cr.walk(PAR, 1, 2001, 50, [1001]) == 0


def test_hits_outside_the_taxonomy_count_in_q_only():
    hits = [1001] * 5 + [7777] * 3 + [1500] * 2          # Q = 10
    assert cr.clade_count(PAR, 1, hits) == 5
    assert cr.walk(PAR, Fraction(1, 2), 1001, 0, hits) == 1001
    assert cr.walk(PAR, Fraction(3, 5), 1001, 0, hits) == 0


def test_exact_ceil_theta_tenth_q_thirty():
    assert cr.required(Fraction("0.1"), 30) == 3
    hits = [1001] * 3 + [2001] * 27
    assert cr.walk(PAR, Fraction("0.1"), 1001, 0, hits) == 1001
    assert cr.walk(PAR, Fraction("0.1"), 1001, 1, hits) == 1           # Q = 31: R = 4


def test_exact_ceil_where_a_double_rounds_up():
    assert cr.required(Fraction("0.07"), 100) == 7
    assert math.ceil(0.07 * 100) == 8                    # 7.000000000000001 in double: the deliberate difference
    hits = [1001] * 7 + [2001] * 93
    assert cr.walk(PAR, Fraction("0.07"), 1001, 0, hits) == 1001


def test_walk_through_the_root_gives_zero():
    assert cr.walk(PAR, Fraction(1, 2), 1001, 8, [1001, 1002]) == 0
    assert cr.walk(PAR, Fraction(1, 2), 1, 8, [1001, 2001]) == 0


def test_boundaries_are_exact():
    hits = [1001] * 2 + [1002] * 3
    b = cr.boundaries(PAR, 1001, 5, hits)
    assert b == {Fraction(2, 10), Fraction(5, 10)}
    for th in b:
        assert cr.walk(PAR, th, 1001, 5, hits) != 0


def test_confidence_fraction():
    assert confidence_fraction(0.1) == (1, 10)
    assert confidence_fraction("0.25") == (1, 4)
    assert confidence_fraction(Fraction(1, 3)) == (1, 3)
    assert confidence_fraction(0) == (0, 1) and confidence_fraction(1) == (1, 1)
    for bad in (1.5, -0.1, "abc", None, True):
        with pytest.raises(ValueError):
            confidence_fraction(bad)


def test_set_confidence_rejects_before_the_library():
    stub = types.SimpleNamespace()                       # no library, no context: the value is refused first
    for bad in (1.5, -0.1):
        with pytest.raises(ValueError):
            Context.set_confidence(stub, bad)
