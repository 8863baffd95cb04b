"""bonsai_amd/csrc/bns_classify_plan.hpp -- the one statement of which classify_kernel / classify_overflow_kernel instantiation a
call launches, and the list of instantiations that exist -- held against the rule as tests/classify_forms.py restates it, on every
point of the domain classify_forms.image() walks.  No device: the header is compiled by g++ on its own (classify_plan_lib).
tests/test_classify_forms_built.py holds the COMPILED set against the same image; tests/test_gpu_classify_forms.py runs it."""
import itertools

import classify_forms as F
import classify_plan_lib as P


def domain():
    """every point image() walks, in its order: (k, canon, spaced, gaps, layout, m of the table, identity bits, heavy, packed, paired)"""
    for k, canon, spaced, layout in itertools.product(range(1, 33), (True, False), (False, True), (0, 1, 2)):
        if spaced and k < 2:
            continue
        gaps = ([1] + [0] * (k - 2)) if spaced else None
        if layout == F.LAYOUT_MINBUCKET and not spaced:
            tables = [(m, bits) for _, m in F.distinct_windows(k) for bits in (32, 52) if bits == 32 or m < k]
        elif layout == F.LAYOUT_MINBUCKET:
            tables = [(k, 32)]
        else:
            tables = [(0, 0)]
        for (m, bits), heavy, packed, paired in itertools.product(tables, (False, True), (False, True), (False, True)):
            yield k, canon, spaced, gaps, layout, m, bits, heavy, packed, paired


def header_form(k, canon, spaced, layout, m, bits, heavy, packed, paired):
    # what the launch passes: the context's strand rule (never canonical for a spaced seed), the launch's m (k without a table m)
    return P.choose_form(k, m or k, canon and not spaced, spaced, layout, bits == 52, heavy, packed, 2 if paired else 1)


def test_domain_is_the_one_image_walks():
    kern, ovf = set(), set()
    n = 0
    for k, canon, spaced, gaps, layout, m, bits, heavy, packed, paired in domain():
        kern.add(F.expected_form(k, canon, gaps, layout, m, bits, heavy, packed, paired))
        ovf.add(F.expected_overflow_form(gaps, layout, bits, packed))
        n += 1
    assert (kern, ovf) == F.image()
    assert n == 3904                                     # exhaustive: every point, none sampled away
    print("%d points" % n)


def test_choose_form_is_the_rule_on_every_point():
    listed, listed_ovf = set(P.forms()), set(P.overflow_forms())
    for k, canon, spaced, gaps, layout, m, bits, heavy, packed, paired in domain():
        point = (k, canon, spaced, layout, m, bits, heavy, packed, paired)
        got = header_form(k, canon, spaced, layout, m, bits, heavy, packed, paired)
        assert got == F.expected_form(k, canon, gaps, layout, m, bits, heavy, packed, paired), point
        assert got in listed, point                      # the launcher finds every key the rule can return
        got_ovf = P.choose_overflow_form(spaced, layout, bits == 52, packed)
        assert got_ovf == F.expected_overflow_form(gaps, layout, bits, packed), point
        assert got_ovf in listed_ovf, point


def test_list_of_forms_is_the_image():
    kern, ovf = F.image()
    forms, oforms = P.forms(), P.overflow_forms()
    print("%d classify_kernel and %d classify_overflow_kernel forms listed" % (len(forms), len(oforms)))
    assert len(set(forms)) == len(forms) and len(set(oforms)) == len(oforms)      # no form twice: one instantiation per entry
    assert set(forms) == kern
    assert set(oforms) == ovf


def test_window_no_candidate_gives_is_generic():
    """(outside the domain: no loader produces it) a common k with an m that is no MIN_CANDS window runs the generic kernel"""
    assert P.choose_form(31, 19, True, False, 2, False, False, False, 1) == (0, 2, 0, 0, 8, 0, 0, 0)
    assert P.choose_form(31, 31, True, False, 2, False, False, False, 1) == (0, 2, 0, 0, 8, 0, 0, 0)
    assert P.choose_form(31, 20, True, False, 2, False, False, False, 1) == (0, 2, 31, 1, 11, 0, 0, 0)


def test_ovf_heavy():
    c = P.constants()
    off, on = c["DBG_OVC_OFF"], c["DBG_OVC_ON"]
    assert (off, on) == (F.DBG_OVC_OFF, F.DBG_OVC_ON)
    assert P.ovf_heavy(on, 0, 10 ** 9) is True            # forced on with nothing in the overflow table
    assert P.ovf_heavy(off, 10 ** 9, 10 ** 9) is False    # forced off with everything there
    assert P.ovf_heavy(on | off, 0, 10 ** 9) is True      # both: on wins
    assert P.ovf_heavy(on | off, 10 ** 9, 10 ** 9) is True
    # more than 1 key in 1000: the boundary, one key either side of it
    assert P.ovf_heavy(0, 5, 5000) is False
    assert P.ovf_heavy(0, 6, 5000) is True
    assert P.ovf_heavy(0, 5, 4999) is True
    assert P.ovf_heavy(0, 5, 5001) is False
    assert P.ovf_heavy(0, 0, 0) is False
    assert P.ovf_heavy(0x100 | 0x4000, 6, 5000) is True   # other bits do not matter
    for dbg, n_ovf, n_keys in itertools.product((0, off, on, on | off, 0x100), (0, 1, 5, 6, 10 ** 7), (0, 999, 1000, 4999, 5000, 5001, 10 ** 10)):
        assert P.ovf_heavy(dbg, n_ovf, n_keys) == F.ovf_heavy(dbg, n_ovf, n_keys), (dbg, n_ovf, n_keys)


def test_unit_can_overflow():
    cap = P.constants()["LDS_CAP"]
    assert cap == F.LDS_CAP == 128
    for c in (31, 46, 1):
        # one mate: 128 k-mers fit the in-LDS counter, 129 need the list
        assert P.max_unit_kmers(1, 128 + c - 1, c) == 128 and not P.can_overflow(1, 128 + c - 1, c)
        assert P.max_unit_kmers(1, 129 + c - 1, c) == 129 and P.can_overflow(1, 129 + c - 1, c)
        # two mates: 2 x 64 fit, 2 x 65 do not (the bound counts both mates at the longest read's length)
        assert P.max_unit_kmers(2, 64 + c - 1, c) == 128 and not P.can_overflow(2, 64 + c - 1, c)
        assert P.max_unit_kmers(2, 65 + c - 1, c) == 130 and P.can_overflow(2, 65 + c - 1, c)
        assert P.can_overflow(2, 100 + c - 1, c) and not P.can_overflow(1, 100 + c - 1, c)
        # a read of exactly c bases is one k-mer; anything shorter is none (and no unsigned wrap-around)
        assert P.max_unit_kmers(1, c, c) == 1 and P.max_unit_kmers(2, c, c) == 2
    for nm in (1, 2):
        for max_len in (0, 1, 30):
            assert P.max_unit_kmers(nm, max_len, 31) == 0 and not P.can_overflow(nm, max_len, 31)


def test_unit_limit():
    lim = (1 << 32) - (1 << 22)
    assert P.constants()["MAX_CLASSIFY_UNITS"] == lim
    assert not P.too_many_units(lim - 1)
    assert P.too_many_units(lim)
    assert not P.too_many_units(0) and P.too_many_units(1 << 32) and P.too_many_units((1 << 64) - 1)


def test_win_scratch_bytes():
    """the queue image of a window over the emitted stream: none up to 64 k-mers, none for windows over positions"""
    LEX, PATH, STRING = 0, 1, 2
    assert P.win_scratch_bytes(False, False, LEX, 31 + 63, 31, 100) == 0                   # 64 k-mers: LDS
    assert P.win_scratch_bytes(False, False, LEX, 31 + 64, 31, 100) == 100 * 4 * 2 * (64 + 65) * 8
    assert P.win_scratch_bytes(False, True, STRING, 31 + 64, 31, 7) == 7 * 4 * 2 * (64 + 65) * 8
    assert P.win_scratch_bytes(False, True, LEX, 31 + 64, 31, 100) == 0                    # canonical, not the string score: positions
    assert P.win_scratch_bytes(False, True, PATH, 31 + 64, 31, 100) == 0
    assert P.win_scratch_bytes(True, False, LEX, 46 + 64, 46, 100) == 0                    # spaced
    assert P.win_scratch_bytes(False, False, LEX, 0, 31, 100) == 0                         # unwindowed
    assert P.win_scratch_bytes(False, False, LEX, 31, 31, 100) == 0
