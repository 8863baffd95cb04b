"""What a table load decides (bonsai_amd/csrc/bns_table_plan.hpp), held on the host against the rules its comments state: the
pick among the trial's candidates (cases from the calibration the thresholds came from), the candidate lists for contiguous and
spaced seeds, the table size and its refusals, arrival-order or group-aware fill, upload or stream.  No GPU: the header is
compiled on its own (tests/table_plan_lib.py)."""
import itertools

import pytest

import table_plan_lib as P

HUGE = 1 << 50                                       # free bytes that refuse nothing


def counters(*miss_per_10000):
    """trial counters of candidates that see 10000 keys each and leave that many outside their home bucket (2 : 1 spilled : chain exhausted)"""
    return [(10000, m - m // 3, m // 3) for m in miss_per_10000]


def test_constants():
    c = P.constants()
    assert c["MINB_CAP"] == 10 and c["MINB_MAX_CHAIN"] == 4 and c["PLAN_MAX_CANDS"] == 6
    assert c["MIN_CANDS"] == [(15, 16), (11, 19), (8, 19)] and c["MINB_TARGET_LOAD"] == 1.0 / 12.0
    for k in range(1, 33):
        for span, floor in c["MIN_CANDS"]:
            assert P.minimizer_len(k, span, floor) == (k if k <= floor else max(k - span, floor))


def test_pinned_cases_are_the_cases():
    """tests/golden/table_plan_parent.json (what tests/test_gpu_table_plan.py holds the loader against) has every case of
    tests/table_plan_cases.py and every field: none differed between two runs of the loader that wrote it"""
    import json
    import os
    import table_plan_cases as T
    with open(os.path.join(P.ROOT, "tests", "golden", "table_plan_parent.json")) as fh:
        pinned = json.load(fh)
    ids = {T.case_id(*g, *c) for g in T.groups() for c in T.group_cases()}
    assert ids == set(pinned["cases"]) and len(ids) == 432
    assert pinned["fields"] == list(T.FIELDS)


# ---- pick
K31 = [0, 0, 0, 1, 1, 1]                             # k = 31, nothing asked for: spans 15, 11, 8 narrow, then wide


def test_pick_narrow_when_the_widest_window_fits():
    """a 9e8-key db of window minimizers: 0.4 % outside -> narrow, the widest window"""
    assert P.pick(K31, counters(40, 10, 5, 1, 1, 1)) == (0, 0.004)


def test_pick_first_window_under_one_per_cent():
    assert P.pick(K31, counters(100, 99, 5, 0, 0, 0)) == (1, 0.0099)       # 1.00 % is not "fewer than 1 in 100"
    assert P.pick([0, 0, 0], counters(500, 300, 99))[0] == 2


def test_pick_wide_when_narrow_is_crowded_and_wide_much_better():
    """every-k-mer dbs: narrow 6.9 % / 12 % outside, wide at most 60 % of that -> wide"""
    assert P.pick(K31, counters(2000, 1500, 690, 1500, 900, 410)) == (5, 0.041)           # 4.1 % <= 0.6 * 6.9 % = 4.14 %
    assert P.pick(K31, counters(3000, 2000, 1200, 50, 0, 0))[0] == 3                      # (the widest wide window under 1 %)


def test_pick_narrow_when_wide_is_not_much_better():
    assert P.pick(K31, counters(2000, 1500, 690, 1500, 900, 418)) == (2, 0.069)           # 4.18 % > 0.6 * 6.9 % = 4.14 %
    assert P.pick(K31, counters(2000, 1500, 199, 0, 0, 0))[0] == 2                        # narrow under 2 %: wide is not worth its cost
    assert P.pick(K31, counters(2000, 1500, 200, 1500, 900, 100))[0] == 5                 # (2 % itself counts as crowded)


def test_pick_narrowest_when_nothing_fits():
    """no candidate under 1 % -> the narrowest window of that identity"""
    assert P.pick([0, 0, 0], counters(900, 700, 500)) == (2, 0.05)
    assert P.pick([1, 1, 1], counters(900, 700, 500)) == (2, 0.05)
    assert P.pick([1, 1], counters(900, 50))[0] == 1                                      # (one identity asked for: the other has no say)


def test_pick_spaced():
    """spaced seeds, two candidates: the longer window (candidate 0) iff fewer than 5 keys in 100 miss their home bucket"""
    assert P.pick([0, 0], counters(499, 0), spaced=True) == (0, 0.0499)
    assert P.pick([0, 0], counters(500, 123), spaced=True) == (1, 0.0123)
    assert P.pick([0, 0], counters(440, 0), spaced=True)[0] == 0                          # configs[2]'s db: 4.4 % outside, taken
    assert P.pick([0, 0], counters(1900, 0), spaced=True)[0] == 1                         # 19 % outside, refused


def test_pick_zero_denominator():
    """a candidate that sampled no key has miss 0"""
    assert P.pick(K31, [(0, 0, 0)] * 6) == (0, 0.0)
    assert P.pick([0, 0], [(0, 7, 7), (10, 0, 0)], spaced=True) == (0, 0.0)


# ---- candidate lists
def spans(cands):
    return [(c["span"], c["wide"]) for c in cands]


def test_contiguous_candidates_k31():
    got = P.cands_contiguous(31)
    assert spans(got) == [(15, 0), (11, 0), (8, 0), (15, 1), (11, 1), (8, 1)]
    assert [c["m"] for c in got] == [16, 20, 23, 16, 20, 23]
    assert all(c["len"] == 31 and c["shift"] == 0 and c["canon"] == 1 for c in got)


def test_contiguous_candidates_requests_filter():
    assert spans(P.cands_contiguous(31, min_span_req=11)) == [(11, 0), (11, 1)]
    assert spans(P.cands_contiguous(31, wide_req=0)) == [(15, 0), (11, 0), (8, 0)]
    assert spans(P.cands_contiguous(31, wide_req=1)) == [(15, 1), (11, 1), (8, 1)]
    assert spans(P.cands_contiguous(31, min_span_req=15, wide_req=1)) == [(15, 1)]       # what a replica's plan amounts to: one candidate


def test_contiguous_candidates_equal_m_neighbours_dropped():
    got = P.cands_contiguous(21)                         # m = 16, 19, 19: the second 19 says nothing new
    assert [(c["m"], c["span"], c["wide"]) for c in got] == [(16, 15, 0), (19, 11, 0), (16, 15, 1), (19, 11, 1)]
    assert [(c["m"], c["span"]) for c in P.cands_contiguous(21, min_span_req=8)] == [(19, 8), (19, 8)]


def test_contiguous_candidates_small_k():
    """minimizer_len == k: no window.  One narrow candidate; the wide identity has nothing to be carried through, and asking
    for it gives the narrow fallback"""
    for k in (5, 16):
        assert [(c["m"], c["wide"]) for c in P.cands_contiguous(k)] == [(k, 0)]
        assert P.cands_contiguous(k, wide_req=1) == [{"m": k, "len": k, "shift": 0, "canon": 1, "wide": 0, "span": 8}]
        assert P.cands_contiguous(k, min_span_req=15, wide_req=1) == [{"m": k, "len": k, "shift": 0, "canon": 1, "wide": 0, "span": 8}]


def spaced_model(k, n_present, R, shift, force, nocluster):
    """the rule as the comments in plan_cands_spaced state it"""
    own = {"m": k, "len": k, "shift": 0, "canon": 1, "wide": 0, "span": 0}
    if R < 12 or nocluster:
        return [own]
    m = 11
    while m < 32 and 4 ** m < n_present:
        m += 1
    if force:
        m = max(8, force)
    if m + 8 < R:
        m = R - 8
    out = []
    if not force and m >= 9 and m + 7 >= R and m <= R:
        out.append({"m": m - 1, "len": R, "shift": shift, "canon": 0, "wide": 0, "span": 0})
    out.append({"m": m, "len": R, "shift": shift, "canon": 0, "wide": 0, "span": 0} if m + 1 <= R else own)
    return out


def test_spaced_candidates():
    seen = set()
    for R, n_present, force, nocluster in itertools.product(range(0, 32), (0, 19000, 4 ** 11 + 1, 230_000_000, 780_000_000, 4 ** 16, 4 ** 20),
                                                              (0, 5, 8, 12, 14, 31), (False, True)):
        dbg = (force << P.DBG_SPACED_M_SHIFT) | (P.DBG_SPACED_NOCLUSTER if nocluster else 0)
        got = P.cands_spaced(31, n_present, R, 2 * (31 - R) if R else 0, dbg)
        assert got == spaced_model(31, n_present, R, 2 * (31 - R) if R else 0, force, nocluster), (R, n_present, force, nocluster)
        seen.add((len(got), got[-1]["m"] == 31))
    assert seen == {(1, True), (1, False), (2, False), (2, True)}
    # R < 12 or SPACED_NOCLUSTER: m = k
    assert P.cands_spaced(31, 10 ** 9, 11)[0]["m"] == 31 and P.cands_spaced(31, 10 ** 9, 16, dbg=P.DBG_SPACED_NOCLUSTER)[0]["m"] == 31
    # configs[2]: 1x15,0x15 (a run of 16), 7.8e8 keys -> m = 15, and 14 tried first
    assert [c["m"] for c in P.cands_spaced(31, 780_000_000, 16, 0)] == [14, 15]
    # the m - 1 candidate exactly when m >= 9, m + 7 >= R, m <= R and m is not forced
    assert [c["m"] for c in P.cands_spaced(31, 19000, 18)] == [10, 11] and [c["m"] for c in P.cands_spaced(31, 19000, 19)] == [11]
    assert [c["m"] for c in P.cands_spaced(31, 4 ** 16, 15)] == [31]                       # m = 16 > R: no window at all
    assert [c["m"] for c in P.cands_spaced(31, 19000, 16, dbg=13 << P.DBG_SPACED_M_SHIFT)] == [13]
    assert [c["m"] for c in P.cands_spaced(31, 19000, 16, dbg=5 << P.DBG_SPACED_M_SHIFT)] == [8]


# ---- sizing
def test_minbucket_size_automatic():
    c = P.constants()
    for n_present in (0, 10, 19357, 1_000_000, 900_000_000):
        want = max(64, int(n_present / (c["MINB_CAP"] * c["MINB_TARGET_LOAD"])))
        assert P.size_minbucket(n_present, HUGE) == (P.OK, want, "")
    assert P.size_minbucket(10, HUGE)[1] == 64                                            # the floor
    assert P.size_minbucket(1_000_000, HUGE)[1] == 1_200_000                              # a twelfth full
    free_b = 85_400_000                                                                   # three quarters of it hold 500390 buckets
    assert free_b // 4 * 3 // 128 == 500390
    assert P.size_minbucket(1_000_000, free_b) == (P.OK, 500390, "")
    assert P.size_minbucket(1_000_000, free_b, n_buckets_req=600_000) == (P.OK, 600_000, "")     # (a request is not capped)
    assert P.size_minbucket(1_000_000, HUGE, slots_log2_req=23) == (P.OK, 1 << 20, "")    # 8 slots per bucket
    assert P.size_minbucket(1, HUGE, slots_log2_req=2) == (P.OK, 1, "")


def test_minbucket_size_hard_cap():
    cap = (1 << 31) - 8
    assert P.size_minbucket(1000, HUGE, n_buckets_req=cap) == (P.OK, cap, "")
    assert P.size_minbucket(1000, HUGE, n_buckets_req=cap + 1) == (P.ERR_ARG, None, "more than 2^31 buckets: bucket indices are 31-bit")
    assert P.size_minbucket(1000, HUGE, slots_log2_req=35)[0] == P.ERR_ARG
    assert P.size_minbucket(20_000_000_000, HUGE) == (P.OK, cap, "")                      # the automatic count is clamped instead


def test_minbucket_size_refusals():
    assert P.size_minbucket(9700, HUGE, n_buckets_req=1000) == (P.OK, 1000, "")
    assert P.size_minbucket(9701, HUGE, n_buckets_req=1000) == (P.ERR_TABLE, None, "bucket table too small for the key count")
    assert P.size_minbucket(100, 1003 * 128, n_buckets_req=1000) == (P.OK, 1000, "")      # + MINB_MAX_CHAIN - 1 spill-only buckets
    assert P.size_minbucket(100, 1003 * 128 - 1, n_buckets_req=1000) == (P.ERR_NOMEM, None, "bucket table does not fit in free HBM")
    # memory so short that the automatic count cannot hold the keys
    assert P.size_minbucket(1_000_000, 128 * 100_000)[0] == P.ERR_TABLE


def test_bucket_size():
    assert P.size_bucket(1 << 15, HUGE) == (P.OK, 16, "")                                 # lg + 1
    assert P.size_bucket((1 << 15) - 1, HUGE)[1] == 16 and P.size_bucket((1 << 15) + 1, HUGE)[1] == 17
    assert P.size_bucket(4, HUGE) == (P.OK, 4, "") and P.size_bucket(4, HUGE, slots_log2_req=2)[1] == 4      # at least 16 slots
    assert P.size_bucket(1 << 15, HUGE, slots_log2_req=20)[1] == 20
    assert P.size_bucket(1 << 15, HUGE, slots_log2_req=15) == (P.ERR_ARG, None, "bucket_slots_log2 too small for this khash")
    assert P.size_bucket(1 << 15, 16 << 16) == (P.OK, 16, "")
    assert P.size_bucket(1 << 15, (16 << 16) - 1) == (P.ERR_NOMEM, None, "bucket table does not fit in free HBM")


# ---- fill
def test_group_fill_decision():
    GROUP, PLAIN = P.DBG_GROUP_FILL, P.DBG_PLAIN_FILL
    # bns_set_table_fill wins over everything
    for n_cands, miss, dbg in itertools.product((1, 6), (0.0, 0.5), (0, GROUP, PLAIN, GROUP | PLAIN)):
        assert P.group_fill(n_cands, miss, 10 ** 6, 1000, fill_req=1, dbg=dbg) is True
        assert P.group_fill(n_cands, miss, 10 ** 6, 1000, fill_req=0, dbg=dbg) is False
    # the debug bits: PLAIN_FILL beats GROUP_FILL and a crowded table, GROUP_FILL fills a table with room group by group
    assert P.group_fill(6, 0.5, 10 ** 6, 1000, dbg=PLAIN | GROUP) is False and P.group_fill(1, 0.0, 10 ** 6, 1000, dbg=PLAIN) is False
    assert P.group_fill(6, 0.0, 10, 1000, dbg=GROUP) is True and P.group_fill(1, 0.0, 10, 1000, dbg=GROUP) is True
    # with a trial: crowded from 1 key in 100 outside its home bucket, whatever the load
    assert P.group_fill(2, 0.01, 10, 1000) is True and P.group_fill(2, 0.0099, 10 ** 6, 1000) is False
    # without one: more than an eighth full (800 buckets of 10: 1000 keys)
    assert P.group_fill(1, 0.5, 1000, 800) is False and P.group_fill(1, 0.0, 1001, 800) is True


def test_overflow_table_size():
    assert P.overflow_slots(0, 1000) == 4096 and P.overflow_slots(1, 1000) == 8192        # at most half full, + 2048 for place
    assert P.overflow_slots(0, 6100 + 60, P.DBG_PLACE_FAIL) == 8192                       # 2 * (2048 + 100 * 10 + 10) = 6116
    assert P.overflow_slots(10 ** 6, 1000) == 1 << 21
    assert P.trial_sample(19357) == 19357 and P.trial_sample(1 << 22) == 1 << 22 and P.trial_sample((1 << 22) + 1) == 1 << 21


# ---- upload or stream
def test_stream_predicate():
    nb = 1 << 20
    need = (nb >> 4) * 4 + nb * 12 + nb * 16           # the arrays and 16 bytes of table per khash bucket
    assert need == 29622272 and need // 85 == 348497 and need % 85
    assert P.stream_load(nb, 348498 * 100) is False     # 85 % of free (in whole per cents) covers it
    assert P.stream_load(nb, 348498 * 100 - 1) is True
    assert P.stream_load(nb, HUGE) is False and P.stream_load(nb, HUGE, P.DBG_STREAM_LOAD) is True
    assert P.stream_load(8, 400) is False and P.stream_load(8, 200) is True               # fewer than 16 buckets: one flag word (4 + 96 + 128 bytes)
