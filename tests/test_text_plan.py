"""What a bns_classify_text call decides (bonsai_amd/csrc/bns_text_plan.hpp), on the host: numbers worked by hand from the lines the
plan was lifted from, then the header against their restatement tests/text_plan_model.py on a grid of sizes, offsets, streams,
debug bits and overrides -- with the properties the kernels' bounds rest on asserted on every point.  No GPU: the header is
compiled on its own (tests/text_plan_lib.py)."""
import itertools

import text_plan_lib as P
import text_plan_model as M

MiB = 1 << 20
SIZES = (0, 1, 63, 64, 8191, 8192, 8193, 64 * MiB - 1, 64 * MiB, 64 * MiB + 1, 128 * MiB - 1, 128 * MiB, 128 * MiB + 1, (1 << 31) - 1)
DBGS = (0, P.DBG_SLICE_8K, P.DBG_SLICE_8K | P.DBG_BATCH_TINY)
OVERRIDES = ((0, 0), (1, 1000), (2048, 0))                   # (BNS_TEXT_PIECE_MB, BNS_TEXT_BATCH_READS): unset, both set, and pieces so large that a pair is "too large"
WANTS = ({"parse_only": True}, {}, {"want_runs": True}, {"want_lines": True}, {"want_words": True}, {"parse_only": True, "want_words": True})


def test_constants():
    c = P.constants()
    assert c == {"TILE": 16384, "REC_BLOCK": 2048, "MAX_PIECES": 64, "sizeof_CallInfo": 184, "CALL_INFO_BYTES": 192, "sizeof_StreamInfo": 64,
                 "DBG_SLICE_8K": 0x4000, "DBG_BATCH_TINY": 0x40}
    assert (M.TILE, M.REC_BLOCK, M.MAX_PIECES, M.SIZEOF_CALL_INFO) == (c["TILE"], c["REC_BLOCK"], c["MAX_PIECES"], c["sizeof_CallInfo"])


def test_pinned_cases_are_the_cases():
    """tests/golden/text_plan_parent.json (what tests/test_gpu_text_plan.py holds bns_classify_text against) has every case of
    tests/text_plan_cases.py and, for every call of a case, every field: none differed between the two runs that wrote it"""
    import json
    import os
    import text_plan_cases as T
    with open(os.path.join(P.ROOT, "tests", "golden", "text_plan_parent.json")) as fh:
        pinned = json.load(fh)
    assert {T.case_id(*c) for c in T.cases()} == set(pinned["cases"]) and len(pinned["cases"]) == 30
    assert pinned["fields"] == list(T.FIELDS)
    for cid, calls in pinned["cases"].items():
        assert len(calls) == (2 if cid.startswith("prefetched") else 1)
        assert all(sorted(call) == sorted(T.FIELDS) for call in calls), cid


def test_pin_small_host_text():
    """one stream, 1000 bytes of host text, no debug bits: one 64 MiB piece, one slice, nothing carried"""
    piece = P.piece_bytes(0, 0, 1000)
    assert piece == 64 * MiB
    rc, p, _ = P.plan([1000], upload_piece=[piece])
    assert rc == P.OK
    assert (p["s0_piece"], p["s0_n"], p["n_slices"]) == (64 * MiB, 1, 1)
    assert (p["range_cap"], p["cap_lines"], p["cap_rec"]) == (1000, 1149, 574)                     # 1000 / 8 + 1024, 1000 / 16 + 512
    assert (p["cap_reads"], p["cap_bases"], p["cap_names"]) == (574, 1000, 1000)
    assert (p["st_tiles"], p["st_groups"], p["st_cand"], p["st_recs"]) == (8, 2, 2, 2)
    assert p["info_bytes"] == 400                                                                  # 192 + 26 * 8


def test_pin_sliced_host_text():
    """one stream, 100000 bytes of host text in 8 KiB pieces: 13 slices, a parse covers two of them, a batch carries what 64 MiB can hold"""
    piece = P.piece_bytes(P.DBG_SLICE_8K, 0, 100000)
    assert piece == 8192
    rc, p, _ = P.plan([100000], upload_piece=[piece], dbg=P.DBG_SLICE_8K)
    assert rc == P.OK
    assert (p["s0_piece"], p["s0_n"], p["n_slices"]) == (8192, 13, 13)
    assert (p["range_cap"], p["window"]) == (16448, 16384)                                         # 2 * 8192 + 64
    assert (p["cap_lines"], p["cap_rec"]) == (3080, 1540)
    assert (p["carry_reads"], p["cap_reads"], p["carry_bases"]) == (1048640, 1050180, 64 * MiB)    # 64 MiB / 64 + 64
    rc, p, _ = P.plan([100000], upload_piece=[piece], dbg=P.DBG_SLICE_8K | P.DBG_BATCH_TINY)
    assert rc == P.OK and (p["batch_reads"], p["cap_reads"]) == (64, 1604)


def test_piece_rule():
    for dbg, mb, n in itertools.product(DBGS, (0, -1, 1, 256), SIZES):
        assert P.piece_bytes(dbg, mb, n) == M.piece_bytes(dbg, mb, n)
        assert P.piece_bytes(dbg, mb, n) * 64 >= n and P.piece_bytes(dbg, mb, n) % 64 == 0         # at most MAX_PIECES events; aligned pieces


def test_tiles_of_a_stretch():
    T = 16384
    for lo, hi in ((0, 0), (0, 1), (0, T), (0, T + 1), (T - 1, T), (T - 1, T + 1), (5, 5), (T, T), (3 * T + 7, 9 * T), ((1 << 31) + 62, (1 << 31) + 63),
                   (0, (1 << 31) + 62)):
        assert P.tile0(lo) == lo // T
        assert P.n_tiles(lo, hi) == ((hi - 1) // T - lo // T + 1 if hi > lo else 1)               # bns_ingest.hip:1279 of the model's commit
        assert (P.tile0(lo) + P.n_tiles(lo, hi)) * T >= hi                                         # the tiles cover the stretch


def stream_sets():
    """one stream of every size; pairs of unequal size: every size with the next one, either way round"""
    one = [(n,) for n in SIZES]
    two = [(SIZES[i], SIZES[(i + 1) % len(SIZES)]) for i in range(len(SIZES))]
    return one + two + [(b, a) for a, b in two]


def placements(sizes, dbg, piece_mb):
    """(on_device, rel, upload_piece) of a grid point: device text at pointer offsets 0, 1, 63; host text at offsets 0, 1, 63 of an
    upload and at one that is no multiple of its piece -- as far as upload and text stay below 2^31 bytes"""
    for r in (0, 1, 63):
        yield True, [r] * len(sizes), [0] * len(sizes)
    for r in (0, 1, 63, None):
        rel, pieces = [], []
        for n in sizes:
            off = r
            if off is None:                                  # behind one piece and a bit, of an upload that goes on a little
                off = P.piece_bytes(dbg, piece_mb, 3 * n + 70000) + 4097
            if off + n > (1 << 31) - 1:
                break
            rel.append(off)
            pieces.append(P.piece_bytes(dbg, piece_mb, off + n + (0 if r == 0 else 1000)))
        else:
            yield False, rel, pieces


def grid():
    for sizes, dbg, (piece_mb, batch_reads), wants in itertools.product(stream_sets(), DBGS, OVERRIDES, WANTS):
        for on_device, rel, pieces in placements(sizes, dbg, piece_mb):
            yield dict(sizes=list(sizes), rel=rel, upload_piece=pieces, on_device=on_device, dbg=dbg, piece_mb=piece_mb, batch_reads=batch_reads, **wants)


def check_point(kw):
    rc, p, msg = P.plan(**kw)
    mrc, m, mmsg = M.plan(**kw)
    # the refusals fire exactly where they did, with their code and their words
    assert (rc, msg) == (mrc, mmsg), kw
    if rc != P.OK:
        return msg
    # every field, the byte size of every buffer included (so: at least what the ensure() line asked for)
    assert p == m, (kw, {f: (p[f], m[f]) for f in P.FIELDS if p[f] != m[f]})
    ns = len(kw["sizes"])
    for s in range(ns):
        st = {f: p["s%d_%s" % (s, f)] for f in P.STREAM_FIELDS}
        n = st["n"]
        assert n <= 65 and st["end"] == st["rel"] + kw["sizes"][s]
        ends = [P.up_to(p, s, k) for k in range(n + 2)]
        assert ends == [M.up_to(st, k) for k in range(n + 2)]
        assert all(a <= b for a, b in zip(ends, ends[1:])) and ends[n - 1] == st["end"] and ends[-1] == st["end"]
        assert ends[0] >= st["rel"] and (n == 1 or ends[0] > st["rel"])
        # the event a slice waits for is one the upload recorded: the last piece that holds text of the call
        assert [P.piece_of(p, s, k) for k in range(n + 2)] == [min(st["j0"] + k, st["j0"] + n - 1) for k in range(n + 2)]
        if not kw["on_device"]:
            assert st["j0"] + n - 1 < 64 or st["end"] == st["rel"]
        # one parse's stretch -- never more than the window when there are several slices, the whole text when there is one -- fits what is sized by range_cap
        assert p["n_slices"] > 1 or kw["sizes"][s] <= p["range_cap"]
    if p["n_slices"] > 1:
        # (a one-slice call does not read the window: there range_cap may be below 64)
        assert p["window"] <= p["range_cap"] - 64
        assert P.n_tiles(63, 63 + p["window"]) + 1 <= p["st_tiles"]
    for f in ("reads", "bases"):
        assert p["slice_%s_cap" % f] + p["carry_" + f] == p["cap_" + f]
    assert p["slice_bases_cap"] + p["carry_names"] == p["cap_names"]
    assert p["cap_reads"] < 1 << 31 and p["cap_bases"] < (1 << 32) - (1 << 20)
    # the CallInfo and the look-back regions lie inside the info buffer, in this order, and do not overlap
    regions = [(0, 184), (p["off_lines"], 2 * p["st_tiles"] * 8), (p["off_groups"], 2 * p["st_groups"] * 8),
               (p["off_compact"], 2 * p["st_cand"] * 8), (p["off_offsets"], p["st_recs"] * 8)]
    for (a, na), (b, _) in zip(regions, regions[1:]):
        assert a + na <= b and b % 8 == 0
    assert regions[-1][0] + regions[-1][1] <= p["info_bytes"] == p["bytes_info"]
    # blocks of compact_kernel (per stream) and of offsets_kernel each have a look-back word
    assert p["cap_rec"] // 2048 + 1 <= p["st_cand"] and p["slice_reads_cap"] // 2048 + 1 <= p["st_recs"]
    return ""


def test_grid_against_the_model():
    seen = {"": 0, M.MSG_WORDS: 0, M.MSG_LARGE: 0}
    for kw in grid():
        seen[check_point(kw)] += 1
    assert seen[""] > 5000 and seen[M.MSG_WORDS] > 100 and seen[M.MSG_LARGE] > 0, seen


def test_refusals_by_hand():
    # the packed words and two slices: 64 MiB + 1 of host text
    piece = P.piece_bytes(0, 0, 64 * MiB + 1)
    assert P.plan([64 * MiB + 1], upload_piece=[piece], want_words=True)[::2] == (P.ERR_ARG, M.MSG_WORDS)
    assert P.plan([64 * MiB], upload_piece=[P.piece_bytes(0, 0, 64 * MiB)], want_words=True)[0] == P.OK
    # a pair of 2^31 - 1 bytes each on the device: 16 slices of 128 MiB, 2 * (256 MiB + 64) + 320 MiB of bases fit; as ONE slice each they would not
    assert P.plan([(1 << 31) - 1] * 2, on_device=True)[0] == P.OK
    rc, _, msg = P.plan([(1 << 31) - 1] * 2, upload_piece=[1 << 31] * 2)
    assert (rc, msg) == (P.ERR_ARG, M.MSG_LARGE)
