"""What a bns_classify_text call decides, restated in Python from bonsai_amd/csrc/bns_ingest.hip as it stood in commit 5887059 --
the last one in which these numbers were computed inside bns_classify_text itself, between its ensure() and HIP calls.  The line
numbers cited are that file's.  tests/test_text_plan.py holds csrc/bns_text_plan.hpp against this on a grid.  C's narrowing casts
and unsigned wrap-around are spelled out (u32 / u64 below): Python's integers do neither on their own."""
OK, ERR_ARG = 0, -1
DBG_SLICE_8K, DBG_BATCH_TINY = 0x4000, 0x40                  # bns_api.hip:60, :57
TILE, REC_BLOCK, MAX_PIECES = 16384, 256 * 8, 64             # bns_ingest.hip:49, :51-52, :657
SIZEOF_CALL_INFO = 2 * 16 * 4 + (2 + 2 + 2 + 6 + 2) * 4      # :56-70: two StreamInfo of 16 words, 14 words
MSG_WORDS = "the packed words come back for one-slice calls only (<= 64 MiB of text)"     # :1159, behind "bns_classify_text: "
MSG_LARGE = "text too large for one batch"                                                # :1185


def u32(x):
    return x & 0xFFFFFFFF


def u64(x):
    return x & 0xFFFFFFFFFFFFFFFF


def piece_bytes(dbg, piece_mb, nbytes):
    """:1008-1015.  piece_mb: what atol made of BNS_TEXT_PIECE_MB, 0 when it is not set, < 0 when it is set to no positive number"""
    piece = 64 << 20                                         # :1010
    if piece_mb > 0:
        piece = piece_mb << 20                               # :1011
    if dbg & DBG_SLICE_8K:
        piece = 8 << 10                                      # :1012
    least = ((nbytes + MAX_PIECES - 1) // MAX_PIECES + 63) & ~63      # :1013
    return max(piece, least)                                 # :1014


def up_to(st, k):
    """:1145-1148; st: a stream of plan()'s result"""
    return st["end"] if k + 1 >= st["n"] else u32(min(st["end"], (st["j0"] + k + 1) * st["piece"]))


def plan(sizes, rel=(0, 0), upload_piece=(0, 0), on_device=False, parse_only=False, want_runs=False, want_lines=False, want_words=False,
         dbg=0, piece_mb=0, batch_reads=0):
    """-> (code, fields or None, message).  want_runs: run_start given and not parse_only (:1206); want_words: words or nmask given (:1159)"""
    ns = len(sizes)
    src = []
    for s in range(ns):
        q = {"rel": rel[s], "end": u32(rel[s] + u32(sizes[s]))}                            # :1121-1122 / :1139
        if on_device:
            pieces_forced = bool(dbg & DBG_SLICE_8K) or piece_mb != 0                      # :1127 (getenv: set at all)
            big = 128 << 20                                                                # :1128
            q["piece"] = piece_bytes(dbg, piece_mb, sizes[s]) if pieces_forced else (big if q["end"] > big else max(64, (q["end"] + 63) & ~63))   # :1129
        else:
            q["piece"] = upload_piece[s]                                                   # :1139
        q["j0"] = u32(q["rel"] // q["piece"])                                              # :1141
        q["n"] = u32(u32((q["end"] - 1) // q["piece"]) - q["j0"] + 1) if q["end"] > q["rel"] else 1     # :1142
        src.append(q)
    n_slices = max(src[0]["n"], src[1]["n"] if ns == 2 else 1)                             # :1144
    if want_words and n_slices > 1:
        return ERR_ARG, None, MSG_WORDS                                                    # :1159
    range_cap = call_text = 0                                                              # :1161
    for s in range(ns):
        range_cap = max(range_cap, sizes[s] if n_slices == 1 else 2 * src[s]["piece"] + 64)   # :1162
        call_text += sizes[s]
    cap_lines = u32(range_cap // 8 + 1024)                                                 # :1163
    cap_rec = u32(range_cap // 16 + 512)                                                   # :1164
    b_reads = 2 << 20                                                                      # :1171
    if batch_reads > 0:
        b_reads = batch_reads                                                              # :1172
    if dbg & DBG_BATCH_TINY:
        b_reads = 64                                                                       # :1173
    b_bases, b_names = 320 << 20, 64 << 20                                                 # :1174
    slice_reads_cap, slice_bases_cap = cap_rec * ns, range_cap * ns                        # :1175
    sized_for = 64 << 20                                                                   # :1179
    while sized_for < call_text:
        sized_for <<= 1                                                                    # :1180
    carry_reads = 0 if n_slices == 1 else min(b_reads, sized_for // 64 + 64)               # :1181
    carry_bases = 0 if n_slices == 1 else min(b_bases, sized_for)                          # :1182
    carry_names = 0 if n_slices == 1 else min(b_names, sized_for)                          # :1183
    cap_reads, cap_bases, cap_names = slice_reads_cap + carry_reads, slice_bases_cap + carry_bases, slice_bases_cap + carry_names   # :1184
    if cap_reads >= 1 << 31 or cap_bases >= (1 << 32) - (1 << 20):
        return ERR_ARG, None, MSG_LARGE                                                    # :1185
    st_tiles, st_cand, st_recs = range_cap // TILE + 8, cap_rec // REC_BLOCK + 2, slice_reads_cap // REC_BLOCK + 2   # :1193
    st_groups = st_tiles // 64 + 2                                                         # :1194
    head = (SIZEOF_CALL_INFO + 63) & ~63
    info_bytes = head + (2 * st_tiles + 2 * st_groups + 2 * st_cand + st_recs) * 8         # :1195
    window = u32(min(u64(range_cap - 64), 0x7FFFFFFF))                                     # :1251 (read when n_slices > 1 only: :1263)
    p = {"pieces_forced": int(bool(dbg & DBG_SLICE_8K) or piece_mb != 0),                  # :1127
         "n_slices": n_slices, "range_cap": range_cap, "window": window, "cap_lines": cap_lines, "cap_rec": cap_rec,
         "batch_reads": b_reads, "batch_bases": b_bases, "batch_names": b_names,
         "slice_reads_cap": slice_reads_cap, "slice_bases_cap": slice_bases_cap,
         "carry_reads": carry_reads, "carry_bases": carry_bases, "carry_names": carry_names,
         "cap_reads": cap_reads, "cap_bases": cap_bases, "cap_names": cap_names,
         "st_tiles": st_tiles, "st_groups": st_groups, "st_cand": st_cand, "st_recs": st_recs, "info_bytes": info_bytes,
         # where the kernels' look-back words start, in bytes from the info buffer: :1272 (st_words), :1284, :1287
         "off_lines": head, "off_groups": head + 2 * st_tiles * 8, "off_compact": head + (2 * st_tiles + 2 * st_groups) * 8,
         "off_offsets": head + (2 * st_tiles + 2 * st_groups + 2 * st_cand) * 8}
    for s in range(2):
        for f in ("rel", "end", "j0", "n", "piece"):
            p["s%d_%s" % (s, f)] = src[s][f] if s < ns else {"n": 1}.get(f, 0)             # :1116 (a Src nobody fills)
    # ---- what the ensure() lines ask for; 0: no such line runs in this call
    e = {}
    for s in range(2):
        e["ls%d" % s] = e["line_off%d" % s] = cap_lines * 4 + 64 if s < ns else 0          # :1187-1188
        e["cand%d" % s] = cap_rec * 4 + 64 if s < ns else 0                                # :1189
    e["seq_len"], e["name_off"], e["pos64"], e["names"] = cap_reads * 4 + 64, (cap_reads + 1) * 4, cap_reads * 8, cap_names + 64    # :1197-1200
    e["offsets"] = (cap_reads + 1) * 8                                                     # :1202
    e["words"], e["nmask"] = (cap_bases // 32 + cap_reads + 2) * 8, (cap_bases // 32 + cap_reads + 2) * 4   # :1203-1204
    e["info"] = info_bytes                                                                 # :1205
    classify = not parse_only                                                              # :1207
    e["out"] = cap_reads * 4 + 64 if classify else 0                                       # :1208
    e["lines_off"] = (cap_reads + 1) * 8 + 64 if classify and want_lines else 0            # :1210
    e["lines_state"] = (cap_reads // 256 + 4) * 8 if classify and want_lines else 0        # :1211
    runs = classify and (want_runs or want_lines)                                          # :1213
    e["hits"] = cap_bases * 4 + 64 if runs else 0                                          # :1214
    e["runs0"], e["runs1"] = (cap_reads * 8 + 64, cap_reads * 4 + 64) if runs else (0, 0)  # :1216-1217
    e["runs2"] = e["runs3"] = cap_bases * 4 + 64 if runs else 0                            # :1218-1219
    for k, v in e.items():
        p["bytes_" + k] = v
    return OK, p, ""
