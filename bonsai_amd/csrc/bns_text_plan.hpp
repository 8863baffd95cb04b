// bns_text_plan.hpp -- what a bns_classify_text call DECIDES before its first launch: where each stream's text lies in its buffer and
// in how many slices it arrives, how much one parse may cover, when the open batch is classified and how much it may carry, the
// look-back words behind the CallInfo, and the byte size of every workspace buffer.  Plain arithmetic on a handful of numbers; the
// uploads, launches and copies that act on the answers are the host half of bns_ingest.hip.  Nothing here needs HIP and nothing
// here reads the environment (tests/test_text_plan.py compiles this header on its own and holds it against the rule restated in
// tests/text_plan_model.py); the constants and the two plain structs the decisions share with the kernels live here.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "bns_table_plan.hpp"     // u32, u64, the BNS_* codes

namespace bns {

// bns_debug_set bits a text call reads (tests; 0 in production; the other bits: bns_api.hip, bns_table_plan.hpp, bns_classify_plan.hpp)
constexpr int BNS_DBG_BATCH_TINY = 0x40;            // bns_classify_text: a classify launch per >= 64 records (many batches on small texts)
constexpr int BNS_DBG_SLICE_8K = 0x4000;            // bns_classify_batch and bns_classify_text upload in 8 KiB slices (the slicing logic on small inputs)

constexpr u32 TILE = 16384;                     // text bytes per pass of a 256-thread block (64 per lane)
constexpr u32 REC_BLOCK = 2048;                 // candidates / records per scan block (256 threads x REC_ITEMS, bns_ingest.hip)
constexpr u32 MAX_PIECES = 64;                  // pieces (and events) of one upload

// ---- what a parse reports (device words, zeroed in front of every parse together with the look-back words behind them)
struct StreamInfo {
    u32 n_nl, n_lines, n_cand, n_hdr;           // n_cand: lines that start with '>' / '@'; n_hdr: those that are headers
    u32 n_take, consumed, why, lo;
    u32 hi, n_eff, n_real, any_inside;          // n_eff: headers that yield a record (a final text that ends in a bare '>' / '@' byte: that one does not)
    u32 why_all, pad[3];                        // n_real: lines that may be looked at (not the unfinished last line of a text that goes on; not the nothing behind a final '\n')
};                                              // any_inside: a walk found candidates inside its record; why_all: what the walks found wrong, all candidates
struct CallInfo {
    StreamInfo s[2];
    u32 n_take;                                 // records per stream this call takes
    u32 n_reads;                                // n_take * n_streams
    u32 max_len, why;
    u32 total_bases, names_bytes;
    u32 ticket[6];                              // block tickets: lines_kernel [0..1], compact_kernel [2..3], offsets_kernel [4]; [5]: compact blocks that are done
    u32 fast, pad;                              // every candidate of either stream is a header: record r is candidate r
};
static_assert(sizeof(CallInfo) == 184, "the look-back words start behind it, at the next multiple of 64");
constexpr size_t CALL_INFO_BYTES = (sizeof(CallInfo) + 63) & ~size_t(63);

// ---- in
struct TextPlanIn {
    u32 ns = 1;                                 // streams: one file, or a pair
    u64 bytes[2] = {0, 0};                      // text of the call, per stream: below 2^31 each (the call's first refusal)
    u32 rel[2] = {0, 0};                        // where it starts in its buffer: device text, the pointer's low six bits; host text, the offset inside the upload
    u64 upload_piece[2] = {0, 0};               // host text: the piece size of the upload it lies in
    bool on_device = false, parse_only = false, want_runs = false, want_lines = false, want_words = false;   // want_words: the packed words or their flag words
    int dbg = 0;                                // the context's debug bits
    long long piece_mb = 0;                     // BNS_TEXT_PIECE_MB (measurements): 0 not set; < 0 set to no positive number (pieces still forced, of the usual size)
    long long batch_reads = 0;                  // BNS_TEXT_BATCH_READS (measurements): <= 0 not set
};

// ---- out
// Everything works in the coordinates of the stream's buffer -- whose base is aligned -- and the call's own offsets come back as
// buffer offset - rel.  Piece j0 + k of the buffer ends slice k: it is parsed -- together with what the pieces in front of it left
// unfinished, which simply lies in front of it in the same buffer -- and classified while k + 1 ... travel.
struct TextStream { u32 rel = 0, end = 0, j0 = 0, n = 1; u64 piece = 0; };
// bytes of every workspace buffer of the call (0: this call does not use the buffer)
struct TextBytes {
    size_t ls[2] = {0, 0}, line_off[2] = {0, 0}, cand[2] = {0, 0};     // per stream; cand: each of the ten per-candidate arrays
    size_t seq_len = 0, name_off = 0, pos64 = 0, names = 0;            // each of the two sets of result arrays
    size_t offsets = 0, words = 0, nmask = 0, info = 0;
    size_t out = 0;                                                    // each of the four unit arrays of either set
    size_t lines_off = 0, lines_state = 0;                             // (the line bytes themselves: sized batch by batch, text_flush_batch)
    size_t hits = 0, runs[4] = {0, 0, 0, 0};                           // runs[i]: either set
};
struct TextPlan {
    u32 ns = 1;
    TextStream s[2];
    u32 n_slices = 1;
    bool pieces_forced = false;                 // device text: cut into pieces although it is all there (BNS_DBG_SLICE_8K, BNS_TEXT_PIECE_MB)
    u64 range_cap = 0;                          // the largest stretch one parse may cover
    u32 window = 0, cap_lines = 0, cap_rec = 0;
    u64 batch_reads = 0, batch_bases = 0, batch_names = 0;             // the open batch is classified when it holds that much
    u64 slice_reads_cap = 0, slice_bases_cap = 0;                      // one slice's worst case
    u64 carry_reads = 0, carry_bases = 0, carry_names = 0;             // what a batch may hold when one more slice is packed behind it
    u64 cap_reads = 0, cap_bases = 0, cap_names = 0;                   // slice + carry: what the packed image is sized for
    size_t st_tiles = 0, st_groups = 0, st_cand = 0, st_recs = 0;      // look-back words: per stream (tiles, groups, cand) and of the call (recs)
    size_t off_lines = 0, off_groups = 0, off_compact = 0, off_offsets = 0, info_bytes = 0;   // bytes into the info buffer; the CallInfo is at 0
    TextBytes bytes;

    // where stream s's text ends after slice k (buffer coordinates)
    u32 up_to(u32 st, u32 k) const
    {
        const TextStream &q = s[st];
        return k + 1 >= q.n ? q.end : (u32)std::min<u64>(q.end, (u64)(q.j0 + k + 1) * q.piece);     // (the minimum is at most end: u32)
    }
    // the piece of the upload that ends slice k -- and with it every piece in front of it: the copy stream is in order
    u32 piece_of(u32 st, u32 k) const { return std::min(s[st].j0 + k, s[st].j0 + s[st].n - 1); }
};

// ---- the rules
// the piece size of an upload of `bytes`: 64 MiB, at most MAX_PIECES of them
inline size_t text_piece_bytes(int dbg, long long piece_mb, u64 bytes)
{
    size_t piece = (size_t)64 << 20;
    if (piece_mb > 0) piece = (size_t)piece_mb << 20;
    if (dbg & BNS_DBG_SLICE_8K) piece = (size_t)8 << 10;
    const u64 least = ((bytes + MAX_PIECES - 1) / MAX_PIECES + 63) & ~63ULL;
    return (size_t)std::max<u64>(piece, least);
}

// the tiles of a stretch [lo, hi) of a buffer
constexpr u32 tile0(u32 lo) { return lo / TILE; }
constexpr u32 n_tiles(u32 lo, u32 hi) { return hi > lo ? (hi - 1) / TILE - tile0(lo) + 1 : 1; }

// Every narrowing to u32 below rests on the call's first refusal: bytes[s] <= 2^31 - 1.  rel is below 64 (device text) or an offset
// into an upload that holds rel + bytes[s] bytes and was refused beyond 2^31 - 1 itself, so end = rel + bytes[s] < 2^31 + 64.
inline int plan_text(const TextPlanIn &in, TextPlan &p, const char *&msg)
{
    p = TextPlan{};
    const u32 ns = p.ns = in.ns;
    p.pieces_forced = (in.dbg & BNS_DBG_SLICE_8K) || in.piece_mb != 0;
    u64 call_text = 0;
    for (u32 s = 0; s < ns; ++s) {
        TextStream &q = p.s[s];
        q.rel = in.rel[s];
        q.end = q.rel + (u32)in.bytes[s];                   // (< 2^31 + 64)
        if (in.on_device) {
            // text that is all there already is ONE slice (nothing travels that a second slice's parse could hide), unless pieces are asked for
            // -- or the text is large: a slice's workspaces are sized by its bytes (4.6 bytes per byte of text), and a call of 1.35 GB -- what one
            // call on a gzip stream inflates -- allocated 6 GB of them, again whenever a call was a little larger than every one before it (a
            // hipFree each, the device drained each time: one call in eight took 4 s).  Slices of 128 MiB beyond that: the same 1.2 GB for every call
            const u64 big_piece = 128ull << 20;
            q.piece = p.pieces_forced ? text_piece_bytes(in.dbg, in.piece_mb, in.bytes[s]) : (q.end > big_piece ? big_piece : std::max<u64>(64, ((u64)q.end + 63) & ~63ULL));
        } else {
            q.piece = in.upload_piece[s];
        }
        q.j0 = (u32)(q.rel / q.piece);                      // (<= rel)
        q.n = q.end > q.rel ? (u32)((q.end - 1) / q.piece) - q.j0 + 1 : 1;
        call_text += in.bytes[s];
    }
    p.n_slices = std::max(p.s[0].n, ns == 2 ? p.s[1].n : 1u);
    if (in.want_words && p.n_slices > 1) { msg = "the packed words come back for one-slice calls only (<= 64 MiB of text)"; return BNS_ERR_ARG; }
    // the largest stretch one parse may cover: two slices' worth (a record longer than a slice is the host parser's)
    for (u32 s = 0; s < ns; ++s) p.range_cap = std::max<u64>(p.range_cap, p.n_slices == 1 ? in.bytes[s] : 2 * p.s[s].piece + 64);
    // (one slice: range_cap < 2^31.  Several: a piece is shorter than its text, 2 * piece + 64 < 2^32 + 192 -- an eighth of it fits easily)
    p.cap_lines = (u32)(p.range_cap / 8 + 1024);            // (more lines than one per 8 bytes: BNS_TEXT_WHY_LINES)
    p.cap_rec = (u32)(p.range_cap / 16 + 512);              // (more records than one per 16 bytes: BNS_TEXT_WHY_LINES as well)
    // what one parse covers of a stream when there are several slices (of a pair of files the denser one is ahead of what its mate
    // lets it hand over: its unparsed text waits, it does not grow the window); a one-slice call does not read it
    p.window = (u32)std::min<u64>(p.range_cap - 64, 0x7FFFFFFFu);
    // ---- batches.  A slice is what one parse covers (one upload piece and what the pieces in front left unfinished); a BATCH is what one
    // classify launch covers: the records of consecutive slices, appended to ONE packed image (offsets, words, flag words, the result
    // rows of the batch's set) until it holds `batch_reads` records (or batch_bases / batch_names), or the call ends.  The fused kernel
    // at 210 k records a launch -- one 64 MiB slice -- ran at a fifth of its rate (26 records per wavefront slot: launch, the first
    // fetches of a cold table and the tail are most of the 430 us); classifier.h:307-318 hands classify_seqs its batch whole, too.
    // Capacities are "what a batch may hold when it is flushed" + one slice's worst case: a slice is packed before its counts are known.
    p.batch_reads = 2u << 20;
    if (in.batch_reads > 0) p.batch_reads = (u64)in.batch_reads;
    if (in.dbg & BNS_DBG_BATCH_TINY) p.batch_reads = 64;    // (tests: many batches on small texts)
    p.batch_bases = 320u << 20; p.batch_names = 64u << 20;
    p.slice_reads_cap = (u64)p.cap_rec * ns; p.slice_bases_cap = p.range_cap * ns;
    // (by the call's text rounded UP to a power of two: the calls of one input differ by a few per cent -- batches of a BGZF file, the first
    // and the later calls of a gzip stream -- and a workspace that grows by a hair is freed and allocated again, every one of them, a hipFree
    // each: with another thread's kernels queueing up all the while one such call was seen to take 4 s instead of 20 ms)
    u64 sized_for = 64u << 20;
    while (sized_for < call_text) sized_for <<= 1;
    const bool one = p.n_slices == 1;
    p.carry_reads = one ? 0 : std::min<u64>(p.batch_reads, sized_for / 64 + 64);
    p.carry_bases = one ? 0 : std::min<u64>(p.batch_bases, sized_for);
    p.carry_names = one ? 0 : std::min<u64>(p.batch_names, sized_for);
    p.cap_reads = p.slice_reads_cap + p.carry_reads; p.cap_bases = p.slice_bases_cap + p.carry_bases; p.cap_names = p.slice_bases_cap + p.carry_names;
    if (p.cap_reads >= (1ULL << 31) || p.cap_bases >= (1ULL << 32) - (1ULL << 20)) { msg = "text too large for one batch"; return BNS_ERR_ARG; }
    // CallInfo and, behind it, the look-back words of the slice's scans (tiles of either stream, groups of 64 tiles of either stream,
    // candidate blocks of either stream, record blocks): zeroed together in front of every parse
    p.st_tiles = (size_t)(p.range_cap / TILE + 8); p.st_cand = (size_t)p.cap_rec / REC_BLOCK + 2; p.st_recs = (size_t)p.slice_reads_cap / REC_BLOCK + 2;
    p.st_groups = p.st_tiles / 64 + 2;
    p.off_lines = CALL_INFO_BYTES;
    p.off_groups = p.off_lines + 2 * p.st_tiles * 8;
    p.off_compact = p.off_groups + 2 * p.st_groups * 8;
    p.off_offsets = p.off_compact + 2 * p.st_cand * 8;
    p.info_bytes = p.off_offsets + p.st_recs * 8;
    // ---- the workspace
    TextBytes &b = p.bytes;
    const size_t cap_reads = (size_t)p.cap_reads, cap_bases = (size_t)p.cap_bases;
    for (u32 s = 0; s < ns; ++s) { b.ls[s] = b.line_off[s] = (size_t)p.cap_lines * 4 + 64; b.cand[s] = (size_t)p.cap_rec * 4 + 64; }
    b.seq_len = cap_reads * 4 + 64; b.name_off = (cap_reads + 1) * 4; b.pos64 = cap_reads * 8; b.names = (size_t)p.cap_names + 64;
    b.offsets = (cap_reads + 1) * 8;
    b.words = (cap_bases / 32 + cap_reads + 2) * 8; b.nmask = (cap_bases / 32 + cap_reads + 2) * 4;
    b.info = p.info_bytes;
    if (!in.parse_only) {
        b.out = cap_reads * 4 + 64;
        if (in.want_lines) { b.lines_off = (cap_reads + 1) * 8 + 64; b.lines_state = (cap_reads / 256 + 4) * 8; }
        if (in.want_runs || in.want_lines) {
            b.hits = cap_bases * 4 + 64;
            b.runs[0] = cap_reads * 8 + 64; b.runs[1] = cap_reads * 4 + 64; b.runs[2] = b.runs[3] = cap_bases * 4 + 64;
        }
    }
    return BNS_OK;
}

}  // namespace bns
