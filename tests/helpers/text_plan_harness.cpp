// Host harness for tests/test_text_plan.py: bonsai_amd/csrc/bns_text_plan.hpp compiled on its own (it needs no HIP), its
// functions as bns_classify_text (bns_ingest.hip) calls them.
#include <cstdint>
#include <cstring>
#include "../../bonsai_amd/csrc/bns_text_plan.hpp"

using namespace bns;

extern "C" {

// [0] TILE, [1] REC_BLOCK, [2] MAX_PIECES, [3] sizeof(CallInfo), [4] CALL_INFO_BYTES, [5] sizeof(StreamInfo), [6] BNS_DBG_SLICE_8K, [7] BNS_DBG_BATCH_TINY
void text_constants(uint64_t *out8)
{
    const uint64_t v[8] = {TILE, REC_BLOCK, MAX_PIECES, sizeof(CallInfo), CALL_INFO_BYTES, sizeof(StreamInfo), (uint64_t)BNS_DBG_SLICE_8K, (uint64_t)BNS_DBG_BATCH_TINY};
    std::memcpy(out8, v, sizeof(v));
}

uint64_t text_piece(int dbg, long long piece_mb, uint64_t bytes) { return text_piece_bytes(dbg, piece_mb, bytes); }
uint32_t text_tile0(uint32_t lo) { return tile0(lo); }
uint32_t text_n_tiles(uint32_t lo, uint32_t hi) { return n_tiles(lo, hi); }

// in15: ns, bytes[2], rel[2], upload_piece[2], on_device, parse_only, want_runs, want_lines, want_words, dbg, piece_mb, batch_reads
// out58: the plan's fields in the order of FIELDS in tests/text_plan_lib.py.  Returns the BNS_ERR_* code; msg (up to 127 characters)
// is written as plan_text leaves it.
int text_plan(const int64_t *in15, uint64_t *out58, char *msg128)
{
    TextPlanIn in;
    in.ns = (u32)in15[0];
    for (int s = 0; s < 2; ++s) { in.bytes[s] = (u64)in15[1 + s]; in.rel[s] = (u32)in15[3 + s]; in.upload_piece[s] = (u64)in15[5 + s]; }
    in.on_device = in15[7] != 0; in.parse_only = in15[8] != 0; in.want_runs = in15[9] != 0; in.want_lines = in15[10] != 0; in.want_words = in15[11] != 0;
    in.dbg = (int)in15[12]; in.piece_mb = in15[13]; in.batch_reads = in15[14];
    TextPlan p;
    const char *msg = "";
    const int rc = plan_text(in, p, msg);
    std::strncpy(msg128, msg, 127); msg128[127] = 0;
    uint64_t *o = out58;
    for (int s = 0; s < 2; ++s) { *o++ = p.s[s].rel; *o++ = p.s[s].end; *o++ = p.s[s].j0; *o++ = p.s[s].n; *o++ = p.s[s].piece; }
    *o++ = p.n_slices; *o++ = p.pieces_forced; *o++ = p.range_cap; *o++ = p.window; *o++ = p.cap_lines; *o++ = p.cap_rec;
    *o++ = p.batch_reads; *o++ = p.batch_bases; *o++ = p.batch_names;
    *o++ = p.slice_reads_cap; *o++ = p.slice_bases_cap;
    *o++ = p.carry_reads; *o++ = p.carry_bases; *o++ = p.carry_names;
    *o++ = p.cap_reads; *o++ = p.cap_bases; *o++ = p.cap_names;
    *o++ = p.st_tiles; *o++ = p.st_groups; *o++ = p.st_cand; *o++ = p.st_recs;
    *o++ = p.off_lines; *o++ = p.off_groups; *o++ = p.off_compact; *o++ = p.off_offsets; *o++ = p.info_bytes;
    const TextBytes &b = p.bytes;
    for (int s = 0; s < 2; ++s) { *o++ = b.ls[s]; *o++ = b.line_off[s]; *o++ = b.cand[s]; }
    *o++ = b.seq_len; *o++ = b.name_off; *o++ = b.pos64; *o++ = b.names;
    *o++ = b.offsets; *o++ = b.words; *o++ = b.nmask; *o++ = b.info;
    *o++ = b.out; *o++ = b.lines_off; *o++ = b.lines_state; *o++ = b.hits;
    for (int i = 0; i < 4; ++i) *o++ = b.runs[i];
    return (o - out58 == 58) ? rc : -1000;
}

// TextPlan::up_to / piece_of for a stream with these numbers
uint32_t text_up_to(uint32_t rel, uint32_t end, uint32_t j0, uint32_t n, uint64_t piece, uint32_t k)
{
    TextPlan p;
    p.s[0] = TextStream{rel, end, j0, n, piece};
    return p.up_to(0, k);
}
uint32_t text_piece_of(uint32_t j0, uint32_t n, uint32_t k)
{
    TextPlan p;
    p.s[0].j0 = j0; p.s[0].n = n;
    return p.piece_of(0, k);
}

}
