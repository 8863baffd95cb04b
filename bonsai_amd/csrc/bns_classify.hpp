// bns_classify.hpp -- the classify path: the launches that act on what bns_classify_plan.hpp decides, one batch on the device
// (classify_device_impl), host batches uploaded in slices around it (classify_host_impl), and the bodies of the bns_classify_batch*
// and bns_pack_reads* entry points.  Which instantiation runs is decided in ONE place, choose_form / choose_overflow_form; launch_form
// and launch_overflow_form walk the plan's lists of forms and launch the entry whose key matches, so nothing here names a form.
// Included by bns_api.hip after its helpers (bns_ctx, ClassifyForm, SmallLayout, HIPCHK, fail, ensure, grid_for, ready) and in front of
// bns_build.hpp / bns_windows.hpp, which use fill_params, pack_reads and set_win_scratch.
#pragma once
#include <utility>

namespace {

int tally_units(bns_ctx *ctx, const u32 *d_taxon, u64 n_units, hipStream_t st, bool neg);                               // bns_api.hip
int sketch_units(bns_ctx *ctx, const ClassifyParams &p, hipStream_t st);                                                // bns_api.hip
int hit_groups_units(bns_ctx *ctx, const ClassifyParams &p, hipStream_t st);                                            // bns_api.hip
int dust_image_span(bns_ctx *ctx, const u64 *words, const u32 *nmask, const u64 *offsets, u64 n_seqs, u64 lo, u64 hi, hipStream_t st);   // bns_dust.hpp

void fill_params(const bns_ctx *ctx, ClassifyParams &p)
{
    std::memset(&p, 0, sizeof(p));
    p.words = (const u64 *)ctx->words.p;
    p.nmask = (const u32 *)ctx->nmask.p;
    p.slots = ctx->layout == BNS_LAYOUT_MINBUCKET ? ctx->ovf_slots : ctx->slots;
    p.ovf_mask = ctx->n_ovf_slots ? ctx->n_ovf_slots / 4 - 1 : 0;
    p.minb = reinterpret_cast<const MinBucket *>(ctx->slots);
    p.bucket_mask = (ctx->n_slots && ctx->layout == BNS_LAYOUT_BUCKET) ? ctx->n_slots / 4 - 1 : 0;
    p.n_mb = ctx->layout == BNS_LAYOUT_MINBUCKET ? ctx->n_mb : 0u;
    p.min_wide = ctx->table_wide ? 1u : 0u;
    p.kflags = ctx->kflags; p.kkeys = ctx->kkeys; p.kvals = ctx->kvals; p.kh_nb = ctx->kh_nb;
    p.nodes = ctx->nodes; p.n_nodes = ctx->n_nodes;
    p.k = ctx->k; p.c = ctx->c; p.canon = ctx->canon ? 1 : 0; p.dbg = ctx->dbg;
    std::memcpy(p.pos, ctx->pos, sizeof(p.pos));
    p.n_runs = ctx->n_runs; p.sample_mask = ctx->sample_mask; p.m = ctx->table_m ? ctx->table_m : ctx->k;
    p.min_len = ctx->table_m ? ctx->table_len : ctx->k; p.min_shift = ctx->table_m ? ctx->table_shift : 0; p.min_canon = ctx->table_m ? ctx->table_canon : 1;
    p.w = ctx->win > ctx->c ? ctx->win : ctx->c; p.score = ctx->score;
    if (ctx->score == BNS_SCORE_ENTROPY_STRING) {                        // CircusEnt::value() terms, entropy.h:46-47 (qszinv_ = 1./qsz)
        const double qi = 1. / (double)ctx->k;
        for (u32 n = 1; n <= ctx->k && n <= 32; ++n) p.ent_tbl[n] = (double)n * qi * std::log((double)n * qi);
    }
    std::memcpy(p.run_start, ctx->run_start, sizeof(p.run_start)); std::memcpy(p.run_len, ctx->run_len, sizeof(p.run_len));
    p.pext_on = (ctx->dbg & BNS_DBG_PEXT_OFF) ? 0 : ctx->pext_on; p.pext_n1 = ctx->pext_n1;
    std::memcpy(p.pext_steps, ctx->pext_steps, sizeof(p.pext_steps)); std::memcpy(p.pext_mask, ctx->pext_mask, sizeof(p.pext_mask));
    std::memcpy(p.pext_top, ctx->pext_top, sizeof(p.pext_top));
    std::memcpy(p.pext_mv, ctx->pext_mv, sizeof(p.pext_mv));
}

// pack ASCII reads (device) into ctx->words / ctx->nmask
int pack_reads(bns_ctx *ctx, const char *d_bases, const u64 *d_offsets, u64 n_reads, u64 total_bases, hipStream_t st)
{
    const size_t n_words = (size_t)(total_bases >> 5) + n_reads + 2;
    int rc;
    if ((rc = ensure(ctx, ctx->words, n_words * 8)) != BNS_OK) return rc;
    if ((rc = ensure(ctx, ctx->nmask, n_words * 4)) != BNS_OK) return rc;
    if (n_reads == 0) return BNS_OK;
    hipLaunchKernelGGL(pack_kernel, dim3(grid_for(ctx, n_reads, 4)), dim3(256), 0, st, (const u8 *)d_bases, d_offsets,
                       n_reads, (u64 *)ctx->words.p, (u32 *)ctx->nmask.p);
    HIPCHK(ctx, hipGetLastError());
    return BNS_OK;
}

// the queue image of windows over the emitted stream wider than 64 k-mers (win_scratch_bytes)
int set_win_scratch(bns_ctx *ctx, ClassifyParams &p, unsigned grid)
{
    p.win_scratch = nullptr;
    const size_t bytes = win_scratch_bytes(ctx->spaced, ctx->canon, ctx->score, ctx->win, ctx->c, grid);
    if (!bytes) return BNS_OK;
    const int rc = ensure(ctx, ctx->scratch, bytes);
    if (rc != BNS_OK) return rc;
    p.win_scratch = (u64 *)ctx->scratch.p;
    return BNS_OK;
}

// ---- the launches ------------------------------------------------------------------------------------------------------------
// Every classify_kernel / classify_overflow_kernel launch goes through these two: the instantiation launched and the one
// recorded in the form are the same template arguments.
// max_blocks: the workgroups that are resident at once (or fewer: bns_debug_set_claim_waves).  Units per claim: the full chunk when
// that leaves every one of their wavefronts at least one, else an even share (>= 4: a claim is an offsets load); the grid and
// the start of the dynamic claims follow from it (bns_claims.hpp).
template <bool SP, int LY, int KT, int NM, int SPAN, bool OVC, bool WIDE, bool PACKED>
void launch_classify(ClassifyForm &f, const ClassifyParams &p0, unsigned max_blocks, hipStream_t st)
{
    ClassifyParams p = p0;
    u32 grid;
    const u32 full = classify_chunk((u32)p.nmates);
    claim_geometry(p.n_units, max_blocks, full, p.chunk, grid);
    p.claim_base = claim_dynamic_start(p.n_units, grid * 4u, p.chunk, full);
    if (p.chunk < full) p.work_counter = nullptr;          // dealt out by the static claims alone: the kernel asks no counter
    f = ClassifyForm{};
    f.w[ClassifyForm::VALID] = 1; f.w[ClassifyForm::SPACED] = SP; f.w[ClassifyForm::LAYOUT] = LY; f.w[ClassifyForm::KT] = KT;
    f.w[ClassifyForm::NM] = NM; f.w[ClassifyForm::SPAN] = SPAN; f.w[ClassifyForm::OVC] = OVC; f.w[ClassifyForm::WIDE] = WIDE;
    f.w[ClassifyForm::PACKED] = PACKED; f.w[ClassifyForm::CHUNK] = p.chunk; f.w[ClassifyForm::GRID] = grid;
    hipLaunchKernelGGL((classify_kernel<SP, LY, KT, NM, SPAN, OVC, WIDE, PACKED>), dim3(grid), dim3(256), 0, st, p);
}
template <bool SP, int LY, bool WIDE, bool PACKED>
void launch_classify_overflow(ClassifyForm &f, const ClassifyParams &p, u32 n_units, unsigned grid, hipStream_t st, u32 *scratch, u64 total_bases)
{
    f.w[ClassifyForm::OVF_LAUNCHED] = 1; f.w[ClassifyForm::OVF_SPACED] = SP; f.w[ClassifyForm::OVF_LAYOUT] = LY;
    f.w[ClassifyForm::OVF_WIDE] = WIDE; f.w[ClassifyForm::OVF_PACKED] = PACKED; f.w[ClassifyForm::OVF_UNITS] = n_units;
    f.w[ClassifyForm::OVF_GRID] = grid;
    hipLaunchKernelGGL((classify_overflow_kernel<SP, LY, WIDE, PACKED>), dim3(grid), dim3(64), 0, st, p, scratch, total_bases);
}

// f(std::integral_constant<size_t, I>) for the entry I of `forms` that equals `key`; false when there is none (it cannot happen:
// tests/test_classify_plan.py finds every key the rule returns on the list)
template <class Forms, class Key, class F, size_t... I>
bool with_form(const Forms &forms, const Key &key, F &&f, std::index_sequence<I...>)
{
    return ((forms[I] == key ? (f(std::integral_constant<size_t, I>{}), true) : false) || ...);
}

// The generic narrow forms alone ask the runtime how many of their blocks a CU holds and cap the grid by it (at most 8 per CU); the
// fixed-k forms and the generic wide ones take the grid as it comes.
int launch_form(bns_ctx *ctx, const ClassifyFormKey &key, const ClassifyParams &p, unsigned grid, hipStream_t st)
{
    const bool found = with_form(CLASSIFY_FORMS, key, [&](auto i) {
        constexpr ClassifyFormKey K = CLASSIFY_FORMS[decltype(i)::value];
        unsigned g = grid;
        if constexpr (K.kt == 0 && !K.wide) {
            int per_cu = 8;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, classify_kernel<K.spaced, K.layout, K.kt, K.nm, K.span, K.ovc, K.wide, K.packed>, 256, 0) != hipSuccess || per_cu < 1) per_cu = 8;
            g = std::min<unsigned>(grid, (unsigned)ctx->n_cu * (unsigned)std::min(per_cu, 8));
        }
        launch_classify<K.spaced, K.layout, K.kt, K.nm, K.span, K.ovc, K.wide, K.packed>(ctx->last_form, p, g, st);
    }, std::make_index_sequence<CLASSIFY_FORMS.size()>{});
    return found ? BNS_OK : fail(ctx, BNS_ERR_STATE, "classify: the form chosen for this call is not among the compiled ones");
}
int launch_overflow_form(bns_ctx *ctx, const OverflowFormKey &key, const ClassifyParams &p, u32 n_units, unsigned grid, hipStream_t st, u32 *scratch,
                         u64 total_bases)
{
    const bool found = with_form(OVERFLOW_FORMS, key, [&](auto i) {
        constexpr OverflowFormKey K = OVERFLOW_FORMS[decltype(i)::value];
        launch_classify_overflow<K.spaced, K.layout, K.wide, K.packed>(ctx->last_form, p, n_units, grid, st, scratch, total_bases);
    }, std::make_index_sequence<OVERFLOW_FORMS.size()>{});
    return found ? BNS_OK : fail(ctx, BNS_ERR_STATE, "classify: the overflow form chosen for this call is not among the compiled ones");
}


// ---- one batch, inputs resident ----------------------------------------------------------------------------------------------
// ASCII (bases) or packed (words [+ nmask]): exactly one of bases / words is set.  max_read_len 0: found on the device.
struct ClassifyIn {
    const char *bases = nullptr; const u64 *words = nullptr; const u32 *nmask = nullptr;
    const u64 *offsets = nullptr; u64 n_reads = 0, total_bases = 0; u32 max_read_len = 0; int paired = 0;
    bool masked = false;                                 // packed input of ours that bns_set_dust's pass has been over already (the text path)
    u64 first_base = 0, end_base = 0;                    // the bases the offsets span, where the caller knows (a slice of a host batch); 0, 0: 0 .. total_bases
};
// The per-unit result arrays (device or host), and the hit stream; taxon is always there, the others where the caller wants them.
struct UnitOut { u32 *taxon = nullptr, *missing = nullptr, *ambig = nullptr, *n_hits = nullptr, *hits = nullptr; };

// what the steps of one launch hand on
struct ClassifyLaunch {
    hipStream_t st = nullptr; int nm = 1; u64 n_units = 0; bool packed = false, can_overflow = false;
    ClassifyParams p;
};

int classify_check(bns_ctx *ctx, const ClassifyIn &in, const UnitOut &out)
{
    BNS_RC(ready(ctx, true, true));
    if (!in.offsets || !out.taxon || (!in.bases && !in.words && in.total_bases)) return BNS_ERR_ARG;
    if (in.paired && (in.n_reads & 1)) return fail(ctx, BNS_ERR_ARG, "paired input needs an even number of reads");
    return BNS_OK;
}

// the launch's words of ctx->small zeroed, the longest read (read back when the caller does not know it), workspace, parameters
int classify_prepare(bns_ctx *ctx, const ClassifyIn &in, const UnitOut &out, ClassifyLaunch &L)
{
    hipStream_t st = L.st;
    SmallLayout *sm = (SmallLayout *)ctx->small.p;
    HIPCHK(ctx, hipMemsetAsync(sm, 0, SMALL_CLASSIFY_ZERO, st));   // the eight work counters, ovf_count, max_len in one memset
    u32 max_read_len = in.max_read_len;
    if (max_read_len == 0) {
        hipLaunchKernelGGL(max_len_kernel, dim3(grid_for(ctx, in.n_reads, 256)), dim3(256), 0, st, in.offsets, (u64)in.n_reads, &sm->max_len);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(&max_read_len, &sm->max_len, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    L.can_overflow = unit_can_overflow(L.nm, max_read_len, ctx->c);
    if (L.can_overflow) BNS_RC(ensure(ctx, ctx->ovf_list, (size_t)L.n_units * 8));

    ClassifyParams &p = L.p;
    fill_params(ctx, p);
    p.offsets = in.offsets; p.n_units = L.n_units; p.nmates = L.nm; p.bases = (const u8 *)in.bases;
    if (L.packed) { p.words = in.words; p.nmask = in.nmask; }
    p.taxon = out.taxon; p.missing = out.missing; p.ambig = out.ambig; p.n_hits = out.n_hits; p.hits = out.hits;
    if ((ctx->conf_num || ctx->sketch_cap) && !out.hits) {   // the confidence and sketch passes read the hit stream: into a buffer of ours when the caller takes none
        BNS_RC(ensure(ctx, ctx->conf_hits, (size_t)in.total_bases * 4 + 4));
        p.hits = (u32 *)ctx->conf_hits.p;
    }
    p.want_hits = p.hits ? 1 : 0;
    BNS_RC(ensure(ctx, ctx->records, (size_t)L.n_units * 16));
    p.records = (uint4 *)ctx->records.p;
    p.ovf_count = &sm->ovf_count; p.ovf_list = L.can_overflow ? (u64 *)ctx->ovf_list.p : nullptr;
    p.work_counter = &sm->work_counter[0][0];
    // reference behaviour for a spaced seed through the string for_each: nothing is emitted
    p.emit_none = (ctx->spaced && !ctx->spaced_intended) ? 1 : 0;
    return BNS_OK;
}

// classify_kernel in the form the plan chooses, between the timing events
int classify_launch(bns_ctx *ctx, const ClassifyLaunch &L)
{
    hipStream_t st = L.st;
    // persistent grid: at most the workgroups that are resident at once, 8 of 4 wavefronts per CU (launch_classify sizes the claims by it)
    unsigned grid = (unsigned)ctx->n_cu * 8u;
    if (ctx->claim_waves) grid = std::max(1u, std::min(grid, ctx->claim_waves / 4u));
    const int evi = ctx->ev_head;
    if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev0[evi], st));
    const bool heavy = ovf_heavy(ctx->dbg, ctx->n_ovf_keys, ctx->n_keys);
    BNS_RC(launch_form(ctx, choose_form(L.p.k, L.p.m, ctx->canon, ctx->spaced, ctx->layout, ctx->table_wide, heavy, L.packed, L.nm), L.p, grid, st));
    HIPCHK(ctx, hipGetLastError());
    if (ctx->timing) {
        HIPCHK(ctx, hipEventRecord(ctx->ev1[evi], st));
        ctx->ev_head = (evi + 1) % bns_ctx::EV_RING;
        ctx->ev_count = std::min(ctx->ev_count + 1, (int)bns_ctx::EV_RING);
    }
    return BNS_OK;
}

// the units classify_kernel listed (more than LDS_CAP distinct taxa): their count read back, classify_overflow_kernel over them
int classify_overflow_pass(bns_ctx *ctx, const ClassifyIn &in, const ClassifyLaunch &L)
{
    hipStream_t st = L.st;
    u32 h_ovf = 0;
    HIPCHK(ctx, hipMemcpyAsync(&h_ovf, L.p.ovf_count, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (!h_ovf) return BNS_OK;
    BNS_RC(ensure(ctx, ctx->scratch, (size_t)in.total_bases * 16));
    const unsigned grid = std::min<u32>(h_ovf, (u32)ctx->n_cu * 8);
    BNS_RC(launch_overflow_form(ctx, choose_overflow_form(ctx->spaced, ctx->layout, ctx->table_wide, L.packed), L.p, h_ovf, grid, st, (u32 *)ctx->scratch.p,
                                (u64)in.total_bases));
    HIPCHK(ctx, hipGetLastError());
    return BNS_OK;
}

// confidence walk, minimum hit groups, the records split into the caller's arrays, tally and sketches
int classify_finish(bns_ctx *ctx, const ClassifyIn &in, const UnitOut &out, const ClassifyLaunch &L)
{
    hipStream_t st = L.st;
    const u64 n_units = L.n_units;
    const bool hit_groups = ctx->min_hit_groups >= 2;    // (1 changes nothing: a taxon implies a hit)
    ClassifyParams p = L.p;
    if ((hit_groups || ctx->sketch_cap) && in.bases) {   // both passes walk the packed image: ASCII input is packed, once
        BNS_RC(pack_reads(ctx, in.bases, in.offsets, in.n_reads, in.total_bases, st));
        p.words = (const u64 *)ctx->words.p; p.nmask = (const u32 *)ctx->nmask.p;
    }
    if (ctx->conf_num) {                             // bns_set_confidence: the taxa of the records walked up to theta's clade
        hipLaunchKernelGGL(confidence_kernel, dim3(grid_for(ctx, (n_units + CONF_GROUP - 1) / CONF_GROUP, 4)), dim3(256), 0, st, (uint4 *)ctx->records.p,
                           (const u64 *)in.offsets, (u32)L.nm, (const u32 *)L.p.hits, (u64)n_units, (const TaxNode *)ctx->nodes, ctx->n_nodes, ctx->conf_num,
                           ctx->conf_den);
        HIPCHK(ctx, hipGetLastError());
    }
    if (hit_groups) BNS_RC(hit_groups_units(ctx, p, st));   // bns_set_min_hit_groups: taxon 0 below n distinct found keys
    hipLaunchKernelGGL(unpack_kernel, dim3(grid_for(ctx, n_units, 256)), dim3(256), 0, st, (const uint4 *)ctx->records.p, (u64)n_units,
                       out.taxon, out.missing, out.ambig, out.n_hits);
    HIPCHK(ctx, hipGetLastError());
    BNS_RC(tally_units(ctx, out.taxon, n_units, st, false));   // (every classifying entry point comes through here, once per unit)
    if (!ctx->sketch_cap) return BNS_OK;
    return sketch_units(ctx, p, st);
}

int classify_device_impl(bns_ctx *ctx, const ClassifyIn &in0, const UnitOut &out, void *stream)
{
    BNS_RC(classify_check(ctx, in0, out));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ClassifyIn in = in0;
    ClassifyLaunch L;
    L.st = stream ? (hipStream_t)stream : ctx->stream;
    L.nm = in.paired ? 2 : 1;
    L.n_units = in.n_reads / (u64)L.nm;
    if (L.n_units == 0) return BNS_OK;
    if (too_many_units(L.n_units)) return fail(ctx, BNS_ERR_ARG, "more than 2^32 - 2^22 units in one batch: split it");
    if (ctx->dust_w && !in.masked && (in.bases || in.words)) {
        // bns_set_dust: ASCII is packed first and masked where it lies; a caller's packed image is masked into a copy of ours.  From
        // here on the call is a packed one over ctx->words / ctx->nmask
        const u64 lo = in.end_base ? in.first_base : 0, hi = in.end_base ? in.end_base : in.total_bases;
        if (in.bases) {
            BNS_RC(pack_reads(ctx, in.bases, in.offsets, in.n_reads, in.total_bases, L.st));
            BNS_RC(dust_image_span(ctx, (const u64 *)ctx->words.p, (const u32 *)ctx->nmask.p, in.offsets, in.n_reads, lo, hi, L.st));
        } else BNS_RC(dust_image_span(ctx, in.words, in.nmask, in.offsets, in.n_reads, lo, hi, L.st));
        in.bases = nullptr; in.words = (const u64 *)ctx->words.p; in.nmask = (const u32 *)ctx->nmask.p;
    }
    L.packed = in.words != nullptr;
    BNS_RC(classify_prepare(ctx, in, out, L));
    BNS_RC(classify_launch(ctx, L));
    if (L.can_overflow) BNS_RC(classify_overflow_pass(ctx, in, L));
    return classify_finish(ctx, in, out, L);
}

// ---- packed reads on the host side -------------------------------------------------------------------------------------------
// 32 ASCII bases -> one image word (2-bit codes, first base in the top two bits) + 32 invalid-base flags (bit 31 - i = base i).
// alphabet.h:128 semantics: A/C/G/T in either case, everything else invalid (its code bits are 0).
inline void pack32_scalar(const unsigned char *s, unsigned n, u64 &word, u32 &bad)
{
    u64 w = 0; u32 b = 0;
    for (unsigned i = 0; i < n; ++i) {
        const unsigned c = s[i] & 0xDFu, h = (c >> 1) & 3u;                    // A0 C1 T2 G3
        const bool ok = c == (unsigned)"ACTG"[h];
        const u64 code = ok ? (h ^ (h >> 1)) : 0u;                             // A0 C1 G2 T3
        w |= code << (62u - 2u * i);
        b |= (ok ? 0u : 1u) << (31u - i);
    }
    word = w; bad = b;
}
#if defined(__x86_64__)
__attribute__((target("avx2,bmi2"))) inline void pack32_avx2(const unsigned char *s, u64 &word, u32 &bad)
{
    const __m256i x = _mm256_loadu_si256((const __m256i *)s);
    const __m256i fold = _mm256_and_si256(x, _mm256_set1_epi8((char)0xDF));
    const __m256i h = _mm256_and_si256(_mm256_srli_epi16(x, 1), _mm256_set1_epi8(3));            // A0 C1 T2 G3
    const __m256i tbl = _mm256_setr_epi8('A', 'C', 'T', 'G', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 'A', 'C', 'T', 'G', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);
    const __m256i ok = _mm256_cmpeq_epi8(fold, _mm256_shuffle_epi8(tbl, h));
    const __m256i code = _mm256_and_si256(_mm256_xor_si256(h, _mm256_and_si256(_mm256_srli_epi16(h, 1), _mm256_set1_epi8(1))), ok);   // A0 C1 G2 T3, 0 where invalid
    const u32 lo = (u32)_mm256_movemask_epi8(_mm256_slli_epi16(code, 7));                        // bit i = low code bit of base i
    const u32 hi = (u32)_mm256_movemask_epi8(_mm256_slli_epi16(code, 6));
    const u32 okm = (u32)_mm256_movemask_epi8(ok);
    // base 0 to the top: reverse the 32-bit planes, then interleave them (hi plane on the odd bits)
    word = _pdep_u64((u64)__builtin_bitreverse32(hi), 0xAAAAAAAAAAAAAAAAULL) | _pdep_u64((u64)__builtin_bitreverse32(lo), 0x5555555555555555ULL);
    bad = __builtin_bitreverse32(~okm);
}
#endif
struct BadList { std::vector<u64> idx; std::vector<u32> mask; };
// src(r) = where read r's bases are (offsets[] say how many)
template <class Src>
void pack_range(Src src, const u64 *offsets, u64 r0, u64 r1, u64 n_total, u64 *words, BadList &bl, bool simd)
{
    for (u64 r = r0; r < r1; ++r) {
        const u64 o = offsets[r], L = offsets[r + 1] - o, wb = (o >> 5) + r;
        const unsigned char *s = (const unsigned char *)src(r);
        const u64 full = L >> 5;
        for (u64 w = 0; w <= full; ++w) {
            const unsigned n = w < full ? 32u : (unsigned)(L & 31u);
            if (!n) break;
            u64 word; u32 bad;
#if defined(__x86_64__)
            if (simd && n == 32u) pack32_avx2(s + 32 * w, word, bad); else
#endif
            pack32_scalar(s + 32 * w, n, word, bad);
            words[wb + w] = word;
            if (bad) { bl.idx.push_back(wb + w); bl.mask.push_back(bad); }
        }
        // the slack word(s) between this read's last word and the next read's first -- and the one behind the last read -- are
        // zeroed: the image is then a pure function of the reads (recycled buffers upload no stale bytes, images compare byte for byte)
        for (u64 w = wb + ((L + 31u) >> 5), e = (offsets[r + 1] >> 5) + r + 1; w <= e && (w < e || r + 1 == n_total); ++w) words[w] = 0;
    }
}

template <class Src>
int pack_reads_impl(Src src, const uint64_t *offsets, uint64_t n_reads, uint64_t *words, uint64_t *bad_word,
                    uint32_t *bad_mask, uint64_t bad_cap, uint64_t *n_bad, int threads)
{
    bool simd = false;
#if defined(__x86_64__)
    simd = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("bmi2");
#endif
    const unsigned nt = (unsigned)std::max(1, std::min<int>(threads, (int)(n_reads / 4096 + 1)));
    std::vector<BadList> bl(nt);
    if (nt == 1) pack_range(src, offsets, 0, n_reads, n_reads, words, bl[0], simd);
    else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; ++t)
            th.emplace_back([&, t] { pack_range(src, offsets, n_reads * t / nt, n_reads * (t + 1) / nt, n_reads, words, bl[t], simd); });
        for (auto &x : th) x.join();
    }
    u64 tot = 0;
    for (auto &b : bl) tot += b.idx.size();
    *n_bad = tot;
    if (tot > bad_cap || (tot && (!bad_word || !bad_mask))) return BNS_ERR_ARG;       // (*n_bad says how much room is needed)
    u64 at = 0;
    for (auto &b : bl) {                                           // (thread ranges are contiguous: the list comes out sorted by word)
        if (b.idx.empty()) continue;
        std::memcpy(bad_word + at, b.idx.data(), b.idx.size() * 8);
        std::memcpy(bad_mask + at, b.mask.data(), b.mask.size() * 4);
        at += b.idx.size();
    }
    return BNS_OK;
}

// ---- host batches ------------------------------------------------------------------------------------------------------------
extern "C" __global__ void scatter_mask_kernel(       // (C linkage: the kernel keeps the plain name it has always had in the code object)
const u64 *__restrict__ idx, const u32 *__restrict__ mask, u64 n, u32 *__restrict__ dense)
{
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dense[idx[i]] = mask[i];
}

// What a host batch is made of: ASCII bases, or packed words + the sparse list of words that hold an invalid base.
struct HostIn {
    bool packed = false; const char *bases = nullptr; const u64 *words = nullptr; const u64 *bad_word = nullptr; const u32 *bad_mask = nullptr; u64 n_bad = 0;
    static HostIn ascii(const char *bases) { HostIn in; in.bases = bases; return in; }
    static HostIn of_words(const u64 *words, const u64 *bad_word, const u32 *bad_mask, u64 n_bad)
    {
        HostIn in; in.packed = true; in.words = words; in.bad_word = bad_word; in.bad_mask = bad_mask; in.n_bad = n_bad; return in;
    }
};

// The prologue of the host-batch entry points: the packed arguments, the context, the entry point's own pointers (args_ok), the
// device; the bases and the units of the batch.
int host_batch_begin(bns_ctx *ctx, const HostIn &in, const u64 *offsets, u64 n_reads, int paired, bool args_ok, u64 &total, u64 &n_units)
{
    if (in.packed && (!in.words || (in.n_bad && (!in.bad_word || !in.bad_mask)))) return BNS_ERR_ARG;
    BNS_RC(ready(ctx, true, true));
    if (!offsets || !args_ok) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    total = offsets[n_reads];
    n_units = n_reads / (paired ? 2 : 1);
    return BNS_OK;
}

// n units of the per-unit arrays a caller asked for, device -> host + dst_off (the hit stream is not per unit: the caller's own copy)
int copy_units_back(bns_ctx *ctx, const UnitOut &host, const UnitOut &dev, u64 dst_off, u64 n, hipStream_t st)
{
    const size_t nb = (size_t)n * 4;
    HIPCHK(ctx, hipMemcpyAsync(host.taxon + dst_off, dev.taxon, nb, hipMemcpyDeviceToHost, st));
    if (host.missing) HIPCHK(ctx, hipMemcpyAsync(host.missing + dst_off, dev.missing, nb, hipMemcpyDeviceToHost, st));
    if (host.ambig) HIPCHK(ctx, hipMemcpyAsync(host.ambig + dst_off, dev.ambig, nb, hipMemcpyDeviceToHost, st));
    if (host.n_hits) HIPCHK(ctx, hipMemcpyAsync(host.n_hits + dst_off, dev.n_hits, nb, hipMemcpyDeviceToHost, st));
    return BNS_OK;
}

// ctx->st_out[0..3] from unit u0 on (+ st_hits), as the arrays of a launch or the source of a copy-back
UnitOut st_out_from(const bns_ctx *ctx, u64 u0)
{
    UnitOut o;
    o.taxon = (u32 *)ctx->st_out[0].p + u0; o.missing = (u32 *)ctx->st_out[1].p + u0; o.ambig = (u32 *)ctx->st_out[2].p + u0;
    o.n_hits = (u32 *)ctx->st_out[3].p + u0; o.hits = (u32 *)ctx->st_hits.p;
    return o;
}

// Upload + classify of one host batch, results left in ctx->st_out[0..3] (+ st_hits): large batches go up in slices on a second
// stream, slice i+1 while slice i is classified (the upload is the longer leg: 150 -- packed 40 -- bytes per read over PCIe against
// ~0.6 ns of kernel).  A slice is a unit-aligned read range; device offsets stay absolute, so a slice is just a shifted offsets
// pointer and a shifted output pointer.
// host: where the per-unit results of the batch go (null: they stay on the device); a sliced batch copies each slice's results back
// as soon as that slice is classified (the copy runs while the next slice is uploaded: the two directions of the link are separate),
// and says so in `copied`.
int classify_host_impl(bns_ctx *ctx, const HostIn &in, const uint64_t *offsets, uint64_t n_reads, int paired, bool want_missing, bool want_ambig,
                       bool want_nhits, bool want_hits, const UnitOut *host = nullptr, bool *copied = nullptr)
{
    int rc;
    const bool packed = in.packed;
    const u64 total = offsets[n_reads];
    const u64 n_units = n_reads / (paired ? 2 : 1);
    // the longest read of a range of the batch (what a launch sizes its rounds by): scanned per slice, next to that slice's
    // launch, so that the scan of 10 M offsets (80 MB) runs under the uploads instead of in front of them
    auto longest = [&](u64 r0, u64 r1) { u32 m = 0; for (u64 r = r0; r < r1; ++r) m = std::max<u32>(m, (u32)(offsets[r + 1] - offsets[r])); return m; };
    const u64 n_words = bns_packed_words(total, n_reads);
    if (packed) {
        if ((rc = ensure(ctx, ctx->st_words, (size_t)n_words * 8 + 8)) != BNS_OK) return rc;
        if (in.n_bad && (rc = ensure(ctx, ctx->st_nmask, (size_t)n_words * 4 + 4)) != BNS_OK) return rc;
        if (in.n_bad && (rc = ensure(ctx, ctx->st_bad, (size_t)in.n_bad * 12)) != BNS_OK) return rc;
    } else if ((rc = ensure(ctx, ctx->st_bases, (size_t)total + 8)) != BNS_OK) return rc;
    if ((rc = ensure(ctx, ctx->st_offsets, (size_t)(n_reads + 1) * 8)) != BNS_OK) return rc;
    for (int i = 0; i < 4; ++i) if ((rc = ensure(ctx, ctx->st_out[i], (size_t)n_units * 4)) != BNS_OK) return rc;
    if (want_hits && (rc = ensure(ctx, ctx->st_hits, (size_t)total * 4 + 4)) != BNS_OK) return rc;
    hipStream_t st = ctx->stream;
    const u32 *d_nmask = nullptr;
    if (packed && in.n_bad) {
        // the dense flag words the kernel reads: zero, then the few words that hold an invalid base scattered in
        u64 *d_idx = (u64 *)ctx->st_bad.p;
        u32 *d_msk = (u32 *)((char *)ctx->st_bad.p + (size_t)in.n_bad * 8);
        HIPCHK(ctx, hipMemsetAsync(ctx->st_nmask.p, 0, (size_t)n_words * 4, st));
        HIPCHK(ctx, hipMemcpyAsync(d_idx, in.bad_word, (size_t)in.n_bad * 8, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(d_msk, in.bad_mask, (size_t)in.n_bad * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(scatter_mask_kernel, dim3(grid_for(ctx, in.n_bad, 256)), dim3(256), 0, st, (const u64 *)d_idx, (const u32 *)d_msk, (u64)in.n_bad,
                           (u32 *)ctx->st_nmask.p);
        HIPCHK(ctx, hipGetLastError());
        d_nmask = (const u32 *)ctx->st_nmask.p;
    }
    auto run = [&](u64 r0, u64 nr, u64 u0) -> int {
        UnitOut o = st_out_from(ctx, u0);
        if (!want_missing) o.missing = nullptr;
        if (!want_ambig) o.ambig = nullptr;
        if (!(want_nhits || want_hits)) o.n_hits = nullptr;
        if (!want_hits) o.hits = nullptr;
        // (packed: the word base of a read is (offsets[r] >> 5) + r with r counted from the START of the batch, so a slice hands the
        // kernel word / flag pointers advanced by r0 words: read r0 + i of the batch is read i of the launch)
        ClassifyIn ci;
        if (packed) { ci.words = (const u64 *)ctx->st_words.p + r0; ci.nmask = d_nmask ? d_nmask + r0 : nullptr; }
        else ci.bases = (const char *)ctx->st_bases.p;
        ci.offsets = (const u64 *)ctx->st_offsets.p + r0; ci.n_reads = nr; ci.total_bases = total;
        ci.max_read_len = std::max<u32>(longest(r0, r0 + nr), 1); ci.paired = paired;
        ci.first_base = offsets[r0]; ci.end_base = offsets[r0 + nr];
        return classify_device_impl(ctx, ci, o, st);
    };
    auto upload = [&](u64 r0, u64 r1, hipStream_t cs) -> int {
        const u64 b0 = offsets[r0], b1 = offsets[r1];
        if (packed) {
            const u64 w0 = (b0 >> 5) + r0, w1 = r1 == n_reads ? n_words : (b1 >> 5) + r1;
            if (w1 > w0) HIPCHK(ctx, hipMemcpyAsync((u64 *)ctx->st_words.p + w0, in.words + w0, (size_t)(w1 - w0) * 8, hipMemcpyHostToDevice, cs));
        } else if (b1 > b0) HIPCHK(ctx, hipMemcpyAsync((char *)ctx->st_bases.p + b0, in.bases + b0, (size_t)(b1 - b0), hipMemcpyHostToDevice, cs));
        HIPCHK(ctx, hipMemcpyAsync((u64 *)ctx->st_offsets.p + r0, offsets + r0, (size_t)(r1 - r0 + 1) * 8, hipMemcpyHostToDevice, cs));
        return BNS_OK;
    };
    size_t slice_bytes = (size_t)64 << 20;                                // (8 .. 128 MiB measured within 5 % of each other; 64 the best)
    if (ctx->dbg & BNS_DBG_SLICE_8K) slice_bytes = (size_t)8 << 10;       // (tests force slicing on small batches)
    const int nmr = paired ? 2 : 1;
    const u64 in_bytes = packed ? n_words * 8 : total;
    u64 n_slices = std::min<u64>(16, std::max<u64>(1, in_bytes / slice_bytes));
    if (n_slices > n_units) n_slices = n_units;
    if (n_slices > 1) {
        if (!ctx->copy_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        if (host && !ctx->back_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->back_stream, hipStreamNonBlocking));
        for (u64 i = 0; i < n_slices; ++i) {
            if (!ctx->slice_ev[i]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->slice_ev[i], hipEventDisableTiming));
            if (host && !ctx->done_ev[i]) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->done_ev[i], hipEventDisableTiming));
        }
        // size the per-call workspaces for the largest slice up front: growing one mid-loop would hipFree, i.e. drain the GPU
        const u64 max_slice_units = n_units / n_slices + 2;
        if ((rc = ensure(ctx, ctx->records, (size_t)max_slice_units * 16)) != BNS_OK) return rc;
        if ((rc = ensure(ctx, ctx->ovf_list, (size_t)max_slice_units * 8)) != BNS_OK) return rc;
        HIPCHK(ctx, hipStreamSynchronize(st));                            // the staging buffers may still be read by earlier work
        hipStream_t cs = ctx->copy_stream;              // (two alternating copy streams were tried: the link, not the DMA engine, is the limit)
        auto slice_end = [&](u64 i) { return (i + 1 == n_slices) ? n_units : n_units * (i + 1) / n_slices; };
        auto send = [&](u64 i) -> int {                 // slice i's upload, and the event the classify stream waits for
            const u64 a = i ? slice_end(i - 1) : 0, b = slice_end(i);
            int rc2 = upload(a * nmr, b * nmr, cs);
            if (rc2 != BNS_OK) return rc2;
            HIPCHK(ctx, hipEventRecord(ctx->slice_ev[i], cs));
            return BNS_OK;
        };
        if ((rc = send(0)) != BNS_OK) return rc;
        u64 u0 = 0;
        for (u64 i = 0; i < n_slices; ++i) {
            const u64 u1 = slice_end(i);
            // slice i + 1 is on its way before slice i is classified (a launch whose units can overflow the in-LDS counter ends
            // with a host-side wait: the next upload must not queue up behind that)
            if (i + 1 < n_slices && (rc = send(i + 1)) != BNS_OK) { (void)hipStreamSynchronize(cs); return rc; }
            HIPCHK(ctx, hipStreamWaitEvent(st, ctx->slice_ev[i], 0));
            if (u1 > u0 && (rc = run(u0 * nmr, (u1 - u0) * nmr, u0)) != BNS_OK) { (void)hipStreamSynchronize(cs); return rc; }
            if (host && u1 > u0) {
                // (on a stream of their own: queued on the classify stream these copies held up the next slice's launch, and with it
                // the upload after that -- 711 -> 860 M reads/s with all four arrays coming back)
                hipStream_t bs = ctx->back_stream;
                HIPCHK(ctx, hipEventRecord(ctx->done_ev[i], st));
                HIPCHK(ctx, hipStreamWaitEvent(bs, ctx->done_ev[i], 0));
                BNS_RC(copy_units_back(ctx, *host, st_out_from(ctx, u0), u0, u1 - u0, bs));
            }
            u0 = u1;
        }
        if (host) {
            *copied = true;
            HIPCHK(ctx, hipStreamSynchronize(ctx->back_stream));       // (the caller's arrays are complete when this returns)
        }
        return BNS_OK;
    }
    if ((rc = upload(0, n_reads, st)) != BNS_OK) return rc;
    return run(0, n_reads, 0);
}

// bns_classify_batch / bns_classify_batch_packed
int classify_host_entry(bns_ctx *ctx, const HostIn &in, const uint64_t *offsets, uint64_t n_reads, int paired, const UnitOut &out)
{
    int rc;
    u64 total, n_units;
    BNS_RC(host_batch_begin(ctx, in, offsets, n_reads, paired, out.taxon != nullptr, total, n_units));
    if (n_units == 0) return BNS_OK;
    bool copied = false;
    if ((rc = classify_host_impl(ctx, in, offsets, n_reads, paired, out.missing != nullptr, out.ambig != nullptr, out.n_hits != nullptr, out.hits != nullptr,
                                 &out, &copied)) != BNS_OK) {
        (void)hipStreamSynchronize(ctx->stream);                  // (copies into the caller's arrays may be in flight)
        if (ctx->back_stream) (void)hipStreamSynchronize(ctx->back_stream);
        return rc;
    }
    hipStream_t st = ctx->stream;
    if (!copied) BNS_RC(copy_units_back(ctx, out, st_out_from(ctx, 0), 0, n_units, st));
    if (out.hits && total) HIPCHK(ctx, hipMemcpyAsync(out.hits, ctx->st_hits.p, (size_t)total * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return BNS_OK;
}

// bns_classify_batch_runs / bns_classify_batch_packed_runs
int classify_runs_entry(bns_ctx *ctx, const HostIn &in, const uint64_t *offsets, uint64_t n_reads, int paired, const UnitOut &out, uint64_t *run_start,
                        uint32_t *n_runs, const uint32_t **run_tax, const uint32_t **run_len, uint64_t *n_runs_total)
{
    int rc;
    u64 total, n_units;
    BNS_RC(host_batch_begin(ctx, in, offsets, n_reads, paired, out.taxon && run_start && n_runs && run_tax && run_len, total, n_units));
    const int nm = paired ? 2 : 1;
    *run_tax = *run_len = nullptr;
    if (n_runs_total) *n_runs_total = 0;
    if (n_units == 0) return BNS_OK;
    if ((rc = ensure(ctx, ctx->st_runs[0], (size_t)n_units * 8)) != BNS_OK) return rc;
    if ((rc = ensure(ctx, ctx->st_runs[1], (size_t)n_units * 4)) != BNS_OK) return rc;
    if ((rc = ensure(ctx, ctx->st_runs[2], (size_t)total * 4 + 4)) != BNS_OK) return rc;      // a run per hit at worst
    if ((rc = ensure(ctx, ctx->st_runs[3], (size_t)total * 4 + 4)) != BNS_OK) return rc;
    if ((rc = classify_host_impl(ctx, in, offsets, n_reads, paired, true, true, true, true)) != BNS_OK) return rc;
    hipStream_t st = ctx->stream;
    unsigned long long *d_cur = &((SmallLayout *)ctx->small.p)->runs_cursor;
    HIPCHK(ctx, hipMemsetAsync(d_cur, 0, 8, st));
    hipLaunchKernelGGL(hit_runs_kernel, dim3(grid_for(ctx, (n_units + HIT_RUNS_GROUP - 1) / HIT_RUNS_GROUP, 4)), dim3(256), 0, st, (const u32 *)ctx->st_hits.p,
                       (const u64 *)ctx->st_offsets.p, (u32)nm, (const u32 *)ctx->st_out[3].p, (u64)n_units, (u64 *)ctx->st_runs[0].p,
                       (u32 *)ctx->st_runs[1].p, (u32 *)ctx->st_runs[2].p, (u32 *)ctx->st_runs[3].p, d_cur);
    HIPCHK(ctx, hipGetLastError());
    unsigned long long n_tot = 0;
    HIPCHK(ctx, hipMemcpyAsync(&n_tot, d_cur, 8, hipMemcpyDeviceToHost, st));
    BNS_RC(copy_units_back(ctx, out, st_out_from(ctx, 0), 0, n_units, st));
    HIPCHK(ctx, hipMemcpyAsync(run_start, ctx->st_runs[0].p, (size_t)n_units * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(n_runs, ctx->st_runs[1].p, (size_t)n_units * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));                    // n_tot is known from here on
    if (ctx->h_run_cap < n_tot) {
        if (ctx->h_run_tax) (void)hipHostFree(ctx->h_run_tax);
        if (ctx->h_run_len) (void)hipHostFree(ctx->h_run_len);
        ctx->h_run_tax = ctx->h_run_len = nullptr; ctx->h_run_cap = 0;
        const size_t want = (size_t)n_tot + (size_t)n_tot / 2;
        HIPCHK(ctx, hipHostMalloc((void **)&ctx->h_run_tax, want * 4, hipHostMallocDefault));
        HIPCHK(ctx, hipHostMalloc((void **)&ctx->h_run_len, want * 4, hipHostMallocDefault));
        ctx->h_run_cap = want;
    }
    if (n_tot) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_run_tax, ctx->st_runs[2].p, (size_t)n_tot * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_run_len, ctx->st_runs[3].p, (size_t)n_tot * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    *run_tax = ctx->h_run_tax; *run_len = ctx->h_run_len;
    if (n_runs_total) *n_runs_total = n_tot;
    return BNS_OK;
}

}  // namespace
