// bns_minqual.hpp -- minimum base quality (bns_set_min_base_quality / `bonsai classify -Q`; gfx950, wave64).  Included by
// bns_ingest.hip in front of pack_text_kernel (same translation unit: StreamArgs, StreamInfo, pack32_scalar, BadList).
//
// A base whose Phred+33 quality byte is below 33 + q behaves like 'N': its invalid flag is set, its code bits are 0 (definition in
// DESIGN.md "Defined behaviour"; Kraken 2's --minimum-base-quality, whose source is not at hand).  Nothing behind the packed image
// knows about it.  Two halves:
//   * device: QualCursor, through which the masked form of pack_text_kernel (pack_text_minq_kernel) reads byte i of a record's
//     quality string -- the string as kseq_read yields it (klib/kseq.h:217: lines joined, one trailing '\r' per appended line
//     dropped by the rule of :135).
//   * host: bns_pack_reads_qual_ptrs, bns_pack_reads_ptrs with a quality string per read.
//
// Where a record's quality lies is NOT recorded by walk_kernel.  line_off[] is per line and race-free only because no two walks
// take the same line for a sequence line; quality lines are walked by several candidates (the header's own walk, and that of every
// false candidate behind a '+'-led line), so per-line quality offsets written there would race.  Instead the record's lane group
// finds its quality itself, from what the walk of its DECIDED header left per candidate: c_line1[j] is the line the sequence lines
// ended at -- the '+' line when the record has one -- and the quality starts on the line behind it.  As a rule that one line holds
// all of it (`single`: aligned 4-byte loads, like the bases); otherwise every lane steps a cursor of its own from line to line (its
// base index only grows from pass to pass, so a lane crosses each line once).  Quality may be wrapped differently from the
// sequence: the cursor does not look at the sequence lines at all.
#pragma once

namespace bns {
namespace ingest {
namespace minqual {

constexpr u32 NONE = 0xFFFFFFFFu;

struct QualCursor {
    u32 single = NONE;                          // where the one quality line starts
    u32 line = NONE;                            // otherwise: the quality line the cursor stands in (NONE: a record without quality)
    u32 before = 0, st = 0, eff = 0;            // quality bytes in front of that line; where it starts; its bytes
    u32 n_lines = 0;

    // bytes that quality line l adds behind `before` bytes (walk_kernel's rule for quality lines: klib/kseq.h:135)
    static __device__ __forceinline__ u32 eff_len(const StreamArgs &a, u32 l, u32 before, u32 &st)
    {
        st = a.ls[l];
        const u32 e = a.ls[l + 1] - 1u, len = e - st;
        return len - ((len && a.text[e - 1u] == '\r' && before + len > 1u) ? 1u : 0u);
    }
    // lp: the line the record's sequence lines ended at (c_line1); L > 0: its bases
    __device__ __forceinline__ void open(const StreamArgs &a, const StreamInfo &si, u32 lp, u32 L)
    {
        n_lines = si.n_lines;
        if (lp >= si.n_real || lp + 1u >= n_lines) return;
        const u32 ps = a.ls[lp];
        if (a.ls[lp + 1u] - 1u == ps || a.text[ps] != '+') return;      // the next header, or the end of the text: FASTA
        line = lp + 1u;
        eff = eff_len(a, line, 0u, st);
        if (eff == L) single = st;
    }
    // quality bytes of bases bi .. bi + nb - 1 (nb <= 4, bi + nb <= L), first in the low byte; 0xFF where there is none.  bi grows from call to call.
    __device__ __forceinline__ u32 fetch(const StreamArgs &a, u32 bi, u32 nb)
    {
        if (single != NONE) {
            const u32 addr = single + bi, mis = addr & 3u;
            const u32 *ap = reinterpret_cast<const u32 *>(a.text + (addr - mis));
            const u32 lo = ap[0], hi = (mis + nb > 4u) ? ap[1] : 0u;
            return (u32)((((u64)hi << 32) | lo) >> (8u * mis)) | (nb < 4u ? 0xFFFFFFFFu << (8u * nb) : 0u);
        }
        if (line == NONE) return 0xFFFFFFFFu;
        u32 qw = 0xFFFFFFFFu;
        for (u32 i = 0; i < nb; ++i) {
            const u32 b = bi + i;
            while (b - before >= eff) {                         // (a taken record is regular: its quality lines hold L bytes, b < L)
                if (line + 2u > n_lines) return 0u;
                before += eff; ++line;
                eff = eff_len(a, line, before, st);
            }
            qw = (qw & ~(0xFFu << (8u * i))) | ((u32)a.text[st + (b - before)] << (8u * i));
        }
        return qw;
    }
};

}  // namespace minqual
}  // namespace ingest
}  // namespace bns

// ---- host: bns_pack_reads_ptrs with qualities -------------------------------------------------------------------------------
namespace {
// flags (bit 31 - i = byte i) of the first n <= 32 bytes of q that are below thr
inline u32 qual_bad32_scalar(const unsigned char *q, unsigned n, unsigned thr)
{
    u32 b = 0;
    for (unsigned i = 0; i < n; ++i) b |= (q[i] < thr ? 1u : 0u) << (31u - i);
    return b;
}
#if defined(__x86_64__)
__attribute__((target("avx2"))) inline u32 qual_bad32_avx2(const unsigned char *q, unsigned thr)
{
    const __m256i x = _mm256_loadu_si256((const __m256i *)q);
    const __m256i ge = _mm256_cmpeq_epi8(_mm256_max_epu8(x, _mm256_set1_epi8((char)thr)), x);      // unsigned x >= thr
    return __builtin_bitreverse32(~(u32)_mm256_movemask_epi8(ge));
}
#endif
// flag bit i -> the two code bits 2 i, 2 i + 1 of the image word
inline u64 spread2(u32 b)
{
    u64 x = b;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFULL;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFULL;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0FULL;
    x = (x | (x << 2)) & 0x3333333333333333ULL;
    x = (x | (x << 1)) & 0x5555555555555555ULL;
    return x | (x << 1);
}
// pack_range with a quality string per read (quals[r] may be null)
void pack_range_qual(const char *const *seqs, const char *const *quals, unsigned thr, const u64 *offsets, u64 r0, u64 r1, u64 n_total, u64 *words,
                     BadList &bl, bool simd)
{
    for (u64 r = r0; r < r1; ++r) {
        const u64 o = offsets[r], L = offsets[r + 1] - o, wb = (o >> 5) + r;
        const unsigned char *s = (const unsigned char *)seqs[r], *q = (const unsigned char *)quals[r];
        const u64 full = L >> 5;
        for (u64 w = 0; w <= full; ++w) {
            const unsigned n = w < full ? 32u : (unsigned)(L & 31u);
            if (!n) break;
            u64 word; u32 bad;
#if defined(__x86_64__)
            if (simd && n == 32u) pack32_avx2(s + 32 * w, word, bad); else
#endif
            pack32_scalar(s + 32 * w, n, word, bad);
            if (q) {
                u32 qb;
#if defined(__x86_64__)
                if (simd && n == 32u) qb = qual_bad32_avx2(q + 32 * w, thr); else
#endif
                qb = qual_bad32_scalar(q + 32 * w, n, thr);
                word &= ~spread2(qb);
                bad |= qb;
            }
            words[wb + w] = word;
            if (bad) { bl.idx.push_back(wb + w); bl.mask.push_back(bad); }
        }
        for (u64 w = wb + ((L + 31u) >> 5), e = (offsets[r + 1] >> 5) + r + 1; w <= e && (w < e || r + 1 == n_total); ++w) words[w] = 0;   // (slack words: as pack_range)
    }
}
}  // namespace

extern "C" int bns_pack_reads_qual_ptrs(const char *const *seqs, const char *const *quals, const uint32_t *lens, uint64_t n_reads, uint32_t min_quality,
                                        uint64_t *offsets, uint64_t *words, uint64_t *bad_word, uint32_t *bad_mask, uint64_t bad_cap, uint64_t *n_bad,
                                        int threads)
{
    if (min_quality > 93u) return BNS_ERR_ARG;
    if (!min_quality || !quals) return bns_pack_reads_ptrs(seqs, lens, n_reads, offsets, words, bad_word, bad_mask, bad_cap, n_bad, threads);
    if (!offsets || !words || !n_bad || (n_reads && (!seqs || !lens))) return BNS_ERR_ARG;
    offsets[0] = 0;
    for (u64 r = 0; r < n_reads; ++r) offsets[r + 1] = offsets[r] + lens[r];
    bool simd = false;
#if defined(__x86_64__)
    simd = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("bmi2");
#endif
    const unsigned thr = 33u + min_quality;
    const unsigned nt = (unsigned)std::max(1, std::min<int>(threads, (int)(n_reads / 4096 + 1)));
    std::vector<BadList> bl(nt);
    if (nt == 1) pack_range_qual(seqs, quals, thr, offsets, 0, n_reads, n_reads, words, bl[0], simd);
    else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; ++t)
            th.emplace_back([&, t] { pack_range_qual(seqs, quals, thr, offsets, n_reads * t / nt, n_reads * (t + 1) / nt, n_reads, words, bl[t], simd); });
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
