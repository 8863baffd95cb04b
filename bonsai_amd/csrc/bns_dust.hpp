// bns_dust.hpp -- low-complexity masking of the packed image: bns_set_dust / bns_dust_mask (`bonsai classify -m`, `bonsai build -m`;
// gfx950, wave64).  Symmetric DUST as DESIGN.md "Defined behaviour" states it; the recurrence, the halo argument and the numbers are in
// docs/DUST_NOTES.md.
//
// Inside a maximal run of valid bases a triplet is three consecutive bases; an interval of l triplets (2 <= l <= W - 2) scores
// S = sum_t c_t (c_t - 1) / 2 / (l - 1); it is perfect when 10 S > T and no sub-interval scores strictly higher; the mask is the union
// of the bases of all perfect intervals.  With M(i, j) the maximum score of the sub-intervals of triplets i..j,
//   M(i, j) = max(S(i, j), M(i + 1, j), M(i, j - 1))   and   (i, j) perfect  <=>  10 S > T  and  S(i, j) >= max(M(i + 1, j), M(i, j - 1)).
// Scores are fractions num / den (num <= 1891, den <= 61) compared by cross-multiplication in u32: no floating point.
//
//   dust_mark_kernel   work item = a piece of DUST_PIECE bases of the BATCH (as windows_pack_kernel cuts it), one wavefront each: the
//                      rounds of 64 start triplets of every sequence that begin inside the piece, right to left.  In a round lane =
//                      start triplet i, step = interval length l: the lane adds triplet i + l - 1 to its numerator (num += cnt[t]++),
//                      takes its right neighbour's M of step l - 1 by one DPP shift across the wavefront and keeps the longest perfect
//                      l it met.  Lane 63's neighbour is lane 0 of the round to the right: that round left its M(s, s + l - 1) in LDS.
//                      The rightmost round of a piece whose sequence goes on is preceded by a HALO round over the next 64 starts with
//                      truncated lengths (start e + h: l <= W - 3 - h), which needs nothing further right and marks nothing.
//                      The union of [i, i + best_i + 2) over a round's lanes is a prefix maximum; it is OR'ed into a flag buffer of
//                      one u32 per packed word with at most four atomics a round (a perfect interval reaches up to W - 1 bases into
//                      the words of the next round, which another wavefront may own).
//                      Triplet counters: 64 counts of one byte per lane in LDS, word (t >> 2) * 64 + lane: a lane only ever touches
//                      its own bank (docs/KERNEL_NOTES.md, "Low-complexity masking").
//   dust_apply_kernel  nmask |= flags, the code bits of flagged bases cleared; from the caller's image into ours (copy) or in place.
//                      A launch of its own behind dust_mark_kernel: scores are computed from the unmasked image.
// Runs end at an invalid base and at the sequence end; the slack word between two sequences is never read as bases (every position is
// checked against the sequence length, whatever its flag word says).
#pragma once

namespace bns {

constexpr u32 DUST_PIECE = 2048;                // bases of the batch per work item; rounds are cut at multiples of 64 bases of a SEQUENCE

__device__ __forceinline__ void dust_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the last sequence s with offsets[s] <= g (offsets[0] <= g < offsets[n_seqs])
__device__ __forceinline__ u64 dust_seq_of(const u64 *__restrict__ offsets, u64 n_seqs, u64 g)
{
    u64 lo = 0, hi = n_seqs;
    while (hi - lo > 1) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// a / b > c / d for packed fractions (num << 8 | den), den >= 1
__device__ __forceinline__ bool dust_gt(u32 x, u32 y) { return (x >> 8) * (y & 0xFFu) > (y >> 8) * (x & 0xFFu); }

// One round: the 64 start triplets s0 .. s0 + 63 of the sequence whose words start at wb (L bases, n_words words).  s0 is a multiple of 64.
__device__ __forceinline__ void dust_round(const u64 *__restrict__ words, const u32 *__restrict__ nmask, u64 wb, u64 L, u64 n_words, u64 s0, bool halo,
                                           u32 W, u32 T, u8 *s_trip, u32 *s_cnt, const u32 *bnd_in, u32 *bnd_out, u32 *__restrict__ flags)
{
    const u32 lane = (u32)lane_id();
    const u64 wi = (s0 >> 5) + (lane >> 5);
    const u32 sh = lane & 31u;
    u64 a[4]; u32 m[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = wi + j < n_words;
        a[j] = in ? words[wb + wi + j] : 0ULL;
        m[j] = in ? (nmask ? nmask[wb + wi + j] : 0u) : 0xFFFFFFFFu;
    }
    // triplets s0 + lane and s0 + 64 + lane: 6 code bits, 3 flag bits, and all three bases inside the sequence
    const u64 x0 = sh ? (a[0] << (2u * sh)) | (a[1] >> (64u - 2u * sh)) : a[0];
    const u64 x1 = sh ? (a[2] << (2u * sh)) | (a[3] >> (64u - 2u * sh)) : a[2];
    const u32 i0 = (u32)(((((u64)m[0] << 32) | m[1]) << sh) >> 61), i1 = (u32)(((((u64)m[2] << 32) | m[3]) << sh) >> 61);
    const u64 q0 = s0 + lane;
    const bool v0 = i0 == 0u && q0 + 3u <= L, v1 = i1 == 0u && q0 + 67u <= L;
    dust_wave_sync();                                         // (the round before this one has read its triplets)
    s_trip[lane] = (u8)(x0 >> 58);
    s_trip[64u + lane] = (u8)(x1 >> 58);
    u32 *cw = s_cnt + lane;
#pragma unroll
    for (int j = 0; j < 16; ++j) cw[j * 64] = 0u;
    const u64 V0 = ballot64(v0), V1 = ballot64(v1);
    const u64 win = lane ? (V0 >> lane) | (V1 << (64u - lane)) : V0;
    const u32 runlen = ~win ? (u32)__builtin_ctzll(~win) : 64u;     // valid triplets in a row from this lane's on
    u32 maxlen = runlen < W - 2u ? runlen : W - 2u;
    if (halo) { const u32 cap = lane + 3u <= W ? W - 3u - lane : 0u; maxlen = maxlen < cap ? maxlen : cap; }
    if (maxlen) { const u32 t = (u32)(x0 >> 58); cw[(t >> 2) * 64u] = 1u << (8u * (t & 3u)); }
    u32 Mo = 1u;                                              // M(i, i): no interval of two triplets inside it -- 0 / 1
    u32 num = 0, best = 0;
    if (lane == 0) bnd_out[1] = Mo;
    dust_wave_sync();
    // bnd_in is read by every round, also where no round to the right has written it (the rightmost round of a sequence, a halo round:
    // stale or never written).  Only lane 63 takes the value, and only while it is active at l, which needs triplet s0 + 64 to be valid:
    // a round to the right then exists and ran at least to l - 1 (the triangle argument, docs/DUST_NOTES.md).
    for (u32 l = 2; ballot64(l <= maxlen); ++l) {
        const u32 bv = bnd_in[l - 1u];
        const u32 Mr = (u32)__builtin_amdgcn_update_dpp((int)bv, (int)Mo, DPP_WAVE_SHL1, 0xf, 0xf, false);
        if (l <= maxlen) {
            const u32 t = s_trip[lane + l - 1u];
            const u32 ix = (t >> 2) * 64u, bs = 8u * (t & 3u);
            const u32 w = cw[ix];
            cw[ix] = w + (1u << bs);
            num += (w >> bs) & 0xFFu;
            const u32 den = l - 1u;
            const u32 Mp = dust_gt(Mr, Mo) ? Mr : Mo;
            const bool ge = num * (Mp & 0xFFu) >= (Mp >> 8) * den;
            if (ge && 10u * num > T * den) best = l;
            Mo = ge ? (num << 8) | den : Mp;
        }
        if (lane == 0) bnd_out[l] = Mo;
    }
    if (halo) return;
    // the union of [lane, lane + best + 2) over the lanes, in bases s0 .. s0 + 127
    u32 pm = best ? lane + best + 2u : 0u;
#pragma unroll
    for (u32 d = 1; d < 64u; d <<= 1) {
        const u32 o = (u32)__shfl_up((int)pm, d);
        if (lane >= d) pm = pm > o ? pm : o;
    }
    const u32 R = readlane(pm, 63);
    const u64 B0 = ballot64(pm > lane), B1 = ballot64(R > 64u + lane);
    if (lane < 4u) {
        const u64 B = lane < 2u ? B0 : B1;
        const u32 f = __builtin_bitreverse32((u32)(B >> (32u * (lane & 1u))));     // base i of a word is bit 31 - i of its flag word
        const u64 fw = (s0 >> 5) + lane;
        if (f && fw < n_words) atomicOr(&flags[wb + fw], f);
    }
}

__global__ __launch_bounds__(256) void dust_mark_kernel(const u64 *__restrict__ words, const u32 *__restrict__ nmask, const u64 *__restrict__ offsets,
                                                        u64 n_seqs, u32 W, u32 T, u32 *__restrict__ flags)
{
    __shared__ u32 s_cnt[4][16 * 64];
    __shared__ u32 s_bnd[4][2][64];
    __shared__ u8 s_trip[4][128];
    const u32 wv = (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 wave = (u64)blockIdx.x * 4 + wv, n_waves = (u64)gridDim.x * 4;
    const u64 base0 = offsets[0], end = offsets[n_seqs];
    const u64 n_pieces = (end - base0 + DUST_PIECE - 1) / DUST_PIECE;
    for (u64 g = wave; g < n_pieces; g += n_waves) {
        const u64 g0 = base0 + g * DUST_PIECE, g1 = g0 + DUST_PIECE < end ? g0 + DUST_PIECE : end;
        for (u64 s = dust_seq_of(offsets, n_seqs, g0); s < n_seqs; ++s) {
            const u64 o = offsets[s];
            if (o >= g1) break;
            const u64 L = offsets[s + 1] - o;
            if (L < 4) continue;                                  // fewer than two triplets: no interval
            const u64 n_trip = L - 2;
            const u64 t_lo = o >= g0 ? 0 : (g0 - o + 63) >> 6;    // rounds whose first base lies inside the piece
            const u64 t_all = (n_trip + 63) >> 6, t_cut = (g1 - o + 63) >> 6;
            const u64 t_hi = t_all < t_cut ? t_all : t_cut;
            if (t_lo >= t_hi) continue;
            const u64 wb = (o >> 5) + s, n_words = (L + 31) >> 5;
            u32 pp = 0;
            if ((t_hi << 6) < n_trip) {
                dust_round(words, nmask, wb, L, n_words, t_hi << 6, true, W, T, s_trip[wv], s_cnt[wv], s_bnd[wv][1], s_bnd[wv][0], flags);
                pp = 1;
            }
            for (u64 t = t_hi; t-- > t_lo;) {
                dust_round(words, nmask, wb, L, n_words, t << 6, false, W, T, s_trip[wv], s_cnt[wv], s_bnd[wv][pp ^ 1u], s_bnd[wv][pp], flags);
                pp ^= 1u;
            }
        }
    }
}

// 32 flag bits -> the 64 code bits of the same bases
__device__ __forceinline__ u64 dust_spread(u32 f)
{
    u64 x = f;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFULL;
    x = (x | (x << 8)) & 0x00FF00FF00FF00FFULL;
    x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0FULL;
    x = (x | (x << 2)) & 0x3333333333333333ULL;
    x = (x | (x << 1)) & 0x5555555555555555ULL;
    return x | (x << 1);
}

// copy: every word that holds a base of the batch is written to dst (the caller's image is only read); else only the flagged ones, in place
__global__ __launch_bounds__(256) void dust_apply_kernel(const u64 *src_words, const u32 *src_nmask, const u64 *__restrict__ offsets, u64 n_seqs,
                                                         const u32 *__restrict__ flags, u64 *dst_words, u32 *dst_nmask, int copy)
{
    const u32 lane = (u32)lane_id();
    const u64 wave = (u64)blockIdx.x * 4 + (u64)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), n_waves = (u64)gridDim.x * 4;
    const u64 base0 = offsets[0], end = offsets[n_seqs];
    const u64 n_pieces = (end - base0 + DUST_PIECE - 1) / DUST_PIECE;
    for (u64 g = wave; g < n_pieces; g += n_waves) {
        const u64 g0 = base0 + g * DUST_PIECE, g1 = g0 + DUST_PIECE < end ? g0 + DUST_PIECE : end;
        for (u64 s = dust_seq_of(offsets, n_seqs, g0); s < n_seqs; ++s) {
            const u64 o = offsets[s];
            if (o >= g1) break;
            const u64 L = offsets[s + 1] - o;
            const u64 wb = (o >> 5) + s, n_words = (L + 31) >> 5;
            const u64 j_lo = o >= g0 ? 0 : (g0 - o + 31) >> 5;    // words whose first base lies inside the piece
            const u64 j_cut = (g1 - o + 31) >> 5;
            const u64 j_hi = n_words < j_cut ? n_words : j_cut;
            for (u64 j = j_lo + lane; j < j_hi; j += 64) {
                const u64 x = wb + j;
                const u32 f = flags[x];
                if (copy || f) {
                    const u64 w = src_words[x];
                    const u32 m = src_nmask ? src_nmask[x] : 0u;
                    dst_words[x] = w & ~dust_spread(f);
                    dst_nmask[x] = m | f;
                }
            }
        }
    }
}

}  // namespace bns

namespace {

// The bases [lo, hi) the offsets of a call span (a whole batch: 0 .. total_bases; a slice of a host batch: its own range, so that a
// batch in 16 slices does not clear the flag words and size the grids of the whole batch 16 times).  Word indices follow the offsets.
struct DustSpan { u64 lo = 0, hi = 0; };

// flag words of the image (words [+ nmask], offsets, n_seqs) into ctx->dust_flags, on st
int dust_mark(bns_ctx *ctx, const u64 *words, const u32 *nmask, const u64 *offsets, u64 n_seqs, DustSpan sp, hipStream_t st)
{
    const size_t w0 = (size_t)(sp.lo >> 5), n_words = (size_t)(sp.hi >> 5) + n_seqs + 2;
    BNS_RC(ensure(ctx, ctx->dust_flags, n_words * 4));
    HIPCHK(ctx, hipMemsetAsync((u32 *)ctx->dust_flags.p + w0, 0, (n_words - w0) * 4, st));
    hipLaunchKernelGGL(dust_mark_kernel, dim3(grid_for(ctx, (sp.hi - sp.lo) / DUST_PIECE + 1, 4)), dim3(256), 0, st, words, nmask, offsets, n_seqs, ctx->dust_w,
                       ctx->dust_t, (u32 *)ctx->dust_flags.p);
    HIPCHK(ctx, hipGetLastError());
    return BNS_OK;
}

// mark, then apply: src masked into dst (copy: a caller's image, which is only read), or src == dst masked where it lies
int dust_apply(bns_ctx *ctx, const u64 *src_words, const u32 *src_nmask, const u64 *offsets, u64 n_seqs, DustSpan sp, u64 *dst_words, u32 *dst_nmask,
               bool copy, hipStream_t st)
{
    BNS_RC(dust_mark(ctx, src_words, src_nmask, offsets, n_seqs, sp, st));
    hipLaunchKernelGGL(dust_apply_kernel, dim3(grid_for(ctx, (sp.hi - sp.lo) / DUST_PIECE + 1, 4)), dim3(256), 0, st, src_words, src_nmask, offsets, n_seqs,
                       (const u32 *)ctx->dust_flags.p, dst_words, dst_nmask, copy ? 1 : 0);
    HIPCHK(ctx, hipGetLastError());
    return BNS_OK;
}

// the masked image in ctx->words / ctx->nmask: of those buffers themselves (words == ctx->words.p: what pack_reads left there), or of a
// caller's image
int dust_image(bns_ctx *ctx, const u64 *words, const u32 *nmask, const u64 *offsets, u64 n_seqs, DustSpan sp, hipStream_t st)
{
    const size_t n_words = (size_t)(sp.hi >> 5) + n_seqs + 2;
    const bool own = words == (const u64 *)ctx->words.p;
    if (!own) {
        BNS_RC(ensure(ctx, ctx->words, n_words * 8));
        BNS_RC(ensure(ctx, ctx->nmask, n_words * 4));
    }
    return dust_apply(ctx, words, nmask, offsets, n_seqs, sp, (u64 *)ctx->words.p, (u32 *)ctx->nmask.p, !own, st);
}

int dust_image_span(bns_ctx *ctx, const u64 *words, const u32 *nmask, const u64 *offsets, u64 n_seqs, u64 lo, u64 hi, hipStream_t st)
{
    return dust_image(ctx, words, nmask, offsets, n_seqs, DustSpan{lo, hi}, st);
}

// pack_reads, and the image masked when bns_set_dust is on (the build entry points)
int pack_reads_dust(bns_ctx *ctx, const char *d_bases, const u64 *d_offsets, u64 n_seqs, u64 total_bases, hipStream_t st)
{
    BNS_RC(pack_reads(ctx, d_bases, d_offsets, n_seqs, total_bases, st));
    if (!ctx->dust_w || n_seqs == 0) return BNS_OK;
    return dust_image(ctx, (const u64 *)ctx->words.p, (const u32 *)ctx->nmask.p, d_offsets, n_seqs, DustSpan{0, total_bases}, st);
}

int set_dust(bns_ctx *ctx, u32 window, u32 level)
{
    if (!ctx) return BNS_ERR_ARG;
    if (ctx->build) return fail(ctx, BNS_ERR_STATE, "bns_set_dust while a build session is open (bns_build_end)");
    if (ctx->windows) return fail(ctx, BNS_ERR_STATE, "bns_set_dust while a window session is open (bns_windows_end)");
    if (window == 0) { ctx->dust_w = 0; ctx->dust_t = 0; return BNS_OK; }
    if (window < 8u || window > 64u) return fail(ctx, BNS_ERR_ARG, "bns_set_dust: window must be 0 (off) or in [8, 64]");
    if (level < 1u || level > 1000u) return fail(ctx, BNS_ERR_ARG, "bns_set_dust: level must be in [1, 1000]");
    ctx->dust_w = window; ctx->dust_t = level;
    return BNS_OK;
}

int stage_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_reads);   // bns_api.hip

int dust_mask_host(bns_ctx *ctx, const char *bases, const u64 *offsets, u64 n_seqs, u32 *flags)
{
    if (!ctx || !offsets || !flags || (!bases && n_seqs && offsets[n_seqs])) return BNS_ERR_ARG;
    if (!ctx->dust_w) return fail(ctx, BNS_ERR_STATE, "bns_dust_mask: low-complexity masking is off (bns_set_dust)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const u64 total = n_seqs ? offsets[n_seqs] : 0;
    const size_t n_words = (size_t)((total >> 5) + n_seqs + 1);
    std::memset(flags, 0, n_words * 4);
    if (n_seqs == 0 || total == 0) return BNS_OK;
    hipStream_t st = ctx->stream;
    BNS_RC(stage_batch(ctx, bases, offsets, n_seqs));
    BNS_RC(pack_reads(ctx, (const char *)ctx->st_bases.p, (const u64 *)ctx->st_offsets.p, n_seqs, total, st));
    BNS_RC(dust_mark(ctx, (const u64 *)ctx->words.p, (const u32 *)ctx->nmask.p, (const u64 *)ctx->st_offsets.p, n_seqs, DustSpan{0, total}, st));
    HIPCHK(ctx, hipMemcpyAsync(flags, ctx->dust_flags.p, n_words * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return BNS_OK;
}

}  // namespace
