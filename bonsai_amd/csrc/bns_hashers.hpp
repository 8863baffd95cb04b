// bns_hashers.hpp -- the hash feeders behind bns_rolling_hash[128][_windowed]_batch, bns_for_each_hash_batch and the three table makers
// (gfx950, wave64; SURVEY 8 rows a11, a+ and f4).  None of them is on the classify path.
//
//   rolling_hash_kernel<W>   RollingHasher<W, CyclicHash<W>> without a window (encoder.h:644-865, rollinghash/cyclichash.h), W = u64 or
//                            W128 (the instantiation test/encoding.cpp:152 constructs):
//                              forward   H_j = rotl1(H_{j-1}) ^ rotl_k(T[s_{j-k}]) ^ T[s_j]
//                              reverse   R_j = rotr1(R_{j-1} ^ rotl_k(Trc[rc s_j]) ^ Trc[rc s_{j-k}])      (canonical path: min(H, R))
//                            Start values per segment (a segment = the run of valid characters the reference restarts on, k + 1 characters
//                            after an invalid one): a k-term XOR for H and, for R, the reference's fill that eats the window's LAST base's
//                            complement k times (encoder.h:721).
//   nthash_kernel            Encoder::for_each_hash (encoder.h:355-394): ntHash of every k-window the reference's loop visits.  The loop, in
//                            closed form: for every maximal run [a, b) of A/C/G/T (either case; a NUL byte ends the string,
//                            encoder.h:371-377) with b - a >= k, the windows a .. b-k in order -- except that a run whose FIRST window ends
//                            exactly at the end of the string emits nothing (`if(*p2 == 0) return;` is tested before `p2 - p == k`,
//                            encoder.h:378-379).  NTC64 (bcgsc/ntHash, un-vendored: restated from the published definition, Mohamadi et
//                            al. 2016, as ntHash 1.0.x ships it):
//                              forward  fh(w) = XOR_j rol^{k-1-j}(T[s_j])      rolling  fh' = rol1(fh) ^ rol^k(T[out]) ^ T[in]
//                              reverse  rh(w) = XOR_j rol^{j}(T[s_j & 7])      rolling  rh' = ror1(rh ^ T[out & 7] ^ rol^k(T[in & 7]))
//                            (the complement's seed sits at index c & 7 of the same table: A&7 = 1 holds T's seed, C&7 = 3 G's, G&7 = 7
//                            C's, T&7 = 4 A's -- the geometry make_nthash_lut builds in-tree, encoder.h:93-103); canonical = min(fh, rh).
//   stream_window_kernel<W>  QueueMap over a finished stream (qmap.h:79-87 as RollingHasher uses it, encoder.h:706-710,771-776,735-736,
//                            794-795): window i = entries i .. i+ws-1 of sequence q's stream, its value the entry with the smallest
//                            (score(v), v); a value of all ones (ENCODE_OVERFLOW) is not emitted; a stream shorter than the window gives
//                            one value, its minimum, whatever it is.
//
// All three recurrences are linear over GF(2) up to a rotation, so rotating position x's term by -x (forward) / +(x-1) (reverse) turns them
// into plain prefix XORs: one wavefront per sequence scans 64 positions per step (xor_roll).  Rolling indexes a window by its last base,
// ntHash by its first; the rotations are the same expressions.  nthash_kernel shares the word operations and the start values but spells
// the scan out: through xor_roll it took two VGPRs more.  The character tables are arguments (parity unpinned).
//
// Included by bns_api.hip after bns_kernels.hip (base_code) and its helpers (fail, ensure, grid_for): the host half below uses them.
#pragma once
#include "bns_device.hpp"
#include "bns_kernels.hpp"

namespace bns {

struct W128 { u64 lo, hi; };
__device__ __forceinline__ W128 operator^(W128 a, W128 b) { return W128{a.lo ^ b.lo, a.hi ^ b.hi}; }

__device__ __forceinline__ u64 shfl_xor64(u64 v, int off) { return ((u64)(u32)__shfl_xor((int)(u32)(v >> 32), off) << 32) | (u32)__shfl_xor((int)(u32)v, off); }
__device__ __forceinline__ u64 shfl_up64(u64 v, int off) { return ((u64)(u32)__shfl_up((int)(u32)(v >> 32), off) << 32) | (u32)__shfl_up((int)(u32)v, off); }
__device__ __forceinline__ u64 bcast63(u64 v)
{
    return ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(v >> 32), 63) << 32) | (u32)__builtin_amdgcn_readlane((int)(u32)v, 63);
}

// What the recurrences and the queue do with a word.  A rotation count is reduced mod the word's bits here, so callers pass positions
// as they are (their low 32 bits: 2^32 is a multiple of both widths).  A 128-bit value or table entry is a (lo, hi) pair of u64.
template <class W> struct Word;
template <> struct Word<u64> {
    static constexpr u32 WORDS = 1;                                        // u64 per value and per table entry
    static __device__ __forceinline__ u64 zero() { return 0; }
    static __device__ __forceinline__ u64 ones() { return ~0ULL; }
    static __device__ __forceinline__ u64 rotl(u64 x, u32 r) { r &= 63u; return r ? (x << r) | (x >> (64u - r)) : x; }
    static __device__ __forceinline__ u64 rotr(u64 x, u32 r) { r &= 63u; return r ? (x >> r) | (x << (64u - r)) : x; }
    static __device__ __forceinline__ bool less(u64 a, u64 b) { return a < b; }
    static __device__ __forceinline__ bool is_ones(u64 a) { return a == ~0ULL; }
    static __device__ __forceinline__ u64 load(const u64 *t, u64 i) { return t[i]; }
    static __device__ __forceinline__ void store(u64 *o, u64 at, u64 v) { o[at] = v; }
    static __device__ __forceinline__ u64 shfl_xor(u64 v, int off) { return shfl_xor64(v, off); }
    static __device__ __forceinline__ u64 shfl_up(u64 v, int off) { return shfl_up64(v, off); }
    static __device__ __forceinline__ u64 last_lane(u64 v) { return bcast63(v); }
    static __device__ __forceinline__ u64 score(u64 v) { return kmer_score(v, 0); }       // lex_score
};
template <> struct Word<W128> {
    static constexpr u32 WORDS = 2;
    static __device__ __forceinline__ W128 zero() { return W128{0, 0}; }
    static __device__ __forceinline__ W128 ones() { return W128{~0ULL, ~0ULL}; }
    static __device__ __forceinline__ W128 rotl(W128 x, u32 r)
    {
        r &= 127u;
        if (r >= 64u) { const u64 t = x.lo; x.lo = x.hi; x.hi = t; r -= 64u; }
        if (r == 0u) return x;
        return W128{(x.lo << r) | (x.hi >> (64u - r)), (x.hi << r) | (x.lo >> (64u - r))};
    }
    static __device__ __forceinline__ W128 rotr(W128 x, u32 r) { return rotl(x, 128u - (r & 127u)); }
    static __device__ __forceinline__ bool less(W128 a, W128 b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
    static __device__ __forceinline__ bool is_ones(W128 a) { return a.lo == ~0ULL && a.hi == ~0ULL; }
    static __device__ __forceinline__ W128 load(const u64 *t, u64 i) { return W128{t[2 * i], t[2 * i + 1]}; }
    static __device__ __forceinline__ void store(u64 *o, u64 at, W128 v) { o[2 * at] = v.lo; o[2 * at + 1] = v.hi; }
    static __device__ __forceinline__ W128 shfl_xor(W128 v, int off) { return W128{shfl_xor64(v.lo, off), shfl_xor64(v.hi, off)}; }
    static __device__ __forceinline__ W128 shfl_up(W128 v, int off) { return W128{shfl_up64(v.lo, off), shfl_up64(v.hi, off)}; }
    static __device__ __forceinline__ W128 last_lane(W128 v) { return W128{bcast63(v.lo), bcast63(v.hi)}; }
    // the reference's is sketch's CEHasher, un-vendored: restated, parity unpinned -- the number of values, which is what
    // test/encoding.cpp:152-156 pins, does not depend on it
    static __device__ __forceinline__ u64 score(W128 v) { return kmer_score(v.lo ^ kmer_score(v.hi, 0), 0); }
};

template <class W> __device__ __forceinline__ W wave_xor_scan(W v)     // inclusive prefix XOR over the wavefront
{
    const int lane = lane_id();
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const W t = Word<W>::shfl_up(v, off);
        if (lane >= off) v = v ^ t;
    }
    return v;
}
template <class W> __device__ __forceinline__ W wave_xor_all(W v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v ^ Word<W>::shfl_xor(v, off);
    return v;
}

// Start values of a run of k characters: F = XOR_t rotl^{k-1-t}(f_t), R = XOR_t rotl^{t}(r_t), sym(t, f, r) giving character t's two terms.
template <class W, class Sym>
__device__ __forceinline__ void start_values(u32 k, Sym sym, W &F, W &R)
{
    using X = Word<W>;
    F = X::zero(); R = X::zero();
    for (u32 t = threadIdx.x & 63u; t < k; t += 64) {
        W f, r;
        sym(t, f, r);
        F = F ^ X::rotl(f, k - 1u - t);
        R = R ^ X::rotl(r, t);
    }
    F = wave_xor_all(F); R = wave_xor_all(R);
}

// The scan.  F, R are the values at index x0; emit(x, forward, reverse) is called by position x's lane for x0 < x < end.  term(x, f, r)
// gives x's unrotated terms, so that  forward_x = rotl1(forward_{x-1}) ^ f  and  reverse_x = rotr1(reverse_{x-1} ^ r).  rev = false (the
// caller is not canonical): term leaves r alone and emit's reverse means nothing.
// Normalised running values: P = rotr^{x}(forward_x), Q = rotl^{x}(reverse_x); lane 63's carry over into the next 64 positions.
template <class W, class Term, class Emit>
__device__ __forceinline__ void xor_roll(W F, W R, u64 x0, u64 end, bool rev, Term term, Emit emit)
{
    using X = Word<W>;
    const u32 lane = threadIdx.x & 63u;
    W P = X::rotr(F, (u32)x0), Q = X::rotl(R, (u32)x0);
    for (u64 c0 = x0 + 1; c0 < end; c0 += 64) {
        const u64 x = c0 + lane;
        W ef = X::zero(), er = X::zero();
        if (x < end) {
            term(x, ef, er);
            ef = X::rotr(ef, (u32)x);
            if (rev) er = X::rotl(er, (u32)(x - 1));
        }
        const W pf = P ^ wave_xor_scan(ef), qr = Q ^ wave_xor_scan(er);
        if (x < end) emit(x, X::rotl(pf, (u32)x), X::rotr(qr, (u32)x));
        P = X::last_lane(pf); Q = X::last_lane(qr);
    }
}

// raw (the input of stream_window_kernel): the canonical path stores BOTH strands' values, forward then reverse, two entries per
// position (what the windowed RollingHasher queues one after the other, encoder.h:724-725,730-731) instead of their minimum; n_out
// counts entries.  tf, tr: 256 entries each.
template <class W>
__global__ __launch_bounds__(256) void rolling_hash_kernel(const u8 *__restrict__ bases, const u64 *__restrict__ offsets, u64 n_seqs,
                                                           u32 k, int canon, int raw, const u64 *__restrict__ tf, const u64 *__restrict__ tr,
                                                           u64 *__restrict__ out, u32 *__restrict__ n_out)
{
    using X = Word<W>;
    const u32 lane = threadIdx.x & 63u;
    const u64 n_waves = (u64)gridDim.x * 4;
    const bool both = raw && canon;
    const u64 per = both ? 2 : 1;
    for (u64 q = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); q < n_seqs; q += n_waves) {
        const u8 *s = bases + offsets[q];
        const u64 l = offsets[q + 1] - offsets[q];
        u64 *o = out + X::WORDS * per * offsets[q];
        u64 n = 0;                                                       // positions emitted so far (wave-uniform)
        auto code_at = [&](u64 i, u32 &bad) -> u32 { return base_code(s[i], bad); };
        auto put = [&](u64 at, W h, W g) {
            if (both) { X::store(o, 2 * at, h); X::store(o, 2 * at + 1, g); }
            else X::store(o, at, canon ? (X::less(h, g) ? h : g) : h);
        };
        u64 r = 0;                                                       // segment start
        while (l >= k && r + k <= l) {
            // first invalid character at or after r
            u64 inv = l;
            for (u64 c0 = r; c0 < l && inv == l; c0 += 64) {
                u32 bad = 0;
                if (c0 + lane < l) (void)code_at(c0 + lane, bad);
                const u64 m = __builtin_amdgcn_ballot_w64(bad != 0);
                if (m) inv = c0 + (u64)__builtin_ctzll(m);
            }
            if (inv >= r + k) {                                          // the fill completes: values for j = r+k-1 .. inv-1
                const u64 j0 = r + k - 1;
                // H_{j0} = XOR_t rotl^{k-1-t}(T[s_{r+t}]);  R_{j0} = XOR_t rotl^{t}(Trc[rc s_{j0}])
                u32 bad;
                const W tlast = canon ? X::load(tr, 3u - code_at(j0, bad)) : X::zero();
                W h0, g0;
                start_values(k, [&](u32 t, W &f, W &g) { f = X::load(tf, code_at(r + t, bad)); g = tlast; }, h0, g0);
                if (lane == 0) put(n, h0, g0);
                xor_roll(h0, g0, j0, inv, canon != 0,
                         [&](u64 j, W &f, W &g) {
                             const u32 cin = code_at(j, bad), cout = code_at(j - k, bad);
                             f = X::rotl(X::load(tf, cout), k) ^ X::load(tf, cin);
                             if (canon) g = X::rotl(X::load(tr, 3u - cin), k) ^ X::load(tr, 3u - cout);
                         },
                         [&](u64 j, W h, W g) { put(n + (j - j0), h, g); });
                n += inv - j0;
            }
            if (inv >= l) break;
            if (canon && inv + 2 * (u64)k >= l) break;                   // encoder.h:714
            r = inv + (u64)k + 1;                                        // i += k_, then the loop's ++i
        }
        if (lane == 0) n_out[q] = (u32)(per * n);
    }
}

__global__ __launch_bounds__(256) void nthash_kernel(const u8 *__restrict__ bases, const u64 *__restrict__ offsets, u64 n_seqs,
                                                     u32 k, int canon, const u64 *__restrict__ T, u64 *__restrict__ out, u32 *__restrict__ n_out)
{
    using X = Word<u64>;
    const u32 lane = threadIdx.x & 63u;
    const u64 n_waves = (u64)gridDim.x * 4;
    for (u64 q = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); q < n_seqs; q += n_waves) {
        const u8 *s = bases + offsets[q];
        u64 l = offsets[q + 1] - offsets[q];
        u64 *o = out + offsets[q];
        u64 n = 0;
        auto invalid = [&](u64 i) -> bool { u32 bad; (void)base_code(s[i], bad); return bad != 0; };
        auto put = [&](u64 at, u64 f, u64 r) { o[at] = canon ? (r < f ? r : f) : f; };
        u64 a = 0;                                                       // scan position
        while (a + k <= l) {
            // first valid character at or after a (a NUL ends the string), then the end of its run
            u64 b = l;
            bool found_start = false;
            for (u64 c0 = a; c0 < l; c0 += 64) {
                const bool in = c0 + lane < l;
                const u8 ch = in ? s[c0 + lane] : (u8)1;
                const u64 nul = __builtin_amdgcn_ballot_w64(in && ch == 0);
                u64 inv = __builtin_amdgcn_ballot_w64(in && invalid(c0 + lane));
                if (nul) { const int z = __builtin_ctzll(nul); l = c0 + (u64)z; inv &= (1ULL << z) - 1ULL; }
                const u64 within = (l - c0 >= 64) ? ~0ULL : ((1ULL << (l - c0)) - 1ULL);
                if (!found_start) {
                    const u64 ok = ~inv & within;
                    if (!ok) { if (nul) break; continue; }
                    const int f = __builtin_ctzll(ok);
                    a = c0 + (u64)f; found_start = true;
                    inv &= ~((2ULL << f) - 1ULL);                        // invalid characters after the start only
                }
                if (inv & within) { b = c0 + (u64)__builtin_ctzll(inv & within); break; }
                if (nul) break;
            }
            if (!found_start) break;
            if (b > l) b = l;
            if (b - a >= (u64)k && !(a + k == l)) {
                u64 fh, rh;
                start_values(k, [&](u32 t, u64 &f, u64 &r) { const u8 ch = s[a + t]; f = T[ch]; r = T[ch & 7u]; }, fh, rh);
                if (lane == 0) put(n, fh, rh);
                // xor_roll's scan, spelled out: through xor_roll this kernel takes 70 VGPRs for 68 (72 with the reverse strand always on)
                u64 P = X::rotr(fh, (u32)a), Q = X::rotl(rh, (u32)a);
                const u64 last = b - k;                                  // last window of the run
                for (u64 c0 = a + 1; c0 <= last; c0 += 64) {
                    const u64 i = c0 + lane;
                    u64 ef = 0, er = 0;
                    if (i <= last) {
                        const u8 cout = s[i - 1], cin = s[i + k - 1];
                        ef = X::rotr(X::rotl(T[cout], k) ^ T[cin], (u32)i);
                        er = X::rotl(T[cout & 7u] ^ X::rotl(T[cin & 7u], k), (u32)(i - 1));
                    }
                    const u64 pf = P ^ wave_xor_scan(ef), qr = Q ^ wave_xor_scan(er);
                    if (i <= last) put(n + (i - a), X::rotl(pf, (u32)i), X::rotr(qr, (u32)i));
                    P = X::last_lane(pf); Q = X::last_lane(qr);
                }
                n += last - a + 1;
            }
            if (b >= l) break;
            a = b + 1;
        }
        if (lane == 0) n_out[q] = (u32)n;
    }
}

// `per` = entries per base the stream buffers are laid out with (sequence q starts at per * offsets[q]).  One wavefront per sequence.
// (score, value) is a total order and equal pairs are equal values, so the short stream's reduction order cannot show.
template <class W>
__global__ __launch_bounds__(256) void stream_window_kernel(const u64 *__restrict__ in, const u32 *__restrict__ n_in, const u64 *__restrict__ offsets,
                                                            u64 n_seqs, u32 per, u32 ws, u64 *__restrict__ out, u32 *__restrict__ n_out)
{
    using X = Word<W>;
    const u32 lane = threadIdx.x & 63u;
    const u64 n_waves = (u64)gridDim.x * 4;
    for (u64 q = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); q < n_seqs; q += n_waves) {
        const u64 *v = in + (u64)X::WORDS * per * offsets[q];
        u64 *o = out + (u64)X::WORDS * per * offsets[q];
        const u32 n = n_in[q];
        u32 emitted = 0;
        // (by reference: with W by value the 64-bit kernel's inner loop loses a fused or-xor of the score, 1 % of its time)
        auto less = [](u64 sa, const W &a, u64 sb, const W &b) { return sa < sb || (sa == sb && X::less(a, b)); };
        if (n >= ws) {
            const u32 nw = n - ws + 1u;
            for (u32 i0 = 0; i0 < nw; i0 += 64u) {
                const u32 i = i0 + lane;
                W be = X::ones();
                u64 bs = ~0ULL;
                if (i < nw) {
                    be = X::load(v, i); bs = X::score(be);
                    for (u32 j = 1; j < ws; ++j) {
                        const W e = X::load(v, i + j);
                        const u64 sc = X::score(e);
                        if (less(sc, e, bs, be)) { bs = sc; be = e; }
                    }
                }
                const bool on = i < nw && !X::is_ones(be);
                const u64 vm = ballot64(on);
                if (on) X::store(o, emitted + (u32)__popcll(vm & lanemask_lt()), be);
                emitted += (u32)__popcll(vm);
            }
        } else if (n) {
            W be = X::ones();
            u64 bs = ~0ULL;
            bool have = false;
            for (u32 i = lane; i < n; i += 64u) {
                const W e = X::load(v, i);
                const u64 sc = X::score(e);
                if (!have || less(sc, e, bs, be)) { bs = sc; be = e; have = true; }
            }
            for (int off = 32; off >= 1; off >>= 1) {
                const W oe = X::shfl_xor(be, off);
                const u64 os = shfl_xor64(bs, off);
                const bool oh = __shfl_xor((int)have, off) != 0;
                if (oh && (!have || less(os, oe, bs, be))) { bs = os; be = oe; have = true; }
            }
            if (lane == 0) X::store(o, 0, be);                 // (max_in_queue().el_ is emitted as is, even all ones)
            emitted = 1;
        }
        if (lane == 0) n_out[q] = emitted;
    }
}

}  // namespace bns

namespace {

// A host batch of sequences goes to the context's staging buffers (st_bases, st_offsets) on ctx->stream; n >= 1.  Callers size their
// other buffers first, so that no buffer is re-allocated behind a copy.
int stage_batch(bns_ctx *ctx, const char *bases, const u64 *offsets, u64 n)
{
    const u64 total = offsets[n];
    BNS_RC(ensure(ctx, ctx->st_bases, (size_t)total + 8));
    BNS_RC(ensure(ctx, ctx->st_offsets, (size_t)(n + 1) * 8));
    if (total) HIPCHK(ctx, hipMemcpyAsync(ctx->st_bases.p, bases, (size_t)total, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(ctx->st_offsets.p, offsets, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    return BNS_OK;
}

// ... and the values (when the caller wants them and there are any) and the n per-sequence counts come back; the call's one sync
int fetch_values(bns_ctx *ctx, void *vals, const void *d_vals, size_t val_bytes, u32 *cnt, const void *d_cnt, u64 n)
{
    if (vals && val_bytes) HIPCHK(ctx, hipMemcpyAsync(vals, d_vals, val_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(cnt, d_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BNS_OK;
}

// wy::WyRand stand-in for the default character tables: Lemire's wyhash64 (state += 0x60bee2bee120fc15, two 64x64->128
// multiply folds), seeded as encoder.h:682-683 seeds the two hashers.  PARITY UNPINNED: pass real tables instead.
u64 wyhash64_next(u64 &state)
{
    state += 0x60bee2bee120fc15ULL;
    unsigned __int128 t = (unsigned __int128)state * 0xa3b195354a39b70dULL;
    const u64 m1 = (u64)(t >> 64) ^ (u64)t;
    t = (unsigned __int128)m1 * 0x1b03738712fad5c9ULL;
    return (u64)(t >> 64) ^ (u64)t;
}

// CharacterHash<W>'s default tables, one draw per u64 of an entry.  Of a 128-bit entry's two draws only the second survives (its 128-bit
// mask is truncated to 64 bits on the way into the uint64_t member maxval_, characterhash.h:82-97): hi = 0 in every entry.
template <class W>
int rolling_tables(u64 seed1, u64 seed2, u64 *fwd, u64 *rc)
{
    constexpr u32 N = Word<W>::WORDS;
    if (!fwd || !rc) return BNS_ERR_ARG;
    u64 state[2] = {(u32)(seed1 ^ seed2), (u32)((seed2 * seed1) ^ (seed2 ^ seed1))};
    u64 *const tab[2] = {fwd, rc};
    for (int s = 0; s < 2; ++s)
        for (u32 i = 0; i < 256; ++i)
            for (u32 d = N; d-- > 0;) { const u64 v = wyhash64_next(state[s]); tab[s][N * i + d] = d ? 0 : v; }
    return BNS_OK;
}

// make_nthash_lut's geometry (encoder.h:93-103): the base's seed at the letter (both cases), its complement's seed at
// index (letter & 7), everything else 0.
int nthash_tables(u64 seed_a, u64 seed_c, u64 seed_g, u64 seed_t, u64 *table256)
{
    if (!table256) return BNS_ERR_ARG;
    std::memset(table256, 0, 256 * sizeof(u64));
    table256[4] = table256['a'] = table256['A'] = seed_a;      // 'T' & 7 == 4: T's complement
    table256[7] = table256['c'] = table256['C'] = seed_c;      // 'G' & 7 == 7
    table256[3] = table256['g'] = table256['G'] = seed_g;      // 'C' & 7 == 3
    table256[1] = table256['t'] = table256['T'] = seed_t;      // 'A' & 7 == 1
    return BNS_OK;
}

// bns_rolling_hash[128]_windowed_batch: the stream of values, then (w > k) its window minimizers.  Buffers hold `per` entries a base.
template <class W>
int rolling_batch(bns_ctx *ctx, const char *bases, const u64 *offsets, u64 n_seqs, u32 k, int canon, u32 w, const u64 *fwd_table,
                  const u64 *rc_table, u64 *hashes, u32 *n_hashes)
{
    constexpr size_t TAB = 256 * Word<W>::WORDS, VAL = 8 * Word<W>::WORDS;   // u64 of a table, bytes of a value
    if (!ctx || !offsets || !n_hashes) return BNS_ERR_ARG;
    const bool windowed = w > k;                                          // RollingHasher::window(): w <= k_ means none (encoder.h:664-665)
    const u32 per = (windowed && canon) ? 2u : 1u;                        // entries per base the buffers are laid out with
    if (k == 0) return fail(ctx, BNS_ERR_ARG, "k must be positive");
    if ((fwd_table == nullptr) != (rc_table == nullptr)) return fail(ctx, BNS_ERR_ARG, "pass both character tables or neither");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n_seqs == 0) return BNS_OK;
    const size_t val_bytes = (size_t)offsets[n_seqs] * VAL * per;
    u64 tabs[2 * TAB];
    if (fwd_table) { std::memcpy(tabs, fwd_table, TAB * 8); std::memcpy(tabs + TAB, rc_table, TAB * 8); }
    else rolling_tables<W>(1337, 137, tabs, tabs + TAB);                  // RollingHasher's default seeds (encoder.h:673)
    BNS_RC(ensure(ctx, ctx->st_kmers, val_bytes + VAL));
    BNS_RC(ensure(ctx, ctx->st_out[0], (size_t)n_seqs * 4));
    BNS_RC(ensure(ctx, ctx->st_aux, sizeof(tabs)));
    if (windowed) {
        BNS_RC(ensure(ctx, ctx->st_hits, val_bytes + VAL));
        BNS_RC(ensure(ctx, ctx->st_out[1], (size_t)n_seqs * 4));
    }
    BNS_RC(stage_batch(ctx, bases, offsets, n_seqs));
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(ctx->st_aux.p, tabs, sizeof(tabs), hipMemcpyHostToDevice, st));
    const unsigned grid = grid_for(ctx, n_seqs, 4);
    hipLaunchKernelGGL(rolling_hash_kernel<W>, dim3(grid), dim3(256), 0, st, (const u8 *)ctx->st_bases.p, (const u64 *)ctx->st_offsets.p,
                       (u64)n_seqs, k, canon ? 1 : 0, windowed ? 1 : 0, (const u64 *)ctx->st_aux.p, (const u64 *)ctx->st_aux.p + TAB,
                       (u64 *)ctx->st_kmers.p, (u32 *)ctx->st_out[0].p);
    HIPCHK(ctx, hipGetLastError());
    if (!windowed) return fetch_values(ctx, hashes, ctx->st_kmers.p, val_bytes, n_hashes, ctx->st_out[0].p, n_seqs);
    hipLaunchKernelGGL(stream_window_kernel<W>, dim3(grid), dim3(256), 0, st, (const u64 *)ctx->st_kmers.p, (const u32 *)ctx->st_out[0].p,
                       (const u64 *)ctx->st_offsets.p, (u64)n_seqs, per, (u32)(w - k + 1), (u64 *)ctx->st_hits.p, (u32 *)ctx->st_out[1].p);
    HIPCHK(ctx, hipGetLastError());
    return fetch_values(ctx, hashes, ctx->st_hits.p, val_bytes, n_hashes, ctx->st_out[1].p, n_seqs);
}

int nthash_batch(bns_ctx *ctx, const char *bases, const u64 *offsets, u64 n_seqs, u32 k, int canon, const u64 *table256, u64 *hashes,
                 u32 *n_hashes)
{
    if (!ctx || !offsets || !n_hashes) return BNS_ERR_ARG;
    if (k == 0) {                                             // encoder.h:357,362: k = 0 means the Spacer's k
        if (!ctx->enc_set) return fail(ctx, BNS_ERR_STATE, "k = 0 takes the encoder's k: configure the encoder first (bns_set_encoder)");
        k = ctx->k;
    }
    if (ctx->enc_set && ctx->spaced) return fail(ctx, BNS_ERR_ARG, "Can't for_each_hash for a spaced spacer");       // encoder.h:364
    if (ctx->enc_set && ctx->win > ctx->c) return fail(ctx, BNS_ERR_ARG, "Can't for_each_hash for a windowed spacer"); // encoder.h:363
    if (canon < 0) canon = (ctx->enc_set && ctx->canon) ? 1 : 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n_seqs == 0) return BNS_OK;
    const size_t val_bytes = (size_t)offsets[n_seqs] * 8;
    u64 tab[256];
    if (table256) std::memcpy(tab, table256, sizeof(tab));
    else nthash_tables(0x3c8bfbb395c60474ULL, 0x3193c18562a02b4cULL, 0x20323ed082572324ULL, 0x295549f54be24456ULL, tab);   // ntHash's published seeds
    BNS_RC(ensure(ctx, ctx->st_kmers, val_bytes + 8));
    BNS_RC(ensure(ctx, ctx->st_out[0], (size_t)n_seqs * 4));
    BNS_RC(ensure(ctx, ctx->st_aux, sizeof(tab)));
    BNS_RC(stage_batch(ctx, bases, offsets, n_seqs));
    HIPCHK(ctx, hipMemcpyAsync(ctx->st_aux.p, tab, sizeof(tab), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(nthash_kernel, dim3(grid_for(ctx, n_seqs, 4)), dim3(256), 0, ctx->stream, (const u8 *)ctx->st_bases.p,
                       (const u64 *)ctx->st_offsets.p, (u64)n_seqs, k, canon ? 1 : 0, (const u64 *)ctx->st_aux.p, (u64 *)ctx->st_kmers.p,
                       (u32 *)ctx->st_out[0].p);
    HIPCHK(ctx, hipGetLastError());
    return fetch_values(ctx, hashes, ctx->st_kmers.p, val_bytes, n_hashes, ctx->st_out[0].p, n_seqs);
}

}  // namespace
