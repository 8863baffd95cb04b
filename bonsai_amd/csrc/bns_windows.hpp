// bns_windows.hpp -- the window session behind bns_windows_begin / _add / _read / _end (gfx950, wave64).
//
// Every window of L bases of every sequence of a batch gets the taxon bns_classify_batch would give that substring as a single
// unpaired read, and the pairs (taxid of the sequence, call) are counted.  resolve_tree's result is a function of the multiset of a
// unit's hits, so a window's call is a function of the lookup results of the k-mers inside it: each k-mer of the batch is looked up
// ONCE, and a window is a range of the results.
//
//   windows_pack_kernel    pack_kernel's 2-bit image of the batch, a wavefront per 2048 bases of it instead of one per sequence.
//   windows_lookup_kernel  one wavefront per piece of WIN_LOOKUP_BASES(c) consecutive bases of the batch (not per sequence: a batch is
//                          a handful of multi-megabase contigs).  A piece walks the sequences it touches as sketch_kernel walks a
//                          unit -- the packed image in registers, rounds of 64 k-mers, the same probe functions and minimizer-identity
//                          dispatch -- and writes a positional stream indexed by the k-mer's first base: vals[pos] (the table value of a
//                          hit; 0 is a legal one) and, out of band, cls[pos] = 2 hit / 1 looked up and missing / 0 not a k-mer.
//   windows_vote_kernel    one wavefront per tile of WIN_TILE consecutive bases of the batch = the window starts among them, sequence by
//                          sequence.  The tile's part of the stream plus its halo of L - c entries is staged in LDS once: a bitmap of
//                          the hits with a running count per 64 positions, and the compacted list of the hit values.  Window p then IS
//                          the range [rank(p), rank(p + L - c + 1)) of that list, two prefix counts.  Consecutive windows with the same
//                          range are one vote (against a db of window minimizers a 150-base window holds a handful of hits, and the
//                          range moves every twenty-odd starts).  A vote counts the range's taxa in position order -- classify's
//                          insertion order -- into the register counter and resolves it with resolve_regs; past WIN_FAST_TAXA distinct
//                          taxa the counter continues in global memory (counter_insert) and resolve_wave resolves it: classify's own
//                          device code on both paths, so ties fold exactly as there.
//                          Pair counts: the lanes of a step that carry the same call are counted with a ballot, equal calls of
//                          consecutive steps are added up in scalars, and one atomicAdd of the sum goes to the pair table when the call
//                          changes or the sequence's part of the tile ends.
//                          CONF (a session opened by bns_windows_begin_conf with theta > 0): a second bitmap with running counts, of the
//                          looked-up-and-missing k-mers, is staged beside the hits', so a window's Q = hits + missing is two more prefix
//                          counts.  Two consecutive windows are one vote only when the hit range AND Q are equal (an N entering or leaving
//                          among missing k-mers changes Q and nothing else), and a vote's call then walks up as confidence_kernel's does:
//                          the first of T, parent(T), ... whose clade holds ceil(theta Q) of the hits hl[lo, hi), by Euler interval.
//
// The pair table: open addressing, linear probing, key = taxid << 32 | call claimed with a compare-and-swap, EMPTY = ~0 (taxid
// 0xFFFFFFFF is BNS_TAX_ABSENT, no sequence's taxon: such a pair with call 0xFFFFFFFF counts as dropped).  A pair that meets no free
// slot within the table's length adds its windows to `dropped`, so stored counts are exact and nothing is lost from the total.
//
// Included by bns_api.hip after its helpers (fail, ensure, grid_for, ready, dispatch_sp_layout) and bns_classify.hpp (fill_params).
#pragma once
#include "bns_device.hpp"
#include "bns_kernels.hpp"
#include "bns_confidence.hpp"

namespace bns {

constexpr u32 WIN_TILE = 256;                       // bases (window starts) per tile of the vote pass
constexpr u32 WIN_FAST_TAXA = 64;                   // distinct taxa of a window the register counter and resolve_regs hold
constexpr u32 WIN_NONE = 0xFFFFFFFFu;               // d_taxon of a base that starts no window
constexpr u64 WIN_PAIR_EMPTY = ~0ULL;
constexpr u32 WIN_CLS_MISSING = 1, WIN_CLS_HIT = 2;
constexpr u32 WIN_LDS_LIST_MAX = 11264;             // entries of a tile + halo whose hit list is staged in LDS (45 KiB); longer: global
constexpr u32 WIN_CONF_CACHED = 2;                  // blocks of 64 hits whose tin stays in registers across the steps of a window's walk
// k-mer starts a lookup piece owns.  A piece starts anywhere in a sequence and reads the packed image from the 32-base word in front of
// it: up to 31 k-mers it does not own, the ones it owns, c - 1 more bases -- within the 2048 bases one register image holds.
__host__ __device__ constexpr u32 win_rounds_per_chunk(u32 c) { return (2048u - (c - 1u)) / 64u; }
__host__ __device__ constexpr u32 win_lookup_bases(u32 c) { return (win_rounds_per_chunk(c) - 1u) * 64u; }

struct WindowParams {
    const u64 *offsets;
    u64 n_seqs, total_bases;
    const u32 *taxid;
    u32 *vals;                   // the positional stream
    u8 *cls;
    u32 *taxon;                  // the caller's d_taxon, or null
    u32 L;                       // window length
    u64 *pair_keys, *pair_counts;
    u64 pair_mask;
    unsigned long long *dropped;
    u32 *scratch;                // vote pass, per workgroup: keys, counts, tin, tout of the counter past the registers [+ the hit list]
    u64 scratch_stride;          // u32 per workgroup
    u32 counter_cap;             // entries of each of the four counter arrays
    u32 list_cap;                // entries of the staged hit list (tile + halo)
};

// the sequence that holds base g of the batch (g < total_bases): the last one that starts at or before it
__device__ __forceinline__ u64 win_seq_of(const u64 *__restrict__ offsets, u64 n_seqs, u64 g)
{
    u64 lo = 0, hi = n_seqs;                         // offsets[lo] <= g < offsets[hi]
    while (hi - lo > 1) {
        const u64 mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// pack_kernel's image (words[(o >> 5) + s + i] = bases 32 i .. of sequence s, nmask beside it) with a wavefront per piece of 2048 bases
// of the BATCH instead of one per sequence, which walks a multi-megabase contig 256 bases at a time on its own (7.3 of a session's
// 14.5 ms on 64 x 2.6 Mb).  A piece packs the 256-base blocks of its sequences that START inside it; the conversion is pack_kernel's.
__global__ __launch_bounds__(256) void windows_pack_kernel(const u8 *__restrict__ bases, const u64 *__restrict__ offsets, u64 n_seqs,
                                                           u64 total_bases, u64 *__restrict__ words, u32 *__restrict__ nmask)
{
    const int lane = lane_id();
    const u64 wave = (u64)blockIdx.x * 4 + (u64)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u64 n_waves = (u64)gridDim.x * 4;
    const u64 n_pieces = (total_bases + 2047) >> 11;
    for (u64 g = wave; g < n_pieces; g += n_waves) {
        const u64 g0 = g << 11, g1 = g0 + 2048 < total_bases ? g0 + 2048 : total_bases;
        for (u64 s = win_seq_of(offsets, n_seqs, g0); s < n_seqs; ++s) {
            const u64 o = offsets[s];
            if (o >= g1) break;
            const u64 L = offsets[s + 1] - o;
            const u64 wb = (o >> 5) + s;
            const u64 n_words = (L + 31) >> 5;
            for (u64 p = g0 > o ? (g0 - o + 255) & ~255ULL : 0; o + p < g1 && p < (n_words << 5); p += 256) {
                const u64 bi = p + (u64)lane * 4;                  // first base of this lane
                u32 w = 0;
                if (bi < L) {
                    const u64 addr = o + bi;
                    const u32 mis = (u32)(addr & 3u);
                    const u32 *ap = reinterpret_cast<const u32 *>(bases + (addr - mis));
                    const u32 nbytes = (L - bi) < 4 ? (u32)(L - bi) : 4u;
                    const u32 lo = ap[0];
                    const u32 hi = (mis + nbytes > 4u) ? ap[1] : 0u;
                    w = (u32)((((u64)hi << 32) | lo) >> (8u * mis));
                }
                u32 codes = 0, bads = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    u32 bad;
                    const u32 cd = base_code((w >> (8 * i)) & 0xFFu, bad);
                    if (bi + i >= L) bad = 1u;
                    codes = (codes << 2) | (bad ? 0u : cd);
                    bads = (bads << 1) | bad;
                }
                const int q = lane & 7;                            // position of this lane's 4 bases inside the word
                u32 hi32 = q < 4 ? codes << (24 - 8 * q) : 0u;
                u32 lo32 = q >= 4 ? codes << (24 - 8 * (q - 4)) : 0u;
                u32 nm = bads << (28 - 4 * q);
                hi32 |= dpp<QP_XOR1>(hi32); lo32 |= dpp<QP_XOR1>(lo32); nm |= dpp<QP_XOR1>(nm);
                hi32 |= dpp<QP_XOR2>(hi32); lo32 |= dpp<QP_XOR2>(lo32); nm |= dpp<QP_XOR2>(nm);
                hi32 |= (u32)__shfl_xor((int)hi32, 4); lo32 |= (u32)__shfl_xor((int)lo32, 4); nm |= (u32)__shfl_xor((int)nm, 4);
                const u64 wi = (p >> 5) + (u64)(lane >> 3);
                if (q == 0 && wi < n_words) {
                    words[wb + wi] = ((u64)hi32 << 32) | lo32;
                    nmask[wb + wi] = nm;
                }
            }
        }
    }
}

template <bool SPACED, int LAYOUT, int MIN = 0>
__global__ __launch_bounds__(256) void windows_lookup_kernel(ClassifyParams p, WindowParams wp)
{
    __shared__ __attribute__((aligned(16))) u32 s_aux[4][MINB_AUX_U32];
    const int lane = lane_id();
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u32 rdesc = SPACED ? run_desc(p) : 0u;
    const u32 k = p.k, c = p.c;
    const u64 piece = win_lookup_bases(c);
    const u64 n_pieces = (wp.total_bases + piece - 1) / piece;
    const u64 n_waves = (u64)gridDim.x * 4;
    for (u64 g = (u64)blockIdx.x * 4 + (u64)wv; g < n_pieces; g += n_waves) {
        const u64 g0 = g * piece, g1 = g0 + piece < wp.total_bases ? g0 + piece : wp.total_bases;
        for (u64 s = win_seq_of(wp.offsets, wp.n_seqs, g0); s < wp.n_seqs; ++s) {
            const u64 o = wp.offsets[s];
            if (o >= g1) break;
            const u32 n = (u32)(wp.offsets[s + 1] - o);
            const u32 nk = (n >= c && !(SPACED && p.emit_none)) ? n - c + 1u : 0u;
            const u32 j_lo = g0 > o ? (u32)(g0 - o) : 0u;
            const u32 j_hi = (g1 - o) < (u64)nk ? (u32)(g1 - o) : nk;
            if (j_lo >= j_hi) continue;
            const u32 j0 = j_lo & ~31u;
            const u64 wb = (o >> 5) + s;
            const u32 n_words = (n + 31u) >> 5;
            const u32 wi = (j0 >> 5) + (u32)lane;
            const u64 W = wi < n_words ? p.words[wb + wi] : 0ULL;
            const u32 M = wi < n_words ? (p.nmask ? p.nmask[wb + wi] : 0u) : 0xFFFFFFFFu;
            for (u32 rd = 0; j0 + rd * 64u < j_hi; ++rd) {
                const u32 j = j0 + rd * 64u + (u32)lane;
                const bool mine = j >= j_lo && j < j_hi;
                u64 key;
                bool valid;
                if (SPACED) valid = p.n_runs ? extract_spaced_runs(W, M, rd, p, rdesc, key) : extract_spaced(W, M, rd, k, rdesc, key);
                else        valid = extract_unspaced(W, M, rd, k, key);
                valid = valid && mine;
                if (!SPACED && p.canon) key = canonical(key, k);
                ProbeResult pr;
                if (LAYOUT == 2) {
                    const u32 minh = MIN == 1 ? key_minhash(key, k, MinSpec{p.m, p.min_len, p.min_shift, p.min_canon, 0u})
                                              : (MIN == 2 ? key_minhash<true>(key, k, p.m) : key_minhash<false>(key, k, p.m));
                    pr = probe_minbucket<true, 16, false, false>(p.minb, key, bucket_of(minh, p.n_mb), valid, s_aux[wv], p.slots, p.ovf_mask);
                }
                else if (LAYOUT == 1) pr = probe_bucket(p.slots, p.bucket_mask, key, valid);
                else                  pr = probe_khash(p.kflags, p.kkeys, p.kvals, p.kh_nb, key, valid);
                if (mine) {
                    const bool hit = valid && pr.found;
                    wp.cls[o + j] = (u8)(hit ? WIN_CLS_HIT : (valid ? WIN_CLS_MISSING : 0u));
                    if (hit) wp.vals[o + j] = pr.val;
                }
            }
        }
    }
}

// n windows of the pair (taxid, call) into the pair table (one lane calls it)
__device__ __forceinline__ void win_pair_add(const WindowParams &wp, u32 taxid, u32 call, u32 n)
{
    const u64 key = ((u64)taxid << 32) | call;
    if (key != WIN_PAIR_EMPTY) {
        u64 i = wang64(key) & wp.pair_mask;
        for (u64 step = 0; step <= wp.pair_mask; ++step) {
            u64 old = __hip_atomic_load(&wp.pair_keys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old == WIN_PAIR_EMPTY)
                old = atomicCAS((unsigned long long *)&wp.pair_keys[i], (unsigned long long)WIN_PAIR_EMPTY, (unsigned long long)key);
            if (old == WIN_PAIR_EMPTY || old == key) { atomicAdd((unsigned long long *)&wp.pair_counts[i], (unsigned long long)n); return; }
            i = (i + 1) & wp.pair_mask;
        }
    }
    atomicAdd(wp.dropped, (unsigned long long)n);
}

// The call of the hits hl[lo, hi) (wave-uniform), counted in position order.  GL: the hit list is in global memory.
__device__ __forceinline__ u32 win_resolve_range(const u32 *hl, u32 lo, u32 hi, u32 *keys, u32 *cnt, u32 *tin, u32 *tout, u32 cap,
                                                 const TaxNode *__restrict__ nodes, u32 n_nodes)
{
    const u32 lane = (u32)lane_id();
    u32 D = 0, ckey = 0, ccnt = 0;
    u64 dmask = 0;
    for (u32 base = lo; base < hi; base += 64u) {
        const bool in = base + lane < hi;
        const u32 v = in ? hl[base + lane] : 0u;
        const u64 fm = ballot64(in);
        u64 rem = fm;
        while (rem) {                                              // classify_unit's vote of one round
            const int l = __builtin_ctzll(rem);
            const u32 t = readlane(v, l);
            const u64 mm = ballot64(v == t) & fm;
            rem &= ~mm;
            const u32 n = (u32)__popcll(mm);
            const bool eq = ckey == t;
            if (ballot64(eq) & dmask) { ccnt = eq ? ccnt + n : ccnt; continue; }
            (void)counter_insert(ckey, ccnt, dmask, keys, cnt, cap, D, t, n);      // (cap >= the hits of a window: it cannot fill up)
        }
    }
    if (D <= 1u) return D ? readlane(ckey, 0) : 0u;
    if (D <= WIN_FAST_TAXA) return resolve_regs(ckey, ccnt, D, nodes, n_nodes);
    keys[lane] = ckey; cnt[lane] = ccnt;
    __builtin_amdgcn_wave_barrier();
    return resolve_wave(keys, cnt, tin, tout, D, nodes, n_nodes);
}

// The confidence walk of one vote (all arguments wave-uniform): t = the call of the hits hl[lo, hi), need = ceil(theta Q) of the window.
// confidence_kernel's rules on the window's own hits: t stays when need = 0, t = 0 or t is no node whose chain reaches a root; 0 when
// the window has fewer hits than need or the walk passes a root; else the first of t, parent(t), ... whose clade holds need hits.
__device__ __forceinline__ u32 win_confidence(const u32 *hl, u32 lo, u32 hi, u64 need, u32 t, const TaxNode *__restrict__ nodes, u32 n_nodes)
{
    if (need == 0 || t == 0u) return t;
    const TaxNode nt = load_node(nodes, n_nodes, t);
    if (!(nt.flags & NODE_CHAIN_OK)) return t;
    if ((u64)(hi - lo) < need) return 0u;                          // no clade can hold more hits than there are
    const u32 lane = (u32)lane_id();
    u32 ct[WIN_CONF_CACHED];
#pragma unroll
    for (u32 c = 0; c < WIN_CONF_CACHED; ++c) {
        const u32 i = lo + c * 64u + lane;
        ct[c] = i < hi ? load_node(nodes, n_nodes, hl[i]).tin : 0u;
    }
    u32 a = t, tin_a = nt.tin, tout_a = nt.tout, par_a = nt.parent;
    for (u32 step = 0; step < n_nodes; ++step) {                   // (a chain that reaches a root is shorter than the taxonomy)
        u64 cnt = 0;
#pragma unroll
        for (u32 c = 0; c < WIN_CONF_CACHED; ++c) cnt += (u64)__popcll(ballot64(conf_in_clade(ct[c], tin_a, tout_a)));
        for (u32 i0 = lo + WIN_CONF_CACHED * 64u; i0 < hi && cnt < need; i0 += 64u) {
            const u32 i = i0 + lane;
            const u32 th = i < hi ? load_node(nodes, n_nodes, hl[i]).tin : 0u;
            cnt += (u64)__popcll(ballot64(conf_in_clade(th, tin_a, tout_a)));
        }
        if (cnt >= need) return a;
        if (par_a == 0u) return 0u;                                // passed the root: unclassified
        const TaxNode np = load_node(nodes, n_nodes, par_a);
        a = par_a; tin_a = np.tin; tout_a = np.tout; par_a = np.parent;
    }
    return 0u;
}

// hits in front of tile position x: the running count of its 64-position word plus the bits below it
__device__ __forceinline__ u32 win_rank(const u64 *bits, const u32 *wpre, u32 x)
{
    return wpre[x >> 6] + (u32)__popcll(bits[x >> 6] & ((1ULL << (x & 63u)) - 1ULL));
}

// CONF: the session has a threshold theta = num / den > 0 of its own (the form without one is the code it was before there was one)
template <bool GL, bool CONF = false>
__global__ __launch_bounds__(64) void windows_vote_kernel(WindowParams wp, const TaxNode *__restrict__ nodes, u32 n_nodes, u32 c, u64 num, u64 den)
{
    extern __shared__ __attribute__((aligned(16))) u64 s_dyn[];
    const u32 lane = (u32)lane_id();
    const u32 L = wp.L, H = L - c;                                 // a window holds the k-mers at its start .. start + H
    const u32 n_bw = (wp.list_cap >> 6) + 2u;                      // bitmap words: one past the last position's, for rank(np)
    u64 *bits = s_dyn;
    u64 *mbits = s_dyn + n_bw;                                     // CONF: the missing k-mers' bitmap and running counts
    u32 *wpre = reinterpret_cast<u32 *>(s_dyn + (CONF ? 2u : 1u) * n_bw);
    u32 *mpre = wpre + n_bw;
    u32 *scr = wp.scratch + (u64)blockIdx.x * wp.scratch_stride;
    u32 *keys = scr, *cnt = scr + wp.counter_cap, *tin = scr + 2u * (u64)wp.counter_cap, *tout = scr + 3u * (u64)wp.counter_cap;
    u32 *hl = GL ? scr + 4u * (u64)wp.counter_cap : wpre + (CONF ? 2u : 1u) * n_bw;
    const u64 n_tiles = (wp.total_bases + WIN_TILE - 1) / WIN_TILE;
    for (u64 g = blockIdx.x; g < n_tiles; g += gridDim.x) {
        const u64 g0 = g * WIN_TILE, g1 = g0 + WIN_TILE < wp.total_bases ? g0 + WIN_TILE : wp.total_bases;
        for (u64 s = win_seq_of(wp.offsets, wp.n_seqs, g0); s < wp.n_seqs; ++s) {
            const u64 o = wp.offsets[s];
            if (o >= g1) break;
            const u32 n = (u32)(wp.offsets[s + 1] - o);
            const u32 nw = n >= L ? n - L + 1u : 0u;
            const u32 p_lo = g0 > o ? (u32)(g0 - o) : 0u;
            const u32 p_hi = (g1 - o) < (u64)nw ? (u32)(g1 - o) : nw;
            if (p_lo >= p_hi) continue;
            const u32 n_win = p_hi - p_lo, np = n_win + H;         // np <= WIN_TILE + H = list_cap stream positions, all of them k-mer starts
            const u64 at = o + p_lo;
            __builtin_amdgcn_wave_barrier();                       // (the previous part's readers are done)
            u32 n_hits = 0, n_miss = 0;
            for (u32 base = 0; base < np + 1u; base += 64u) {      // (+ 1: the word rank(np) reads exists and is complete)
                const u32 i = base + lane;
                bool hit;
                if constexpr (CONF) {
                    const u32 cl = i < np ? (u32)wp.cls[at + i] : 0u;
                    hit = cl == WIN_CLS_HIT;
                    const u64 mm = ballot64(cl == WIN_CLS_MISSING);
                    if (lane == 0) { mbits[base >> 6] = mm; mpre[base >> 6] = n_miss; }
                    n_miss += (u32)__popcll(mm);
                } else hit = i < np && wp.cls[at + i] == WIN_CLS_HIT;
                const u64 hm = ballot64(hit);
                if (lane == 0) { bits[base >> 6] = hm; wpre[base >> 6] = n_hits; }
                if (hit) hl[n_hits + (u32)__popcll(hm & lanemask_lt())] = wp.vals[at + i];
                n_hits += (u32)__popcll(hm);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            const u32 taxid = wp.taxid[s];
            u32 c_lo = 0, c_hi = 0, c_tax = 0, c_q = 0;            // the range, call (and Q) of the window in front of the step
            bool c_have = false;
            u32 pend_call = 0, pend_n = 0;                         // windows counted and not yet in the pair table
            for (u32 base = 0; base < n_win; base += 64u) {
                const u32 i = base + lane;
                const bool act = i < n_win;
                const u32 lo = act ? win_rank(bits, wpre, i) : 0u, hi = act ? win_rank(bits, wpre, i + H + 1u) : 0u;
                u32 plo = (u32)__shfl_up((int)lo, 1, 64), phi = (u32)__shfl_up((int)hi, 1, 64);
                bool head = act && (lo != plo || hi != phi);
                if (lane == 0) head = !c_have || lo != c_lo || hi != c_hi;
                u32 q = 0;                                         // CONF: the window's Q = hits + missing, and R = ceil(theta Q)
                u64 need = 0;
                if constexpr (CONF) {
                    q = act ? (hi - lo) + win_rank(mbits, mpre, i + H + 1u) - win_rank(mbits, mpre, i) : 0u;
                    const u32 pq = (u32)__shfl_up((int)q, 1, 64);
                    head = head || (act && q != (lane == 0 ? c_q : pq));
                    need = act ? conf_required(num, den, (u64)q) : 0ULL;
                }
                u64 heads = ballot64(head);
                u32 tx = c_tax;
                while (heads) {
                    const int l = __builtin_ctzll(heads);
                    heads &= heads - 1;
                    u32 t = win_resolve_range(hl, readlane(lo, l), readlane(hi, l), keys, cnt, tin, tout, wp.counter_cap, nodes, n_nodes);
                    if constexpr (CONF) t = win_confidence(hl, readlane(lo, l), readlane(hi, l), readlane64(need, l), t, nodes, n_nodes);
                    tx = lane >= (u32)l ? t : tx;                  // (the lanes from the next head on are overwritten by it)
                }
                const int last = (int)((n_win - base < 64u ? n_win - base : 64u) - 1u);
                c_lo = readlane(lo, last); c_hi = readlane(hi, last); c_tax = readlane(tx, last); c_have = true;
                if constexpr (CONF) c_q = readlane(q, last);
                if (act && wp.taxon) wp.taxon[at + i] = tx;
                u64 rem = ballot64(act);
                while (rem) {
                    const int l = __builtin_ctzll(rem);
                    const u32 t = readlane(tx, l);
                    const u64 mm = ballot64(act && tx == t);
                    rem &= ~mm;
                    const u32 cn = (u32)__popcll(mm);
                    if (pend_n && t == pend_call) { pend_n += cn; continue; }
                    if (pend_n && lane == 0) win_pair_add(wp, taxid, pend_call, pend_n);
                    pend_call = t; pend_n = cn;
                }
            }
            if (pend_n && lane == 0) win_pair_add(wp, taxid, pend_call, pend_n);
        }
    }
}

__global__ __launch_bounds__(256) void windows_pair_clear_kernel(u64 *__restrict__ keys, u64 *__restrict__ counts, u64 n, unsigned long long *dropped)
{
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) { keys[i] = WIN_PAIR_EMPTY; counts[i] = 0; }
    if (blockIdx.x == 0 && threadIdx.x == 0) *dropped = 0;
}

// The session: window length, the pair table, and the positional stream of the batch in flight (grow-only).
struct WindowSession {
    u32 L = 0;
    u64 conf_num = 0, conf_den = 1;                  // the session's own threshold (bns_windows_begin_conf); 0: none
    u64 pair_cap = 0;
    u64 *pair_keys = nullptr, *pair_counts = nullptr;
    unsigned long long *dropped = nullptr;
    void *vals = nullptr, *cls = nullptr, *scratch = nullptr;
    size_t vals_cap = 0, cls_cap = 0, scratch_cap = 0;
    // bns_set_timing at begin: events around the three stages of an add, and their milliseconds summed over the adds (bns_windows_timing)
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms[3] = {0, 0, 0};                        // pack + clears | lookup pass | vote pass
    u64 n_adds = 0;
};

}  // namespace bns

namespace {

void windows_free(bns_ctx *ctx)
{
    WindowSession *w = ctx->windows;
    if (!w) return;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();                            // (bns_windows_add may have run on a stream of the caller's)
    for (void *p : {(void *)w->pair_keys, (void *)w->pair_counts, (void *)w->dropped, w->vals, w->cls, w->scratch})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : w->ev) if (e) (void)hipEventDestroy(e);
    delete w;
    ctx->windows = nullptr;
}

int windows_grow(bns_ctx *ctx, void *&p, size_t &cap, size_t bytes)
{
    if (bytes <= cap) return BNS_OK;
    if (p) { HIPCHK(ctx, hipFree(p)); p = nullptr; cap = 0; }
    const size_t want = (bytes + bytes / 4 + 255) & ~size_t(255);
    HIPCHK(ctx, hipMalloc(&p, want));
    cap = want;
    return BNS_OK;
}

int windows_clear(bns_ctx *ctx, WindowSession *w, hipStream_t st)
{
    hipLaunchKernelGGL(windows_pair_clear_kernel, dim3(grid_for(ctx, w->pair_cap, 256)), dim3(256), 0, st, w->pair_keys, w->pair_counts,
                       w->pair_cap, w->dropped);
    HIPCHK(ctx, hipGetLastError());
    return BNS_OK;
}

// what a session needs of the context, at begin and at every add
int windows_ready(bns_ctx *ctx, u32 L)
{
    int rc = ready(ctx, true, true);
    if (rc != BNS_OK) return rc;
    if (ctx->conf_num) return fail(ctx, BNS_ERR_STATE, "window session: a confidence threshold is set on the context (bns_set_confidence); a session takes its own (bns_windows_begin_conf)");
    if (win_rounds_per_chunk(ctx->c) < 2u) return fail(ctx, BNS_ERR_ARG, "window session: the seed spans more than 1921 bases");
    if (L < ctx->c) return fail(ctx, BNS_ERR_ARG, "window_len is shorter than the seed (" + std::to_string(ctx->c) + " bases)");
    if ((u64)L - ctx->c + 1 > 65535) return fail(ctx, BNS_ERR_ARG, "window_len - seed span + 1 exceeds 65535 k-mers (the vote's counts are 16 bits wide)");
    return BNS_OK;
}

int windows_begin(bns_ctx *ctx, u32 window_len, u32 pair_cap, u64 num = 0, u64 den = 1)
{
    if (!ctx) return BNS_ERR_ARG;
    if (den == 0 || num > den) return fail(ctx, BNS_ERR_ARG, "confidence num / den: den > 0 and num <= den");
    if (ctx->windows) return fail(ctx, BNS_ERR_STATE, "a window session is already open (bns_windows_end)");
    if (ctx->dust_w) return fail(ctx, BNS_ERR_STATE, "bns_windows_begin while low-complexity masking is on (bns_set_dust): a window's call is classify's call of that substring as a read, and the mask of a substring is not the genome's mask restricted to it");
    if (ctx->min_hit_groups) return fail(ctx, BNS_ERR_STATE, "bns_windows_begin while a minimum of hit groups is set (bns_set_min_hit_groups): a window's distinct-key count cannot be read from the session's prefix ranges");
    int rc = windows_ready(ctx, window_len);
    if (rc != BNS_OK) return rc;
    if (pair_cap == 0) return fail(ctx, BNS_ERR_ARG, "pair_cap is 0");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    WindowSession *w = new (std::nothrow) WindowSession();
    if (!w) return BNS_ERR_NOMEM;
    ctx->windows = w;
    w->L = window_len;
    const u64 g = num ? std::gcd(num, den) : 1;      // (bns_set_confidence's lowest terms; the session's theta, never the context's)
    w->conf_num = num / g; w->conf_den = num ? den / g : 1;
    w->pair_cap = 1;
    while (w->pair_cap < pair_cap) w->pair_cap <<= 1;
    hipError_t e = hipMalloc((void **)&w->pair_keys, (size_t)w->pair_cap * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&w->pair_counts, (size_t)w->pair_cap * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&w->dropped, 8);
    for (int i = 0; i < 4 && ctx->timing && e == hipSuccess; ++i) e = hipEventCreate(&w->ev[i]);
    if (e == hipSuccess && (rc = windows_clear(ctx, w, ctx->stream)) == BNS_OK) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess || rc != BNS_OK) {
        if (e != hipSuccess) { ctx->err = std::string("bns_windows_begin: ") + hipGetErrorString(e); rc = e == hipErrorOutOfMemory ? BNS_ERR_NOMEM : BNS_ERR_HIP; }
        (void)hipGetLastError();
        windows_free(ctx);
        return rc;
    }
    return BNS_OK;
}

int windows_add(bns_ctx *ctx, const char *d_bases, const u64 *d_offsets, u64 n_seqs, u64 total_bases, const u32 *d_taxid, u32 *d_taxon,
                void *stream)
{
    if (!ctx) return BNS_ERR_ARG;
    WindowSession *w = ctx->windows;
    if (!w) return fail(ctx, BNS_ERR_STATE, "bns_windows_add: no window session is open (bns_windows_begin)");
    int rc = windows_ready(ctx, w->L);
    if (rc != BNS_OK) return rc == BNS_ERR_ARG ? fail(ctx, BNS_ERR_STATE, "bns_windows_add: the encoder changed under the session: " + ctx->err) : rc;
    if (n_seqs == 0 || total_bases == 0) return BNS_OK;
    if (!d_bases || !d_offsets || !d_taxid) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    if (st != ctx->stream) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // (begin / a reset cleared the pair table there)
    const bool timed = w->ev[0] != nullptr;
    if (timed) HIPCHK(ctx, hipEventRecord(w->ev[0], st));
    const size_t n_words = (size_t)(total_bases >> 5) + n_seqs + 2;             // (pack_reads' image, packed piece by piece)
    if ((rc = ensure(ctx, ctx->words, n_words * 8)) != BNS_OK) return rc;
    if ((rc = ensure(ctx, ctx->nmask, n_words * 4)) != BNS_OK) return rc;
    hipLaunchKernelGGL(windows_pack_kernel, dim3(grid_for(ctx, (total_bases + 2047) >> 11, 4)), dim3(256), 0, st, (const u8 *)d_bases, d_offsets,
                       n_seqs, total_bases, (u64 *)ctx->words.p, (u32 *)ctx->nmask.p);
    HIPCHK(ctx, hipGetLastError());
    if ((rc = windows_grow(ctx, w->vals, w->vals_cap, (size_t)total_bases * 4)) != BNS_OK) return rc;
    if ((rc = windows_grow(ctx, w->cls, w->cls_cap, (size_t)total_bases)) != BNS_OK) return rc;

    ClassifyParams p;
    fill_params(ctx, p);
    p.offsets = d_offsets; p.n_units = n_seqs; p.nmates = 1;
    p.emit_none = (ctx->spaced && !ctx->spaced_intended) ? 1 : 0;
    WindowParams wp;
    std::memset(&wp, 0, sizeof(wp));
    wp.offsets = d_offsets; wp.n_seqs = n_seqs; wp.total_bases = total_bases; wp.taxid = d_taxid;
    wp.vals = (u32 *)w->vals; wp.cls = (u8 *)w->cls; wp.taxon = d_taxon; wp.L = w->L;
    wp.pair_keys = w->pair_keys; wp.pair_counts = w->pair_counts; wp.pair_mask = w->pair_cap - 1; wp.dropped = w->dropped;
    const u32 n_kw = w->L - ctx->c + 1;                                          // k-mers of a window
    wp.counter_cap = (n_kw + 63u) & ~63u;
    wp.list_cap = WIN_TILE + (w->L - ctx->c);
    const bool gl = wp.list_cap > WIN_LDS_LIST_MAX;
    wp.scratch_stride = 4ull * wp.counter_cap + (gl ? wp.list_cap : 0u);
    const u64 n_tiles = (total_bases + WIN_TILE - 1) / WIN_TILE;
    // a wavefront per workgroup, each with its counter arrays: as many as are resident, within 256 MiB of them
    const u64 vgrid = std::max<u64>(1, std::min<u64>({n_tiles, (u64)ctx->n_cu * 32, (256ull << 20) / (wp.scratch_stride * 4)}));
    if ((rc = windows_grow(ctx, w->scratch, w->scratch_cap, (size_t)(vgrid * wp.scratch_stride * 4))) != BNS_OK) return rc;
    wp.scratch = (u32 *)w->scratch;

    // a base that starts no k-mer is no hit, one that starts no window has no call: the kernels write the rest
    HIPCHK(ctx, hipMemsetAsync(w->cls, 0, (size_t)total_bases, st));
    if (d_taxon) HIPCHK(ctx, hipMemsetAsync(d_taxon, 0xFF, (size_t)total_bases * 4, st));
    if (timed) HIPCHK(ctx, hipEventRecord(w->ev[1], st));
    const u64 n_pieces = (total_bases + win_lookup_bases(ctx->c) - 1) / win_lookup_bases(ctx->c);
    const unsigned grid = grid_for(ctx, n_pieces, 4);
    const bool whole_key = ctx->table_canon && ctx->table_shift == 0 && ctx->table_len == ctx->table_k;    // (bns_probe_device's dispatch)
    dispatch_sp_layout(ctx->spaced, ctx->layout, [&](auto sp, auto ly) {
        constexpr bool SP = decltype(sp)::value;
        constexpr int LY = decltype(ly)::value;
        if constexpr (LY == 2) {
            if (!whole_key)           hipLaunchKernelGGL((windows_lookup_kernel<SP, 2, 1>), dim3(grid), dim3(256), 0, st, p, wp);
            else if (ctx->table_wide) hipLaunchKernelGGL((windows_lookup_kernel<SP, 2, 2>), dim3(grid), dim3(256), 0, st, p, wp);
            else                      hipLaunchKernelGGL((windows_lookup_kernel<SP, 2, 0>), dim3(grid), dim3(256), 0, st, p, wp);
        } else hipLaunchKernelGGL((windows_lookup_kernel<SP, LY, 0>), dim3(grid), dim3(256), 0, st, p, wp);
    });
    HIPCHK(ctx, hipGetLastError());
    if (timed) HIPCHK(ctx, hipEventRecord(w->ev[2], st));
    const u32 n_bw = (wp.list_cap >> 6) + 2u;
    const bool conf = w->conf_num != 0;                      // (a second bitmap with its running counts)
    const size_t lds = (size_t)n_bw * (conf ? 24 : 12) + (gl ? 0 : (size_t)wp.list_cap * 4);
    const TaxNode *nodes = (const TaxNode *)ctx->nodes;
    const u64 num = w->conf_num, den = w->conf_den;
    if (conf && gl) hipLaunchKernelGGL((windows_vote_kernel<true, true>), dim3((unsigned)vgrid), dim3(64), lds, st, wp, nodes, ctx->n_nodes, ctx->c, num, den);
    else if (conf)  hipLaunchKernelGGL((windows_vote_kernel<false, true>), dim3((unsigned)vgrid), dim3(64), lds, st, wp, nodes, ctx->n_nodes, ctx->c, num, den);
    else if (gl)    hipLaunchKernelGGL((windows_vote_kernel<true>), dim3((unsigned)vgrid), dim3(64), lds, st, wp, nodes, ctx->n_nodes, ctx->c, num, den);
    else            hipLaunchKernelGGL((windows_vote_kernel<false>), dim3((unsigned)vgrid), dim3(64), lds, st, wp, nodes, ctx->n_nodes, ctx->c, num, den);
    HIPCHK(ctx, hipGetLastError());
    if (timed) {                                             // (a timed add waits for its batch)
        HIPCHK(ctx, hipEventRecord(w->ev[3], st));
        HIPCHK(ctx, hipEventSynchronize(w->ev[3]));
        for (int i = 0; i < 3; ++i) {
            float ms = 0.0f;
            HIPCHK(ctx, hipEventElapsedTime(&ms, w->ev[i], w->ev[i + 1]));
            w->ms[i] += ms;
        }
        ++w->n_adds;
    }
    return BNS_OK;
}

int windows_read(bns_ctx *ctx, u32 *seq_taxid, u32 *called, u64 *count, u64 cap, u64 *n_pairs, u64 *n_dropped, int reset)
{
    if (!ctx) return BNS_ERR_ARG;
    WindowSession *w = ctx->windows;
    if (!w) return fail(ctx, BNS_ERR_STATE, "bns_windows_read: no window session is open (bns_windows_begin)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipDeviceSynchronize());                     // (adds on a stream of the caller's)
    std::vector<u64> keys((size_t)w->pair_cap), counts((size_t)w->pair_cap);
    unsigned long long dropped = 0;
    HIPCHK(ctx, hipMemcpyAsync(keys.data(), w->pair_keys, (size_t)w->pair_cap * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(counts.data(), w->pair_counts, (size_t)w->pair_cap * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(&dropped, w->dropped, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    std::vector<std::pair<u64, u64>> pairs;
    for (size_t i = 0; i < keys.size(); ++i)
        if (keys[i] != WIN_PAIR_EMPTY) pairs.emplace_back(keys[i], counts[i]);
    std::sort(pairs.begin(), pairs.end());                   // (taxid in the high word: ascending by (seq_taxid, called))
    if (n_pairs) *n_pairs = pairs.size();
    if (n_dropped) *n_dropped = dropped;
    if ((seq_taxid || called || count) && cap < pairs.size()) return fail(ctx, BNS_ERR_ARG, "cap is smaller than the number of pairs");
    for (size_t i = 0; i < pairs.size(); ++i) {
        if (seq_taxid) seq_taxid[i] = (u32)(pairs[i].first >> 32);
        if (called) called[i] = (u32)pairs[i].first;
        if (count) count[i] = pairs[i].second;
    }
    if (reset) {
        const int rc = windows_clear(ctx, w, st);
        if (rc != BNS_OK) return rc;
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    return BNS_OK;
}

}  // namespace
