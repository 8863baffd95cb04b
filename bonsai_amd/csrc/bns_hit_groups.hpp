// bns_hit_groups.hpp -- the minimum number of hit groups behind bns_set_min_hit_groups / `bonsai classify -M` (gfx950, wave64).
//
//   hit_groups_kernel   per unit, after classify, its overflow kernel and the confidence walk, before unpack: G = the number of DISTINCT
//                       keys among the k-mers of all mates that classify looks up and finds.  A unit with a taxon and G < N gets taxon 0;
//                       nothing else of its record changes.  Launched only while N >= 2 (N = 1 changes nothing: a taxon implies a hit).
//
// One wavefront per group of HG_GROUP units, as confidence_kernel: the records are read lane-parallel (one unit per lane), and the units
// that need no walk are settled there -- taxon 0 stays, fewer than N hits (records.w: found positions, an upper bound of G) is 0 at once.
// The others run one after another over the whole wavefront, walking the packed image as sketch_kernel does (chunks of 2048 bases,
// rounds of 64 k-mers, the same extract_* / probe_* and the same minimizer-identity dispatch).  The distinct keys found so far are kept
// one per lane (N <= 64): for each found lane of a round, in a wave-uniform loop over the ballot, that lane's key is read, one compare
// and ballot tests it against the list, and a new key goes to lane `cnt`.  The walk ends as soon as the list holds N keys -- for nearly
// every classified read inside its first chunk.  The set of distinct keys has no order, so neither has the result.
// No reference counterpart (Kraken 2's --minimum-hit-groups counts runs of one minimizer): defined behaviour, DESIGN.md.
#pragma once
#include "bns_device.hpp"
#include "bns_kernels.hpp"

namespace bns {

constexpr u32 HG_GROUP = 16;          // units per wavefront
constexpr u32 HG_MAX = 64;            // the largest N: one listed key per lane

// MIN as in sketch_kernel.  p.offsets / p.n_units / p.nmates: the launch's units; p.words / p.nmask: their packed image (nmask may be
// null); p.records[u].x rewritten in place for u < p.n_units.  2 <= n_min <= HG_MAX (the launch site only launches it then).
template <bool SPACED, int LAYOUT, int MIN = 0>
__global__ __launch_bounds__(256) void hit_groups_kernel(ClassifyParams p, u32 n_min)
{
    __shared__ __attribute__((aligned(16))) u32 s_aux[4][MINB_AUX_U32];
    const int lane = lane_id();
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u32 rdesc = SPACED ? run_desc(p) : 0u;
    const u64 n_waves = (u64)gridDim.x * 4;
    const u64 n_groups = (p.n_units + HG_GROUP - 1) / HG_GROUP;
    const u32 k = p.k, c = p.c;
    const u32 rounds_per_chunk = (2048u - (c - 1u)) / 64u;
    const u32 nm = (u32)p.nmates;
    for (u64 g = (u64)blockIdx.x * 4 + (u64)wv; g < n_groups; g += n_waves) {
        const u64 u0 = g * HG_GROUP;
        const u32 nu = (u32)(p.n_units - u0 < HG_GROUP ? p.n_units - u0 : HG_GROUP);
        bool walk = false;
        if ((u32)lane < nu) {                                        // lane j < nu: unit u0 + j
            const uint4 rec = p.records[u0 + (u32)lane];
            if (rec.x != 0u) {
                if (rec.w < n_min) p.records[u0 + (u32)lane].x = 0u;     // no more distinct keys than found positions
                else walk = true;
            }
        }
        u64 todo = __ballot(walk);
        while (todo) {                                               // (wave-uniform)
            const u64 u = u0 + (u64)__builtin_ctzll(todo);
            todo &= todo - 1;
            u64 mine = 0;                                            // lane i < cnt: the i-th distinct key found
            u32 cnt = 0;
            for (u32 m = 0; m < nm && cnt < n_min; ++m) {
                const u64 r = u * nm + m;
                const u64 o = p.offsets[r];
                const u32 L = (u32)(p.offsets[r + 1] - o);
                const u64 wb = (o >> 5) + r;
                const u32 n_words = (L + 31u) >> 5;
                const u32 nk = (L >= c && !(SPACED && p.emit_none)) ? L - c + 1u : 0u;
                for (u32 j0 = 0; j0 < nk && cnt < n_min; j0 += rounds_per_chunk * 64u) {
                    const u32 wi = (j0 >> 5) + (u32)lane;
                    const u64 W = wi < n_words ? p.words[wb + wi] : 0ULL;
                    const u32 M = wi < n_words ? (p.nmask ? p.nmask[wb + wi] : 0u) : 0xFFFFFFFFu;
                    const u32 chunk_nk = (nk - j0) < rounds_per_chunk * 64u ? (nk - j0) : rounds_per_chunk * 64u;
                    for (u32 rd = 0; rd * 64u < chunk_nk && cnt < n_min; ++rd) {
                        u64 key;
                        bool valid;
                        if (SPACED) valid = p.n_runs ? extract_spaced_runs(W, M, rd, p, rdesc, key) : extract_spaced(W, M, rd, k, rdesc, key);
                        else        valid = extract_unspaced(W, M, rd, k, key);
                        valid = valid && rd * 64u + (u32)lane < chunk_nk;
                        if (!SPACED && p.canon) key = canonical(key, k);
                        ProbeResult pr;
                        if (LAYOUT == 2) {
                            const u32 minh = MIN == 1 ? key_minhash(key, k, MinSpec{p.m, p.min_len, p.min_shift, p.min_canon, 0u})
                                                      : (MIN == 2 ? key_minhash<true>(key, k, p.m) : key_minhash<false>(key, k, p.m));
                            pr = probe_minbucket<true, 16, false, false>(p.minb, key, bucket_of(minh, p.n_mb), valid, s_aux[wv], p.slots, p.ovf_mask);
                        }
                        else if (LAYOUT == 1) pr = probe_bucket(p.slots, p.bucket_mask, key, valid);
                        else                  pr = probe_khash(p.kflags, p.kkeys, p.kvals, p.kh_nb, key, valid);
                        u64 found = __ballot(valid && pr.found);
                        while (found && cnt < n_min) {               // (wave-uniform)
                            const u64 kq = readlane64(key, __builtin_ctzll(found));
                            found &= found - 1;
                            if (__ballot((u32)lane < cnt && mine == kq) == 0ULL) {
                                if ((u32)lane == cnt) mine = kq;
                                ++cnt;
                            }
                        }
                    }
                }
            }
            if (cnt < n_min && lane == 0) p.records[u].x = 0u;
        }
    }
}

}  // namespace bns
