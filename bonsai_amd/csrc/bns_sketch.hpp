// bns_sketch.hpp -- distinct k-mers per taxon behind bns_sketch_enable / bns_sketch_read (gfx950, wave64).
//
// One HyperLogLog sketch (p = 12: 4096 one-byte registers) per bin of tally_bin that a sample touches, kept in a pool of max_taxa
// slots; slot_of[n + 1] maps a bin to its slot.  A separate pass behind a classify launch, launched only while the feature is on:
//
//   sketch_seen_kernel    the launch's compact hit stream (hit_runs_kernel's indexing) -> seen[tally_bin(hit)] = 1.  Plain byte stores
//                         of the same value: idempotent, no order.
//   sketch_assign_kernel  bins with seen set and no slot yet take the next free slots in ascending bin order: an exclusive scan over
//                         the n + 1 flags, one workgroup (clade_scan_kernel's shape).  Slots past max_taxa are not given; the bins
//                         left without one are counted.  It runs BEFORE sketch_kernel, so no wavefront of the hot path ever waits
//                         for another one: there is nothing to claim and nothing to publish.
//   sketch_kernel         one wavefront per unit, walking the packed image as encode_kernel does (chunks of 2048 bases, rounds of 64
//                         k-mers, window = k); every k-mer classify_unit looks up is looked up again through the same probe functions
//                         and the same minimizer-identity dispatch as probe_kernel.  A found lane with a slot hashes its key, reads the
//                         register byte and only when its rank is larger raises it: an atomic max on the byte through its aligned 32-bit
//                         word (compare-and-swap; a lane retries only while ITS word changed under it and its rank is still larger).
//
// Registers are a maximum over a set of keys: no arrival order, so the bytes are exactly reproducible, and classifying a unit twice
// (bns_classify_text's roll-back) changes nothing.  No reference counterpart (Kraken 2's --report-minimizer-data, KrakenUniq): the
// sketch and the estimate are defined behaviour, DESIGN.md.
#pragma once
#include "bns_device.hpp"
#include "bns_kernels.hpp"
#include "bns_tally.hpp"

namespace bns {

constexpr u32 SKETCH_P = 12;
constexpr u32 SKETCH_M = 1u << SKETCH_P;                // registers (bytes) per sketch
constexpr u32 SKETCH_NO_SLOT = 0xFFFFFFFFu;
constexpr u32 SKETCH_SCAN_BLOCK = 1024;
// state words of a context's sketches (device): slots given so far | bins seen that have none (as of the last assignment)
constexpr u32 SKETCH_ST_USED = 0, SKETCH_ST_DROPPED = 1, SKETCH_ST_WORDS = 2;

// MurmurHash3's 64-bit finaliser
__device__ __forceinline__ u64 fmix64(u64 x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL;
    x ^= x >> 33;
    return x;
}

// hits of unit u: hits[offsets[u * nmates]], records[u].w of them.  One wavefront per unit; a hit equal to the one in front of it
// (the usual case: runs) has nothing new to say.
__global__ __launch_bounds__(256) void sketch_seen_kernel(const u32 *__restrict__ hits, const u64 *__restrict__ offsets, u32 nmates,
                                                          const uint4 *__restrict__ records, u64 n_units, const TaxNode *__restrict__ nodes,
                                                          u32 n, u8 *__restrict__ seen)
{
    const u32 lane = (u32)lane_id();
    const u64 n_waves = (u64)gridDim.x * 4;
    for (u64 u = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); u < n_units; u += n_waves) {
        const u32 *h = hits + offsets[u * nmates];
        const u32 nh = records[u].w;
        for (u32 i = lane; i < nh; i += 64u) {
            const u32 t = h[i];
            if (i && h[i - 1u] == t) continue;
            seen[tally_bin(nodes, n, t)] = 1;
        }
    }
}

// slot_of[b] for the bins b in [0, n_bins) with seen[b] and no slot: state[USED], state[USED] + 1, ... in ascending b while they are
// below max_taxa; slot_bin[slot] = b.  One workgroup, tile by tile, the carry in LDS.
__global__ __launch_bounds__(SKETCH_SCAN_BLOCK) void sketch_assign_kernel(const u8 *__restrict__ seen, u32 *__restrict__ slot_of,
                                                                          u32 *__restrict__ slot_bin, u32 n_bins, u32 max_taxa,
                                                                          u32 *__restrict__ state)
{
    constexpr u32 PER = 4, TILE = SKETCH_SCAN_BLOCK * PER, WAVES = SKETCH_SCAN_BLOCK / 64;
    __shared__ u32 s_wave[WAVES];
    __shared__ u32 s_carry;
    const u32 t = threadIdx.x, lane = (u32)lane_id(), wave = t >> 6;
    const u32 used0 = state[SKETCH_ST_USED];
    if (t == 0) s_carry = 0;
    __syncthreads();
    for (u32 base = 0; base < n_bins; base += TILE) {
        bool want[PER];
        u32 sum = 0;
        for (u32 j = 0; j < PER; ++j) {
            const u32 b = base + t * PER + j;
            want[j] = b < n_bins && seen[b] && slot_of[b] == SKETCH_NO_SLOT;
            sum += want[j] ? 1u : 0u;
        }
        u32 incl = sum;
        for (u32 d = 1; d < 64; d <<= 1) {
            const u32 o = (u32)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        if (wave == 0) {
            u32 w = lane < WAVES ? s_wave[lane] : 0u;
            for (u32 d = 1; d < WAVES; d <<= 1) {
                const u32 o = (u32)__shfl_up((int)w, d, 64);
                if (lane >= d) w += o;
            }
            if (lane < WAVES) s_wave[lane] = w;
        }
        __syncthreads();
        const u32 carry = s_carry;
        u32 idx = used0 + carry + (wave ? s_wave[wave - 1] : 0u) + (incl - sum);     // (< 2^29 + 2^28: bins and slots are <= 2^28 each)
        for (u32 j = 0; j < PER; ++j) {
            if (!want[j]) continue;
            if (idx < max_taxa) { const u32 b = base + t * PER + j; slot_of[b] = idx; slot_bin[idx] = b; }
            ++idx;
        }
        __syncthreads();
        if (t == 0) s_carry = carry + s_wave[WAVES - 1];
        __syncthreads();
    }
    if (t == 0) {
        const u32 all = used0 + s_carry;                    // bins seen so far, with a slot or without
        const u32 used = all < max_taxa ? all : max_taxa;
        state[SKETCH_ST_USED] = used;
        state[SKETCH_ST_DROPPED] = all - used;
    }
}

// reg = max(reg, rho) on one byte of the pool.  The plain read in front can only be stale towards SMALLER values (registers never
// go down), which costs an atomic that changes nothing, never a lost update.
__device__ __forceinline__ void sketch_update(u8 *__restrict__ regs, u64 idx, u32 rho)
{
    if (regs[idx] >= rho) return;
    u32 *wp = reinterpret_cast<u32 *>(regs + (idx & ~3ULL));
    const u32 sh = 8u * (u32)(idx & 3ULL);
    u32 old = __hip_atomic_load(wp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (((old >> sh) & 0xFFu) < rho) {
        const u32 want = (old & ~(0xFFu << sh)) | (rho << sh);
        const u32 prev = atomicCAS(wp, old, want);
        if (prev == old) break;
        old = prev;
    }
}

// MIN as in probe_kernel: 0 = the table's minimizer over the whole canonical key, 1 = inside a sub-run of the key (MinSpec), 2 = whole
// key with the wide identity.  p.offsets / p.n_units / p.nmates: the launch's units; p.words / p.nmask: their packed image (nmask may
// be null: no flagged base).  slot_of[n_nodes + 1], regs[max_taxa * SKETCH_M].
template <bool SPACED, int LAYOUT, int MIN = 0>
__global__ __launch_bounds__(256) void sketch_kernel(ClassifyParams p, const u32 *__restrict__ slot_of, u8 *__restrict__ regs)
{
    __shared__ __attribute__((aligned(16))) u32 s_aux[4][MINB_AUX_U32];
    const int lane = lane_id();
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const u32 rdesc = SPACED ? run_desc(p) : 0u;
    const u64 wave = (u64)blockIdx.x * 4 + (u64)wv;
    const u64 n_waves = (u64)gridDim.x * 4;
    const u32 k = p.k, c = p.c;
    const u32 rounds_per_chunk = (2048u - (c - 1u)) / 64u;
    const u32 nm = (u32)p.nmates;
    for (u64 u = wave; u < p.n_units; u += n_waves) {
        for (u32 m = 0; m < nm; ++m) {
            const u64 r = u * nm + m;
            const u64 o = p.offsets[r];
            const u32 L = (u32)(p.offsets[r + 1] - o);
            const u64 wb = (o >> 5) + r;
            const u32 n_words = (L + 31u) >> 5;
            const u32 nk = (L >= c && !(SPACED && p.emit_none)) ? L - c + 1u : 0u;
            for (u32 j0 = 0; j0 < nk; j0 += rounds_per_chunk * 64u) {
                const u32 wi = (j0 >> 5) + (u32)lane;
                const u64 W = wi < n_words ? p.words[wb + wi] : 0ULL;
                const u32 M = wi < n_words ? (p.nmask ? p.nmask[wb + wi] : 0u) : 0xFFFFFFFFu;
                const u32 chunk_nk = (nk - j0) < rounds_per_chunk * 64u ? (nk - j0) : rounds_per_chunk * 64u;
                for (u32 rd = 0; rd * 64u < chunk_nk; ++rd) {
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
                    if (valid && pr.found) {
                        const u32 slot = slot_of[tally_bin(p.nodes, p.n_nodes, pr.val)];
                        if (slot != SKETCH_NO_SLOT) {
                            const u64 h = fmix64(key);
                            const u64 w = h << SKETCH_P;
                            const u32 rho = w ? (u32)__builtin_clzll(w) + 1u : 64u - SKETCH_P + 1u;
                            sketch_update(regs, (u64)slot * SKETCH_M + (h >> (64u - SKETCH_P)), rho);
                        }
                    }
                }
            }
        }
    }
}

}  // namespace bns
