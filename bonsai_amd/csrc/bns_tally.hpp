// bns_tally.hpp -- the per-taxon tally behind bns_tally_enable / bns_tally_read (gfx950, wave64).
//
//   tally_kernel         per unit: taxon -> bin (0 unclassified, t for a taxon whose chain reaches a root with parent 0, n for anything
//                        else); equal bins of a wavefront are combined by a match loop, those of a workgroup in an LDS hash; one 64-bit
//                        atomic per distinct bin per workgroup reaches HBM
//   clade_scatter_kernel direct[v] -> S[tin[v]]
//   clade_scan_kernel    inclusive scan of S over the 2 x (forest size) Euler positions, one workgroup
//   clade_kernel         clade[v] = S[tout[v]] - S[tin[v] - 1]; bins 0 and n copied through
//
// No reference counterpart: the reference counts classified / unclassified reads (classifier.h:138,238) and prints neither.
#pragma once
#include "bns_device.hpp"

namespace bns {

constexpr u32 TALLY_BLOCK = 256;
constexpr u32 TALLY_SLOTS_LOG2 = 10;
constexpr u32 TALLY_SLOTS = 1u << TALLY_SLOTS_LOG2;     // distinct bins a workgroup combines in LDS (8 KiB)
constexpr u32 TALLY_PROBES = 32;                        // linear probes before a bin goes straight to HBM
constexpr u32 TALLY_EMPTY = 0xFFFFFFFFu;                // (a bin is <= n <= 2^28)
constexpr u32 CLADE_SCAN_BLOCK = 1024;

// the bin of one unit's taxon; no taxon indexes anything unchecked (resolve_tree may return any u32 the db holds, lca_dev 0xFFFFFFFF)
__device__ __forceinline__ u32 tally_bin(const TaxNode *__restrict__ nodes, u32 n, u32 t)
{
    if (t == 0u) return 0u;
    if (t < n && (nodes[t].flags & NODE_CHAIN_OK)) return t;
    return n;
}

__device__ __forceinline__ unsigned long long tally_delta(u32 c, int neg) { return neg ? 0ULL - (unsigned long long)c : (unsigned long long)c; }

// one lane: c units of bin b into the workgroup's LDS hash (or HBM when the probe sequence is full)
__device__ __forceinline__ void tally_lds_add(u32 *s_key, u32 *s_cnt, u32 b, u32 c, unsigned long long *__restrict__ direct, int neg)
{
    u32 h = (b * 0x9E3779B1u) >> (32u - TALLY_SLOTS_LOG2);
    for (u32 p = 0; p < TALLY_PROBES; ++p) {
        const u32 k = atomicCAS(&s_key[h], TALLY_EMPTY, b);
        if (k == TALLY_EMPTY || k == b) { atomicAdd(&s_cnt[h], c); return; }
        h = (h + 1u) & (TALLY_SLOTS - 1u);
    }
    atomicAdd(&direct[b], tally_delta(c, neg));
}

// direct[bin(taxon[i])] += 1 for i < n_units (neg: -= 1, a batch handed back after it was counted)
__global__ __launch_bounds__(TALLY_BLOCK) void tally_kernel(const u32 *__restrict__ taxon, u64 n_units, const TaxNode *__restrict__ nodes, u32 n,
                                                            unsigned long long *__restrict__ direct, int neg)
{
    __shared__ u32 s_key[TALLY_SLOTS];
    __shared__ u32 s_cnt[TALLY_SLOTS];
    for (u32 i = threadIdx.x; i < TALLY_SLOTS; i += TALLY_BLOCK) { s_key[i] = TALLY_EMPTY; s_cnt[i] = 0u; }
    __syncthreads();
    const int lane = lane_id();
    const u64 stride = (u64)gridDim.x * TALLY_BLOCK;
    for (u64 base = (u64)blockIdx.x * TALLY_BLOCK; base < n_units; base += stride) {       // (uniform: every lane runs every round)
        const u64 i = base + threadIdx.x;
        const u32 bin = i < n_units ? tally_bin(nodes, n, taxon[i]) : TALLY_EMPTY;
        // match loop: the lowest lane of each group of equal bins adds the group's size; a sample's units sit on a few taxa, so a
        // wavefront takes a few rounds, not 64
        u64 todo = __ballot(bin != TALLY_EMPTY);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const u32 b = (u32)__shfl((int)bin, leader);
            const u64 same = __ballot(bin == b);
            if (lane == leader) tally_lds_add(s_key, s_cnt, b, (u32)__popcll(same), direct, neg);
            todo &= ~same;
        }
    }
    __syncthreads();
    for (u32 i = threadIdx.x; i < TALLY_SLOTS; i += TALLY_BLOCK) {
        const u32 k = s_key[i];
        if (k != TALLY_EMPTY) atomicAdd(&direct[k], tally_delta(s_cnt[i], neg));
    }
}

// S[tin[v]] = direct[v] for the forest's nodes (S zeroed first; the tout positions stay 0)
__global__ __launch_bounds__(256) void clade_scatter_kernel(const TaxNode *__restrict__ nodes, u32 n, const unsigned long long *__restrict__ direct,
                                                            unsigned long long *__restrict__ S, u32 n_pos)
{
    const u32 stride = gridDim.x * blockDim.x;
    for (u32 v = 1u + blockIdx.x * blockDim.x + threadIdx.x; v < n; v += stride) {
        const u32 tin = nodes[v].tin;
        if (tin && tin < n_pos) S[tin] = direct[v];
    }
}

// inclusive scan of S[0, n_pos) in place, tile by tile (runs once per bns_tally_read: one workgroup is plenty)
__global__ __launch_bounds__(CLADE_SCAN_BLOCK) void clade_scan_kernel(unsigned long long *__restrict__ S, u64 n_pos)
{
    constexpr u32 PER = 4, TILE = CLADE_SCAN_BLOCK * PER, WAVES = CLADE_SCAN_BLOCK / 64;
    __shared__ unsigned long long s_wave[WAVES];
    __shared__ unsigned long long s_carry;
    const u32 t = threadIdx.x, lane = (u32)lane_id(), wave = t >> 6;
    if (t == 0) s_carry = 0;
    __syncthreads();
    for (u64 base = 0; base < n_pos; base += TILE) {
        unsigned long long v[PER], sum = 0;
        for (u32 j = 0; j < PER; ++j) {
            const u64 i = base + (u64)t * PER + j;
            v[j] = i < n_pos ? S[i] : 0ULL;
            sum += v[j];
            v[j] = sum;
        }
        unsigned long long incl = sum;                                      // inclusive scan of the threads' sums inside the wavefront
        for (u32 d = 1; d < 64; d <<= 1) {
            const unsigned long long o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        if (wave == 0) {
            unsigned long long w = lane < WAVES ? s_wave[lane] : 0ULL;
            for (u32 d = 1; d < WAVES; d <<= 1) {
                const unsigned long long o = __shfl_up(w, d, 64);
                if (lane >= d) w += o;
            }
            if (lane < WAVES) s_wave[lane] = w;                              // inclusive prefix of the wave totals
        }
        __syncthreads();
        const unsigned long long carry = s_carry;
        const unsigned long long before = carry + (wave ? s_wave[wave - 1] : 0ULL) + (incl - sum);
        for (u32 j = 0; j < PER; ++j) {
            const u64 i = base + (u64)t * PER + j;
            if (i < n_pos) S[i] = before + v[j];
        }
        __syncthreads();                                                    // (every thread has read s_carry and s_wave)
        if (t == 0) s_carry = carry + s_wave[WAVES - 1];
        __syncthreads();
    }
}

// clade[v] for v in [0, n]: the sum of direct[] over v's subtree = S[tout] - S[tin - 1]
__global__ __launch_bounds__(256) void clade_kernel(const TaxNode *__restrict__ nodes, u32 n, const unsigned long long *__restrict__ direct,
                                                    const unsigned long long *__restrict__ S, u32 n_pos, unsigned long long *__restrict__ clade)
{
    const u32 stride = gridDim.x * blockDim.x;
    for (u32 v = blockIdx.x * blockDim.x + threadIdx.x; v <= n; v += stride) {
        unsigned long long c = 0;
        if (v == 0u || v == n) c = direct[v];
        else {
            const TaxNode nd = nodes[v];
            if (nd.tin && nd.tout < n_pos) c = S[nd.tout] - S[nd.tin - 1u];
        }
        clade[v] = c;
    }
}

}  // namespace bns
