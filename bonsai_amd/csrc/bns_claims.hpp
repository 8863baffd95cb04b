// bns_claims.hpp -- how classify_kernel's batch is dealt out to its persistent wavefronts: which units a wavefront takes first
// (a closed form of its index, no atomic) and which units the i-th claim from the work counter stands for.  One set of
// functions for the kernel and for the launcher (and for tests/test_claim_schedule.py, which compiles this header on its own:
// nothing here needs HIP).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BNS_CLAIMS_HD __host__ __device__ __forceinline__
#else
#define BNS_CLAIMS_HD inline
#endif

namespace bns {

// static part    wavefront w of the G launched takes its first units without asking anybody:
//                  a batch too small for full claims   [w * chunk, (w + 1) * chunk)   -- and that is all of the batch
//                  otherwise, staggered                1 + (w mod full) units, the base their prefix sum: the wavefronts'
//                                                      later claims are then spread over one claim's duration from the start,
//                                                      as they are in the steady state, instead of coming in step
// dynamic part   claim index g (claims are counted from 0) stands for the `full` units from dyn_base + g * full, dyn_base = the
//                units of the static part.  A base at or past n_units means: past the end.
//                The indices are handed out by CLAIM_SHARDS work counters, one per XCD, each on a cache line of its own: draw d
//                from counter x is claim g = CLAIM_SHARDS * d + x, so every counter holds an interleaved eighth of the one tiling
//                and none of them a stretch of its own that could finish late.  A wavefront draws from its XCD's counter; when that
//                one is past the end (it stays so: a counter only grows) it goes on to the next, and after the eighth the batch is
//                dealt out.  Draws past the end: one per wavefront and counter at the most, so the farthest index lies
//                CLAIM_SHARDS * wavefronts claims behind the last -- with 8192 wavefronts 2.03 M units, which is why a batch has
//                fewer than 2^32 - 2^22 units: the 32-bit base does not wrap.
// Every claim is at most `full` units (full * mates + 1 offsets must fit one 64-lane load); the last one is cut at n_units by
// the caller (claim_cnt).
// (Claims that shrink over the end of the batch -- 16, 8, 4 units over the last 32 per resident wavefront -- were built and
// measured on ONE counter: 8192 wavefronts draw them faster than it hands them out, docs/KERNEL_NOTES.md "Dealing the batch out".)

// units of wavefronts [0, w) of a staggered static part
BNS_CLAIMS_HD uint32_t claim_stagger_prefix(uint32_t w, uint32_t full)
{
    const uint32_t q = w / full, r = w - q * full;               // (full is a compile-time constant in the kernel: no division there)
    return q * (full * (full + 1u) / 2u) + r * (r + 1u) / 2u;
}

// the static claim of wavefront w: chunk < full says "small batch, even shares"
BNS_CLAIMS_HD void claim_static(uint32_t w, uint32_t chunk, uint32_t full, uint32_t &base, uint32_t &size)
{
    if (chunk < full) { base = w * chunk; size = chunk; return; }
    base = claim_stagger_prefix(w, full);
    size = 1u + w % full;
}

// draw d from work counter x -> the dynamic claim it stands for
constexpr uint32_t CLAIM_SHARDS = 8;
constexpr uint32_t CLAIM_COUNTER_STRIDE = 32;                // u32 words from one counter to the next: a 128-byte line each
BNS_CLAIMS_HD uint32_t claim_shard_global(uint32_t d, uint32_t x) { return d * CLAIM_SHARDS + x; }

// dynamic claim d -> its first unit
BNS_CLAIMS_HD uint32_t claim_dynamic_base(uint32_t dyn_base, uint32_t d, uint32_t full) { return dyn_base + d * full; }

BNS_CLAIMS_HD uint32_t claim_cnt(uint32_t base, uint32_t size, uint32_t n_units)
{
    const uint32_t left = n_units - base;
    return left < size ? left : size;
}

// Host side.  The launch geometry: units per claim as ClassifyForm reports them (`full` for a batch that gives every one of the
// max_blocks * 4 resident wavefronts a claim that size, else an even share, at least 4: a claim is an offsets load) and the
// workgroups of 4 wavefronts to launch.
inline void claim_geometry(uint64_t n_units, uint32_t max_blocks, uint32_t full, uint32_t &chunk, uint32_t &grid)
{
    const uint64_t W = (uint64_t)max_blocks * 4u;
    uint64_t share = (n_units + W - 1) / W;
    if (share < 4) share = 4;
    chunk = (uint32_t)(share < full ? share : full);
    const uint64_t need = ((n_units + chunk - 1) / chunk + 3) / 4;
    grid = (uint32_t)(need < max_blocks ? need : max_blocks);
    if (grid < 1) grid = 1;
}

// where the dynamic claims start, for `launched` wavefronts (n_units < 2^32 - 2^22): behind the staggered static part; at
// n_units when the static claims are the whole batch (chunk < full), so that claim 0 already lies past the end
inline uint32_t claim_dynamic_start(uint64_t n_units, uint32_t launched, uint32_t chunk, uint32_t full)
{
    if (chunk < full) return (uint32_t)n_units;
    const uint64_t stat = claim_stagger_prefix(launched, full);
    return (uint32_t)(stat < n_units ? stat : n_units);
}

}  // namespace bns
