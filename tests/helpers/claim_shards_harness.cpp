// Host harness for tests/test_claim_shards.py: bonsai_amd/csrc/bns_claims.hpp compiled on its own, with the eight work counters
// of classify_kernel played on the host.  A draw from counter x is the kernel's: d = counter[x]++, global claim index
// claim_shard_global(d, x), base claim_dynamic_base(dyn_base, g, full) in 32-bit arithmetic, "past the end" when base >= n_units.
#include <cstdint>
#include <vector>
#include "../../bonsai_amd/csrc/bns_claims.hpp"

using namespace bns;

namespace {
struct Rng {                                                 // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9E3779B97F4A7C15ULL); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL; z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL; return z ^ (z >> 31); }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
};

struct Deal {
    uint32_t chunk, grid, full, n, dyn_base;
    uint32_t counter[CLAIM_SHARDS] = {0};
    bool dry[CLAIM_SHARDS] = {false};
    uint64_t covered = 0, slots = 0;
    std::vector<uint64_t> seen;                              // one bit per full-sized slot of the dynamic part
    int err = 0;
    Deal(uint64_t n_units, uint32_t max_blocks, uint32_t full_) : full(full_), n((uint32_t)n_units)
    {
        claim_geometry(n_units, max_blocks, full, chunk, grid);
        dyn_base = claim_dynamic_start(n_units, grid * 4u, chunk, full);
        slots = ((uint64_t)n - dyn_base + full - 1) / full;
        seen.assign((slots + 63) / 64, 0);
    }
    void fail(int e) { if (!err) err = e; }
    // the static claims, by wavefront: they tile [0, dyn_base) in order
    void statics()
    {
        uint64_t at = 0;
        for (uint32_t w = 0; w < grid * 4u; ++w) {
            uint32_t b, c;
            claim_static(w, chunk, full, b, c);
            if (b >= n) continue;
            c = claim_cnt(b, c, n);
            if (b != at || c == 0) fail(1);
            if (c > full) fail(2);
            at += c;
        }
        if (at != dyn_base) fail(1);
        covered = at;
    }
    // one draw from counter x, as the kernel makes it; false: past the end
    bool draw(uint32_t x)
    {
        const uint32_t d = counter[x]++;
        const uint32_t base = claim_dynamic_base(dyn_base, claim_shard_global(d, x), full);
        if (base >= n) { dry[x] = true; return false; }
        if (dry[x]) fail(4);                                 // a shard that said "past the end" once hands out a claim again
        const uint32_t c = claim_cnt(base, full, n);
        if (c == 0 || c > full) fail(2);
        const uint64_t off = (uint64_t)base - dyn_base, slot = off / full;
        if (off % full || slot >= slots) { fail(1); return true; }
        if (c != (slot + 1 == slots ? n - base : full)) fail(1);
        if (seen[slot >> 6] >> (slot & 63) & 1) fail(3);     // a unit dealt out twice
        seen[slot >> 6] |= 1ULL << (slot & 63);
        covered += c;
        return true;
    }
    bool all_dry() const { for (bool b : dry) if (!b) return false; return true; }
};
}  // namespace

extern "C" {

// Draw all eight counters dry in a given order and check the tiling.  order 0: round-robin over the shards that are not dry yet; 1: shard
// `first` drained before the others are touched, then round-robin; 2: a random shard every draw (seeded), the dry ones included
// (small batches only: the kernel draws a dry shard once per wavefront, and the 32-bit base allows for no more).  Every shard is
// drawn `extra` more times after all of them ran dry.  0 = all properties hold, else the first that does not:
//   1 static and dynamic claims do not tile [0, n_units)   2 an empty claim, or one of more than `full` units
//   3 a unit dealt out twice   4 a shard that was past the end handed out a claim again
//   5 eight dry shards, and units that nobody was given   6 the small-batch path (no counter) has a dynamic part
int shards_drain(uint64_t n_units, uint32_t max_blocks, uint32_t full, int order, uint32_t first, uint32_t extra, uint64_t seed)
{
    Deal d(n_units, max_blocks, full);
    d.statics();
    if (d.chunk < full) return d.err ? d.err : (d.dyn_base == d.n && d.covered == n_units ? 0 : 6);
    Rng r{seed};
    if (order == 1) while (d.draw(first & 7u)) {}
    if (order == 2) { while (!d.all_dry()) d.draw(r.below(CLAIM_SHARDS)); }
    else for (uint32_t x = 0; !d.all_dry(); x = (x + 1) & 7u) { if (!d.dry[x]) d.draw(x); }
    if (d.covered != n_units) d.fail(5);
    for (uint32_t x = 0; x < CLAIM_SHARDS; ++x)
        for (uint32_t k = 0; k < extra; ++k) if (d.draw(x)) d.fail(4);
    return d.err;
}

// The kernel's own loop, wavefront by wavefront: grid * 4 wavefronts, wavefront w at home on shard home(w) (w & 7 with by_wave,
// else a random XCD per workgroup); a random wavefront takes the next step each time (seeded).  A step is one draw from the
// wavefront's current shard; past the end, it draws from (x + s) & 7 for s = 1 .. 7 on the spot and leaves after the eighth dry
// shard.  Checked beside the properties above: when the FIRST wavefront leaves, the batch is dealt out (5); no wavefront makes
// more than seven draws past the end beyond its first (7); *max_base_over = the farthest any draw's index lay past the last claim,
// in units (it must stay below 2^22 for the 32-bit base not to wrap).
int shards_waves(uint64_t n_units, uint32_t max_blocks, uint32_t full, int by_wave, uint64_t seed, uint64_t *max_base_over)
{
    Deal d(n_units, max_blocks, full);
    d.statics();
    *max_base_over = 0;
    if (d.chunk < full) return d.err ? d.err : (d.dyn_base == d.n && d.covered == n_units ? 0 : 6);
    Rng r{seed};
    const uint32_t W = d.grid * 4u;
    std::vector<uint8_t> shard(W), dry_seen(W, 0);
    std::vector<uint32_t> live(W);
    uint32_t xcd0 = r.below(8);
    for (uint32_t w = 0; w < W; ++w) { shard[w] = (uint8_t)(by_wave ? (w & 7u) : ((w / 4u + xcd0) & 7u)); live[w] = w; }
    uint32_t n_live = W;
    bool first_left = false;
    while (n_live) {
        const uint32_t i = r.below(n_live), w = live[i];
        bool got = d.draw(shard[w]);
        while (!got && ++dry_seen[w] < CLAIM_SHARDS) {       // the shard ran dry: the next one, on the spot
            shard[w] = (uint8_t)((shard[w] + 1u) & 7u);
            got = d.draw(shard[w]);
        }
        if (got) continue;
        if (!first_left) { first_left = true; if (d.covered != n_units) d.fail(5); }
        if (dry_seen[w] != CLAIM_SHARDS) d.fail(7);
        live[i] = live[--n_live];
    }
    if (d.covered != n_units || !d.all_dry()) d.fail(5);
    for (uint32_t x = 0; x < CLAIM_SHARDS; ++x) {
        if (d.counter[x] > (d.slots + 7) / 8 + W + 1) d.fail(7);                 // at most one draw past the end per wavefront and shard
        const uint64_t g = (uint64_t)(d.counter[x] - 1u) * CLAIM_SHARDS + x;     // the farthest draw of this shard
        const uint64_t over = g >= d.slots ? (g - d.slots + 1) * full : 0;
        if (over > *max_base_over) *max_base_over = over;
    }
    return d.err;
}

}
