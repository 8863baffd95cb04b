// Host harness for tests/test_claim_schedule.py: bonsai_amd/csrc/bns_claims.hpp compiled on its own (it needs no HIP), the way the
// launcher (claim_geometry, claim_dynamic_start) and the kernel (claim_static, claim_dynamic_base, claim_cnt) use it.
#include <cstdint>
#include "../../bonsai_amd/csrc/bns_claims.hpp"

using namespace bns;

namespace {
struct Deal {
    uint32_t chunk, grid, full, n, dyn_base;
    Deal(uint64_t n_units, uint32_t max_blocks, uint32_t full_) : full(full_), n((uint32_t)n_units)
    {
        claim_geometry(n_units, max_blocks, full, chunk, grid);
        dyn_base = claim_dynamic_start(n_units, grid * 4u, chunk, full);
    }
    // what the kernel does with a wavefront's first claim / with claim index d: false when there is nothing to take
    bool stat(uint32_t w, uint32_t &base, uint32_t &cnt) const
    {
        claim_static(w, chunk, full, base, cnt);
        if (base >= n) return false;
        cnt = claim_cnt(base, cnt, n);
        return true;
    }
    bool dyn(uint32_t d, uint32_t &base, uint32_t &cnt) const
    {
        base = claim_dynamic_base(dyn_base, d, full);
        if (base >= n) return false;
        cnt = claim_cnt(base, full, n);
        return true;
    }
};
}  // namespace

extern "C" {

// chunk and grid as the launcher reports them, and where the dynamic claims start
void claims_geometry(uint64_t n_units, uint32_t max_blocks, uint32_t full, uint32_t *chunk, uint32_t *grid, uint32_t *dyn_base)
{
    Deal d(n_units, max_blocks, full);
    *chunk = d.chunk; *grid = d.grid; *dyn_base = d.dyn_base;
}

// every claim of the launch in the order (static by wavefront, then dynamic by index): base[], cnt[]; returns how many there are
// (more than cap: only the first cap are written), *n_static = how many of them are static
uint64_t claims_list(uint64_t n_units, uint32_t max_blocks, uint32_t full, uint32_t *base, uint32_t *cnt, uint64_t cap, uint64_t *n_static)
{
    Deal d(n_units, max_blocks, full);
    uint64_t k = 0;
    uint32_t b, c;
    for (uint32_t w = 0; w < d.grid * 4u; ++w)
        if (d.stat(w, b, c)) { if (k < cap) { base[k] = b; cnt[k] = c; } ++k; }
    *n_static = k;
    if (d.chunk == full)                                     // (the kernel is given no counter otherwise)
        for (uint32_t i = 0; d.dyn(i, b, c); ++i) { if (k < cap) { base[k] = b; cnt[k] = c; } ++k; }
    return k;
}

// The properties of tests/test_claim_schedule.py checked claim by claim without storing them (the large batches of the sweep);
// 0 = all hold, else the number of the first that does not:
//   1 the static claims, by wavefront, and the dynamic ones behind them, by index, do not tile [0, n_units) in that order
//   2 a claim of more than `full` units, or one whose offsets (cnt * mates + 1, mates = 2) do not fit 64 lanes
//   3 a dynamic claim larger than the one before it
//   4 a wavefront with nothing static to take in front of one that has, or an empty claim
//   5 one of the grid * 4 claim indices past the last one that does not say "past the end"
//   7 a small batch (chunk < full) whose claim 0 does not lie past the end, or whose chunk is not the even share (at least 4)
int claims_verify(uint64_t n_units, uint32_t max_blocks, uint32_t full)
{
    Deal d(n_units, max_blocks, full);
    const uint64_t W = (uint64_t)max_blocks * 4u;
    uint64_t at = 0;
    uint32_t b, c;
    bool dry = false;
    for (uint32_t w = 0; w < d.grid * 4u; ++w) {
        if (!d.stat(w, b, c)) { dry = true; continue; }
        if (dry || c == 0) return 4;
        if (b != at) return 1;
        if (c > full || c * 2u + 1u > 64u) return 2;
        at += c;
    }
    uint64_t share = (n_units + W - 1) / W;
    if (share < 4) share = 4;
    if (d.chunk != (share < full ? share : full)) return 7;
    if (d.chunk < full) {
        if (d.dyn(0, b, c)) return 7;
        return at == n_units ? 0 : 1;
    }
    uint32_t prev = full, i = 0;
    for (; d.dyn(i, b, c); ++i) {
        if (c == 0) return 4;
        if (b != at) return 1;
        if (c > full || c * 2u + 1u > 64u) return 2;
        if (c > prev) return 3;
        prev = c;
        at += c;
    }
    if (at != n_units) return 1;
    for (uint32_t k = 0; k < d.grid * 4u; ++k)
        if (d.dyn(i + k, b, c)) return 5;
    return 0;
}

}
