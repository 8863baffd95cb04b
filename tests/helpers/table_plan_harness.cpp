// Host harness for tests/test_table_plan.py: bonsai_amd/csrc/bns_table_plan.hpp compiled on its own (it needs no HIP), its
// functions as the table load (bns_table_load.hpp) calls them.
#include <cstdint>
#include <cstring>
#include "../../bonsai_amd/csrc/bns_table_plan.hpp"

using namespace bns;

namespace {
// candidates out as rows of (m, len, shift, canon, wide, span); returns how many
uint32_t rows(const PlanCands &c, uint32_t *out6)
{
    for (uint32_t i = 0; i < c.n; ++i) {
        const uint32_t r[6] = {c.c[i].m, c.c[i].len, c.c[i].shift, c.c[i].canon, c.c[i].wide, c.span[i]};
        std::memcpy(out6 + 6 * i, r, sizeof(r));
    }
    return c.n;
}
}  // namespace

extern "C" {

// [0] MINB_CAP, [1] MINB_MAX_CHAIN, [2] PLAN_MAX_CANDS, [3..8] MIN_CANDS as (span, floor) pairs; returns MINB_TARGET_LOAD
double plan_constants(uint32_t *out9)
{
    out9[0] = MINB_CAP; out9[1] = MINB_MAX_CHAIN; out9[2] = PLAN_MAX_CANDS;
    for (int i = 0; i < 3; ++i) { out9[3 + 2 * i] = MIN_CANDS[i].span; out9[4 + 2 * i] = MIN_CANDS[i].floor; }
    return MINB_TARGET_LOAD;
}

uint32_t plan_minimizer_len(uint32_t k, uint32_t span, uint32_t floor) { return minimizer_len(k, MinCand{span, floor}); }

// the BNS_ERR_* code; *n_mb and msg (up to 127 characters) are written as the function leaves them
int plan_size_minbucket(uint64_t n_present, uint64_t free_b, uint64_t n_buckets_req, uint32_t slots_log2_req, uint64_t *n_mb, char *msg128)
{
    const char *msg = "";
    const int rc = plan_minbucket_buckets(n_present, (size_t)free_b, n_buckets_req, slots_log2_req, *n_mb, msg);
    std::strncpy(msg128, msg, 127); msg128[127] = 0;
    return rc;
}

int plan_size_bucket(uint64_t n_buckets, uint64_t free_b, uint32_t slots_log2_req, uint32_t *slots_log2, char *msg128)
{
    const char *msg = "";
    const int rc = plan_bucket_slots(n_buckets, (size_t)free_b, slots_log2_req, *slots_log2, msg);
    std::strncpy(msg128, msg, 127); msg128[127] = 0;
    return rc;
}

uint32_t plan_list_spaced(uint32_t k, uint64_t n_present, uint32_t run_len, uint32_t run_shift, int dbg, uint32_t *out36)
{
    return rows(plan_cands_spaced(k, n_present, run_len, run_shift, dbg), out36);
}

uint32_t plan_list_contiguous(uint32_t k, uint32_t min_span_req, int wide_req, uint32_t *out36)
{
    return rows(plan_cands_contiguous(k, min_span_req, wide_req), out36);
}

// the pick among n candidates whose `wide` flags are given, from the trial's 3 counters per candidate
uint32_t plan_pick_of(uint32_t n, const uint32_t *wide, int spaced, const unsigned long long *tr, double *miss)
{
    PlanCands c;
    for (uint32_t i = 0; i < n; ++i) c.add(MinSpec{0u, 0u, 0u, 1u, wide[i]}, 0u);
    return plan_pick(c, spaced != 0, tr, *miss);
}

int plan_fill(uint32_t n_cands, double trial_miss, uint64_t n_present, uint64_t n_mb, int fill_req, int dbg)
{
    return plan_group_fill(n_cands, trial_miss, n_present, n_mb, fill_req, dbg) ? 1 : 0;
}

uint64_t plan_ovf_slots(uint64_t n_ovf_keys, uint64_t n_alloc, int dbg) { return plan_overflow_slots(n_ovf_keys, n_alloc, dbg); }
uint32_t plan_sample(uint64_t n_mb) { return plan_trial_sample(n_mb); }
int plan_stream(uint64_t n_buckets, uint64_t free_b, int dbg) { return plan_stream_load(n_buckets, (size_t)free_b, dbg) ? 1 : 0; }

}
