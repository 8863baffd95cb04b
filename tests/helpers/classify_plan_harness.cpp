// Host harness for tests/test_classify_plan.py: bonsai_amd/csrc/bns_classify_plan.hpp compiled on its own (it needs no HIP), its
// functions as the classify launch path (bns_classify.hpp) calls them.
#include <cstdint>
#include "../../bonsai_amd/csrc/bns_classify_plan.hpp"

using namespace bns;

namespace {
void put(const ClassifyFormKey &f, int *o) { o[0] = f.spaced; o[1] = f.layout; o[2] = f.kt; o[3] = f.nm; o[4] = f.span; o[5] = f.ovc; o[6] = f.wide; o[7] = f.packed; }
void put(const OverflowFormKey &f, int *o) { o[0] = f.spaced; o[1] = f.layout; o[2] = f.wide; o[3] = f.packed; }
}  // namespace

extern "C" {

// [0] LDS_CAP, [1] BNS_DBG_OVC_OFF, [2] BNS_DBG_OVC_ON, [3] MAX_CLASSIFY_UNITS
void cplan_constants(uint64_t *out4) { out4[0] = LDS_CAP; out4[1] = BNS_DBG_OVC_OFF; out4[2] = BNS_DBG_OVC_ON; out4[3] = MAX_CLASSIFY_UNITS; }

void cplan_choose(uint32_t k, uint32_t m, int canon, int spaced, int layout, int table_wide, int heavy, int packed, int nmates, int *out8)
{
    put(choose_form(k, m, canon != 0, spaced != 0, layout, table_wide != 0, heavy != 0, packed != 0, nmates), out8);
}

void cplan_choose_overflow(int spaced, int layout, int table_wide, int packed, int *out4)
{
    put(choose_overflow_form(spaced != 0, layout, table_wide != 0, packed != 0), out4);
}

// the two lists of forms that exist, as rows of 8 / 4 ints; returns how many rows there are (written: at most cap)
int cplan_forms(int *out, int cap)
{
    for (size_t i = 0; i < CLASSIFY_FORMS.size() && (int)i < cap; ++i) put(CLASSIFY_FORMS[i], out + 8 * i);
    return (int)CLASSIFY_FORMS.size();
}
int cplan_overflow_forms(int *out, int cap)
{
    for (size_t i = 0; i < OVERFLOW_FORMS.size() && (int)i < cap; ++i) put(OVERFLOW_FORMS[i], out + 4 * i);
    return (int)OVERFLOW_FORMS.size();
}

int cplan_ovf_heavy(int dbg, uint64_t n_ovf_keys, uint64_t n_keys) { return ovf_heavy(dbg, n_ovf_keys, n_keys) ? 1 : 0; }
uint64_t cplan_max_unit_kmers(int nmates, uint32_t max_read_len, uint32_t c) { return max_unit_kmers(nmates, max_read_len, c); }
int cplan_can_overflow(int nmates, uint32_t max_read_len, uint32_t c) { return unit_can_overflow(nmates, max_read_len, c) ? 1 : 0; }
int cplan_too_many_units(uint64_t n_units) { return too_many_units(n_units) ? 1 : 0; }
uint64_t cplan_win_scratch(int spaced, int canon, int score, uint32_t win, uint32_t c, unsigned grid)
{
    return win_scratch_bytes(spaced != 0, canon != 0, score, win, c, grid);
}

}
