// bns_classify_plan.hpp -- what a classify launch DECIDES: which instantiation of classify_kernel and of classify_overflow_kernel a
// call runs, which form of the overflow-table lookup is in force, whether a unit of the batch can overflow the in-LDS counter, how
// many units a batch may hold, how much scratch a windowed encode needs.  Plain arithmetic on a handful of numbers; the launches that
// act on the answers are bns_classify.hpp.  The rule is stated ONCE, in choose_form / choose_overflow_form, and the instantiations
// that exist are its image over everything the API accepts (CLASSIFY_FORMS / OVERFLOW_FORMS): the launcher walks those two lists,
// so a form is compiled if and only if some call can reach it.  Nothing here needs HIP (tests/test_classify_plan.py compiles this
// header on its own and holds it against the rule restated in tests/classify_forms.py).
#pragma once
#include <array>
#include <cstddef>
#include "bns_table_plan.hpp"     // MIN_CANDS, minimizer_len: the windows a loaded table can have

namespace bns {

// bns_debug_set bits a classify launch reads (tests and profiling; 0 in production; the other bits: bns_api.hip, bns_table_plan.hpp)
constexpr int BNS_DBG_OVC_OFF = 0x2000;             // classify: never the cooperative overflow lookup (A/B of the two forms)
constexpr int BNS_DBG_OVC_ON = 0x8000;              // classify: always the cooperative overflow lookup
constexpr int BNS_DBG_SHARD_BY_WAVE = 0x200000;     // classify_kernel: a wavefront's work counter by its index & 7 instead of its XCD (tests: two workgroups reach all eight counters and the stealing; same results)

constexpr u32 LDS_CAP = 128;   // distinct taxa per unit held in LDS; beyond that the overflow kernel takes over

// The template arguments of classify_kernel<SPACED, LAYOUT, KT, NM, SPAN, OVC, WIDE, PACKED> ...
struct ClassifyFormKey {
    bool spaced; int layout, kt, nm, span; bool ovc, wide, packed;
    constexpr bool operator==(const ClassifyFormKey &o) const
    {
        return spaced == o.spaced && layout == o.layout && kt == o.kt && nm == o.nm && span == o.span && ovc == o.ovc && wide == o.wide && packed == o.packed;
    }
};
// ... and of classify_overflow_kernel<SPACED, LAYOUT, WIDE, PACKED>
struct OverflowFormKey {
    bool spaced; int layout; bool wide, packed;
    constexpr bool operator==(const OverflowFormKey &o) const { return spaced == o.spaced && layout == o.layout && wide == o.wide && packed == o.packed; }
};

// ---- the rule.  Contiguous canonical seeds on the clustered table with a common k: k, the mates per unit and the minimizer window
// (SPAN = k - m, for the (k, window) pairs the loader can produce) are compile-time constants -- k = 31 in every form (either
// overflow lookup, either minimizer identity, or packed input in the usual form), k = 21, 25, 27, 32 in the usual form only (per-lane
// overflow lookup, 32-bit identity, ASCII input).  Everything else -- another k, a window no MIN_CANDS entry gives, non-canonical
// contiguous seeds, spaced seeds, the other layouts, packed input with the cooperative lookup or the wide identity -- runs a generic
// kernel that reads k from its arguments: KT = NM = 0, SPAN = GENERIC_SPAN (unused), OVC = 0, one per (SPACED, LAYOUT, PACKED) and
// on the clustered table one more per PACKED for the wide identity.
constexpr u32 FIXED_K_FULL = 31;
constexpr u32 FIXED_K_USUAL[4] = {21, 25, 27, 32};
constexpr int GENERIC_SPAN = 8;

constexpr bool fixed_k_window(u32 k, u32 m)
{
    bool common = k == FIXED_K_FULL;
    for (u32 ku : FIXED_K_USUAL) common = common || k == ku;
    if (!common) return false;
    for (const MinCand &c : MIN_CANDS) if (minimizer_len(k, c) == m) return true;
    return false;
}

// k, canon, spaced, layout: the encoder and the loaded table; m: the table's minimizer length (read on the clustered table only);
// table_wide: its identity; heavy: ovf_heavy() below; packed: the input; nmates: 1 or 2
constexpr ClassifyFormKey choose_form(u32 k, u32 m, bool canon, bool spaced, int layout, bool table_wide, bool heavy, bool packed, int nmates)
{
    const int ly = layout == BNS_LAYOUT_MINBUCKET ? 2 : (layout == BNS_LAYOUT_BUCKET ? 1 : 0);
    const bool clustered = !spaced && ly == 2;
    const bool wide = clustered && table_wide;
    if (clustered && canon && fixed_k_window(k, m)) {
        const int nm = nmates == 1 ? 1 : 2;
        if (!(heavy || wide || packed)) return {false, 2, (int)k, nm, (int)(k - m), false, false, false};
        if (k == FIXED_K_FULL && !(packed && (heavy || wide))) return {false, 2, (int)k, nm, (int)(k - m), heavy, wide, packed};
    }
    return {spaced, ly, 0, 0, GENERIC_SPAN, false, wide, packed};
}

// units with more than LDS_CAP distinct taxa go on to classify_overflow_kernel; WIDE again only on the clustered table with contiguous seeds
constexpr OverflowFormKey choose_overflow_form(bool spaced, int layout, bool table_wide, bool packed)
{
    const int ly = layout == BNS_LAYOUT_MINBUCKET ? 2 : (layout == BNS_LAYOUT_BUCKET ? 1 : 0);
    return {spaced, ly, !spaced && ly == 2 && table_wide, packed};
}

// the form of the overflow-table lookup: cooperative when more than 1 key in 1000 lives there (see probe_minbucket); the debug bits
// force it on or off, on wins
constexpr bool ovf_heavy(int dbg, u64 n_ovf_keys, u64 n_keys)
{
    return (dbg & BNS_DBG_OVC_ON) || (!(dbg & BNS_DBG_OVC_OFF) && n_ovf_keys * 1000ULL > n_keys);
}

// a unit can hold more than LDS_CAP distinct taxa only if it has more than LDS_CAP k-mers: the launch then keeps an overflow list and
// reads its count back
constexpr u64 max_unit_kmers(int nmates, u32 max_read_len, u32 c) { return max_read_len >= c ? (u64)nmates * (max_read_len - c + 1) : 0; }
constexpr bool unit_can_overflow(int nmates, u32 max_read_len, u32 c) { return max_unit_kmers(nmates, max_read_len, c) > LDS_CAP; }

// units of one batch (headroom below 2^32: every wavefront draws one claim past the end)
constexpr u64 MAX_CLASSIFY_UNITS = (1ULL << 32) - (1ULL << 22);
constexpr bool too_many_units(u64 n_units) { return n_units >= MAX_CLASSIFY_UNITS; }

// windows over the emitted stream (-C, real-entropy score) wider than 64 k-mers keep their queue image in global memory: bytes of
// scratch for a grid of 4-wavefront workgroups, 0 when the window fits LDS or runs over positions
constexpr size_t win_scratch_bytes(bool spaced, bool canon, int score, u32 win, u32 c, unsigned grid)
{
    const bool stream_windows = !spaced && (!canon || score == BNS_SCORE_ENTROPY_STRING);
    if (!stream_windows || win <= c || win - c + 1 <= 64) return 0;
    return (size_t)grid * 4 * ((size_t)2 * (win - c + 65u) * 8);
}

// ---- the forms that exist: the image of the rule over what the API accepts -- k = 1 .. 32, either strand rule, contiguous or spaced
// (a 1-mer has no gaps), the three layouts, every window the loader can build a table with, either identity where there is a window to
// carry it, either overflow lookup, ASCII or packed, one or two mates.  This is the only place that names instantiations.
template <class K, size_t CAP>
struct FormSet {
    K v[CAP] = {};
    size_t n = 0;
    constexpr bool has(const K &key) const { for (size_t i = 0; i < n; ++i) if (v[i] == key) return true; return false; }
    constexpr void add(const K &key) { if (!has(key)) v[n++] = key; }      // (past CAP: not a constant expression, the build stops)
};
struct FormSets { FormSet<ClassifyFormKey, 96> kern; FormSet<OverflowFormKey, 24> ovf; };

constexpr FormSets enumerate_forms()
{
    FormSets s;
    for (u32 k = 1; k <= 32; ++k)
        for (int spaced = 0; spaced < 2; ++spaced)
            for (int layout = 0; layout < 3; ++layout) {
                if (spaced && k < 2) continue;
                const bool clustered = !spaced && layout == 2;
                for (u32 ci = 0; ci < (clustered ? 3u : 1u); ++ci)
                    for (int wide = 0; wide < (clustered ? 2 : 1); ++wide) {
                        const u32 m = clustered ? minimizer_len(k, MIN_CANDS[ci]) : k;
                        if (wide && m >= k) continue;
                        for (int bits = 0; bits < 16; ++bits) {
                            const bool canon = bits & 1, heavy = bits & 2, packed = bits & 4;
                            s.kern.add(choose_form(k, m, canon && !spaced, spaced, layout, wide, heavy, packed, (bits & 8) ? 2 : 1));
                            s.ovf.add(choose_overflow_form(spaced, layout, wide, packed));
                        }
                    }
            }
    return s;
}
constexpr FormSets FORM_SETS = enumerate_forms();

template <size_t N, class K, size_t CAP>
constexpr std::array<K, N> form_list(const FormSet<K, CAP> &s)
{
    std::array<K, N> a{};
    for (size_t i = 0; i < N; ++i) a[i] = s.v[i];
    return a;
}
constexpr auto CLASSIFY_FORMS = form_list<FORM_SETS.kern.n>(FORM_SETS.kern);
constexpr auto OVERFLOW_FORMS = form_list<FORM_SETS.ovf.n>(FORM_SETS.ovf);

}  // namespace bns
