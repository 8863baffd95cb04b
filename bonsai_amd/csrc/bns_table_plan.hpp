// bns_table_plan.hpp -- what a table load DECIDES: how many buckets, which minimizer candidates go into the trial, which one wins,
// how the table is filled, how large the overflow table is, whether the khash arrays are uploaded or streamed.  Plain arithmetic
// on a handful of numbers; the launches that produce those numbers and act on the answers are bns_table_load.hpp.  The answers
// of one load are a TablePlan: the root of a multi-context load decides, every replica is handed the root's plan and follows it.
// Nothing here needs HIP (tests/test_table_plan.py compiles this header on its own); the constants and small types the decisions
// share with the kernels live here and reach device code through bns_device.hpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "../../include/bonsai_amd.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BNS_PLAN_HD __device__ __host__
#else
#define BNS_PLAN_HD
#endif

namespace bns {

using u32 = uint32_t;
using u64 = uint64_t;

// bns_debug_set bits the table load reads (tests and profiling; 0 in production; the other bits: bns_api.hip)
constexpr int BNS_DBG_PLAIN_FILL = 0x10;            // bns_load_table: keys in arrival order even into a crowded table (A/B of the group-aware fill)
constexpr int BNS_DBG_GROUP_FILL = 0x20;            // bns_load_table: the group-aware fill even for a table with room (tests reach it on small tables)
constexpr int BNS_DBG_PLACE_FAIL = 0x100;           // every 61st bucket pretends to have no perfect hash (-> overflow table)
constexpr int BNS_DBG_SPACED_NOCLUSTER = 0x200;     // spaced seeds: m = k, every k-mer its own bucket
constexpr int BNS_DBG_STREAM_LOAD = 0x1000;         // bns_load_table streams the host arrays even when they would fit
constexpr int BNS_DBG_STREAM_CHUNK_SHIFT = 16, BNS_DBG_STREAM_CHUNK_MASK = 0x1F << 16;   // log2 of the streamed chunk (0 = 27)
constexpr int BNS_DBG_SPACED_M_SHIFT = 24, BNS_DBG_SPACED_M_MASK = 0x1F << 24;           // spaced seeds: force the run minimizer's m

constexpr u32 MINB_CAP = 10;                   // keys of a MinBucket (bns_device.hpp)
constexpr u32 MINB_MAX_CHAIN = 4;              // a key lives in one of its first 4 buckets (40 keys) or in the overflow table
// a clustered table is filled to this fraction of its 10 keys per bucket unless the caller fixes its size: the knee of the
// load sweep (profiles/): kernel time within 2 % of a table eight times the size, a quarter of the memory of round 2's default
constexpr double MINB_TARGET_LOAD = 1.0 / 12.0;

// Minimizer length m (contiguous seeds): the window of a k-mer is its k - m + 1 m-mers.  A wider window means fewer minimizer runs
// per read (density 2 / (k - m + 2): 25 bucket fetches per 150-bp read at k - m = 8, 16 at 15) but groups of up to k - m + 1
// keys -- of which a bucket holds 10.  Which one a table uses is decided when it is loaded (bns_load_table_device): a db of every
// k-mer fills its groups and needs the narrow window; a db of window minimizers (bonsai build -w 50: one k-mer in ten) leaves
// them nearly empty and takes the wide one.  m never goes below `floor`: 4^m must dwarf the number of minimizer groups.  The
// wide candidate is k - 15 rather than k - 14 because for k = 31 that is m = 16: an m-mer that fits ONE word, whose canonical
// form is a v_min_u32 (round_minhash) -- 2 % faster than m = 17, while m = 15 (k - 16) puts unrelated k-mers into one group.
struct MinCand { u32 span, floor; };
constexpr MinCand MIN_CANDS[3] = {{15u, 16u}, {11u, 19u}, {8u, 19u}};        // widest first; the last one always fits (groups <= 9)
BNS_PLAN_HD constexpr u32 minimizer_len(u32 k, MinCand c) { return k <= c.floor ? k : (k - c.span > c.floor ? k - c.span : c.floor); }
BNS_PLAN_HD constexpr u32 minimizer_len(u32 k) { return minimizer_len(k, MIN_CANDS[2]); }     // the narrow window
// Which part of a key the minimizer is taken from: m-mers of `len` consecutive key bases whose last base sits `shift` bits above
// the key's low end.  Contiguous seeds: the whole key (len = k, shift = 0), canonical m-mers -- the m-mer sets of a k-mer and of
// its reverse complement coincide.  Spaced seeds: the k sampled bases are not consecutive in the read except inside a run of
// adjacent sampled positions; the LONGEST such run (16 bases for 1x15,0x15) is the only thing neighbouring spaced k-mers share
// position by position (k-mers j and j+1 overlap in len-1 of its bases), so the minimizer is taken inside it, over plain m-mers
// (spaced k-mers are never canonicalised, encoder.h:148-150).  len == m == k: no clustering, the one m-mer.
struct MinSpec { u32 m, len, shift, canon, wide; };

// Everything a load decides and a replica must repeat.
struct TablePlan {
    int layout = -1;                // BNS_LAYOUT_BUCKET or BNS_LAYOUT_MINBUCKET
    u32 slots_log2 = 0;             // BUCKET: the table is 2^slots_log2 16-byte slots
    u64 n_mb = 0;                   // MINBUCKET: buckets a key can call home
    MinSpec spec = {0, 0, 0, 1, 0}; // MINBUCKET: where the minimizer comes from
    u32 span = 0;                   // ... and the MIN_CANDS span it came from (0: none -- a spaced seed)
    bool group_fill = false;        // MINBUCKET: filled group by group
};

// the minimizer candidates of one load, in trial order: at most two identities x three windows (minbucket_trial_kernel's TrialCands
// holds as many)
constexpr u32 PLAN_MAX_CANDS = 6;
struct PlanCands {
    MinSpec c[PLAN_MAX_CANDS];
    u32 span[PLAN_MAX_CANDS];
    u32 n = 0;
    void add(MinSpec s, u32 sp) { c[n] = s; span[n] = sp; ++n; }
};

// a db whose arrays and a useful table (16 bytes per khash bucket) do not fit the HBM together is streamed from the host
// buffers instead of being uploaded whole (BNS_DBG_STREAM_LOAD forces that path: tests)
inline size_t khash_flag_words(u64 n_buckets) { return n_buckets < 16 ? 1 : (size_t)(n_buckets >> 4); }
inline bool plan_stream_load(u64 n_buckets, size_t free_b, int dbg)
{
    const size_t arrays = khash_flag_words(n_buckets) * 4 + (size_t)n_buckets * 12;
    return (dbg & BNS_DBG_STREAM_LOAD) || arrays + (size_t)n_buckets * 16 > free_b / 100 * 85;
}

// plain bucket layout: a power of two of 16-byte slots, 2x the khash bucket count by default; capacity must cover even a
// khash with every slot present, or the fill could never terminate
inline int plan_bucket_slots(u64 n_buckets, size_t free_b, u32 slots_log2_req, u32 &slots_log2, const char *&msg)
{
    u32 lg = 0;
    while ((1ULL << lg) < n_buckets) ++lg;
    u32 want = slots_log2_req ? slots_log2_req : lg + 1;
    if (want < 4) want = 4;
    if (((size_t)16 << want) > free_b) { msg = "bucket table does not fit in free HBM"; return BNS_ERR_NOMEM; }
    if ((1ULL << want) <= n_buckets) { msg = "bucket_slots_log2 too small for this khash"; return BNS_ERR_ARG; }
    slots_log2 = want;
    return BNS_OK;
}

// ---- clustered layout: how many buckets.  Automatic: MINB_TARGET_LOAD, or what fits in three quarters of the free HBM
// (the overflow table and the caller's batches need room too); any count will do, the bucket index is a multiply-high.
inline int plan_minbucket_buckets(u64 n_present, size_t free_b, u64 n_buckets_req, u32 slots_log2_req, u64 &n_mb, const char *&msg)
{
    const u64 mem_cap = (u64)(free_b / 4 * 3 / 128);          // (128: sizeof(MinBucket))
    const u64 hard_cap = (1ULL << 31) - 8;                    // bucket indices are 31-bit
    u64 want = n_buckets_req ? n_buckets_req
             : slots_log2_req ? std::max<u64>(1, (1ULL << slots_log2_req) / 8)
             : std::max<u64>(64, (u64)((double)n_present / (MINB_CAP * MINB_TARGET_LOAD)));
    if (!n_buckets_req && !slots_log2_req) want = std::min(want, mem_cap);
    if (want > hard_cap) {
        if (n_buckets_req || slots_log2_req) { msg = "more than 2^31 buckets: bucket indices are 31-bit"; return BNS_ERR_ARG; }
        want = hard_cap;
    }
    const u64 n_alloc = want + MINB_MAX_CHAIN - 1;            // spill-only buckets behind the last home: chains never wrap
    if (n_alloc * 128 > free_b) { msg = "bucket table does not fit in free HBM"; return BNS_ERR_NOMEM; }
    if ((double)want * MINB_CAP * 0.97 < (double)n_present) { msg = "bucket table too small for the key count"; return BNS_ERR_TABLE; }
    n_mb = want;
    return BNS_OK;
}

// ---- where the minimizer comes from.  Contiguous seeds: canonical m-mers of the whole key.  Spaced seeds: plain m-mers
// inside the mask's longest run of adjacent sampled bases, if there is one long enough -- m is then the smallest length
// with 4^m >= the number of keys (so that minimizer groups rarely share a value: groups are 2-3 keys, a bucket holds 10),
// at least run - 8 (a group must fit a bucket) and at most run - 1 (a window of two m-mers is the least that lets
// neighbours share); otherwise m = k: every k-mer its own bucket.
inline PlanCands plan_cands_spaced(u32 k, u64 n_present, u32 run_len, u32 run_shift, int dbg)
{
    PlanCands cands;
    MinSpec ms{k, k, 0u, 1u, 0u};
    const u32 R = run_len;
    if (R >= 12 && !(dbg & BNS_DBG_SPACED_NOCLUSTER)) {
        u32 m = 11;
        while (m < 32 && (1ULL << (2 * m)) < n_present) ++m;
        const int force = (dbg & BNS_DBG_SPACED_M_MASK) >> BNS_DBG_SPACED_M_SHIFT;
        if (force) m = (u32)std::max(8, force);   // profiling aid
        const bool forced = force != 0;
        if (m + 8 < R) m = R - 8;
        // one base shorter is tried first: a window of one more m-mer means a third fewer bucket fetches per run, and a kernel
        // bound by its fetches gains from that as long as the groups still fit -- accepted below when fewer than 5 keys in
        // 100 miss their home bucket (configs[2]'s 7.8e8-key db: m = 14 instead of 15, 4.4 % outside, 14.28 -> 13.45 ms; a
        // 2.3e8-key db: m = 13 would leave 19 % outside, 12.1 -> 16.6 ms, and is refused)
        if (!forced && m >= 9 && m + 7 >= R && m <= R) cands.add(MinSpec{m - 1, R, run_shift, 0u, 0u}, 0u);
        if (m + 1 <= R) ms = MinSpec{m, R, run_shift, 0u, 0u};
    }
    cands.add(ms, 0u);
    return cands;
}

// Contiguous seeds: the widest minimizer window whose groups still fit their buckets (MIN_CANDS: k - m = 15, 11, 8; a
// wider window means fewer bucket fetches per read -- 16 instead of 25 per 150-bp read -- but groups of up to k - m + 1
// keys in buckets of 10).  A candidate is taken when fewer than 1 key in 100 misses its home bucket when the table is
// filled with it (tools/span_calib.sh); the last one always is.  A db of every k-mer fails the wide windows at once and
// ends at 8; a db of window minimizers (bonsai build -w 50: one k-mer in ten) takes 15.  bns_set_minimizer_span() fixes
// the window, bns_set_minimizer_identity() the identity (default: wide from WIDE_MIN_KEYS keys on).
inline PlanCands plan_cands_contiguous(u32 k, u32 min_span_req, int wide_req)
{
    PlanCands cands;
    // the identity: fixed by bns_set_minimizer_identity(), else both forms go into the trial (narrow ones first)
    for (u32 wide = 0; wide < 2; ++wide) {
        if (wide_req >= 0 && (u32)wide_req != wide) continue;
        for (int ci = 0; ci < 3; ++ci) {
            const MinCand cand = MIN_CANDS[ci];
            if (min_span_req && cand.span != min_span_req) continue;
            const u32 m = minimizer_len(k, cand);
            if (wide && m >= k) continue;           // (no window, nothing to carry through it)
            if (cands.n && cands.c[cands.n - 1].m == m && cands.c[cands.n - 1].wide == wide) continue;
            cands.add(MinSpec{m, k, 0u, 1u, wide}, cand.span);
        }
    }
    // (the wide identity asked for, but k so small that there is no window to carry it through: the narrow form it is)
    if (!cands.n) cands.add(MinSpec{minimizer_len(k, MIN_CANDS[2]), k, 0u, 1u, 0u}, MIN_CANDS[2].span);
    return cands;
}

// buckets the trial samples: every bucket for a small table, one in 2^j for a large one
inline u32 plan_trial_sample(u64 n_mb)
{
    u32 sample = (u32)n_mb;
    while (sample > (1u << 22)) sample >>= 1;               // at most 4 M sampled buckets: plenty of groups
    return sample;
}

// ---- choose, from minbucket_trial_kernel's three counters per candidate (tr[3 c + {0,1,2}] = keys sampled / spilled / chain
// exhausted).  Returns the winner's index; miss = its share of keys outside their home bucket.
inline u32 plan_pick(const PlanCands &cands, bool spaced, const unsigned long long *tr, double &miss)
{
    auto missfrac = [&](u32 ci) { return tr[3 * ci] ? (double)(tr[3 * ci + 1] + tr[3 * ci + 2]) / (double)tr[3 * ci] : 0.0; };
    // per identity: the widest window with fewer than 1 key in 100 outside its home bucket, else the narrowest
    u32 best[2] = {cands.n, cands.n};
    for (u32 wide = 0; wide < 2; ++wide) {
        u32 last = cands.n;
        for (u32 ci = 0; ci < cands.n; ++ci) {
            if (cands.c[ci].wide != wide) continue;
            last = ci;
            if (missfrac(ci) < 0.01) break;
        }
        best[wide] = last;
    }
    // the wide identity costs ~7 % of kernel time (a 64-bit ring, v_min_f64 per window entry): worth it when the narrow
    // table leaves more than 2 keys in 100 outside their home bucket and the wide one at most 60 % of that (calibrated:
    // a 9e8-key db of window minimizers 0.4 % -> narrow, 6.49 vs 6.94 ms; every-k-mer dbs of 9e8 / 1.8e9 keys 6.9 % /
    // 12 % -> wide, 8.05 vs 8.26 and 8.44 vs 9.26 ms)
    u32 pick = best[0] < cands.n ? best[0] : best[1];
    if (best[0] < cands.n && best[1] < cands.n && missfrac(best[0]) >= 0.02 && missfrac(best[1]) <= 0.6 * missfrac(best[0])) pick = best[1];
    if (spaced) pick = missfrac(0) < 0.05 ? 0 : cands.n - 1;       // (two candidates: the longer window when its groups fit)
    miss = missfrac(pick);
    return pick;
}

// ---- fill.  A table with room takes its keys in arrival order; a crowded one -- the trial left more than 1 key in 100
// outside its home bucket, or (no trial: one candidate) the table is more than an eighth full -- is filled group by group
// (minbucket_tagcount_kernel: count, decide, residents, the rest): two more passes over the arrays, and about half as many
// of a read's runs need a second probe pass.  BNS_DBG_PLAIN_FILL / BNS_DBG_GROUP_FILL force one or the other (tests, A/B).
inline bool plan_group_fill(u32 n_cands, double trial_miss, u64 n_present, u64 n_mb, int fill_req, int dbg)
{
    const bool crowded = n_cands > 1 ? trial_miss >= 0.01 : (double)n_present > 0.125 * (double)n_mb * MINB_CAP;
    return fill_req >= 0 ? fill_req == 1 : (!(dbg & BNS_DBG_PLAIN_FILL) && (crowded || (dbg & BNS_DBG_GROUP_FILL)));
}

// slots of the overflow table: at most half full (+2048: room for the buckets minbucket_place_kernel may move here -- about one
// in 1e8; under the test switch that fails every 61st bucket, room for all of those)
inline u64 plan_overflow_slots(u64 n_ovf_keys, u64 n_alloc, int dbg)
{
    const u64 place_room = 2048 + ((dbg & BNS_DBG_PLACE_FAIL) ? n_alloc / 61 * MINB_CAP + MINB_CAP : 0);
    u64 n_ovf_slots = 64;
    while (n_ovf_slots < 2 * (n_ovf_keys + place_room)) n_ovf_slots <<= 1;
    return n_ovf_slots;
}

}  // namespace bns
