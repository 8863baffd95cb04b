// bns_api.hip -- the C ABI of include/bonsai_amd.h: context, HBM residency, and the entry points; classify, table load, build and
// window sessions and the hash feeders (RollingHasher, ntHash) are thin forwards into bns_classify.hpp, bns_table_load.hpp, bns_build.hpp
// (+ bns_minimize.hpp), bns_windows.hpp and bns_hashers.hpp.
// Single translation unit for the device library: the kernels are included so their templates are visible.
#include "../../include/bonsai_amd.h"
#include "bns_kernels.hip"
#include "bns_tally.hpp"
#include "bns_inspect.hpp"
#include "bns_confidence.hpp"
#include "bns_sketch.hpp"
#include "bns_hit_groups.hpp"
#include "bns_text_plan.hpp"

#include <dlfcn.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif
#include <rccl/rccl.h>          // types and declarations only: the library itself is dlopen()ed (see Rccl below)
#include <mutex>
#include <numeric>
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>
#include <chrono>
#include <type_traits>
#include <thread>
#include <vector>

using namespace bns;

namespace {

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

// ctx->small: the few device words the entry points share with their kernels.  Every entry point zeroes ITS words on its own
// stream before use; nothing here persists across calls.
struct SmallLayout {
    u32 work_counter[CLAIM_SHARDS][CLAIM_COUNTER_STRIDE];   // [0,1024)     classify_kernel's claim counters, one per XCD, each on a line of its own (one word: 86 M atomics/s)
    u32 ovf_count, max_len; u32 pad1[30];      // [1024,1152) classify: units handed to the overflow kernel; longest read of the batch
    unsigned long long load_cnt[8];            // [1152,1216) table load / device build counters
    unsigned long long runs_cursor;            // [1216,1224) hit_runs_kernel's output cursor
    unsigned long long lines_cursor;           // [1224,1232) lines_len_kernel: line bytes of the call so far
};
constexpr size_t SMALL_BYTES = 1536;
constexpr size_t SMALL_CLASSIFY_ZERO = offsetof(SmallLayout, max_len) + sizeof(u32);   // what a classify call zeroes, in one memset
static_assert(sizeof(SmallLayout) <= SMALL_BYTES, "ctx->small is allocated with SMALL_BYTES");
static_assert(offsetof(SmallLayout, load_cnt) >= SMALL_CLASSIFY_ZERO, "classify's memset must not reach the other entry points' words");

// bns_debug_set bits (tests and profiling; 0 in production); the table load's -- 0x10, 0x20, 0x100, 0x200, 0x1000, bits 16-20 and
// 24-28 -- are in bns_table_plan.hpp, the classify launch's -- 0x2000, 0x8000 -- in bns_classify_plan.hpp, the text calls' -- 0x40,
// 0x4000 -- in bns_text_plan.hpp
constexpr int BNS_DBG_PEXT_OFF = 0x400;             // spaced seeds: gather run by run instead of through the compress network
constexpr int BNS_DBG_FORCE_RCCL = 0x800;           // bns_load_table_multi with ONE context still broadcasts through RCCL (1-rank communicator)
constexpr int BNS_DBG_INSPECT_TINY = 0x8;           // bns_table_tally: grids of at most 4 workgroups that flush their LDS counters every 3 rounds (tests: many rounds, a full LDS hash and the mid-walk flush on small tables; same counts)
constexpr int BNS_DBG_INSPECT_WHOLE = 0x80;         // bns_table_tally: fetch whole 128-byte buckets instead of their upper halves (A/B; same counts)

// What the last classify dispatch launched (bns_debug_last_classify_form, a test aid): the template arguments of the
// classify_kernel instantiation, of the classify_overflow_kernel one when units went there, and the launch geometry.  Written
// by launch_classify / launch_classify_overflow from their own template arguments, so it cannot say anything but what ran.
struct ClassifyForm {
    enum { VALID, SPACED, LAYOUT, KT, NM, SPAN, OVC, WIDE, PACKED, OVF_LAUNCHED, OVF_SPACED, OVF_LAYOUT, OVF_WIDE, OVF_PACKED, OVF_UNITS,
           OVF_GRID, CHUNK, GRID, N_WORDS };
    u32 w[N_WORDS] = {0};
};

}  // namespace

struct bns_text_work;                                     // bns_ingest.hip: workspace of bns_classify_text
namespace bns { struct BuildSession; }                    // bns_build.hpp: the table a build session grows
namespace bns { struct WindowSession; }                   // bns_windows.hpp: window length, pair table and workspace of a window session
void text_work_free(struct bns_ctx *ctx);

struct bns_ctx {
    int device = 0;
    bns_text_work *text_work = nullptr;
    bns::BuildSession *build = nullptr;                  // bns_build_begin .. bns_build_end; while it is open the encoder, the window and the taxonomy stay
    bns::WindowSession *windows = nullptr;               // bns_windows_begin .. bns_windows_end
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;                   // host-buffer entry points: uploads of the next slice while one is classified
    hipStream_t back_stream = nullptr;                   // ... and the copy-back of a classified slice's results, behind neither of the two
    hipEvent_t slice_ev[16] = {}, done_ev[16] = {};
    std::string err;
    int n_cu = 256;
    // encoder
    bool enc_set = false;
    u32 k = 0, c = 0;
    bool canon = true, spaced = false, spaced_intended = false;
    u16 pos[32] = {0};
    u32 n_runs = 0;
    u8 run_start[32] = {0}, run_len[32] = {0};
    u64 sample_mask = 0;
    u32 table_m = 0;            // minimizer length the MINBUCKET table was built with
    u32 min_span_req = 0;       // bns_set_minimizer_span: 0 = chosen from the db when the table is loaded
    u64 n_spilled = 0;          // keys of the MINBUCKET table that are not in their home bucket
    bool group_fill = false;    // the table was filled group by group (crowded tables: minbucket_tagcount_kernel)
    u32 table_len = 0, table_shift = 0, table_canon = 1;   // MinSpec of the loaded table (where in the key the minimizer lives)
    u32 sp_run_len = 0, sp_run_shift = 0;                  // spaced seeds: the mask's longest run of adjacent sampled bases
    u32 pext_on = 0, pext_n1 = 0, pext_steps[2] = {0, 0}, pext_top[2] = {0xFF, 0xFF};  // compress network for masks with many runs (ClassifyParams)
    u64 pext_mask[2] = {0, 0}, pext_mv[2][6] = {{0}};
    u32 win = 0;                // Spacer window in bases (0 / <= comb: unwindowed)
    int score = 0;              // BNS_SCORE_*
    // table
    int layout = -1;
    u64 kh_nb = 0;
    const u32 *kflags = nullptr;
    const u64 *kkeys = nullptr;
    const u32 *kvals = nullptr;
    bool own_khash = false;
    Slot *slots = nullptr;          // BUCKET: n_slots x 16 B; MINBUCKET: the same allocation viewed as MinBucket[n_slots / 8]
    u64 n_slots = 0;                // allocated 16-byte slots (MINBUCKET: 8 per bucket, n_mb + MINB_MAX_CHAIN - 1 buckets)
    u32 n_mb = 0;                   // MINBUCKET: buckets a key can call home (any count: the index is a multiply-high)
    Slot *ovf_slots = nullptr;      // MINBUCKET: plain-hashed overflow table for keys beyond MINB_MAX_CHAIN buckets
    u64 n_ovf_slots = 0, n_ovf_keys = 0;
    u64 n_keys = 0;
    u32 slots_log2_req = 0;
    u64 n_buckets_req = 0;          // bns_set_table_buckets: exact number of home buckets (0 = automatic)
    int fill_req = -1;              // bns_set_table_fill: -1 the loader decides, 0 arrival order, 1 group-aware fill
    int wide_req = -1;              // bns_set_minimizer_identity: -1 chosen from the key count, 0 narrow (32-bit), 1 wide (52-bit)
    bool table_wide = false;        // the loaded MINBUCKET table's identity
    u32 table_span = 0;             // the window candidate (MIN_CANDS span: 15 / 11 / 8) the loaded table was built with; 0: none (spaced seed)
    std::string warn;               // what the last table load has to say about the table it built (bns_table_warning)
    int dbg = 0;
    unsigned claim_waves = 0;   // bns_debug_set_claim_waves
    ClassifyForm last_form;     // bns_debug_last_classify_form
    u32 table_k = 0;            // k the minimizer-clustered layout was built for
    // taxonomy
    TaxNode *nodes = nullptr;
    u32 n_nodes = 0;
    u32 tax_clock = 0;              // Euler positions of the forest: tin / tout run over [1, tax_clock]
    // bns_tally_enable: direct[n_nodes + 1] counts of classified units per bin; clade / scan: bns_tally_read's workspace
    bool tally_on = false;
    DevBuf tally_direct, tally_clade, tally_scan;
    // bns_set_confidence: theta = conf_num / conf_den (0: off); conf_hits: the hit stream of a launch whose caller wants none
    u64 conf_num = 0, conf_den = 1;
    DevBuf conf_hits;
    // bns_set_min_hit_groups: a classified unit needs this many distinct found keys (bns_hit_groups.hpp); 0: off, 1: no effect
    u32 min_hit_groups = 0;
    // bns_sketch_enable: one HyperLogLog sketch per bin a sample touches (bns_sketch.hpp); sketch_cap = max_taxa, 0: off.  While it is on
    // the hit stream of a launch whose caller wants none goes to conf_hits as well
    u32 sketch_cap = 0;
    DevBuf sk_regs, sk_slot_of, sk_slot_bin, sk_seen, sk_state;
    // bns_set_dust: window and level of the low-complexity mask (dust_w 0: off); dust_flags: one flag word per packed word (bns_dust.hpp)
    u32 dust_w = 0, dust_t = 0;
    DevBuf dust_flags;
    // workspace (grow-only)
    DevBuf words, nmask, ovf_list, scratch, small, records;      // small: ovf_count + misc counters
    DevBuf st_bases, st_offsets, st_out[4], st_hits, st_kmers, st_aux, st_runs[4], st_words, st_nmask, st_bad;   // st_words..: packed host batches   // st_runs: run_start, n_runs, run_tax, run_len
    u32 *h_run_tax = nullptr, *h_run_len = nullptr;      // host side of bns_classify_batch_runs (valid until the next call); page-locked:
    size_t h_run_cap = 0;                                // a copy into pageable memory is staged by the runtime at a fraction of the link rate
    void *peer_stage = nullptr; size_t peer_stage_cap = 0;   // bns_dev_copy_peer between two devices: page-locked staging of this (the receiving) context
    // timing
    bool timing = false;
    static constexpr int EV_RING = 64;
    hipEvent_t ev0[EV_RING] = {nullptr}, ev1[EV_RING] = {nullptr};
    int ev_head = 0, ev_count = 0;          // recorded-but-unsummarised pairs are the last ev_count before ev_head
};

namespace {

#define HIPCHK(ctx, expr)                                                                         \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(_e);                        \
            return _e == hipErrorOutOfMemory ? BNS_ERR_NOMEM : BNS_ERR_HIP;                        \
        }                                                                                         \
    } while (0)

#define BNS_RC(x) do { const int rc__ = (x); if (rc__ != BNS_OK) return rc__; } while (0)

int fail(bns_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

int ensure(bns_ctx *ctx, DevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return BNS_OK;
    // a buffer that GROWS grows by at least a quarter: a stream of batches whose sizes wander (the slices of a text: 207 k records, give
    // or take) would otherwise re-allocate at every new maximum, and a hipFree drains the whole device (6.7 ms each, 45 of them per 7.5 GB
    // of BGZF text in round 5's trace)
    const size_t grown = b.p ? b.cap + b.cap / 4 : 0;
    if (b.p) { HIPCHK(ctx, hipFree(b.p)); b.p = nullptr; b.cap = 0; }
    const size_t want = (std::max(bytes, grown) + 255) & ~size_t(255);
    HIPCHK(ctx, hipMalloc(&b.p, want));
    b.cap = want;
    return BNS_OK;
}

void release(DevBuf &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
}

inline unsigned grid_for(const bns_ctx *ctx, u64 items, unsigned per_block, unsigned blocks_per_cu = 8)
{
    const u64 need = (items + per_block - 1) / per_block;
    const u64 cap = (u64)ctx->n_cu * blocks_per_cu;
    return (unsigned)std::max<u64>(1, std::min(need, cap));
}

template <class F>
void dispatch_sp_layout(bool spaced, int layout, F &&f)
{
    if (spaced) {
        if (layout == 2) f(std::true_type{}, std::integral_constant<int, 2>{});
        else if (layout == 1) f(std::true_type{}, std::integral_constant<int, 1>{});
        else f(std::true_type{}, std::integral_constant<int, 0>{});
    } else {
        if (layout == 2) f(std::false_type{}, std::integral_constant<int, 2>{});
        else if (layout == 1) f(std::false_type{}, std::integral_constant<int, 1>{});
        else f(std::false_type{}, std::integral_constant<int, 0>{});
    }
}

void free_table(bns_ctx *ctx)
{
    if (ctx->own_khash) {
        if (ctx->kflags) (void)hipFree((void *)ctx->kflags);
        if (ctx->kkeys) (void)hipFree((void *)ctx->kkeys);
        if (ctx->kvals) (void)hipFree((void *)ctx->kvals);
    }
    ctx->kflags = nullptr; ctx->kkeys = nullptr; ctx->kvals = nullptr; ctx->own_khash = false; ctx->kh_nb = 0;
    if (ctx->slots) (void)hipFree(ctx->slots);
    if (ctx->ovf_slots) (void)hipFree(ctx->ovf_slots);
    ctx->ovf_slots = nullptr; ctx->n_ovf_slots = 0; ctx->n_ovf_keys = 0;
    ctx->slots = nullptr; ctx->n_slots = 0; ctx->n_mb = 0; ctx->n_keys = 0; ctx->layout = -1; ctx->table_wide = false;
}

int ready(bns_ctx *ctx, bool need_table, bool need_tax)
{
    if (!ctx) return BNS_ERR_ARG;
    if (!ctx->enc_set) return fail(ctx, BNS_ERR_STATE, "encoder not configured (bns_set_encoder)");
    if (need_table && ctx->layout < 0) return fail(ctx, BNS_ERR_STATE, "no table loaded (bns_load_table)");
    if (need_table && ctx->layout == BNS_LAYOUT_MINBUCKET && ctx->table_k != ctx->k)
        return fail(ctx, BNS_ERR_STATE, "encoder k changed after a BNS_LAYOUT_MINBUCKET table was built; reload the table");
    if (need_tax && !ctx->nodes) return fail(ctx, BNS_ERR_STATE, "no taxonomy loaded (bns_load_taxonomy)");
    return BNS_OK;
}

}  // namespace

#include "bns_classify.hpp"
#include "bns_dust.hpp"
#include "bns_build.hpp"
#include "bns_fewest.hpp"
#include "bns_minimize.hpp"
#include "bns_table_load.hpp"
#include "bns_windows.hpp"
#include "bns_hashers.hpp"

extern "C" {

int bns_version(void) { return 115; }

int bns_device_pci_bus_id(int device, char *out, int cap)
{
    if (!out || cap < 16) return BNS_ERR_ARG;
    return hipDeviceGetPCIBusId(out, cap, device) == hipSuccess ? BNS_OK : BNS_ERR_HIP;
}

int bns_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

/* test / profiling aid, not part of the public header: BNS_DBG_* bits (above).  The ablation bits (1: no probe, 2: no vote,
 * 4: no minimizer window; BNS_ABLATION builds only) make results WRONG; the others select code paths that a small test could
 * not reach otherwise (streamed load, sliced upload, one-rank RCCL broadcast). */
int bns_debug_set(bns_ctx *ctx, int bits) { if (!ctx) return BNS_ERR_ARG; ctx->dbg = bits; return BNS_OK; }
/* test aid like bns_debug_set, not part of the public header: classify_kernel's claims are sized for `waves` resident
 * wavefronts and its grid capped at waves / 4 workgroups (0: the device's own).  With 4 or 8, a batch of a few hundred short reads runs
 * staggered static claims and full dynamic ones, on wavefronts that go on claiming. */
int bns_debug_set_claim_waves(bns_ctx *ctx, unsigned waves) { if (!ctx || (waves & 3u)) return BNS_ERR_ARG; ctx->claim_waves = waves; return BNS_OK; }
/* test aid like bns_debug_set, not part of the public header: which kernels the last classify dispatch of this context launched.
 * Copies min(n, 18) words to out and returns how many; the words, in order: valid (0 until something was classified) | SPACED,
 * LAYOUT, KT, NM, SPAN, OVC, WIDE, PACKED of the classify_kernel instantiation | classify_overflow_kernel: launched (0 / 1), its
 * SPACED, LAYOUT, WIDE, PACKED, the units handed to it, its grid | the units per claim (chunk) and the grid of classify_kernel. */
int bns_debug_last_classify_form(const bns_ctx *ctx, uint32_t *out, int n)
{
    if (!ctx || !out || n < 0) return BNS_ERR_ARG;
    const int c = std::min<int>(n, ClassifyForm::N_WORDS);
    for (int i = 0; i < c; ++i) out[i] = ctx->last_form.w[i];
    return c;
}
#ifdef BNS_WAVE_TIMES
// measurement builds only: the WAVE_STAMPS (8) words (five wall-clock stamps, three claim-wait figures) of each of the 8192 wavefronts of the last classify_kernel launch
extern "C" int bns_debug_wave_times(bns_ctx *ctx, unsigned long long *out65536)
{
    if (!ctx || !out65536) return BNS_ERR_ARG;
    if (hipDeviceSynchronize() != hipSuccess) return BNS_ERR_HIP;
    if (hipMemcpyFromSymbol(out65536, HIP_SYMBOL(bns::g_wave_times), sizeof(bns::g_wave_times)) != hipSuccess) return BNS_ERR_HIP;
    return BNS_OK;
}
#endif
#ifdef BNS_COUNT_FETCHES
__global__ void ovf_stats_kernel(const bns::Slot *ovf, unsigned long long n_slots, unsigned long long *out)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    unsigned long long occ = 0, full = 0;
    for (unsigned long long b = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; b < n_slots / 4; b += stride) {
        unsigned c = 0;
        for (int q = 0; q < 4; ++q) c += ovf[b * 4 + q].occ ? 1u : 0u;
        occ += c; full += c == 4u;
    }
    atomicAdd(out, occ); atomicAdd(out + 1, full);
}
extern "C" int bns_debug_ovf_stats(bns_ctx *ctx, unsigned long long *out3)
{
    if (!ctx || !out3) return BNS_ERR_ARG;
    out3[0] = out3[1] = 0; out3[2] = ctx->n_ovf_slots;
    if (!ctx->ovf_slots) return BNS_OK;
    unsigned long long *d = ((SmallLayout *)ctx->small.p)->load_cnt;
    if (hipMemset(d, 0, 16) != hipSuccess) return BNS_ERR_HIP;
    hipLaunchKernelGGL(ovf_stats_kernel, dim3(1024), dim3(256), 0, 0, ctx->ovf_slots, (unsigned long long)ctx->n_ovf_slots, d);
    if (hipDeviceSynchronize() != hipSuccess) return BNS_ERR_HIP;
    if (hipMemcpy(out3, d, 16, hipMemcpyDeviceToHost) != hipSuccess) return BNS_ERR_HIP;
    return BNS_OK;
}
extern "C" int bns_debug_ovf_copy(bns_ctx *ctx, void *host, unsigned long long bytes)
{
    if (!ctx || !host || !ctx->ovf_slots) return BNS_ERR_ARG;
    const unsigned long long have = ctx->n_ovf_slots * sizeof(bns::Slot);
    if (hipMemcpy(host, ctx->ovf_slots, bytes < have ? bytes : have, hipMemcpyDeviceToHost) != hipSuccess) return BNS_ERR_HIP;
    return BNS_OK;
}
// measurement builds only: {distinct 128-byte buckets fetched, probe passes, lanes sent to the overflow table, rounds with such lanes} since the last call (then reset)
extern "C" int bns_debug_fetch_count(bns_ctx *ctx, unsigned long long *out8)
{
    if (!ctx || !out8) return BNS_ERR_ARG;
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipDeviceSynchronize() != hipSuccess) return BNS_ERR_HIP;
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(bns::g_fetch_count), sizeof(z)) != hipSuccess) return BNS_ERR_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(bns::g_fetch_count), z, sizeof(z)) != hipSuccess) return BNS_ERR_HIP;
    return BNS_OK;
}
#endif

const char *bns_strerror(int code)
{
    switch (code) {
        case BNS_OK: return "ok";
        case BNS_ERR_ARG: return "bad argument";
        case BNS_ERR_HIP: return "HIP runtime error";
        case BNS_ERR_NOMEM: return "out of memory";
        case BNS_ERR_STATE: return "context not ready";
        case BNS_ERR_TAX_CYCLE: return "taxonomy contains a cycle";
        case BNS_ERR_TAX_RANGE: return "taxid out of range for the flat parent array";
        case BNS_ERR_TABLE: return "inconsistent khash table";
        case BNS_ERR_NO_DEVICE: return "no usable GPU device";
        default: return "unknown error";
    }
}

const char *bns_last_error(const bns_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int bns_create(int device, bns_ctx **out)
{
    if (!out) return BNS_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return BNS_ERR_NO_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return BNS_ERR_NO_DEVICE;
    bns_ctx *ctx = new (std::nothrow) bns_ctx();
    if (!ctx) return BNS_ERR_NOMEM;
    ctx->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return BNS_ERR_HIP; }
    for (int i = 0; i < bns_ctx::EV_RING; ++i)
        if (hipEventCreate(&ctx->ev0[i]) != hipSuccess || hipEventCreate(&ctx->ev1[i]) != hipSuccess) { delete ctx; return BNS_ERR_HIP; }
    if (hipMalloc(&ctx->small.p, SMALL_BYTES) != hipSuccess) { delete ctx; return BNS_ERR_NOMEM; }
    ctx->small.cap = SMALL_BYTES;
    *out = ctx;
    return BNS_OK;
}

void bns_destroy(bns_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    free_table(ctx);
    build_free(ctx);
    windows_free(ctx);
    text_work_free(ctx);
    if (ctx->nodes) (void)hipFree(ctx->nodes);
    DevBuf *bufs[] = {&ctx->words, &ctx->nmask, &ctx->ovf_list, &ctx->scratch, &ctx->small, &ctx->records, &ctx->st_bases, &ctx->st_offsets,
                      &ctx->st_out[0], &ctx->st_out[1], &ctx->st_out[2], &ctx->st_out[3], &ctx->st_hits, &ctx->st_kmers, &ctx->st_aux,
                      &ctx->st_runs[0], &ctx->st_runs[1], &ctx->st_runs[2], &ctx->st_runs[3], &ctx->st_words, &ctx->st_nmask, &ctx->st_bad,
                      &ctx->tally_direct, &ctx->tally_clade, &ctx->tally_scan, &ctx->conf_hits,
                      &ctx->sk_regs, &ctx->sk_slot_of, &ctx->sk_slot_bin, &ctx->sk_seen, &ctx->sk_state, &ctx->dust_flags};
    for (DevBuf *b : bufs) release(*b);
    if (ctx->peer_stage) (void)hipHostFree(ctx->peer_stage);
    if (ctx->h_run_tax) (void)hipHostFree(ctx->h_run_tax);
    if (ctx->h_run_len) (void)hipHostFree(ctx->h_run_len);
    for (int i = 0; i < bns_ctx::EV_RING; ++i) {
        if (ctx->ev0[i]) (void)hipEventDestroy(ctx->ev0[i]);
        if (ctx->ev1[i]) (void)hipEventDestroy(ctx->ev1[i]);
    }
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    if (ctx->back_stream) (void)hipStreamDestroy(ctx->back_stream);
    for (hipEvent_t e : ctx->slice_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->done_ev) if (e) (void)hipEventDestroy(e);
    delete ctx;
}

int bns_set_encoder(bns_ctx *ctx, uint32_t k, const uint16_t *gaps, int canonicalize, int spaced_intended)
{
    if (!ctx) return BNS_ERR_ARG;
    if (ctx->build) return fail(ctx, BNS_ERR_STATE, "bns_set_encoder while a build session is open (bns_build_end)");
    if (k < 1 || k > 32) return fail(ctx, BNS_ERR_ARG, "k must be in [1,32] (u64 k-mers)");
    u32 c = 1;
    ctx->pos[0] = 0;
    bool spaced = false;
    for (u32 i = 0; i + 1 < k; ++i) {
        const u32 g = gaps ? gaps[i] : 0;
        if (g) spaced = true;
        c += g + 1;                                   // Spacer ctor: offsets = gaps + 1 (spacer.h:64)
        if (c > 1024) return fail(ctx, BNS_ERR_ARG, "comb size > 1024 is not supported");
        ctx->pos[i + 1] = (u16)(c - 1);
    }
    // runs of adjacent sampled bases (fast spaced gather when the comb fits a 64-base window)
    ctx->n_runs = 0; ctx->sample_mask = 0;
    if (spaced && c <= 64) {
        u32 i = 0;
        while (i < k) {
            u32 j = i;
            while (j + 1 < k && ctx->pos[j + 1] == ctx->pos[j] + 1) ++j;
            ctx->run_start[ctx->n_runs] = (u8)ctx->pos[i];
            ctx->run_len[ctx->n_runs] = (u8)(j - i + 1);
            ++ctx->n_runs;
            i = j + 1;
        }
        for (u32 q = 0; q < k; ++q) ctx->sample_mask |= 1ULL << (63 - ctx->pos[q]);
    }
    // masks with many runs: the compress network of each 32-base half of the 64-base window (Hacker's Delight, fig. 7-4 "compress":
    // mv[i] = the bits that move right by 2^i in step i)
    ctx->pext_on = 0;
    if (spaced && c <= 64 && ctx->n_runs > 4) {
        u64 m2[2] = {0, 0};
        u32 cnt[2] = {0, 0};
        for (u32 q = 0; q < k; ++q) { const u32 pb = ctx->pos[q]; m2[pb >> 5] |= 3ULL << (62 - 2 * (pb & 31)); ++cnt[pb >> 5]; }
        for (int h = 0; h < 2; ++h) {
            u64 m = m2[h], mk = ~m << 1;
            ctx->pext_mask[h] = m2[h]; ctx->pext_steps[h] = 0; ctx->pext_top[h] = 0xFF;
            if (m == (cnt[h] ? ~0ULL << (64 - 2 * cnt[h]) : 0ULL)) { ctx->pext_top[h] = cnt[h]; std::memset(ctx->pext_mv[h], 0, sizeof(ctx->pext_mv[h])); continue; }
            for (int i = 0; i < 6; ++i) {
                u64 mp = mk ^ (mk << 1);
                mp ^= mp << 2; mp ^= mp << 4; mp ^= mp << 8; mp ^= mp << 16; mp ^= mp << 32;
                const u64 mv = mp & m;
                ctx->pext_mv[h][i] = mv;
                if (mv) ctx->pext_steps[h] |= 1u << i;
                m = (m ^ mv) | (mv >> (1u << i));
                mk &= ~mp;
            }
        }
        ctx->pext_n1 = cnt[1];
        ctx->pext_on = 1;
    }
    // longest run of adjacent sampled bases, in KEY coordinates (key base q, 0 = first = most significant, sits at bits
    // [2(k-1-q), 2(k-q))): the stretch neighbouring spaced k-mers share position by position (bns_device.hpp, MinSpec)
    ctx->sp_run_len = 0; ctx->sp_run_shift = 0;
    if (spaced) {
        u32 i = 0;
        while (i < k) {
            u32 j = i;
            while (j + 1 < k && ctx->pos[j + 1] == ctx->pos[j] + 1) ++j;
            if (j - i + 1 > ctx->sp_run_len) { ctx->sp_run_len = j - i + 1; ctx->sp_run_shift = 2u * (k - 1u - j); }
            i = j + 1;
        }
    }
    ctx->k = k; ctx->c = c; ctx->spaced = spaced;
    ctx->canon = canonicalize && !spaced;             // encoder.h:148-150
    ctx->spaced_intended = spaced_intended != 0;
    ctx->enc_set = true;
    ctx->win = 0; ctx->score = 0;                     // a new Spacer starts unwindowed
    return BNS_OK;
}

int bns_set_window(bns_ctx *ctx, uint32_t w, int score)
{
    if (!ctx) return BNS_ERR_ARG;
    if (!ctx->enc_set) return fail(ctx, BNS_ERR_STATE, "configure the encoder first (bns_set_encoder)");
    if (ctx->build) return fail(ctx, BNS_ERR_STATE, "bns_set_window while a build session is open (bns_build_end)");
    if (score != BNS_SCORE_LEX && score != BNS_SCORE_ENTROPY_PATH && score != BNS_SCORE_ENTROPY_STRING) return fail(ctx, BNS_ERR_ARG, "unknown score");
    if (score == BNS_SCORE_ENTROPY_STRING && ctx->spaced)
        return fail(ctx, BNS_ERR_ARG, "BNS_SCORE_ENTROPY_STRING is the contiguous-seed string overload (encoder.h:425,434); a spaced seed scores through the path rule");
    if (w > ctx->c) {
        // up to 1024 k-mers per window: one 128-entry LDS image up to 64, beyond that a running minimum over 64-entry
        // segments (position windows) or a queue image in global memory (windows over the emitted stream)
        if (w > 1920u) return fail(ctx, BNS_ERR_ARG, "window of more than 1920 bases is not supported (a wavefront works on 2048-base chunks)");
        if (w - ctx->c + 1 > 1024u) return fail(ctx, BNS_ERR_ARG, "window of more than 1024 k-mers is not supported");
    }
    ctx->win = w; ctx->score = score;
    return BNS_OK;
}

int bns_set_bucket_slots_log2(bns_ctx *ctx, uint32_t log2_slots)
{
    if (!ctx || (log2_slots && (log2_slots < 2 || log2_slots > 40))) return BNS_ERR_ARG;
    ctx->slots_log2_req = log2_slots;
    if (log2_slots) ctx->n_buckets_req = 0;
    return BNS_OK;
}

int bns_set_table_buckets(bns_ctx *ctx, uint64_t n_home_buckets)
{
    if (!ctx || n_home_buckets >= (1ULL << 31) - 8) return BNS_ERR_ARG;
    ctx->n_buckets_req = n_home_buckets;
    if (n_home_buckets) ctx->slots_log2_req = 0;
    return BNS_OK;
}

int bns_set_table_fill(bns_ctx *ctx, int mode)
{
    if (!ctx || mode < 0 || mode > 2) return BNS_ERR_ARG;
    ctx->fill_req = mode - 1;                                    // 0 = the loader decides, 1 = arrival order, 2 = group-aware
    return BNS_OK;
}

int bns_set_minimizer_identity(bns_ctx *ctx, int bits)
{
    if (!ctx || (bits != 0 && bits != 32 && bits != 52)) return BNS_ERR_ARG;
    ctx->wide_req = bits == 0 ? -1 : (bits == 52 ? 1 : 0);
    return BNS_OK;
}

int bns_load_table_device(bns_ctx *ctx, uint64_t n_buckets, const uint32_t *d_flags, const uint64_t *d_keys,
                          const uint32_t *d_vals, int layout, void *stream)
{
    if (!ctx || !d_flags || !d_keys || !d_vals) return BNS_ERR_ARG;
    return load_table_resident(ctx, n_buckets, d_flags, d_keys, d_vals, layout, stream);
}

int bns_load_table(bns_ctx *ctx, uint64_t n_buckets, const uint32_t *flags, const uint64_t *keys, const uint32_t *vals, int layout)
{
    if (!ctx || !flags || !keys || !vals) return BNS_ERR_ARG;
    return load_table_host(ctx, n_buckets, flags, keys, vals, layout);
}

int bns_load_table_multi(bns_ctx **ctxs, int n_ctx, uint64_t n_buckets, const uint32_t *flags, const uint64_t *keys,
                         const uint32_t *vals, int layout)
{
    if (!ctxs || n_ctx < 1 || !flags || !keys || !vals) return BNS_ERR_ARG;
    for (int i = 0; i < n_ctx; ++i) if (!ctxs[i]) return BNS_ERR_ARG;
    bns_ctx *root = ctxs[0];
    // (BNS_DBG_FORCE_RCCL, tests: a single context still takes the replicate path -- a one-rank communicator and real ncclBroadcast
    // calls -- so that a one-GPU box executes the RCCL code)
    if (n_ctx == 1 && !(root->dbg & BNS_DBG_FORCE_RCCL)) return bns_load_table(root, n_buckets, flags, keys, vals, layout);
    BNS_RC(check_n_buckets(root, n_buckets));
    bns_ctx *failed = nullptr;
    const int rc = load_table_multi(ctxs, n_ctx, n_buckets, flags, keys, vals, layout, failed);
    if (rc != BNS_OK) {
        // the caller reads bns_last_error(ctxs[0]); and no context keeps half a replica (raw khash copies next to built tables)
        if (failed && failed != root) root->err = failed->err;
        const std::string msg = root->err;
        for (int i = 0; i < n_ctx; ++i) { (void)hipSetDevice(ctxs[i]->device); free_table(ctxs[i]); }
        root->err = msg;
    }
    return rc;
}

int bns_rccl_info(int *version, int *n_ranks)
{
    if (version) *version = g_rccl.version;
    if (n_ranks) *n_ranks = g_rccl.last_ranks;
    return BNS_OK;
}

int bns_table_info(const bns_ctx *ctx, uint64_t *n_keys, uint64_t *device_bytes, int *layout)
{
    if (!ctx) return BNS_ERR_ARG;
    if (n_keys) *n_keys = ctx->n_keys;
    if (layout) *layout = ctx->layout;
    if (device_bytes) {
        if (ctx->layout == BNS_LAYOUT_BUCKET || ctx->layout == BNS_LAYOUT_MINBUCKET) *device_bytes = (ctx->n_slots + ctx->n_ovf_slots) * sizeof(Slot);
        else if (ctx->layout == BNS_LAYOUT_KHASH) *device_bytes = ctx->kh_nb * 12 + (ctx->kh_nb < 16 ? 4 : ctx->kh_nb / 4);
        else *device_bytes = 0;
    }
    return BNS_OK;
}

int bns_table_stats(const bns_ctx *ctx, uint64_t *stats4)
{
    if (!ctx || !stats4) return BNS_ERR_ARG;
    stats4[0] = ctx->n_keys; stats4[1] = ctx->n_ovf_keys;
    stats4[2] = ctx->layout == BNS_LAYOUT_KHASH ? ctx->kh_nb * 12 + (ctx->kh_nb < 16 ? 4 : ctx->kh_nb / 4) : ctx->n_slots * sizeof(Slot);
    stats4[3] = ctx->n_ovf_slots * sizeof(Slot);
    return BNS_OK;
}

int bns_set_minimizer_span(bns_ctx *ctx, uint32_t span)
{
    if (!ctx) return BNS_ERR_ARG;
    bool ok = span == 0;
    for (const MinCand &c : MIN_CANDS) ok = ok || span == c.span;
    if (!ok) return fail(ctx, BNS_ERR_ARG, "minimizer span must be 0 (chosen from the db), 8, 11 or 15");
    ctx->min_span_req = span;
    return BNS_OK;
}

int bns_table_minimizer(const bns_ctx *ctx, uint32_t *m, uint64_t *spilled_keys)
{
    if (!ctx) return BNS_ERR_ARG;
    if (m) *m = ctx->layout == BNS_LAYOUT_MINBUCKET ? ctx->table_m : 0u;
    if (spilled_keys) *spilled_keys = ctx->layout == BNS_LAYOUT_MINBUCKET ? ctx->n_spilled : 0ULL;
    return BNS_OK;
}

int bns_table_geometry(const bns_ctx *ctx, uint64_t *geo8)
{
    if (!ctx || !geo8) return BNS_ERR_ARG;
    const bool mb = ctx->layout == BNS_LAYOUT_MINBUCKET;
    geo8[0] = mb ? ctx->n_mb : (ctx->layout == BNS_LAYOUT_BUCKET ? ctx->n_slots / 4 : ctx->kh_nb);
    geo8[1] = mb ? ctx->table_m : 0;
    geo8[2] = mb ? (ctx->table_wide ? 52 : 32) : 0;
    geo8[3] = mb ? ctx->n_spilled : 0;
    geo8[4] = mb ? ctx->table_span : 0;
    geo8[5] = mb ? ctx->n_ovf_keys : 0;
    geo8[6] = (mb && ctx->group_fill) ? 1 : 0;
    geo8[7] = 0;
    return BNS_OK;
}

const char *bns_table_warning(const bns_ctx *ctx) { return ctx ? ctx->warn.c_str() : ""; }

}  // extern "C"
namespace {
// direct[n_nodes + 1] allocated (kept when it is large enough) and zeroed
int tally_zero(bns_ctx *ctx)
{
    const size_t bytes = ((size_t)ctx->n_nodes + 1) * 8;
    const int rc = ensure(ctx, ctx->tally_direct, bytes);
    if (rc != BNS_OK) return rc;
    HIPCHK(ctx, hipMemsetAsync(ctx->tally_direct.p, 0, bytes, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return BNS_OK;
}

// the units of one classify launch into the tally, on the launch's stream behind it (neg: out again -- a batch the caller did not take)
int tally_units(bns_ctx *ctx, const u32 *d_taxon, u64 n_units, hipStream_t st, bool neg = false)
{
    if (!ctx->tally_on || n_units == 0) return BNS_OK;
    const unsigned grid = grid_for(ctx, n_units, TALLY_BLOCK * 16, 2);
    hipLaunchKernelGGL(tally_kernel, dim3(grid), dim3(TALLY_BLOCK), 0, st, d_taxon, (u64)n_units, (const TaxNode *)ctx->nodes, ctx->n_nodes,
                       (unsigned long long *)ctx->tally_direct.p, neg ? 1 : 0);
    HIPCHK(ctx, hipGetLastError());
    return BNS_OK;
}
// registers, seen and slots of the context's sketches allocated for the loaded taxonomy (kept when large enough) and zeroed
int sketch_zero(bns_ctx *ctx)
{
    const size_t n_bins = (size_t)ctx->n_nodes + 1;
    int rc;
    if ((rc = ensure(ctx, ctx->sk_regs, (size_t)ctx->sketch_cap * SKETCH_M)) != BNS_OK) return rc;
    if ((rc = ensure(ctx, ctx->sk_slot_bin, (size_t)ctx->sketch_cap * 4)) != BNS_OK) return rc;
    if ((rc = ensure(ctx, ctx->sk_slot_of, n_bins * 4)) != BNS_OK) return rc;
    if ((rc = ensure(ctx, ctx->sk_seen, n_bins)) != BNS_OK) return rc;
    if ((rc = ensure(ctx, ctx->sk_state, SKETCH_ST_WORDS * 4)) != BNS_OK) return rc;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemsetAsync(ctx->sk_regs.p, 0, (size_t)ctx->sketch_cap * SKETCH_M, st));
    HIPCHK(ctx, hipMemsetAsync(ctx->sk_slot_of.p, 0xFF, n_bins * 4, st));           // SKETCH_NO_SLOT
    HIPCHK(ctx, hipMemsetAsync(ctx->sk_seen.p, 0, n_bins, st));
    HIPCHK(ctx, hipMemsetAsync(ctx->sk_state.p, 0, SKETCH_ST_WORDS * 4, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return BNS_OK;
}

// f(spaced, layout, MIN) for the passes that look a launch's k-mers up again (sketch_kernel, hit_groups_kernel): MIN is the minimizer
// identity of the clustered layout, 0 for the others
template <class F>
void dispatch_reprobe(const bns_ctx *ctx, F &&f)
{
    const bool whole_key = ctx->table_canon && ctx->table_shift == 0 && ctx->table_len == ctx->table_k;    // (bns_probe_device's dispatch)
    dispatch_sp_layout(ctx->spaced, ctx->layout, [&](auto sp, auto ly) {
        if constexpr (decltype(ly)::value == 2) {
            if (!whole_key)           f(sp, ly, std::integral_constant<int, 1>{});
            else if (ctx->table_wide) f(sp, ly, std::integral_constant<int, 2>{});
            else                      f(sp, ly, std::integral_constant<int, 0>{});
        } else f(sp, ly, std::integral_constant<int, 0>{});
    });
}

// the k-mers of one classify launch into the sketches, on the launch's stream behind it.  p: the launch's parameters (offsets, units,
// mates, hit stream, records, and the packed image: classify_finish has packed ASCII input).
int sketch_units(bns_ctx *ctx, const ClassifyParams &p, hipStream_t st)
{
    const u32 n_bins = ctx->n_nodes + 1u;
    hipLaunchKernelGGL(sketch_seen_kernel, dim3(grid_for(ctx, p.n_units, 4)), dim3(256), 0, st, (const u32 *)p.hits, p.offsets, (u32)p.nmates,
                       (const uint4 *)p.records, (u64)p.n_units, (const TaxNode *)ctx->nodes, ctx->n_nodes, (u8 *)ctx->sk_seen.p);
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(sketch_assign_kernel, dim3(1), dim3(SKETCH_SCAN_BLOCK), 0, st, (const u8 *)ctx->sk_seen.p, (u32 *)ctx->sk_slot_of.p,
                       (u32 *)ctx->sk_slot_bin.p, n_bins, ctx->sketch_cap, (u32 *)ctx->sk_state.p);
    HIPCHK(ctx, hipGetLastError());
    const unsigned grid = grid_for(ctx, p.n_units, 4);
    const u32 *slot_of = (const u32 *)ctx->sk_slot_of.p;
    u8 *regs = (u8 *)ctx->sk_regs.p;
    dispatch_reprobe(ctx, [&](auto sp, auto ly, auto mn) {
        hipLaunchKernelGGL((sketch_kernel<decltype(sp)::value, decltype(ly)::value, decltype(mn)::value>), dim3(grid), dim3(256), 0, st, p, slot_of, regs);
    });
    HIPCHK(ctx, hipGetLastError());
    return BNS_OK;
}

// bns_set_min_hit_groups: the taxa of the launch's records zeroed where a unit has fewer distinct found keys, on the launch's stream
// behind the confidence walk.  p: the launch's parameters, with the packed image.
int hit_groups_units(bns_ctx *ctx, const ClassifyParams &p, hipStream_t st)
{
    const unsigned grid = grid_for(ctx, (p.n_units + HG_GROUP - 1) / HG_GROUP, 4);
    const u32 n_min = ctx->min_hit_groups;
    dispatch_reprobe(ctx, [&](auto sp, auto ly, auto mn) {
        hipLaunchKernelGGL((hit_groups_kernel<decltype(sp)::value, decltype(ly)::value, decltype(mn)::value>), dim3(grid), dim3(256), 0, st, p, n_min);
    });
    HIPCHK(ctx, hipGetLastError());
    return BNS_OK;
}
}  // namespace
extern "C" {

int bns_tally_enable(bns_ctx *ctx, int on)
{
    if (!ctx) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!on) {
        if (ctx->tally_on) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        release(ctx->tally_direct); release(ctx->tally_clade); release(ctx->tally_scan);
        ctx->tally_on = false;
        return BNS_OK;
    }
    if (!ctx->nodes) return fail(ctx, BNS_ERR_STATE, "no taxonomy loaded (bns_load_taxonomy)");
    const int rc = tally_zero(ctx);
    if (rc != BNS_OK) return rc;
    ctx->tally_on = true;
    return BNS_OK;
}

int bns_tally_read(bns_ctx *ctx, uint64_t *direct, uint64_t *clade, uint32_t len, int reset)
{
    if (!ctx) return BNS_ERR_ARG;
    if (!ctx->tally_on) return fail(ctx, BNS_ERR_STATE, "tally not enabled (bns_tally_enable)");
    if (len != ctx->n_nodes + 1u) return fail(ctx, BNS_ERR_ARG, "len must be n + 1 (n as given to bns_load_taxonomy)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u32 n = ctx->n_nodes;
    const size_t bytes = ((size_t)n + 1) * 8;
    if (clade) {
        const u32 n_pos = ctx->tax_clock + 1u;                               // positions 0 (nothing in front of the first tin) .. tax_clock
        int rc;
        if ((rc = ensure(ctx, ctx->tally_clade, bytes)) != BNS_OK) return rc;
        if ((rc = ensure(ctx, ctx->tally_scan, (size_t)n_pos * 8)) != BNS_OK) return rc;
        unsigned long long *S = (unsigned long long *)ctx->tally_scan.p;
        const unsigned long long *d = (const unsigned long long *)ctx->tally_direct.p;
        HIPCHK(ctx, hipMemsetAsync(S, 0, (size_t)n_pos * 8, st));
        hipLaunchKernelGGL(clade_scatter_kernel, dim3(grid_for(ctx, n, 256)), dim3(256), 0, st, (const TaxNode *)ctx->nodes, n, d, S, n_pos);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(clade_scan_kernel, dim3(1), dim3(CLADE_SCAN_BLOCK), 0, st, S, (u64)n_pos);
        HIPCHK(ctx, hipGetLastError());
        hipLaunchKernelGGL(clade_kernel, dim3(grid_for(ctx, (u64)n + 1, 256)), dim3(256), 0, st, (const TaxNode *)ctx->nodes, n, d,
                           (const unsigned long long *)S, n_pos, (unsigned long long *)ctx->tally_clade.p);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(clade, ctx->tally_clade.p, bytes, hipMemcpyDeviceToHost, st));
    }
    if (direct) HIPCHK(ctx, hipMemcpyAsync(direct, ctx->tally_direct.p, bytes, hipMemcpyDeviceToHost, st));
    if (reset) HIPCHK(ctx, hipMemsetAsync(ctx->tally_direct.p, 0, bytes, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return BNS_OK;
}

int bns_table_tally(bns_ctx *ctx, uint64_t *direct, uint64_t *clade, uint32_t len)
{
    if (!ctx) return BNS_ERR_ARG;
    if (ctx->layout < 0) return fail(ctx, BNS_ERR_STATE, "no table loaded (bns_load_table)");
    if (!ctx->nodes) return fail(ctx, BNS_ERR_STATE, "no taxonomy loaded (bns_load_taxonomy)");
    if (len != ctx->n_nodes + 1u) return fail(ctx, BNS_ERR_ARG, "len must be n + 1 (n as given to bns_load_taxonomy)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u32 n = ctx->n_nodes;
    const TaxNode *nodes = (const TaxNode *)ctx->nodes;
    const size_t bins = (size_t)n + 1;
    const u32 n_pos = ctx->tax_clock + 1u;
    // scratch of this call only: direct | clade | S
    unsigned long long *d = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&d, (2 * bins + (clade ? (size_t)n_pos : 0)) * 8));
    unsigned long long *c = d + bins, *S = c + bins;
    int rc = [&]() -> int {
        HIPCHK(ctx, hipMemsetAsync(d, 0, bins * 8, st));
        const bool whole = (ctx->dbg & BNS_DBG_INSPECT_WHOLE) != 0, tiny = (ctx->dbg & BNS_DBG_INSPECT_TINY) != 0;
        const u32 flush = tiny ? 3u : INSPECT_FLUSH_ROUNDS;
        auto grid_of = [&](u64 items, unsigned per_block) { const unsigned g = grid_for(ctx, items, per_block); return tiny ? std::min(g, 4u) : g; };
        if (ctx->layout == BNS_LAYOUT_KHASH)
            hipLaunchKernelGGL(inspect_khash_kernel, dim3(grid_of(ctx->kh_nb, TALLY_BLOCK)), dim3(TALLY_BLOCK), 0, st, ctx->kflags, ctx->kvals,
                               (u64)ctx->kh_nb, nodes, n, d, flush);
        else if (ctx->layout == BNS_LAYOUT_BUCKET)
            hipLaunchKernelGGL(inspect_slots_kernel, dim3(grid_of(ctx->n_slots, TALLY_BLOCK)), dim3(TALLY_BLOCK), 0, st, (const Slot *)ctx->slots,
                               (u64)ctx->n_slots, nodes, n, d, flush);
        else {
            const u64 n_bucket = ctx->n_slots / 8;                               // home buckets and the spill-only ones behind them
            const unsigned grid = grid_of(n_bucket, TALLY_BLOCK / 4 * INSPECT_MINB_UNROLL);
            if (whole) hipLaunchKernelGGL(inspect_minb_kernel<true>, dim3(grid), dim3(TALLY_BLOCK), 0, st, (const MinBucket *)ctx->slots, n_bucket, nodes, n, d, flush);
            else       hipLaunchKernelGGL(inspect_minb_kernel<false>, dim3(grid), dim3(TALLY_BLOCK), 0, st, (const MinBucket *)ctx->slots, n_bucket, nodes, n, d, flush);
            HIPCHK(ctx, hipGetLastError());
            if (ctx->n_ovf_slots)
                hipLaunchKernelGGL(inspect_slots_kernel, dim3(grid_of(ctx->n_ovf_slots, TALLY_BLOCK)), dim3(TALLY_BLOCK), 0, st,
                                   (const Slot *)ctx->ovf_slots, (u64)ctx->n_ovf_slots, nodes, n, d, flush);
        }
        HIPCHK(ctx, hipGetLastError());
        if (clade) {
            HIPCHK(ctx, hipMemsetAsync(S, 0, (size_t)n_pos * 8, st));
            hipLaunchKernelGGL(clade_scatter_kernel, dim3(grid_for(ctx, n, 256)), dim3(256), 0, st, nodes, n, (const unsigned long long *)d, S, n_pos);
            HIPCHK(ctx, hipGetLastError());
            hipLaunchKernelGGL(clade_scan_kernel, dim3(1), dim3(CLADE_SCAN_BLOCK), 0, st, S, (u64)n_pos);
            HIPCHK(ctx, hipGetLastError());
            hipLaunchKernelGGL(clade_kernel, dim3(grid_for(ctx, (u64)n + 1, 256)), dim3(256), 0, st, nodes, n, (const unsigned long long *)d,
                               (const unsigned long long *)S, n_pos, c);
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, hipMemcpyAsync(clade, c, bins * 8, hipMemcpyDeviceToHost, st));
        }
        if (direct) HIPCHK(ctx, hipMemcpyAsync(direct, d, bins * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        return BNS_OK;
    }();
    if (rc != BNS_OK) (void)hipStreamSynchronize(st);                            // nothing of the call may still use the scratch
    (void)hipFree(d);
    return rc;
}

int bns_set_confidence(bns_ctx *ctx, uint64_t num, uint64_t den)
{
    if (!ctx) return BNS_ERR_ARG;
    if (den == 0 || num > den) return fail(ctx, BNS_ERR_ARG, "confidence num / den: den > 0 and num <= den");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (num == 0) {
        if (ctx->conf_num) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        if (!ctx->sketch_cap) release(ctx->conf_hits);  // (shared with the sketch pass)
        ctx->conf_num = 0; ctx->conf_den = 1;
        return BNS_OK;
    }
    if (!ctx->nodes) return fail(ctx, BNS_ERR_STATE, "no taxonomy loaded (bns_load_taxonomy)");
    const u64 g = std::gcd(num, den);                // (the same theta; small terms keep the device's exact ceil on its short path)
    ctx->conf_num = num / g; ctx->conf_den = den / g;
    return BNS_OK;
}

int bns_set_min_hit_groups(bns_ctx *ctx, uint32_t n)
{
    if (!ctx) return BNS_ERR_ARG;
    if (ctx->build) return fail(ctx, BNS_ERR_STATE, "bns_set_min_hit_groups while a build session is open (bns_build_end)");
    if (ctx->windows) return fail(ctx, BNS_ERR_STATE, "bns_set_min_hit_groups while a window session is open (bns_windows_end)");
    if (n > HG_MAX) return fail(ctx, BNS_ERR_ARG, "bns_set_min_hit_groups: n must be in [0, 64]");
    ctx->min_hit_groups = n;
    return BNS_OK;
}

int bns_sketch_enable(bns_ctx *ctx, uint32_t max_taxa)
{
    if (!ctx) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (max_taxa == 0) {
        if (ctx->sketch_cap) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        release(ctx->sk_regs); release(ctx->sk_slot_of); release(ctx->sk_slot_bin); release(ctx->sk_seen); release(ctx->sk_state);
        if (!ctx->conf_num) release(ctx->conf_hits);
        ctx->sketch_cap = 0;
        return BNS_OK;
    }
    if (!ctx->nodes) return fail(ctx, BNS_ERR_STATE, "no taxonomy loaded (bns_load_taxonomy)");
    if (max_taxa > (1u << 20)) return fail(ctx, BNS_ERR_ARG, "max_taxa > 2^20 (4 GiB of sketches)");
    if (ctx->sketch_cap) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->sketch_cap = max_taxa;
    const int rc = sketch_zero(ctx);
    if (rc != BNS_OK) {                                  // (no room: off, with nothing held)
        const std::string why = ctx->err;
        (void)bns_sketch_enable(ctx, 0);
        ctx->err = why;
    }
    return rc;
}

int bns_sketch_read(bns_ctx *ctx, uint32_t *bins, uint8_t *registers, uint32_t cap, uint32_t *n_sketched, uint32_t *n_dropped_bins, int reset)
{
    if (!ctx) return BNS_ERR_ARG;
    if (!ctx->sketch_cap) return fail(ctx, BNS_ERR_STATE, "sketches not enabled (bns_sketch_enable)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    u32 state[SKETCH_ST_WORDS] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(state, ctx->sk_state.p, sizeof(state), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const u32 s = state[SKETCH_ST_USED];
    if (n_sketched) *n_sketched = s;
    if (n_dropped_bins) *n_dropped_bins = state[SKETCH_ST_DROPPED];
    if ((bins || registers) && cap < s) return fail(ctx, BNS_ERR_ARG, "cap is smaller than the number of sketched bins");
    if ((bins || registers) && s) {
        // slots were given launch by launch, ascending inside a launch only: the caller gets them in ascending bin order
        std::vector<u32> slot_bin(s), order(s);
        HIPCHK(ctx, hipMemcpyAsync(slot_bin.data(), ctx->sk_slot_bin.p, (size_t)s * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        std::iota(order.begin(), order.end(), 0u);
        std::sort(order.begin(), order.end(), [&](u32 a, u32 b) { return slot_bin[a] < slot_bin[b]; });
        if (bins) for (u32 i = 0; i < s; ++i) bins[i] = slot_bin[order[i]];
        if (registers) {
            // runs of slots that are already in order come back in one copy each (one launch: one run)
            for (u32 i = 0; i < s;) {
                u32 j = i + 1;
                while (j < s && order[j] == order[j - 1] + 1u) ++j;
                HIPCHK(ctx, hipMemcpyAsync(registers + (size_t)i * SKETCH_M, (const u8 *)ctx->sk_regs.p + (size_t)order[i] * SKETCH_M,
                                           (size_t)(j - i) * SKETCH_M, hipMemcpyDeviceToHost, st));
                i = j;
            }
            HIPCHK(ctx, hipStreamSynchronize(st));
        }
    }
    if (reset) {
        const int rc = sketch_zero(ctx);
        if (rc != BNS_OK) return rc;
    }
    return BNS_OK;
}

// Host-side flattening of the parent map into {parent, Euler interval, flags} records.
int bns_load_taxonomy(bns_ctx *ctx, const uint32_t *parent, uint32_t n)
{
    if (!ctx || !parent || n < 2) return BNS_ERR_ARG;
    if (ctx->build) return fail(ctx, BNS_ERR_STATE, "bns_load_taxonomy while a build session is open (bns_build_end)");
    if (n > (1u << 28)) return fail(ctx, BNS_ERR_TAX_RANGE, "taxid >= 2^28");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    std::vector<TaxNode> nodes(n);
    std::vector<u8> inforest(n, 0);
    std::vector<u32> child_cnt(n + 1, 0);
    for (u32 x = 0; x < n; ++x) {
        const u32 p = parent[x];
        nodes[x] = TaxNode{p, 0u, 0u, p != TAX_ABSENT ? NODE_PRESENT : 0u};
        if (p == TAX_ABSENT || x == 0) continue;
        if (p >= n) return fail(ctx, BNS_ERR_ARG, "parent id outside [0,n)");
        inforest[x] = 1;
        if (p != 0) { inforest[p] = 1; ++child_cnt[p]; }
    }
    // CSR of children
    std::vector<u32> child_off(n + 1, 0);
    for (u32 x = 0; x < n; ++x) child_off[x + 1] = child_off[x] + child_cnt[x];
    std::vector<u32> children(child_off[n]);
    {
        std::vector<u32> fillp(child_off.begin(), child_off.end() - 1);
        for (u32 x = 1; x < n; ++x) {
            const u32 p = parent[x];
            if (p != TAX_ABSENT && p != 0) children[fillp[p]++] = x;
        }
    }
    // iterative DFS from every root (forest node that is not a key, or whose parent is 0)
    u32 clock = 0;
    u64 visited = 0, n_forest = 0;
    std::vector<std::pair<u32, u32>> stack;   // (node, next child index)
    for (u32 x = 1; x < n; ++x) n_forest += inforest[x];
    for (u32 root = 1; root < n; ++root) {
        if (!inforest[root]) continue;
        const u32 pr = parent[root];
        if (!(pr == TAX_ABSENT || pr == 0)) continue;
        nodes[root].tin = ++clock;
        if (pr == 0) nodes[root].flags |= NODE_CHAIN_OK;
        ++visited;
        stack.emplace_back(root, child_off[root]);
        while (!stack.empty()) {
            auto &top = stack.back();
            const u32 x = top.first;
            if (top.second < child_off[x + 1]) {
                const u32 ch = children[top.second++];
                nodes[ch].tin = ++clock;
                if (nodes[x].flags & NODE_CHAIN_OK) nodes[ch].flags |= NODE_CHAIN_OK;   // ch is a key by construction
                ++visited;
                stack.emplace_back(ch, child_off[ch]);
            } else {
                nodes[x].tout = ++clock;
                stack.pop_back();
            }
        }
    }
    if (visited != n_forest) return fail(ctx, BNS_ERR_TAX_CYCLE, "parent map has a cycle: the reference's walks would not terminate");
    TaxNode *d = nullptr;
    HIPCHK(ctx, hipMalloc((void **)&d, (size_t)n * sizeof(TaxNode)));
    HIPCHK(ctx, hipMemcpy(d, nodes.data(), (size_t)n * sizeof(TaxNode), hipMemcpyHostToDevice));
    if (ctx->nodes) (void)hipFree(ctx->nodes);
    ctx->nodes = d; ctx->n_nodes = n; ctx->tax_clock = clock;
    if (ctx->sketch_cap) {                                // a new taxonomy, new bins: sketches and tally start again
        const int rc = sketch_zero(ctx);
        if (rc != BNS_OK) return rc;
    }
    return ctx->tally_on ? tally_zero(ctx) : BNS_OK;
}

int bns_set_timing(bns_ctx *ctx, int enabled)
{
    if (!ctx) return BNS_ERR_ARG;
    ctx->timing = enabled != 0;
    ctx->ev_count = 0;
    return BNS_OK;
}

float bns_last_kernel_ms(const bns_ctx *ctx)
{
    if (!ctx || ctx->ev_count == 0) return -1.0f;
    const int i = (ctx->ev_head + bns_ctx::EV_RING - 1) % bns_ctx::EV_RING;
    float ms = -1.0f;
    if (hipEventSynchronize(ctx->ev1[i]) != hipSuccess) return -1.0f;
    if (hipEventElapsedTime(&ms, ctx->ev0[i], ctx->ev1[i]) != hipSuccess) return -1.0f;
    return ms;
}

int bns_timing_summary(bns_ctx *ctx, double *sum_ms, int *count)
{
    if (!ctx || !sum_ms || !count) return BNS_ERR_ARG;
    double sum = 0.0;
    int n = 0;
    for (int j = 0; j < ctx->ev_count; ++j) {
        const int i = (ctx->ev_head + bns_ctx::EV_RING - 1 - j) % bns_ctx::EV_RING;
        float ms = 0.0f;
        HIPCHK(ctx, hipEventSynchronize(ctx->ev1[i]));
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev0[i], ctx->ev1[i]));
        sum += ms; ++n;
    }
    *sum_ms = sum; *count = n;
    ctx->ev_count = 0;
    return BNS_OK;
}

// ---- classify: thin forwards into bns_classify.hpp -------------------------------------------------------------------------
int bns_classify_batch_device(bns_ctx *ctx, const char *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                              uint64_t total_bases, uint32_t max_read_len, int paired, uint32_t *d_taxon,
                              uint32_t *d_missing, uint32_t *d_ambig, uint32_t *d_n_hits, uint32_t *d_hits, void *stream)
{
    if (!d_bases && total_bases) return BNS_ERR_ARG;
    ClassifyIn in;
    in.bases = d_bases; in.offsets = d_offsets; in.n_reads = n_reads; in.total_bases = total_bases; in.max_read_len = max_read_len; in.paired = paired;
    return classify_device_impl(ctx, in, UnitOut{d_taxon, d_missing, d_ambig, d_n_hits, d_hits}, stream);
}

int bns_classify_batch_packed_device(bns_ctx *ctx, const uint64_t *d_words, const uint32_t *d_nmask, const uint64_t *d_offsets,
                                     uint64_t n_reads, uint64_t total_bases, uint32_t max_read_len, int paired, uint32_t *d_taxon,
                                     uint32_t *d_missing, uint32_t *d_ambig, uint32_t *d_n_hits, uint32_t *d_hits, void *stream)
{
    if (!d_words) return BNS_ERR_ARG;
    ClassifyIn in;
    in.words = d_words; in.nmask = d_nmask; in.offsets = d_offsets; in.n_reads = n_reads; in.total_bases = total_bases; in.max_read_len = max_read_len;
    in.paired = paired;
    return classify_device_impl(ctx, in, UnitOut{d_taxon, d_missing, d_ambig, d_n_hits, d_hits}, stream);
}

uint64_t bns_packed_words(uint64_t total_bases, uint64_t n_reads) { return (total_bases >> 5) + n_reads + 1; }

int bns_pack_reads(const char *bases, const uint64_t *offsets, uint64_t n_reads, uint64_t *words, uint64_t *bad_word,
                   uint32_t *bad_mask, uint64_t bad_cap, uint64_t *n_bad, int threads)
{
    if (!offsets || !words || !n_bad || (!bases && n_reads && offsets[n_reads])) return BNS_ERR_ARG;
    return pack_reads_impl([=](u64 r) { return bases + offsets[r]; }, offsets, n_reads, words, bad_word, bad_mask, bad_cap, n_bad, threads);
}

int bns_pack_reads_ptrs(const char *const *seqs, const uint32_t *lens, uint64_t n_reads, uint64_t *offsets, uint64_t *words,
                        uint64_t *bad_word, uint32_t *bad_mask, uint64_t bad_cap, uint64_t *n_bad, int threads)
{
    if (!offsets || !words || !n_bad || (n_reads && (!seqs || !lens))) return BNS_ERR_ARG;
    offsets[0] = 0;
    for (u64 r = 0; r < n_reads; ++r) offsets[r + 1] = offsets[r] + lens[r];
    return pack_reads_impl([=](u64 r) { return seqs[r]; }, offsets, n_reads, words, bad_word, bad_mask, bad_cap, n_bad, threads);
}

int bns_classify_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_reads, int paired,
                       uint32_t *taxon, uint32_t *missing, uint32_t *ambig, uint32_t *n_hits, uint32_t *hits)
{
    return classify_host_entry(ctx, HostIn::ascii(bases), offsets, n_reads, paired, UnitOut{taxon, missing, ambig, n_hits, hits});
}

int bns_classify_batch_packed(bns_ctx *ctx, const uint64_t *words, const uint64_t *bad_word, const uint32_t *bad_mask, uint64_t n_bad,
                              const uint64_t *offsets, uint64_t n_reads, int paired,
                              uint32_t *taxon, uint32_t *missing, uint32_t *ambig, uint32_t *n_hits, uint32_t *hits)
{
    return classify_host_entry(ctx, HostIn::of_words(words, bad_word, bad_mask, n_bad), offsets, n_reads, paired, UnitOut{taxon, missing, ambig, n_hits, hits});
}

int bns_classify_batch_runs(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_reads, int paired,
                            uint32_t *taxon, uint32_t *missing, uint32_t *ambig, uint32_t *n_hits, uint64_t *run_start,
                            uint32_t *n_runs, const uint32_t **run_tax, const uint32_t **run_len, uint64_t *n_runs_total)
{
    return classify_runs_entry(ctx, HostIn::ascii(bases), offsets, n_reads, paired, UnitOut{taxon, missing, ambig, n_hits, nullptr}, run_start, n_runs,
                               run_tax, run_len, n_runs_total);
}

int bns_classify_batch_packed_runs(bns_ctx *ctx, const uint64_t *words, const uint64_t *bad_word, const uint32_t *bad_mask, uint64_t n_bad,
                                   const uint64_t *offsets, uint64_t n_reads, int paired,
                                   uint32_t *taxon, uint32_t *missing, uint32_t *ambig, uint32_t *n_hits, uint64_t *run_start,
                                   uint32_t *n_runs, const uint32_t **run_tax, const uint32_t **run_len, uint64_t *n_runs_total)
{
    return classify_runs_entry(ctx, HostIn::of_words(words, bad_word, bad_mask, n_bad), offsets, n_reads, paired, UnitOut{taxon, missing, ambig, n_hits, nullptr},
                               run_start, n_runs, run_tax, run_len, n_runs_total);
}

int bns_encode_batch_device(bns_ctx *ctx, const char *d_bases, const uint64_t *d_offsets, uint64_t n_reads,
                            uint64_t total_bases, uint64_t *d_kmers, uint32_t *d_n_kmers, void *stream)
{
    int rc = ready(ctx, false, false);
    if (rc != BNS_OK) return rc;
    if (!d_offsets || !d_n_kmers || (!d_kmers && total_bases)) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    if (n_reads == 0) return BNS_OK;
    if ((rc = pack_reads(ctx, d_bases, d_offsets, n_reads, total_bases, st)) != BNS_OK) return rc;
    ClassifyParams p;
    fill_params(ctx, p);
    p.offsets = d_offsets; p.n_units = n_reads; p.nmates = 1;
    p.emit_none = (ctx->spaced && !ctx->spaced_intended) ? 1 : 0;
    const unsigned grid = grid_for(ctx, n_reads, 4);
    if ((rc = set_win_scratch(ctx, p, grid)) != BNS_OK) return rc;
    if (ctx->spaced) hipLaunchKernelGGL(encode_kernel<true>, dim3(grid), dim3(256), 0, st, p, d_kmers, d_n_kmers);
    else             hipLaunchKernelGGL(encode_kernel<false>, dim3(grid), dim3(256), 0, st, p, d_kmers, d_n_kmers);
    HIPCHK(ctx, hipGetLastError());
    return BNS_OK;
}

int bns_encode_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_reads, uint64_t *kmers, uint32_t *n_kmers)
{
    int rc = ready(ctx, false, false);
    if (rc != BNS_OK) return rc;
    if (!offsets || !n_kmers) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n_reads == 0) return BNS_OK;
    const u64 total = offsets[n_reads];
    BNS_RC(ensure(ctx, ctx->st_kmers, (size_t)total * 8 + 8));
    BNS_RC(ensure(ctx, ctx->st_out[0], (size_t)n_reads * 4));
    BNS_RC(stage_batch(ctx, bases, offsets, n_reads));
    BNS_RC(bns_encode_batch_device(ctx, (const char *)ctx->st_bases.p, (const u64 *)ctx->st_offsets.p, n_reads, total,
                                   (u64 *)ctx->st_kmers.p, (u32 *)ctx->st_out[0].p, ctx->stream));
    return fetch_values(ctx, kmers, ctx->st_kmers.p, (size_t)total * 8, n_kmers, ctx->st_out[0].p, n_reads);
}

// the hash feeders: bns_hashers.hpp
int bns_rolling_tables(uint64_t seed1, uint64_t seed2, uint64_t *fwd, uint64_t *rc) { return rolling_tables<u64>(seed1, seed2, fwd, rc); }
int bns_rolling_tables128(uint64_t seed1, uint64_t seed2, uint64_t *fwd_lohi, uint64_t *rc_lohi)
{
    return rolling_tables<W128>(seed1, seed2, fwd_lohi, rc_lohi);
}
int bns_nthash_tables(uint64_t seed_a, uint64_t seed_c, uint64_t seed_g, uint64_t seed_t, uint64_t *table256)
{
    return nthash_tables(seed_a, seed_c, seed_g, seed_t, table256);
}
int bns_rolling_hash_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, int canon,
                           const uint64_t *fwd_table, const uint64_t *rc_table, uint64_t *hashes, uint32_t *n_hashes)
{
    return rolling_batch<u64>(ctx, bases, offsets, n_seqs, k, canon, 0, fwd_table, rc_table, hashes, n_hashes);
}
int bns_rolling_hash_windowed_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, int canon,
                                    uint32_t w, const uint64_t *fwd_table, const uint64_t *rc_table, uint64_t *hashes, uint32_t *n_hashes)
{
    return rolling_batch<u64>(ctx, bases, offsets, n_seqs, k, canon, w, fwd_table, rc_table, hashes, n_hashes);
}
int bns_rolling_hash128_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, int canon,
                              const uint64_t *fwd_lohi, const uint64_t *rc_lohi, uint64_t *hashes_lohi, uint32_t *n_hashes)
{
    return rolling_batch<W128>(ctx, bases, offsets, n_seqs, k, canon, 0, fwd_lohi, rc_lohi, hashes_lohi, n_hashes);
}
int bns_rolling_hash128_windowed_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, int canon,
                                       uint32_t w, const uint64_t *fwd_lohi, const uint64_t *rc_lohi, uint64_t *hashes_lohi, uint32_t *n_hashes)
{
    return rolling_batch<W128>(ctx, bases, offsets, n_seqs, k, canon, w, fwd_lohi, rc_lohi, hashes_lohi, n_hashes);
}
int bns_for_each_hash_batch(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_seqs, uint32_t k, int canon,
                            const uint64_t *table256, uint64_t *hashes, uint32_t *n_hashes)
{
    return nthash_batch(ctx, bases, offsets, n_seqs, k, canon, table256, hashes, n_hashes);
}

int bns_probe_device(bns_ctx *ctx, const uint64_t *d_kmers, uint64_t n, uint32_t *d_vals, uint8_t *d_found, void *stream)
{
    if (!ctx) return BNS_ERR_ARG;
    if (ctx->layout < 0) return fail(ctx, BNS_ERR_STATE, "no table loaded (bns_load_table)");
    if (n == 0) return BNS_OK;
    if (!d_kmers || !d_vals) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    ClassifyParams p;
    fill_params(ctx, p);
    const unsigned grid = grid_for(ctx, n, 256);
    const int evi = ctx->ev_head;
    if (ctx->timing) HIPCHK(ctx, hipEventRecord(ctx->ev0[evi], st));
    if (ctx->layout == BNS_LAYOUT_MINBUCKET && ctx->table_k != ctx->k)
        return fail(ctx, BNS_ERR_STATE, "encoder k changed after a BNS_LAYOUT_MINBUCKET table was built; reload the table");
    const bool whole_key = ctx->table_canon && ctx->table_shift == 0 && ctx->table_len == ctx->table_k;
    if (ctx->layout == 2 && !whole_key) hipLaunchKernelGGL((probe_kernel<2, 1>), dim3(grid), dim3(256), 0, st, p, d_kmers, (u64)n, d_vals, d_found);
    else if (ctx->layout == 2 && ctx->table_wide) hipLaunchKernelGGL((probe_kernel<2, 2>), dim3(grid), dim3(256), 0, st, p, d_kmers, (u64)n, d_vals, d_found);
    else if (ctx->layout == 2) hipLaunchKernelGGL(probe_kernel<2>, dim3(grid), dim3(256), 0, st, p, d_kmers, (u64)n, d_vals, d_found);
    else if (ctx->layout == 1) hipLaunchKernelGGL(probe_kernel<1>, dim3(grid), dim3(256), 0, st, p, d_kmers, (u64)n, d_vals, d_found);
    else                       hipLaunchKernelGGL(probe_kernel<0>, dim3(grid), dim3(256), 0, st, p, d_kmers, (u64)n, d_vals, d_found);
    HIPCHK(ctx, hipGetLastError());
    if (ctx->timing) {
        HIPCHK(ctx, hipEventRecord(ctx->ev1[evi], st));
        ctx->ev_head = (evi + 1) % bns_ctx::EV_RING;
        ctx->ev_count = std::min(ctx->ev_count + 1, (int)bns_ctx::EV_RING);
    }
    return BNS_OK;
}

int bns_probe(bns_ctx *ctx, const uint64_t *kmers, uint64_t n, uint32_t *vals, uint8_t *found)
{
    if (!ctx) return BNS_ERR_ARG;
    if (n == 0) return BNS_OK;
    if (!kmers || !vals) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = ensure(ctx, ctx->st_kmers, (size_t)n * 8)) != BNS_OK) return rc;
    if ((rc = ensure(ctx, ctx->st_out[0], (size_t)n * 4)) != BNS_OK) return rc;
    if ((rc = ensure(ctx, ctx->st_aux, (size_t)n)) != BNS_OK) return rc;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(ctx->st_kmers.p, kmers, (size_t)n * 8, hipMemcpyHostToDevice, st));
    rc = bns_probe_device(ctx, (const u64 *)ctx->st_kmers.p, n, (u32 *)ctx->st_out[0].p, (u8 *)ctx->st_aux.p, st);
    if (rc != BNS_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(vals, ctx->st_out[0].p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    if (found) HIPCHK(ctx, hipMemcpyAsync(found, ctx->st_aux.p, (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return BNS_OK;
}

int bns_resolve_batch(bns_ctx *ctx, const uint32_t *keys, const uint16_t *counts, const uint64_t *starts,
                      uint64_t n_units, uint32_t *taxon)
{
    if (!ctx || !starts || !taxon) return BNS_ERR_ARG;
    if (!ctx->nodes) return fail(ctx, BNS_ERR_STATE, "no taxonomy loaded (bns_load_taxonomy)");
    if (n_units == 0) return BNS_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const u64 total = starts[n_units];
    std::vector<u32> c32((size_t)total);
    for (u64 i = 0; i < total; ++i) c32[(size_t)i] = counts[i];
    int rc;
    if ((rc = ensure(ctx, ctx->st_kmers, (size_t)total * 4 + 4)) != BNS_OK) return rc;       // keys
    if ((rc = ensure(ctx, ctx->st_hits, (size_t)total * 4 + 4)) != BNS_OK) return rc;        // counts
    if ((rc = ensure(ctx, ctx->st_offsets, (size_t)(n_units + 1) * 8)) != BNS_OK) return rc;
    if ((rc = ensure(ctx, ctx->scratch, (size_t)total * 8 + 8)) != BNS_OK) return rc;
    if ((rc = ensure(ctx, ctx->st_out[0], (size_t)n_units * 4)) != BNS_OK) return rc;
    hipStream_t st = ctx->stream;
    if (total) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->st_kmers.p, keys, (size_t)total * 4, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->st_hits.p, c32.data(), (size_t)total * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->st_offsets.p, starts, (size_t)(n_units + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)std::min<u64>(n_units, (u64)ctx->n_cu * 16)), dim3(64), 0, st,
                       (const u32 *)ctx->st_kmers.p, (const u32 *)ctx->st_hits.p, (const u64 *)ctx->st_offsets.p, (u64)n_units,
                       (u32 *)ctx->scratch.p, (u64)total, (const TaxNode *)ctx->nodes, ctx->n_nodes, (u32 *)ctx->st_out[0].p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(taxon, ctx->st_out[0].p, (size_t)n_units * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return BNS_OK;
}

int bns_build_table_device(bns_ctx *ctx, const char *d_bases, const uint64_t *d_offsets, uint64_t n_genomes,
                           uint64_t total_bases, const uint32_t *d_taxid, uint64_t n_buckets, uint32_t *d_flags,
                           uint64_t *d_keys, uint32_t *d_vals, uint64_t *header4, void *stream)
{
    int rc = ready(ctx, false, true);
    if (rc != BNS_OK) return rc;
    if (!d_offsets || !d_taxid || !d_flags || !d_keys || !d_vals) return BNS_ERR_ARG;
    if (n_buckets < 4 || (n_buckets & (n_buckets - 1))) return fail(ctx, BNS_ERR_TABLE, "n_buckets must be a power of two >= 4");
    // ~0 marks an empty slot while building: a contiguous non-canonical 32-mer can BE ~0 (a spaced one equal to ~0 is never
    // emitted, encoder.h:236-238; a canonical one is never ~0)
    if (ctx->k == 32 && !ctx->canon && !ctx->spaced && !(ctx->win > ctx->c)) return fail(ctx, BNS_ERR_ARG, "device build needs canonical or spaced k-mers when k == 32");
    if (ctx->spaced && !ctx->spaced_intended) return fail(ctx, BNS_ERR_ARG, "spaced build needs spaced_intended=1");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    if ((rc = pack_reads_dust(ctx, d_bases, d_offsets, n_genomes, total_bases, st)) != BNS_OK) return rc;
    const unsigned fgrid = grid_for(ctx, n_buckets, 256);
    hipLaunchKernelGGL(fill_u64_kernel, dim3(fgrid), dim3(256), 0, st, d_keys, (u64)n_buckets, BUILD_EMPTY);
    hipLaunchKernelGGL(fill_u32_kernel, dim3(fgrid), dim3(256), 0, st, d_vals, (u64)n_buckets, 0u);
    unsigned long long *d_cnt = ((SmallLayout *)ctx->small.p)->load_cnt;
    HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 16, st));           // [0] keys inserted, [1] "table too small" flag of pass 1
    ClassifyParams p;
    fill_params(ctx, p);
    p.offsets = d_offsets; p.n_units = n_genomes; p.nmates = 1;
    const unsigned grid = (unsigned)ctx->n_cu * 8;
    if ((rc = set_win_scratch(ctx, p, grid)) != BNS_OK) return rc;
    if (ctx->spaced) {
        hipLaunchKernelGGL((build_kernel<true, 1>), dim3(grid), dim3(256), 0, st, p, d_taxid, (u64)n_buckets, d_keys, d_vals, d_cnt);
    } else {
        hipLaunchKernelGGL((build_kernel<false, 1>), dim3(grid), dim3(256), 0, st, p, d_taxid, (u64)n_buckets, d_keys, d_vals, d_cnt);
    }
    HIPCHK(ctx, hipGetLastError());
    // the load-factor contract (khash64.h:198) must hold before pass 2, and a full table would never terminate
    unsigned long long h_cnt2[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(h_cnt2, d_cnt, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const unsigned long long h_cnt = h_cnt2[0];
    const u64 upper = (u64)(n_buckets * 0.77 + 0.5);
    if (h_cnt2[1]) return fail(ctx, BNS_ERR_TABLE, "n_buckets too small: the table filled up while inserting");
    if (h_cnt > upper) return fail(ctx, BNS_ERR_TABLE, "n_buckets too small: load factor would exceed 0.77");
    if (ctx->spaced) {
        hipLaunchKernelGGL((build_kernel<true, 2>), dim3(grid), dim3(256), 0, st, p, d_taxid, (u64)n_buckets, d_keys, d_vals, d_cnt);
    } else {
        hipLaunchKernelGGL((build_kernel<false, 2>), dim3(grid), dim3(256), 0, st, p, d_taxid, (u64)n_buckets, d_keys, d_vals, d_cnt);
    }
    hipLaunchKernelGGL(build_finish_kernel, dim3(grid_for(ctx, std::max<u64>(1, n_buckets >> 4), 256)), dim3(256), 0, st,
                       (u64)n_buckets, d_flags, d_keys, d_vals);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (header4) { header4[0] = n_buckets; header4[1] = h_cnt; header4[2] = h_cnt; header4[3] = upper; }
    return BNS_OK;
}

int bns_set_dust(bns_ctx *ctx, uint32_t window, uint32_t level) { return set_dust(ctx, window, level); }
int bns_dust_mask(bns_ctx *ctx, const char *bases, const uint64_t *offsets, uint64_t n_seqs, uint32_t *flags)
{
    return dust_mask_host(ctx, bases, offsets, n_seqs, flags);
}

int bns_build_begin(bns_ctx *ctx, uint64_t n_buckets_hint) { return build_begin(ctx, n_buckets_hint); }
int bns_build_seed(bns_ctx *ctx, uint64_t n_buckets, const uint32_t *flags, const uint64_t *keys, const uint32_t *vals)
{
    return build_seed(ctx, n_buckets, flags, keys, vals);
}
int bns_build_add(bns_ctx *ctx, const char *d_bases, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t total_bases,
                  const uint32_t *d_taxid, void *stream)
{
    return build_add(ctx, d_bases, d_offsets, n_seqs, total_bases, d_taxid, stream);
}
int bns_build_finish(bns_ctx *ctx, uint64_t *header4) { return build_finish(ctx, header4); }
int bns_build_export(bns_ctx *ctx, uint32_t *flags, uint64_t *keys, uint32_t *vals) { return build_export(ctx, flags, keys, vals); }
int bns_build_stats(const bns_ctx *ctx, uint64_t *out6)
{
    if (!ctx || !out6) return BNS_ERR_ARG;
    if (!ctx->build) return BNS_ERR_STATE;
    out6[0] = ctx->build->n_batches; out6[1] = ctx->build->n_grows; out6[2] = ctx->build->n_seeded; out6[3] = ctx->build->n_keys;
    out6[4] = (u64)(ctx->build->s_add * 1e6); out6[5] = (u64)(ctx->build->s_grow * 1e6);
    return BNS_OK;
}
int bns_build_minimize_begin(bns_ctx *ctx, uint32_t w, uint64_t n_buckets_hint) { return bns_build_minimize_begin_score(ctx, w, n_buckets_hint, BNS_MINIMIZE_DEPTH); }
int bns_build_minimize_begin_score(bns_ctx *ctx, uint32_t w, uint64_t n_buckets_hint, int score) { return minimize_begin(ctx, w, n_buckets_hint, score); }
int bns_build_count_begin(bns_ctx *ctx) { return count_begin(ctx); }
int bns_build_count_add(bns_ctx *ctx, const char *d_bases, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t total_bases,
                        const uint32_t *h_genome, void *stream)
{
    return count_add(ctx, d_bases, d_offsets, n_seqs, total_bases, h_genome, stream);
}
int bns_build_count_get(bns_ctx *ctx, const uint64_t *h_keys, uint64_t n, uint32_t *h_counts) { return count_get(ctx, h_keys, n, h_counts); }
int bns_build_count_stats(const bns_ctx *ctx, uint64_t *out6) { return count_stats(ctx, out6); }
int bns_build_minimize_add(bns_ctx *ctx, const char *d_bases, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t total_bases, void *stream)
{
    return minimize_add(ctx, d_bases, d_offsets, n_seqs, total_bases, stream);
}
int bns_build_minimize_stats(const bns_ctx *ctx, uint64_t *out6) { return minimize_stats(ctx, out6); }
int bns_build_end(bns_ctx *ctx)
{
    if (!ctx) return BNS_ERR_ARG;
    build_free(ctx);
    return BNS_OK;
}

int bns_windows_begin(bns_ctx *ctx, uint32_t window_len, uint32_t pair_cap) { return windows_begin(ctx, window_len, pair_cap); }
int bns_windows_begin_conf(bns_ctx *ctx, uint32_t window_len, uint32_t pair_cap, uint64_t num, uint64_t den)
{
    return windows_begin(ctx, window_len, pair_cap, num, den);
}
int bns_windows_add(bns_ctx *ctx, const char *d_bases, const uint64_t *d_offsets, uint64_t n_seqs, uint64_t total_bases,
                    const uint32_t *d_taxid, uint32_t *d_taxon, void *stream)
{
    return windows_add(ctx, d_bases, d_offsets, n_seqs, total_bases, d_taxid, d_taxon, stream);
}
int bns_windows_read(bns_ctx *ctx, uint32_t *seq_taxid, uint32_t *called, uint64_t *count, uint64_t cap, uint64_t *n_pairs,
                     uint64_t *n_dropped, int reset)
{
    return windows_read(ctx, seq_taxid, called, count, cap, n_pairs, n_dropped, reset);
}
int bns_windows_timing(bns_ctx *ctx, double *ms3, uint64_t *n_adds)
{
    if (!ctx || !ms3) return BNS_ERR_ARG;
    if (!ctx->windows) return fail(ctx, BNS_ERR_STATE, "bns_windows_timing: no window session is open (bns_windows_begin)");
    if (!ctx->windows->ev[0]) return fail(ctx, BNS_ERR_STATE, "bns_windows_timing: timing was off when the session began (bns_set_timing)");
    for (int i = 0; i < 3; ++i) { ms3[i] = ctx->windows->ms[i]; ctx->windows->ms[i] = 0; }
    if (n_adds) *n_adds = ctx->windows->n_adds;
    ctx->windows->n_adds = 0;
    return BNS_OK;
}
int bns_windows_end(bns_ctx *ctx)
{
    if (!ctx) return BNS_ERR_ARG;
    windows_free(ctx);
    return BNS_OK;
}

int bns_dev_alloc(bns_ctx *ctx, size_t bytes, void **out)
{
    if (!ctx || !out) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMalloc(out, bytes ? bytes : 4));
    return BNS_OK;
}
int bns_host_alloc(bns_ctx *ctx, size_t bytes, void **out)
{
    if (!ctx || !out) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // (portable: a block read for one device may be classified by another -- `bonsai classify -g 0-7` hands blocks to whichever is free)
    HIPCHK(ctx, hipHostMalloc(out, bytes ? bytes : 4, hipHostMallocPortable));
    return BNS_OK;
}
int bns_host_free(bns_ctx *ctx, void *p)
{
    if (!ctx) return BNS_ERR_ARG;
    if (p) HIPCHK(ctx, hipHostFree(p));
    return BNS_OK;
}
int bns_dev_free(bns_ctx *ctx, void *p)
{
    if (!ctx) return BNS_ERR_ARG;
    if (p) HIPCHK(ctx, hipFree(p));
    return BNS_OK;
}
int bns_dev_upload(bns_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!ctx) return BNS_ERR_ARG;
    if (bytes) HIPCHK(ctx, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return BNS_OK;
}
int bns_dev_download(bns_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    if (!ctx) return BNS_ERR_ARG;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (bytes) HIPCHK(ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return BNS_OK;
}
int bns_dev_sync(bns_ctx *ctx)
{
    if (!ctx) return BNS_ERR_ARG;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipDeviceSynchronize());
    return BNS_OK;
}

}  // extern "C"

#include "bns_ingest.hip"
