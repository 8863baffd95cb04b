// bns_table_load.hpp -- loading a db into the plain (BNS_LAYOUT_BUCKET) or clustered (BNS_LAYOUT_MINBUCKET) bucket table, on one
// context or on several: the launches and copies.  What they decide on the way -- table size, minimizer, fill, upload or stream
// -- is bns_table_plan.hpp; the answers of one load are a TablePlan, and a load that is handed one (a replica of a multi-context
// load: the root's) follows it instead of deciding.  Included by bns_api.hip (bns_ctx, HIPCHK, BNS_RC, fail, free_table, grid_for,
// SmallLayout); the extern "C" entry points there are thin calls into load_table_resident / load_table_host / load_table_multi.
#pragma once

namespace {

// a device allocation that is freed when its scope ends, unless it was handed on first
template <class T>
struct DevOwned {
    T *p = nullptr;
    DevOwned() = default;
    DevOwned(const DevOwned &) = delete;
    DevOwned &operator=(const DevOwned &) = delete;
    ~DevOwned() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t n) { return hipMalloc((void **)&p, n * sizeof(T)); }
    T *hand_on() { T *q = p; p = nullptr; return q; }
};

int check_n_buckets(bns_ctx *ctx, u64 n_buckets)
{
    if (n_buckets == 0 || (n_buckets & (n_buckets - 1))) return fail(ctx, BNS_ERR_TABLE, "n_buckets must be a power of two");
    return BNS_OK;
}

inline u64 stream_chunk(int dbg)                     // slots per streamed chunk (tests run many small ones: debug bits 16-20)
{
    const int l = (dbg & BNS_DBG_STREAM_CHUNK_MASK) >> BNS_DBG_STREAM_CHUNK_SHIFT;
    return l >= 4 ? 1ULL << l : 1ULL << 27;
}

// Where the khash arrays are read from while a bucket table is built: resident on the device (one "chunk"), or on the host,
// streamed through a device staging buffer 2^27 slots at a time -- for dbs whose arrays and table do not fit the HBM together
// (8e9 keys: 210 GB of arrays + a 230 GB table).  The fill / overflow kernels see one chunk at a time.
struct KhSource {
    bns_ctx *ctx;
    hipStream_t st;
    u64 n_buckets;
    const u32 *d_flags = nullptr; const u64 *d_keys = nullptr; const u32 *d_vals = nullptr;     // resident, or
    const u32 *h_flags = nullptr; const u64 *h_keys = nullptr; const u32 *h_vals = nullptr;     // on the host, with
    u64 chunk = 0;                                                                              // slots per chunk and
    DevOwned<u32> sf; DevOwned<u64> sk; DevOwned<u32> sv;                                       // the staging buffers

    bool streamed() const { return h_flags != nullptr; }
    int stage()
    {
        if (!streamed()) return BNS_OK;
        const u64 cn = std::min<u64>(n_buckets, chunk);
        HIPCHK(ctx, sf.alloc(std::max<u64>(1, cn >> 4)));
        HIPCHK(ctx, sk.alloc(cn));
        HIPCHK(ctx, sv.alloc(cn));
        return BNS_OK;
    }
    // every pass over the khash arrays goes through here: fn(flags, keys, vals, n) once for resident arrays, once per chunk
    // (uploaded into the staging buffers, stream-ordered behind the previous chunk's kernel) for streamed ones.  flags_only: the
    // pass reads nothing else (the key count), so nothing else crosses PCIe; no_vals: flags and keys (the trial, the group count).
    template <class F>
    int for_chunks(F fn, bool flags_only = false, bool no_vals = false)
    {
        if (!streamed()) { fn(d_flags, d_keys, d_vals, n_buckets); return BNS_OK; }
        for (u64 o = 0; o < n_buckets; o += chunk) {
            const u64 cn = std::min<u64>(chunk, n_buckets - o);
            HIPCHK(ctx, hipMemcpyAsync(sf.p, h_flags + (o >> 4), std::max<u64>(1, cn >> 4) * 4, hipMemcpyHostToDevice, st));
            if (!flags_only) {
                HIPCHK(ctx, hipMemcpyAsync(sk.p, h_keys + o, cn * 8, hipMemcpyHostToDevice, st));
                if (!no_vals) HIPCHK(ctx, hipMemcpyAsync(sv.p, h_vals + o, cn * 4, hipMemcpyHostToDevice, st));
            }
            fn((const u32 *)sf.p, (const u64 *)sk.p, (const u32 *)sv.p, cn);
            HIPCHK(ctx, hipGetLastError());
        }
        return BNS_OK;
    }
};

// One load of a bucket table, step by step (load_table below calls them in order).
struct TableLoad {
    bns_ctx *ctx;
    hipStream_t st;
    KhSource &src;
    unsigned long long *d_cnt;      // SmallLayout::load_cnt
    unsigned long long n_present = 0;
    TablePlan plan;
    DevOwned<Slot> slots, ovf;      // tens of GB each: released on every early return (HIPCHK returns from the function), handed to the context by commit()
    u64 n_slots = 0, n_alloc = 0, n_ovf_slots = 0, n_ovf_keys = 0, n_spilled = 0;

    TableLoad(bns_ctx *c, hipStream_t s, KhSource &k) : ctx(c), st(s), src(k), d_cnt(((SmallLayout *)c->small.p)->load_cnt) {}
    int zero_counters() { HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, sizeof(SmallLayout::load_cnt), st)); return BNS_OK; }
    MinBucket *mb() const { return reinterpret_cast<MinBucket *>(slots.p); }

    // present keys (what kh_size would say): the table is sized from them, not from the khash bucket count (a khash is
    // anywhere between 38 % and 77 % full)
    int count_present()
    {
        BNS_RC(zero_counters());
        BNS_RC(src.for_chunks([&](const u32 *cf, const u64 *, const u32 *, u64 cn) {
            hipLaunchKernelGGL(count_present_kernel, dim3(grid_for(ctx, std::max<u64>(1, cn >> 4), 256)), dim3(256), 0, st, cf, cn, d_cnt);
        }, true));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(&n_present, d_cnt, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        return BNS_OK;
    }

    // plan, first half: how large, from the caller's requests and what is free here -- and the table, allocated and zeroed.  A
    // replica takes the root's size as an exact request: what its own device has free is still checked.
    int size_table(int layout, const TablePlan *follow)
    {
        size_t free_b = 0, total_b = 0;
        HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
        const char *msg = "";
        plan.layout = layout;
        if (layout == BNS_LAYOUT_BUCKET) {
            const int rc = plan_bucket_slots(src.n_buckets, free_b, follow ? follow->slots_log2 : ctx->slots_log2_req, plan.slots_log2, msg);
            if (rc != BNS_OK) return fail(ctx, rc, msg);
            n_slots = 1ULL << plan.slots_log2;
        } else {
            const int rc = plan_minbucket_buckets(n_present, free_b, follow ? follow->n_mb : ctx->n_buckets_req, follow ? 0u : ctx->slots_log2_req,
                                                  plan.n_mb, msg);
            if (rc != BNS_OK) return fail(ctx, rc, msg);
            n_alloc = plan.n_mb + MINB_MAX_CHAIN - 1;              // spill-only buckets behind the last home: chains never wrap
            n_slots = n_alloc * 8;
        }
        HIPCHK(ctx, slots.alloc(n_slots));
        HIPCHK(ctx, hipMemsetAsync(slots.p, 0, n_slots * sizeof(Slot), st));
        return BNS_OK;
    }

    // plan, second half (clustered layout): the minimizer and the fill.  One candidate, or a plan to follow: nothing to try.
    int choose_minimizer(const TablePlan *follow)
    {
        if (follow) { plan.spec = follow->spec; plan.span = follow->span; plan.group_fill = follow->group_fill; return BNS_OK; }
        const PlanCands cands = ctx->spaced ? plan_cands_spaced(ctx->k, n_present, ctx->sp_run_len, ctx->sp_run_shift, ctx->dbg)
                                            : plan_cands_contiguous(ctx->k, ctx->min_span_req, ctx->wide_req);
        u32 pick = cands.n - 1;
        double trial_miss = 0.0;                                   // the chosen candidate's share of keys outside their home bucket
        if (cands.n > 1) BNS_RC(run_trial(cands, pick, trial_miss));
        plan.spec = cands.c[pick];
        plan.span = cands.span[pick];
        plan.group_fill = plan_group_fill(cands.n, trial_miss, n_present, plan.n_mb, ctx->fill_req, ctx->dbg);
        return BNS_OK;
    }

    // ---- choose.  One pass over the khash arrays tries all candidates at once on a sample of the BUCKETS (every bucket for a
    // small table, one in 2^j for a large one: whole minimizer groups, at the table's own load) and counts the keys that miss
    // their home bucket (minbucket_trial_kernel); then ONE fill with the winner.  Streamed arrays cross PCIe twice (flags and
    // keys for the trial, everything for the fill) whatever the number of candidates; round 2 filled the whole table once per
    // candidate.
    int run_trial(const PlanCands &cands, u32 &pick, double &trial_miss)
    {
        const u32 n_mb = (u32)plan.n_mb, sample = plan_trial_sample(plan.n_mb);
        const size_t img = (size_t)(sample + MINB_MAX_CHAIN);
        DevOwned<u32> d_img;
        HIPCHK(ctx, d_img.alloc(cands.n * img));
        HIPCHK(ctx, hipMemsetAsync(d_img.p, 0, cands.n * img * sizeof(u32), st));
        DevOwned<unsigned long long> d_trial;
        unsigned long long tr[3 * PLAN_MAX_CANDS] = {0};
        HIPCHK(ctx, d_trial.alloc(3 * PLAN_MAX_CANDS));
        HIPCHK(ctx, hipMemsetAsync(d_trial.p, 0, sizeof(tr), st));
        TrialCands tc;
        tc.n = cands.n;
        for (u32 ci = 0; ci < cands.n; ++ci) tc.c[ci] = cands.c[ci];
        BNS_RC(src.for_chunks([&](const u32 *cf, const u64 *ck, const u32 *, u64 cn) {
            hipLaunchKernelGGL(minbucket_trial_kernel, dim3(grid_for(ctx, cn, 256)), dim3(256), 0, st, cf, ck, cn, n_mb, sample, d_img.p, d_trial.p, ctx->k, tc);
        }, false, true));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(tr, d_trial.p, sizeof(tr), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        pick = plan_pick(cands, ctx->spaced, tr, trial_miss);
        return BNS_OK;
    }

    int fill_bucket()
    {
        BNS_RC(zero_counters());
        BNS_RC(src.for_chunks([&](const u32 *cf, const u64 *ck, const u32 *cv, u64 cn) {
            hipLaunchKernelGGL(rebucket_kernel, dim3(grid_for(ctx, cn, 256)), dim3(256), 0, st, cf, ck, cv, cn, slots.p, n_slots / 4 - 1, d_cnt);
        }));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(st));
        return BNS_OK;
    }

    // arrival order: one pass; group by group: count, decide, residents, the rest (plan_group_fill says which and why)
    int fill_minbucket()
    {
        const u32 n_mb = (u32)plan.n_mb, k = ctx->k;
        const MinSpec spec = plan.spec;
        unsigned long long h[5] = {0, 0, 0, 0, 0};
        BNS_RC(zero_counters());   // [0] present, [1] chain exhausted, [2] moved by place, [3] error, [4] spilled, [5] [6] decide
        if (plan.group_fill) {
            BNS_RC(src.for_chunks([&](const u32 *cf, const u64 *ck, const u32 *, u64 cn) {
                hipLaunchKernelGGL(minbucket_tagcount_kernel, dim3(grid_for(ctx, cn, 256)), dim3(256), 0, st, cf, ck, cn, mb(), n_mb, k, spec);
            }, false, true));
            hipLaunchKernelGGL(minbucket_decide_kernel, dim3(grid_for(ctx, plan.n_mb, 256)), dim3(256), 0, st, mb(), plan.n_mb, d_cnt + 5);
            BNS_RC(src.for_chunks([&](const u32 *cf, const u64 *ck, const u32 *cv, u64 cn) {
                hipLaunchKernelGGL(minbucket_fill_kernel<1>, dim3(grid_for(ctx, cn, 256)), dim3(256), 0, st, cf, ck, cv, cn, mb(), n_mb, d_cnt, k, spec);
            }));
            BNS_RC(src.for_chunks([&](const u32 *cf, const u64 *ck, const u32 *cv, u64 cn) {
                hipLaunchKernelGGL(minbucket_fill_kernel<2>, dim3(grid_for(ctx, cn, 256)), dim3(256), 0, st, cf, ck, cv, cn, mb(), n_mb, d_cnt, k, spec);
            }));
        } else
            BNS_RC(src.for_chunks([&](const u32 *cf, const u64 *ck, const u32 *cv, u64 cn) {
                hipLaunchKernelGGL(minbucket_fill_kernel<0>, dim3(grid_for(ctx, cn, 256)), dim3(256), 0, st, cf, ck, cv, cn, mb(), n_mb, d_cnt, k, spec);
            }));
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(h, d_cnt, 40, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        n_spilled = h[4];
        n_ovf_keys = h[1];
        if (h[0] && (h[4] + h[1]) * 100ULL >= h[0]) {
            char buf[256];
            std::snprintf(buf, sizeof(buf), "%llu of %llu keys (%.1f %%) are not in their home bucket (minimizer window %u, %.0f %% load): lookups of "
                          "this table take extra probe passes; a larger table (bns_set_table_buckets) or a narrower window helps",
                          (unsigned long long)(h[4] + h[1]), (unsigned long long)h[0], 100.0 * (double)(h[4] + h[1]) / (double)h[0],
                          k - spec.m, 100.0 * (double)h[0] / ((double)plan.n_mb * MINB_CAP));
            ctx->warn = buf;
        }
        return BNS_OK;
    }

    // the overflow table: the keys whose chain was full, then every bucket gets its perfect hash (minbucket_place_kernel; a bucket
    // without one moves its keys here too)
    int place_overflow()
    {
        const u32 n_mb = (u32)plan.n_mb, k = ctx->k;
        const MinSpec spec = plan.spec;
        unsigned long long h[4] = {0, 0, 0, 0};
        n_ovf_slots = plan_overflow_slots(n_ovf_keys, n_alloc, ctx->dbg);
        HIPCHK(ctx, ovf.alloc(n_ovf_slots));
        HIPCHK(ctx, hipMemsetAsync(ovf.p, 0, n_ovf_slots * sizeof(Slot), st));
        u32 *d_err = reinterpret_cast<u32 *>(d_cnt + 3);
        if (n_ovf_keys)
            BNS_RC(src.for_chunks([&](const u32 *cf, const u64 *ck, const u32 *cv, u64 cn) {
                hipLaunchKernelGGL(minbucket_overflow_kernel, dim3(grid_for(ctx, cn, 256)), dim3(256), 0, st, cf, ck, cv, cn,
                                   (const MinBucket *)mb(), n_mb, ovf.p, n_ovf_slots / 4 - 1, k, spec, d_err);
            }));
        hipLaunchKernelGGL(minbucket_place_kernel, dim3(grid_for(ctx, n_alloc, 4)), dim3(256), 0, st, mb(), n_alloc, n_mb, ovf.p, n_ovf_slots / 4 - 1, d_cnt + 2, d_err,
                           (u32)((ctx->dbg & BNS_DBG_PLACE_FAIL) ? 61 : 0), k, spec);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(h, d_cnt, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        n_ovf_keys += h[2];
        if (h[3]) return fail(ctx, BNS_ERR_TABLE, "overflow table full while placing bucket keys");
        return BNS_OK;
    }

    // the table and its plan into the context; `same`: the arrays were the context's own (the host-upload path)
    int commit(bool same)
    {
        unsigned long long h_cnt = 0;
        HIPCHK(ctx, hipMemcpyAsync(&h_cnt, d_cnt, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        if (plan.layout == BNS_LAYOUT_BUCKET && h_cnt >= n_slots) return fail(ctx, BNS_ERR_TABLE, "bucket table too small for the key count");
        ctx->slots = slots.hand_on(); ctx->n_slots = n_slots; ctx->n_mb = (u32)plan.n_mb; ctx->n_keys = h_cnt;
        ctx->ovf_slots = ovf.hand_on(); ctx->n_ovf_slots = n_ovf_slots; ctx->n_ovf_keys = n_ovf_keys;
        ctx->layout = plan.layout; ctx->table_k = ctx->k;
        if (plan.layout == BNS_LAYOUT_MINBUCKET) { ctx->table_span = plan.span; ctx->group_fill = plan.group_fill; ctx->n_spilled = n_spilled; }
        const MinSpec spec = plan.layout == BNS_LAYOUT_MINBUCKET ? plan.spec : MinSpec{ctx->k, ctx->k, 0u, 1u, 0u};
        ctx->table_m = spec.m; ctx->table_len = spec.len; ctx->table_shift = spec.shift; ctx->table_canon = spec.canon;
        ctx->table_wide = spec.wide != 0;
        if (same && ctx->own_khash) {                     // host-upload path: the khash copy is no longer needed
            (void)hipFree((void *)ctx->kflags); (void)hipFree((void *)ctx->kkeys); (void)hipFree((void *)ctx->kvals);
            ctx->own_khash = false;
        }
        ctx->kflags = nullptr; ctx->kkeys = nullptr; ctx->kvals = nullptr; ctx->kh_nb = 0;
        return BNS_OK;
    }
};

// what the loaded table of a context was built to: the plan its replicas follow
TablePlan loaded_plan(const bns_ctx *c)
{
    TablePlan p;
    p.layout = c->layout;
    if (c->layout == BNS_LAYOUT_BUCKET) while ((1ULL << p.slots_log2) < c->n_slots) ++p.slots_log2;
    if (c->layout == BNS_LAYOUT_MINBUCKET) {
        p.n_mb = c->n_mb;
        p.spec = MinSpec{c->table_m, c->table_len, c->table_shift, c->table_canon, c->table_wide ? 1u : 0u};
        p.span = c->table_span;
        p.group_fill = c->group_fill;
    }
    return p;
}

// BNS_LAYOUT_KHASH: the arrays themselves are the table
int load_khash(bns_ctx *ctx, KhSource &src)
{
    if (src.streamed()) return fail(ctx, BNS_ERR_ARG, "BNS_LAYOUT_KHASH probes the arrays themselves: they must be resident");
    ctx->kflags = src.d_flags; ctx->kkeys = src.d_keys; ctx->kvals = src.d_vals; ctx->kh_nb = src.n_buckets;
    ctx->layout = BNS_LAYOUT_KHASH;
    // present keys (what kh_size would say): one pass over the flag words, so that bns_table_info says what the other layouts'
    // loads say and bns_table_tally's sum(direct) can be held against it
    TableLoad load(ctx, src.st, src);
    BNS_RC(load.count_present());
    ctx->n_keys = load.n_present;
    return BNS_OK;
}

// follow: the plan of another context's load of the same db (a replica); nullptr: this load decides
int load_table(bns_ctx *ctx, KhSource &src, int layout, const TablePlan *follow)
{
    BNS_RC(check_n_buckets(ctx, src.n_buckets));
    if (layout != BNS_LAYOUT_KHASH && layout != BNS_LAYOUT_BUCKET && layout != BNS_LAYOUT_MINBUCKET) return BNS_ERR_ARG;
    if (layout == BNS_LAYOUT_MINBUCKET && !ctx->enc_set)
        return fail(ctx, BNS_ERR_STATE, "BNS_LAYOUT_MINBUCKET needs the encoder (k) configured before the table is loaded");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // keep caller-owned arrays alive across free_table when they are the same pointers
    const bool same = !src.streamed() && (src.d_flags == ctx->kflags);
    if (!same) free_table(ctx);
    else {
        if (ctx->slots) (void)hipFree(ctx->slots);
        if (ctx->ovf_slots) (void)hipFree(ctx->ovf_slots);
        ctx->slots = nullptr; ctx->n_slots = 0; ctx->n_mb = 0; ctx->ovf_slots = nullptr; ctx->n_ovf_slots = 0; ctx->n_ovf_keys = 0;
    }
    ctx->warn.clear();
    if (layout == BNS_LAYOUT_KHASH) return load_khash(ctx, src);

    TableLoad load(ctx, src.st, src);
    BNS_RC(src.stage());
    BNS_RC(load.count_present());
    BNS_RC(load.size_table(layout, follow));
    if (layout == BNS_LAYOUT_BUCKET) BNS_RC(load.fill_bucket());
    else {
        BNS_RC(load.choose_minimizer(follow));
        BNS_RC(load.fill_minbucket());
        BNS_RC(load.place_overflow());
    }
    return load.commit(same);
}

int load_table_resident(bns_ctx *ctx, u64 n_buckets, const u32 *d_flags, const u64 *d_keys, const u32 *d_vals, int layout, void *stream,
                        const TablePlan *follow = nullptr)
{
    KhSource src{ctx, stream ? (hipStream_t)stream : ctx->stream, n_buckets};
    src.d_flags = d_flags; src.d_keys = d_keys; src.d_vals = d_vals;
    return load_table(ctx, src, layout, follow);
}

// host arrays: streamed (plan_stream_load; stream_bits: the root's BNS_DBG_STREAM_* bits, for a replica of a streamed load) or
// uploaded whole and loaded from the copy
int load_table_host(bns_ctx *ctx, u64 n_buckets, const u32 *flags, const u64 *keys, const u32 *vals, int layout,
                    const TablePlan *follow = nullptr, int stream_bits = 0)
{
    BNS_RC(check_n_buckets(ctx, n_buckets));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    free_table(ctx);
    if (layout != BNS_LAYOUT_KHASH) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
        if (plan_stream_load(n_buckets, free_b, ctx->dbg | stream_bits)) {
            KhSource src{ctx, ctx->stream, n_buckets};
            src.h_flags = flags; src.h_keys = keys; src.h_vals = vals; src.chunk = stream_chunk(ctx->dbg | stream_bits);
            return load_table(ctx, src, layout, follow);
        }
    }
    const size_t fs = khash_flag_words(n_buckets);
    u32 *df = nullptr; u64 *dk = nullptr; u32 *dv = nullptr;
    // each pointer goes into the context as soon as it exists, so free_table() releases it whatever fails next
    ctx->own_khash = true; ctx->kh_nb = n_buckets;
    HIPCHK(ctx, hipMalloc((void **)&df, fs * 4));
    ctx->kflags = df;
    HIPCHK(ctx, hipMalloc((void **)&dk, (size_t)n_buckets * 8));
    ctx->kkeys = dk;
    HIPCHK(ctx, hipMalloc((void **)&dv, (size_t)n_buckets * 4));
    ctx->kvals = dv;
    HIPCHK(ctx, hipMemcpyAsync(df, flags, fs * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dk, keys, (size_t)n_buckets * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(dv, vals, (size_t)n_buckets * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const int rc = load_table_resident(ctx, n_buckets, df, dk, dv, layout, ctx->stream, follow);
    if (rc == BNS_OK && layout == BNS_LAYOUT_KHASH) ctx->own_khash = true;
    return rc;
}

// ---- multi-GPU table load: one upload, RCCL broadcast over xGMI, one device-side re-hash per GPU -------------------------
// librccl is opened lazily and privately (RTLD_LOCAL) the first time a broadcast is wanted: a single-GPU process never maps it,
// and a host that already carries its own RCCL (PyTorch ships one) does not get a second set of nccl* symbols in its global
// namespace.  The entry points' types come from <rccl/rccl.h> itself (decltype of the declarations): a signature or enum that
// drifts is a compile error here, not a silent ABI mismatch behind dlsym.
struct Rccl {
    void *lib = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclGetVersion) GetVersion = nullptr;
    int version = 0, last_ranks = 0;            // what bns_rccl_info reports: the library's version code, the ranks of the last broadcast
    std::once_flag once;
    std::string open_err;
    bool ok = false;
    bool open(std::string &err)
    {
        std::call_once(once, [this] {
            for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
                lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
                if (lib) break;
            }
            if (!lib) { const char *de = dlerror(); open_err = std::string("cannot open librccl: ") + (de ? de : "?"); return; }
            auto sym = [&](const char *n) { void *q = dlsym(lib, n); if (!q && open_err.empty()) open_err = std::string("librccl lacks ") + n; return q; };
            CommInitAll = (decltype(CommInitAll))sym("ncclCommInitAll");
            CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
            GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
            GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
            Broadcast = (decltype(Broadcast))sym("ncclBroadcast");
            GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
            GetVersion = (decltype(GetVersion))dlsym(lib, "ncclGetVersion");
            if (GetVersion) (void)GetVersion(&version);
            ok = CommInitAll && CommDestroy && GroupStart && GroupEnd && Broadcast && GetErrorString;
        });
        if (!ok) err = open_err;
        return ok;
    }
};
Rccl g_rccl;

// One communicator over the contexts' devices (a single process driving several devices: every rank's call inside one group),
// one grouped ncclBroadcast per array from rank 0.  n_ctx == 1 is legal (a one-rank communicator: how a one-GPU box executes the
// real RCCL calls); duplicate devices are not (RCCL admits a device once per communicator).
int rccl_broadcast(bns_ctx **ctxs, int n_ctx, const std::vector<std::array<void *, 3>> &dev, const size_t bytes[3], std::string &err)
{
    if (!g_rccl.open(err)) return BNS_ERR_HIP;
    std::vector<int> devs((size_t)n_ctx);
    for (int i = 0; i < n_ctx; ++i) devs[(size_t)i] = ctxs[i]->device;
    std::vector<ncclComm_t> comms((size_t)n_ctx, nullptr);
    ncclResult_t rc = g_rccl.CommInitAll(comms.data(), n_ctx, devs.data());
    if (rc != ncclSuccess) { err = std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(rc); return BNS_ERR_HIP; }
    bool hip_fail = false;
    for (int a = 0; a < 3 && rc == ncclSuccess && !hip_fail; ++a) {
        rc = g_rccl.GroupStart();
        for (int i = 0; i < n_ctx && rc == ncclSuccess; ++i) {
            if (hipSetDevice(ctxs[i]->device) != hipSuccess) { hip_fail = true; break; }
            // (every rank passes its OWN buffer as send and receive buffer: in place on the root, ignored as a source elsewhere)
            rc = g_rccl.Broadcast(dev[(size_t)i][a], dev[(size_t)i][a], bytes[a], ncclUint8, 0, comms[(size_t)i], ctxs[i]->stream);
        }
        const ncclResult_t rc2 = g_rccl.GroupEnd();
        if (rc == ncclSuccess) rc = rc2;
    }
    for (int i = 0; i < n_ctx; ++i) { (void)hipSetDevice(ctxs[i]->device); (void)hipStreamSynchronize(ctxs[i]->stream); }
    for (int i = 0; i < n_ctx; ++i) if (comms[(size_t)i]) (void)g_rccl.CommDestroy(comms[(size_t)i]);
    if (rc == ncclSuccess && !hip_fail) g_rccl.last_ranks = n_ctx;
    if (rc != ncclSuccess || hip_fail) {
        err = std::string("RCCL broadcast of the table: ") + (hip_fail ? "hipSetDevice failed" : g_rccl.GetErrorString(rc));
        return BNS_ERR_HIP;
    }
    return BNS_OK;
}

// HIPCHK for the multi-context loader: remembers WHICH context failed, so the wrapper can hand its message to the root
#define HIPCHK_M(c, expr) do { failed = (c); HIPCHK((c), expr); failed = nullptr; } while (0)

// 0. a db whose arrays do not fit the HBM next to its table cannot be replicated array by array: every context streams the
//    host buffers into its own table (load_table_host), the first alone (its plan is everyone's), the others side by side --
//    each over its own PCIe link, with the root's stream switches.  One candidate and no trial on a replica: its trial pass
//    (flags + keys over PCIe once more) is not repeated and every replica is the same table.
int load_table_multi_streamed(bns_ctx **ctxs, int n_ctx, u64 n_buckets, const u32 *flags, const u64 *keys, const u32 *vals, int layout, bns_ctx *&failed)
{
    bns_ctx *root = ctxs[0];
    failed = root;
    const int rc = load_table_host(root, n_buckets, flags, keys, vals, layout);
    if (rc != BNS_OK) return rc;
    failed = nullptr;
    const TablePlan plan = loaded_plan(root);
    const int stream_bits = root->dbg & (BNS_DBG_STREAM_LOAD | BNS_DBG_STREAM_CHUNK_MASK);
    std::vector<int> rcs((size_t)n_ctx, BNS_OK);
    std::vector<std::thread> th;
    for (int i = 1; i < n_ctx; ++i)
        th.emplace_back([&, i] { rcs[(size_t)i] = load_table_host(ctxs[i], n_buckets, flags, keys, vals, layout, &plan, stream_bits); });
    for (auto &t : th) t.join();
    for (int i = 1; i < n_ctx; ++i) if (rcs[(size_t)i] != BNS_OK) { failed = ctxs[i]; return rcs[(size_t)i]; }
    return BNS_OK;
}

// (n_buckets was checked by bns_load_table_multi, before any context's table is touched)
int load_table_multi(bns_ctx **ctxs, int n_ctx, u64 n_buckets, const u32 *flags, const u64 *keys, const u32 *vals, int layout, bns_ctx *&failed)
{
    bns_ctx *root = ctxs[0];
    const size_t bytes[3] = {khash_flag_words(n_buckets) * 4, (size_t)n_buckets * 8, (size_t)n_buckets * 4};
    const void *host[3] = {flags, keys, vals};
    if (layout != BNS_LAYOUT_KHASH) {
        size_t free_b = 0, total_b = 0;
        HIPCHK_M(root, hipSetDevice(root->device));
        HIPCHK_M(root, hipMemGetInfo(&free_b, &total_b));
        if (plan_stream_load(n_buckets, free_b, root->dbg)) return load_table_multi_streamed(ctxs, n_ctx, n_buckets, flags, keys, vals, layout, failed);
    }
    // 1. device copies of the khash arrays on every context's device (owned by the contexts: free_table releases them)
    std::vector<std::array<void *, 3>> dev((size_t)n_ctx, std::array<void *, 3>{nullptr, nullptr, nullptr});
    for (int i = 0; i < n_ctx; ++i) {
        bns_ctx *c = ctxs[i];
        HIPCHK_M(c, hipSetDevice(c->device));
        free_table(c);
        c->own_khash = true; c->kh_nb = n_buckets;
        HIPCHK_M(c, hipMalloc(&dev[i][0], bytes[0])); c->kflags = (const u32 *)dev[i][0];
        HIPCHK_M(c, hipMalloc(&dev[i][1], bytes[1])); c->kkeys = (const u64 *)dev[i][1];
        HIPCHK_M(c, hipMalloc(&dev[i][2], bytes[2])); c->kvals = (const u32 *)dev[i][2];
    }
    // 2. ONE host-to-device upload (root), then device-to-device replication
    HIPCHK_M(root, hipSetDevice(root->device));
    for (int a = 0; a < 3; ++a) HIPCHK_M(root, hipMemcpyAsync(dev[0][a], host[a], bytes[a], hipMemcpyHostToDevice, root->stream));
    HIPCHK_M(root, hipStreamSynchronize(root->stream));
    bool distinct = true;
    for (int i = 0; i < n_ctx; ++i) for (int j = 0; j < i; ++j) if (ctxs[i]->device == ctxs[j]->device) distinct = false;
    if (distinct) {
        std::string err;
        const int rc = rccl_broadcast(ctxs, n_ctx, dev, bytes, err);       // RCCL over xGMI
        if (rc != BNS_OK) { failed = root; return fail(root, rc, err); }
    } else {
        // several contexts on ONE device (how a one-GPU box exercises the shard / stitch logic; RCCL refuses duplicate devices):
        // plain copies
        for (int i = 1; i < n_ctx; ++i) {
            HIPCHK_M(ctxs[i], hipSetDevice(ctxs[i]->device));
            for (int a = 0; a < 3; ++a) HIPCHK_M(ctxs[i], hipMemcpyAsync(dev[(size_t)i][a], dev[0][a], bytes[a], hipMemcpyDeviceToDevice, ctxs[i]->stream));
            HIPCHK_M(ctxs[i], hipStreamSynchronize(ctxs[i]->stream));
        }
    }
    // 3. every device lays out its own table; one plan for all (the first context's), whatever each finds free
    TablePlan plan;
    for (int i = 0; i < n_ctx; ++i) {
        bns_ctx *c = ctxs[i];
        failed = c;
        const int rc = load_table_resident(c, n_buckets, c->kflags, c->kkeys, c->kvals, layout, c->stream, i > 0 && layout != BNS_LAYOUT_KHASH ? &plan : nullptr);
        if (rc != BNS_OK) return rc;
        failed = nullptr;
        if (layout == BNS_LAYOUT_KHASH) c->own_khash = true;
        if (i == 0) plan = loaded_plan(c);
    }
    return BNS_OK;
}

}  // namespace
