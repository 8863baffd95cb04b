// bns_build.hpp -- the build session behind bns_build_begin / _seed / _add / _finish / _export / _end (gfx950, wave64).
//
// bns_build_table_device builds one table from one batch into arrays of a size the caller guessed.  A session keeps the table in
// the context across calls instead: batches of whole sequences are added one after the other, the table doubles when a batch does
// not fit, and it can start from the present slots of an existing khash table (a bns.db).  What makes that sound:
//   * build_kernel's pass 1 (CAS on the key array) leaves a key it finds alone, and its pass 2 folds with lca(), whose identity is 0 and
//     for which lca(tx, lca(tx, cur)) == lca(tx, cur): applying a batch twice, or after a part of it went in, changes nothing.  So a
//     batch that raised pass 1's "filled up" flag, or left more than 0.77 n_buckets keys, is simply applied again after a grow --
//     that batch alone, never an earlier one.
//   * the fold is order-free, so (table of A) + B == table of A u B, whatever order the sequences of either arrive in.
// Both passes are build_kernel's as they are; a fused form (CAS the key, then CAS-fold the value) was not built.
//
//   build_rehash_kernel<false>  grow / compact: one lane per slot of the old table, key and value read coalesced; a slot whose key is
//                               not BUILD_EMPTY claims a slot on the triangular probe path of the new table (wang64(key) & mask,
//                               i += ++step) with a device-scope CAS, as pass 1 does, and stores its value there with a plain store.
//                               A key sits in ONE slot of the old table, so a slot of the new one has one writer, and nothing in the
//                               launch reads a value: no lane ever sees another wavefront's plain store.
//   build_rehash_kernel<true>   seed: the same over a piece of a khash table, "present" read from the flag pair (00) and never from
//                               the key; empty and deleted slots are skipped whatever their key and value words hold.
//
// Memory.  The table takes 12 bytes a bucket (keys 8, values 4; the flags of the finished table 0.25 more).  A grow holds the old
// table and the new one side by side until the stream has passed the kernel: 12 (n + 2n) bytes for n -> 2n, so a session cannot grow
// past the size at which three times the current table no longer fits beside the batch's workspace.  A grow that cannot be allocated
// is refused with BNS_ERR_TABLE; the table as it was stays in the session, which then only bns_build_end may follow.
//
// Included by bns_api.hip after its helpers (fail, ensure, grid_for, ready) and bns_classify.hpp (pack_reads, set_win_scratch): the host half below uses them.
#pragma once

namespace bns {

template <bool KHASH>
__global__ __launch_bounds__(256) void build_rehash_kernel(const u64 *__restrict__ src_keys, const u32 *__restrict__ src_vals,
                                                           const u32 *__restrict__ src_flags, u64 n_src, u64 *__restrict__ dst_keys,
                                                           u32 *__restrict__ dst_vals, u64 dst_nb, unsigned long long *cnt)
{
    const u64 stride = (u64)gridDim.x * blockDim.x;
    const u64 mask = dst_nb - 1;
    u32 local = 0;
    for (u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x; s < n_src; s += stride) {
        const u64 key = src_keys[s];
        bool present;
        // (~0 cannot be held by a table under construction: no encoder a session accepts emits it, so a seed slot that claims it is skipped)
        if (KHASH) present = ((src_flags[s >> 4] >> ((s & 15u) << 1)) & 3u) == 0u && key != BUILD_EMPTY;
        else       present = key != BUILD_EMPTY;
        if (!present) continue;
        const u32 val = src_vals[s];
        u64 i = wang64(key) & mask, step = 0;
        // the new table has room for every key (the host sized it), so an empty slot is met within dst_nb steps; bounded all the same
        for (;;) {
            const u64 old = atomicCAS((unsigned long long *)&dst_keys[i], (unsigned long long)BUILD_EMPTY, (unsigned long long)key);
            if (old == BUILD_EMPTY) { ++local; dst_vals[i] = val; break; }
            if (old == key) { if (KHASH) dst_vals[i] = val; break; }     // (only a malformed seed names a key twice: one of its values stays)
            i = (i + (++step)) & mask;
            if (step >= dst_nb) { atomicExch(&cnt[1], 1ULL); break; }
        }
    }
    for (int off = 32; off >= 1; off >>= 1) local += (u32)__shfl_xor((int)local, off);
    if (lane_id() == 0 && local) atomicAdd(cnt, (unsigned long long)local);
}

// The session: the table under construction (keys BUILD_EMPTY / vals 0 where empty) and what bns_build_stats reports.
struct BuildSession {
    u64 nb = 0;
    u64 *keys = nullptr;
    u32 *vals = nullptr;
    u32 *flags = nullptr;            // after bns_build_finish
    u64 n_keys = 0, n_seeded = 0, n_batches = 0, n_grows = 0;
    double s_add = 0, s_grow = 0;    // wall seconds inside bns_build_add, and the part of them spent growing (bns_build_stats)
    bool added = false, seeded = false, finished = false, failed = false;
    // bns_build_minimize_begin (bns_minimize.hpp): the table above becomes M, the one it held until then is F, kept here and only read
    bool minimizing = false;
    u32 min_w = 0;                   // the window in bases, at least the comb
    u64 f_nb = 0, f_n_keys = 0;
    u64 *f_keys = nullptr;
    u32 *f_vals = nullptr;
    u32 *depth = nullptr;            // depth[id] for id in [0, n_nodes): nodes on the chain id -> root, 0 where the chain reaches none
    u64 m_batches = 0, m_grows = 0, m_lookups = 0;
    double s_min = 0;                // wall seconds inside bns_build_minimize_add
    // bns_build_count_begin (bns_fewest.hpp): two words per bucket of F, which is frozen from there on
    bool counting = false;
    u32 *g_count = nullptr;          // distinct genome ids among the sequences that hold the bucket's k-mer
    u32 *g_stamp = nullptr;          // id + 1 of the genome that counted the bucket last, 0: none yet
    bool g_any = false;              // a sequence has been counted: g_last is the id of the last one
    u32 g_last = 0;
    u64 g_batches = 0, g_launches = 0, g_genomes = 0, g_lookups = 0, g_largest = 0;
    double s_count = 0;              // wall seconds inside bns_build_count_add
    int min_score = 0;               // BNS_MINIMIZE_DEPTH / BNS_MINIMIZE_FEWEST of bns_build_minimize_begin_score
};

inline u64 build_upper(u64 nb) { return (u64)(nb * 0.77 + 0.5); }                  // khash64.h:198
// khash grows when n_occupied has REACHED upper_bound and another key comes (khash64.h:330): upper_bound keys still fit
inline u64 build_pow2_for(u64 keys) { u64 nb = 4; while (build_upper(nb) < keys) nb <<= 1; return nb; }

}  // namespace bns

namespace {

constexpr u64 BUILD_SEED_CHUNK = 1ULL << 22;         // slots of the seed table uploaded and inserted per launch (a multiple of 16)

void build_free(bns_ctx *ctx)
{
    BuildSession *s = ctx->build;
    if (!s) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (s->keys) (void)hipFree(s->keys);
    if (s->vals) (void)hipFree(s->vals);
    if (s->flags) (void)hipFree(s->flags);
    if (s->f_keys) (void)hipFree(s->f_keys);
    if (s->f_vals) (void)hipFree(s->f_vals);
    if (s->depth) (void)hipFree(s->depth);
    if (s->g_count) (void)hipFree(s->g_count);
    if (s->g_stamp) (void)hipFree(s->g_stamp);
    delete s;
    ctx->build = nullptr;
}

// an empty table of nb buckets; BNS_ERR_TABLE (nothing allocated) when the device has no room for it
int build_alloc_table(bns_ctx *ctx, u64 nb, u64 **keys, u32 **vals, hipStream_t st)
{
    *keys = nullptr; *vals = nullptr;
    if (hipMalloc((void **)keys, (size_t)nb * 8) != hipSuccess || hipMalloc((void **)vals, (size_t)nb * 4) != hipSuccess) {
        (void)hipGetLastError();
        if (*keys) (void)hipFree(*keys);
        *keys = nullptr; *vals = nullptr;
        return fail(ctx, BNS_ERR_TABLE, "build session: no device memory for a table of " + std::to_string(nb) +
                                            " buckets (a grow holds the old and the new table side by side, 12 bytes a bucket each)");
    }
    const unsigned fgrid = grid_for(ctx, nb, 256);
    hipLaunchKernelGGL(fill_u64_kernel, dim3(fgrid), dim3(256), 0, st, *keys, nb, BUILD_EMPTY);
    hipLaunchKernelGGL(fill_u32_kernel, dim3(fgrid), dim3(256), 0, st, *vals, nb, 0u);
    HIPCHK(ctx, hipGetLastError());
    return BNS_OK;
}

// the session's table rehashed into one of new_nb buckets (larger: a grow; smaller: bns_build_finish compacting)
int build_rehash(bns_ctx *ctx, BuildSession *s, u64 new_nb, hipStream_t st)
{
    u64 *nk; u32 *nv;
    int rc = build_alloc_table(ctx, new_nb, &nk, &nv, st);
    if (rc != BNS_OK) return rc;
    unsigned long long *d_cnt = ((SmallLayout *)ctx->small.p)->load_cnt;
    unsigned long long h_cnt[2] = {0, 0};
    hipError_t e = hipMemsetAsync(d_cnt, 0, 16, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL((build_rehash_kernel<false>), dim3(grid_for(ctx, s->nb, 256)), dim3(256), 0, st, (const u64 *)s->keys,
                           (const u32 *)s->vals, (const u32 *)nullptr, s->nb, nk, nv, new_nb, d_cnt);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_cnt, d_cnt, 16, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess || h_cnt[1] || h_cnt[0] != s->n_keys) {
        (void)hipFree(nk); (void)hipFree(nv);
        if (e != hipSuccess) { ctx->err = std::string("build session rehash: ") + hipGetErrorString(e); return BNS_ERR_HIP; }
        return fail(ctx, BNS_ERR_TABLE, "build session: the rehash moved " + std::to_string(h_cnt[0]) + " of " + std::to_string(s->n_keys) + " keys");
    }
    (void)hipFree(s->keys); (void)hipFree(s->vals);          // (the stream has passed the kernel)
    s->keys = nk; s->vals = nv; s->nb = new_nb;
    return BNS_OK;
}

int build_session(bns_ctx *ctx, BuildSession **out, const char *what)
{
    if (!ctx) return BNS_ERR_ARG;
    if (!ctx->build) return fail(ctx, BNS_ERR_STATE, std::string(what) + ": no build session is open (bns_build_begin)");
    if (ctx->build->failed) return fail(ctx, BNS_ERR_STATE, std::string(what) + ": an earlier call of this session failed; its table is incomplete (bns_build_end)");
    *out = ctx->build;
    return BNS_OK;
}

int build_begin(bns_ctx *ctx, u64 hint)
{
    int rc = ready(ctx, false, true);
    if (rc != BNS_OK) return rc;
    if (ctx->build) return fail(ctx, BNS_ERR_STATE, "a build session is already open (bns_build_end)");
    // ~0 marks an empty slot while building (see bns_build_table_device)
    if (ctx->k == 32 && !ctx->canon && !ctx->spaced && !(ctx->win > ctx->c)) return fail(ctx, BNS_ERR_ARG, "device build needs canonical or spaced k-mers when k == 32");
    if (ctx->spaced && !ctx->spaced_intended) return fail(ctx, BNS_ERR_ARG, "spaced build needs spaced_intended=1");
    if (hint > (1ULL << 40)) return fail(ctx, BNS_ERR_TABLE, "n_buckets_hint beyond 2^40");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    u64 nb = 4;
    while (nb < hint) nb <<= 1;
    BuildSession *s = new (std::nothrow) BuildSession();
    if (!s) return BNS_ERR_NOMEM;
    rc = build_alloc_table(ctx, nb, &s->keys, &s->vals, ctx->stream);
    if (rc != BNS_OK) { delete s; return rc; }
    s->nb = nb;
    ctx->build = s;
    return BNS_OK;
}

int build_seed(bns_ctx *ctx, u64 n_buckets, const u32 *flags, const u64 *keys, const u32 *vals)
{
    BuildSession *s;
    int rc = build_session(ctx, &s, "bns_build_seed");
    if (rc != BNS_OK) return rc;
    if (s->minimizing) return fail(ctx, BNS_ERR_STATE, "bns_build_seed after bns_build_minimize_begin: the scored table is frozen");
    if (s->counting) return fail(ctx, BNS_ERR_STATE, "bns_build_seed after bns_build_count_begin: the scored table is frozen");
    if (s->added || s->seeded || s->finished) return fail(ctx, BNS_ERR_STATE, "bns_build_seed comes once, between bns_build_begin and the first bns_build_add");
    if (n_buckets && (!flags || !keys || !vals)) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    u64 n_present = 0;
    for (u64 i = 0; i < n_buckets; ++i) n_present += ((flags[i >> 4] >> ((i & 15u) << 1)) & 3u) == 0u;
    const u64 want = build_pow2_for(n_present);
    if (want > s->nb) {                                       // (the table is still empty: a fresh one, nothing to move)
        HIPCHK(ctx, hipStreamSynchronize(st));
        (void)hipFree(s->keys); (void)hipFree(s->vals);
        s->keys = nullptr; s->vals = nullptr; s->nb = 0;
        s->failed = true;
        if ((rc = build_alloc_table(ctx, want, &s->keys, &s->vals, st)) != BNS_OK) return rc;
        s->failed = false;
        s->nb = want;
    }
    unsigned long long *d_cnt = ((SmallLayout *)ctx->small.p)->load_cnt;
    HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 16, st));
    for (u64 at = 0; at < n_buckets; at += BUILD_SEED_CHUNK) {
        const u64 n = std::min(BUILD_SEED_CHUNK, n_buckets - at);
        const u64 n_fw = (n + 15) >> 4;
        if ((rc = ensure(ctx, ctx->st_kmers, (size_t)n * 8)) != BNS_OK) return rc;
        if ((rc = ensure(ctx, ctx->st_hits, (size_t)n * 4)) != BNS_OK) return rc;
        if ((rc = ensure(ctx, ctx->st_aux, (size_t)n_fw * 4)) != BNS_OK) return rc;
        HIPCHK(ctx, hipMemcpyAsync(ctx->st_kmers.p, keys + at, (size_t)n * 8, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->st_hits.p, vals + at, (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->st_aux.p, flags + (at >> 4), (size_t)n_fw * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL((build_rehash_kernel<true>), dim3(grid_for(ctx, n, 256)), dim3(256), 0, st, (const u64 *)ctx->st_kmers.p,
                           (const u32 *)ctx->st_hits.p, (const u32 *)ctx->st_aux.p, n, s->keys, s->vals, s->nb, d_cnt);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(st));               // (the staging buffers are written again by the next piece)
    }
    unsigned long long h_cnt[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(h_cnt, d_cnt, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    s->n_keys = h_cnt[0]; s->n_seeded = h_cnt[0]; s->seeded = true;
    if (h_cnt[1]) { s->failed = true; return fail(ctx, BNS_ERR_TABLE, "bns_build_seed: the session table filled up (more present slots than the flags count)"); }
    return BNS_OK;
}

int build_add(bns_ctx *ctx, const char *d_bases, const u64 *d_offsets, u64 n_seqs, u64 total_bases, const u32 *d_taxid, void *stream)
{
    BuildSession *s;
    int rc = build_session(ctx, &s, "bns_build_add");
    if (rc != BNS_OK) return rc;
    if (s->finished) return fail(ctx, BNS_ERR_STATE, "bns_build_add after bns_build_finish");
    if (s->minimizing) return fail(ctx, BNS_ERR_STATE, "bns_build_add after bns_build_minimize_begin: the scored table is frozen");
    if (s->counting) return fail(ctx, BNS_ERR_STATE, "bns_build_add after bns_build_count_begin: the scored table is frozen");
    if (n_seqs == 0) { s->added = true; ++s->n_batches; return BNS_OK; }
    if (!d_offsets || !d_taxid) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    if (st != ctx->stream) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // (begin / seed / a grow of an earlier add ran there)
    if ((rc = pack_reads_dust(ctx, d_bases, d_offsets, n_seqs, total_bases, st)) != BNS_OK) return rc;
    unsigned long long *d_cnt = ((SmallLayout *)ctx->small.p)->load_cnt;
    ClassifyParams p;
    fill_params(ctx, p);
    p.offsets = d_offsets; p.n_units = n_seqs; p.nmates = 1;
    const unsigned grid = (unsigned)ctx->n_cu * 8;
    if ((rc = set_win_scratch(ctx, p, grid)) != BNS_OK) return rc;
    const auto t_add = std::chrono::steady_clock::now();
    auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
    s->added = true;
    s->failed = true;                                        // until the batch is in: a call that returns early leaves keys without their values
    for (;;) {
        HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 16, st));       // [0] keys inserted, [1] "table too small" flag of pass 1
        if (ctx->spaced) hipLaunchKernelGGL((build_kernel<true, 1>), dim3(grid), dim3(256), 0, st, p, d_taxid, s->nb, s->keys, s->vals, d_cnt);
        else             hipLaunchKernelGGL((build_kernel<false, 1>), dim3(grid), dim3(256), 0, st, p, d_taxid, s->nb, s->keys, s->vals, d_cnt);
        HIPCHK(ctx, hipGetLastError());
        unsigned long long h_cnt[2] = {0, 0};
        HIPCHK(ctx, hipMemcpyAsync(h_cnt, d_cnt, 16, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        s->n_keys += h_cnt[0];                               // (a key found again is not counted: the sum over all launches is the table's size)
        if (!h_cnt[1] && s->n_keys <= build_upper(s->nb)) break;
        // The batch does not fit: double (more than once when the keys that DID go in are already too many for twice the size) and
        // apply the same batch again.  The keys of this batch that are in stay in, with value 0 until pass 2 has run.
        const auto t_grow = std::chrono::steady_clock::now();
        do {
            if (s->nb >= (1ULL << 40)) return fail(ctx, BNS_ERR_TABLE, "build session: table beyond 2^40 buckets");
            if ((rc = build_rehash(ctx, s, s->nb << 1, st)) != BNS_OK) return rc;
            ++s->n_grows;
        } while (s->n_keys > build_upper(s->nb));
        s->s_grow += since(t_grow);
    }
    if (ctx->spaced) hipLaunchKernelGGL((build_kernel<true, 2>), dim3(grid), dim3(256), 0, st, p, d_taxid, s->nb, s->keys, s->vals, d_cnt);
    else             hipLaunchKernelGGL((build_kernel<false, 2>), dim3(grid), dim3(256), 0, st, p, d_taxid, s->nb, s->keys, s->vals, d_cnt);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));                   // the caller may free or overwrite the batch once the call is back
    s->failed = false;
    ++s->n_batches;
    s->s_add += since(t_add);
    return BNS_OK;
}

int build_finish(bns_ctx *ctx, u64 *header4)
{
    BuildSession *s;
    int rc = build_session(ctx, &s, "bns_build_finish");
    if (rc != BNS_OK) return rc;
    if (s->finished) return fail(ctx, BNS_ERR_STATE, "bns_build_finish called twice");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const u64 want = build_pow2_for(s->n_keys);
    if (want < s->nb) {
        s->failed = true;
        if ((rc = build_rehash(ctx, s, want, st)) != BNS_OK) return rc;
        s->failed = false;
    }
    const u64 n_fw = s->nb < 16 ? 1 : s->nb >> 4;
    HIPCHK(ctx, hipMalloc((void **)&s->flags, (size_t)n_fw * 4));
    hipLaunchKernelGGL(build_finish_kernel, dim3(grid_for(ctx, n_fw, 256)), dim3(256), 0, st, s->nb, s->flags, s->keys, s->vals);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(st));
    s->finished = true;
    if (header4) { header4[0] = s->nb; header4[1] = s->n_keys; header4[2] = s->n_keys; header4[3] = build_upper(s->nb); }
    return BNS_OK;
}

int build_export(bns_ctx *ctx, u32 *flags, u64 *keys, u32 *vals)
{
    BuildSession *s;
    int rc = build_session(ctx, &s, "bns_build_export");
    if (rc != BNS_OK) return rc;
    if (!s->finished) return fail(ctx, BNS_ERR_STATE, "bns_build_export before bns_build_finish");
    if (!flags || !keys || !vals) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(flags, s->flags, (size_t)(s->nb < 16 ? 1 : s->nb >> 4) * 4, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(keys, s->keys, (size_t)s->nb * 8, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(vals, s->vals, (size_t)s->nb * 4, hipMemcpyDeviceToHost));
    return BNS_OK;
}

}  // namespace
