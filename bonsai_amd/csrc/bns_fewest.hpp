// bns_fewest.hpp -- fewest-genome minimizers, the count pass: bns_build_count_begin / _add / _get / _stats (gfx950, wave64).
//
// A build session that has folded every k-mer of every sequence into its table (F) is frozen, and the same sequences are streamed
// once more, each with the id of the genome it belongs to.  Every bucket of F gets two more words, parallel to F's arrays: the number
// n(x) of DISTINCT genome ids among the sequences that hold the bucket's k-mer, and a stamp, id + 1 of the genome that counted it
// last (0: nobody yet).  bns_build_minimize_begin_score(.., BNS_MINIMIZE_FEWEST) then selects by (n << 32 | F[x], x): bns_minimize.hpp.
//
//   count_kernel<SPACED>  minimize_kernel's fill without the image: work item = (sequence, chunk of up to 1984 positions), one wavefront
//                         each, the chunk's 64 words held one per lane.  64 positions a round: extract, canonical, probe F (wang64(key)
//                         & mask, triangular steps, until the key or BUILD_EMPTY), and at the slot
//                             old = atomicExch(&stamp[i], id + 1); if (old != id + 1) atomicAdd(&count[i], 1);
//                         Chunks are cut so that every position belongs to ONE chunk (no window reaches into the neighbour here).
//                         A key that F does not hold raises cnt[3]; the probe stops at the empty slot it met.
//   count_get_kernel      one lane per queried key: the count of its slot, 0 for a key F does not hold.
//
// Why the stamp is exact.  A counter is not idempotent, and a genome must count once however often a k-mer occurs in it -- in one
// contig or several, in two chunks, in two calls.  Every lane of ONE launch carries the same id: whichever lane exchanges first sees
// another genome's stamp (or 0) and adds one, every later one sees id + 1 and adds nothing.  So the host half cuts a call's sequences
// into runs of equal id and launches once per run, over that run's range of units, on the call's stream: launches on one stream are
// ordered, and a run that goes on in the next call meets its own stamp.  That needs the ids of a session to be non-decreasing in stream
// order, which the call checks on the host before it enqueues anything.  (A launch per genome is what small genomes pay: see
// docs/TAXDEPTH_NOTES.md for the cost and for the form with 32 genomes a launch, which is not built.)
// The two atomics are a one-lane-per-row scatter into a table of all k-mers: a cache miss per position, like the gather of pass B.
//
// cnt[0] positions looked up, cnt[1] the largest count this launch wrote, cnt[3] "not in F".
//
// Included by bns_api.hip after bns_build.hpp (the session) and before bns_minimize.hpp.
#pragma once

namespace bns {

constexpr u32 COUNT_CHUNK = 31u * 64u;                // positions a chunk holds (extract_* read words 2 rd .. 2 rd + 3 of 64)

// positions per chunk for a comb of c bases, a multiple of 64: every k-mer of a chunk lies inside its 2048 bases
__host__ __device__ inline u32 count_chunk(u32 c) { return (2049u - c < COUNT_CHUNK ? 2049u - c : COUNT_CHUNK) / 64u * 64u; }

template <bool SPACED>
__global__ __launch_bounds__(256) void count_kernel(ClassifyParams p, u64 r0, u64 r1, u32 stamp_id, const u64 *__restrict__ fkeys, u64 f_nb,
                                                    u32 *__restrict__ count, u32 *__restrict__ stamp, unsigned long long *cnt)
{
    const int lane = lane_id();
    const u32 rdesc = SPACED ? run_desc(p) : 0u;
    const u64 wave = (u64)blockIdx.x * 4u + (threadIdx.x >> 6), n_waves = (u64)gridDim.x * 4u;
    const u32 k = p.k, c = p.c;
    const u64 chunk_k = count_chunk(c);
    const u64 fmask = f_nb - 1;
    u64 lookups = 0;
    u32 largest = 0;
    bool missing = false;
    u64 before = 0;                                               // chunks of the sequences r0 .. r - 1: chunk g belongs to wave g % n_waves
    for (u64 r = r0; r < r1; ++r) {
        const u64 o = p.offsets[r];
        const u64 Lg = p.offsets[r + 1] - o;
        const u64 wb = (o >> 5) + r;                              // (r is the unit's index in the CALL, whatever r0)
        const u64 n_words = (Lg + 31u) >> 5;
        const u64 nk = Lg >= c ? Lg - c + 1u : 0u;                // positions of the sequence
        const u64 n_chunks = (nk + chunk_k - 1) / chunk_k;
        const u64 first = (wave + n_waves - before % n_waves) % n_waves;
        before += n_chunks;
        for (u64 ch = first; ch < n_chunks; ch += n_waves) {
            const u64 j0 = ch * chunk_k;
            const u64 wi = (j0 >> 5) + (u64)lane;
            const u64 W = wi < n_words ? p.words[wb + wi] : 0ULL;
            const u32 M = wi < n_words ? p.nmask[wb + wi] : 0xFFFFFFFFu;
            const u32 n_ent = (nk - j0) < chunk_k ? (u32)(nk - j0) : (u32)chunk_k;
            for (u32 rd = 0; rd * 64u < n_ent; ++rd) {
                const u32 e = rd * 64u + (u32)lane;
                u64 kmer;
                bool valid;
                if (SPACED) valid = p.n_runs ? extract_spaced_runs(W, M, rd, p, rdesc, kmer) : extract_spaced(W, M, rd, k, rdesc, kmer);
                else        valid = extract_unspaced(W, M, rd, k, kmer);
                valid = valid && e < n_ent;
                if (!SPACED && p.canon) kmer = canonical(kmer, k);
                if (valid) {
                    u64 i = wang64(kmer) & fmask, step = 0;
                    bool found = false;
                    for (;;) {                                    // F sits at a load <= 0.77: an empty slot ends a probe that finds nothing
                        const u64 key = fkeys[i];
                        if (key == kmer) { found = true; break; }
                        if (key == BUILD_EMPTY) break;
                        i = (i + (++step)) & fmask;
                        if (step >= f_nb) break;
                    }
                    if (found) {
                        const u32 old = atomicExch(&stamp[i], stamp_id);
                        if (old != stamp_id) {
                            const u32 now = atomicAdd(&count[i], 1u) + 1u;
                            largest = now > largest ? now : largest;
                        }
                    } else { missing = true; valid = false; }
                }
                lookups += (u64)__popcll(ballot64(valid));
            }
        }
    }
    for (int off = 32; off >= 1; off >>= 1) { const u32 x = (u32)__shfl_xor((int)largest, off); largest = x > largest ? x : largest; }
    const bool any_missing = ballot64(missing) != 0ULL;
    if (lane == 0) {
        if (lookups) atomicAdd(&cnt[0], (unsigned long long)lookups);
        if (largest) atomicMax(&cnt[1], (unsigned long long)largest);
        if (any_missing) atomicExch(&cnt[3], 1ULL);
    }
}

__global__ __launch_bounds__(256) void count_get_kernel(const u64 *__restrict__ q, u64 n, const u64 *__restrict__ fkeys, u64 f_nb,
                                                        const u32 *__restrict__ count, u32 *__restrict__ out)
{
    const u64 stride = (u64)gridDim.x * blockDim.x;
    const u64 fmask = f_nb - 1;
    for (u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += stride) {
        const u64 kmer = q[x];
        u32 v = 0;
        if (kmer != BUILD_EMPTY) {                                // (~0 is no key a session holds; its slots are the empty ones)
            u64 i = wang64(kmer) & fmask, step = 0;
            for (;;) {
                const u64 key = fkeys[i];
                if (key == kmer) { v = count[i]; break; }
                if (key == BUILD_EMPTY) break;
                i = (i + (++step)) & fmask;
                if (step >= f_nb) break;
            }
        }
        out[x] = v;
    }
}

}  // namespace bns

namespace {

// F of a counting session: the session's table until bns_build_minimize_begin moves it aside
inline const u64 *count_fkeys(const BuildSession *s) { return s->minimizing ? s->f_keys : s->keys; }
inline u64 count_fnb(const BuildSession *s) { return s->minimizing ? s->f_nb : s->nb; }

int count_begin(bns_ctx *ctx)
{
    BuildSession *s;
    int rc = build_session(ctx, &s, "bns_build_count_begin");
    if (rc != BNS_OK) return rc;
    if (s->finished) return fail(ctx, BNS_ERR_STATE, "bns_build_count_begin after bns_build_finish");
    if (s->minimizing) return fail(ctx, BNS_ERR_STATE, "bns_build_count_begin after bns_build_minimize_begin");
    if (s->counting) return fail(ctx, BNS_ERR_STATE, "bns_build_count_begin called twice");
    if (ctx->win > ctx->c) return fail(ctx, BNS_ERR_STATE, "bns_build_count_begin needs a session that scored every k-mer: bns_set_window is beyond the comb");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    u32 *cn = nullptr, *sp = nullptr;
    if (hipMalloc((void **)&cn, (size_t)s->nb * 4) != hipSuccess || hipMalloc((void **)&sp, (size_t)s->nb * 4) != hipSuccess) {
        (void)hipGetLastError();
        if (cn) (void)hipFree(cn);
        return fail(ctx, BNS_ERR_TABLE, "bns_build_count_begin: no device memory for the counts of " + std::to_string(s->nb) + " buckets (8 bytes a bucket)");
    }
    hipError_t e = hipMemsetAsync(cn, 0, (size_t)s->nb * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(sp, 0, (size_t)s->nb * 4, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(cn); (void)hipFree(sp);
        ctx->err = std::string("bns_build_count_begin: ") + hipGetErrorString(e);
        return BNS_ERR_HIP;
    }
    s->g_count = cn; s->g_stamp = sp;
    s->counting = true;
    return BNS_OK;
}

int count_add(bns_ctx *ctx, const char *d_bases, const u64 *d_offsets, u64 n_seqs, u64 total_bases, const u32 *h_genome, void *stream)
{
    BuildSession *s;
    int rc = build_session(ctx, &s, "bns_build_count_add");
    if (rc != BNS_OK) return rc;
    if (!s->counting) return fail(ctx, BNS_ERR_STATE, "bns_build_count_add before bns_build_count_begin");
    if (s->finished) return fail(ctx, BNS_ERR_STATE, "bns_build_count_add after bns_build_finish");
    if (s->minimizing) return fail(ctx, BNS_ERR_STATE, "bns_build_count_add after bns_build_minimize_begin: the counts are what the selection reads");
    if (n_seqs == 0) { ++s->g_batches; return BNS_OK; }
    if (!d_offsets || !h_genome) return BNS_ERR_ARG;
    // the order of the ids is what makes the stamp exact: checked before anything is enqueued
    for (u64 i = 0; i < n_seqs; ++i) {
        if (h_genome[i] == 0xFFFFFFFFu) return fail(ctx, BNS_ERR_ARG, "bns_build_count_add: 0xFFFFFFFF is no genome id");
        if (i ? h_genome[i] < h_genome[i - 1] : (s->g_any && h_genome[0] < s->g_last))
            return fail(ctx, BNS_ERR_ARG, "bns_build_count_add: genome ids must not decrease, within a call and from one call to the next (sequence " +
                                              std::to_string(i) + " has id " + std::to_string(h_genome[i]) + " after " +
                                              std::to_string(i ? h_genome[i - 1] : s->g_last) + ")");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    if (st != ctx->stream) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // (begin zeroed the counts there)
    const auto t_add = std::chrono::steady_clock::now();
    if ((rc = pack_reads_dust(ctx, d_bases, d_offsets, n_seqs, total_bases, st)) != BNS_OK) return rc;
    std::vector<u64> off(n_seqs + 1);                            // the lengths size every run's grid
    HIPCHK(ctx, hipMemcpyAsync(off.data(), d_offsets, (n_seqs + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    unsigned long long *d_cnt = ((SmallLayout *)ctx->small.p)->load_cnt;
    ClassifyParams p;
    fill_params(ctx, p);
    p.offsets = d_offsets; p.n_units = n_seqs; p.nmates = 1;
    const u64 chunk_k = count_chunk(ctx->c);
    const u64 max_blocks = (u64)ctx->n_cu * 8;
    s->failed = true;                                            // until the batch is in: a call that returns early has counted a part of it
    HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 32, st));
    u64 launches = 0, genomes = 0;
    for (u64 r0 = 0; r0 < n_seqs;) {
        u64 r1 = r0 + 1, chunks = 0;
        while (r1 < n_seqs && h_genome[r1] == h_genome[r0]) ++r1;
        for (u64 r = r0; r < r1; ++r) {
            const u64 L = off[r + 1] - off[r];
            if (L >= ctx->c) chunks += (L - ctx->c + 1 + chunk_k - 1) / chunk_k;
        }
        if (r0 || !(s->g_any && h_genome[0] == s->g_last)) ++genomes;   // (the first run may go on with the previous call's genome)
        if (chunks) {
            const unsigned grid = (unsigned)std::min<u64>(max_blocks, (chunks + 3) / 4);
            const u32 id1 = h_genome[r0] + 1u;
            if (ctx->spaced) hipLaunchKernelGGL((count_kernel<true>), dim3(grid), dim3(256), 0, st, p, r0, r1, id1, count_fkeys(s), count_fnb(s), s->g_count, s->g_stamp, d_cnt);
            else             hipLaunchKernelGGL((count_kernel<false>), dim3(grid), dim3(256), 0, st, p, r0, r1, id1, count_fkeys(s), count_fnb(s), s->g_count, s->g_stamp, d_cnt);
            HIPCHK(ctx, hipGetLastError());
        }
        ++launches;                                              // (a run of sequences all shorter than the comb has nothing to launch, and is a run)
        r0 = r1;
    }
    unsigned long long h_cnt[4] = {0, 0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(h_cnt, d_cnt, 32, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));                       // the caller may free or overwrite the batch once the call is back
    s->g_lookups += h_cnt[0];
    if (h_cnt[1] > s->g_largest) s->g_largest = h_cnt[1];
    if (h_cnt[3]) return fail(ctx, BNS_ERR_TABLE, "bns_build_count_add: a sequence of this batch was not part of the scored build (a k-mer of it is not in the table of all k-mers)");
    s->failed = false;
    s->g_any = true; s->g_last = h_genome[n_seqs - 1];
    s->g_launches += launches; s->g_genomes += genomes;
    ++s->g_batches;
    s->s_count += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_add).count();
    return BNS_OK;
}

int count_get(bns_ctx *ctx, const u64 *h_keys, u64 n, u32 *h_counts)
{
    BuildSession *s;
    int rc = build_session(ctx, &s, "bns_build_count_get");
    if (rc != BNS_OK) return rc;
    if (!s->counting) return fail(ctx, BNS_ERR_STATE, "bns_build_count_get before bns_build_count_begin");
    if (s->finished && !s->minimizing) return fail(ctx, BNS_ERR_STATE, "bns_build_count_get after bns_build_finish compacted the table the counts belong to");
    if (n == 0) return BNS_OK;
    if (!h_keys || !h_counts) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    u64 *dq = nullptr; u32 *dout = nullptr;
    if (hipMalloc((void **)&dq, (size_t)n * 8) != hipSuccess || hipMalloc((void **)&dout, (size_t)n * 4) != hipSuccess) {
        (void)hipGetLastError();
        if (dq) (void)hipFree(dq);
        return fail(ctx, BNS_ERR_NOMEM, "bns_build_count_get: no device memory for " + std::to_string(n) + " keys");
    }
    hipError_t e = hipMemcpyAsync(dq, h_keys, (size_t)n * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(count_get_kernel, dim3(grid_for(ctx, n, 256)), dim3(256), 0, st, (const u64 *)dq, n, count_fkeys(s), count_fnb(s), (const u32 *)s->g_count, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_counts, dout, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(dq); (void)hipFree(dout);
    if (e != hipSuccess) { ctx->err = std::string("bns_build_count_get: ") + hipGetErrorString(e); return BNS_ERR_HIP; }
    return BNS_OK;
}

int count_stats(const bns_ctx *ctx, u64 *out6)
{
    if (!ctx || !out6) return BNS_ERR_ARG;
    const BuildSession *s = ctx->build;
    if (!s || !s->counting) return BNS_ERR_STATE;
    out6[0] = s->g_batches; out6[1] = s->g_launches; out6[2] = s->g_genomes; out6[3] = s->g_lookups; out6[4] = s->g_largest;
    out6[5] = (u64)(s->s_count * 1e6);
    return BNS_OK;
}

}  // namespace
