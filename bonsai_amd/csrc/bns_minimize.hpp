// bns_minimize.hpp -- taxonomic-depth minimizers chosen on the device: bns_build_minimize_begin / _add / _stats (gfx950, wave64).
//
// A build session that has folded every k-mer of every sequence into its table (F: key -> LCA of all sequences that hold it) is
// frozen, and the same sequences are streamed once more.  Every position window of w bases selects, among its valid k-mers, the one
// whose LCA lies deepest in the taxonomy (then the smaller taxid, then the smaller k-mer: DESIGN.md, "Defined behaviour"); the
// selected k-mers go into a second table M with the value F holds for them.  From bns_build_minimize_begin on the session's table
// IS M: bns_build_finish / _export / _end and build_rehash act on it as they are.
//
//   depth_kernel            one lane per taxonomy id: the number of nodes on the chain id -> root, walked iteratively along parent
//                           (0 for an id whose chain does not reach a root: NODE_CHAIN_OK is what bns_load_taxonomy found out).
//   minimize_kernel<SPACED> work item = (sequence, chunk), one wavefront each, the chunk's 64 words held one per lane as in
//                           build_kernel.  Two phases over a chunk-wide image in LDS of (score, k-mer) per position:
//                             fill   64 positions a round: extract (extract_unspaced / extract_spaced[_runs], canonical), probe F
//                                    (wang64(key) & mask, triangular steps, until the key or BUILD_EMPTY), read vals[slot], read
//                                    depth[val]; score = (0xFFFFFFFF - depth) << 32 | val.  ONE lookup per position and chunk: the
//                                    gather into a table of all k-mers is a cache miss per position and what this kernel costs.
//                                    (SCORE 1, fewest-genome minimizers: count[slot] of bns_fewest.hpp in depth's place, score =
//                                    count << 32 | val; bns_build_minimize_begin_score.  The SCORE 0 form is the code as it was.)
//                             sweep  64 windows a round: the (score, k-mer) minimum of entries p .. p + ws - 1, read from LDS at
//                                    lane-consecutive addresses (no bank conflict), ws = w - c + 1 from 1 to 1024.
//                           An invalid position holds (~0, ~0), which no valid one does (~0 is no key a session accepts), so it never
//                           wins and a window of nothing but invalid positions selects nothing.  A lane whose minimizer is its
//                           left neighbour's skips it (DPP); the others claim a slot of M by CAS and store F's value with a plain
//                           store: whoever writes a key's value writes the same, so one pass suffices and a batch may be applied
//                           twice, or again after M grew.
// LDS.  31 rounds x 64 entries x 16 bytes = 31 KiB a wavefront, so a block is ONE wavefront and five of them share a CU's 160 KiB;
// with 64 probes in flight per wavefront that is 320 independent gathers a CU.  The windows of a chunk re-read ws - 1 positions of
// the next one: 19 of 1920 at k 31, w 50.
// A key that F does not hold raises cnt[3] (the host fails the call); the probe stops at the empty slot it met and reads nothing
// beyond the arrays.  cnt[0] keys newly inserted, cnt[1] "M is too small", cnt[2] positions looked up, cnt[3] "not in F".
//
// Included by bns_api.hip after bns_build.hpp, whose session, build_alloc_table and build_rehash the host half below uses.
#pragma once

namespace bns {

constexpr u32 MINZ_ROUNDS = 31;                       // rounds of 64 positions a chunk image holds (extract_* read words 2 rd .. 2 rd + 3)
constexpr u32 MINZ_ENTRIES = MINZ_ROUNDS * 64u;

// positions a chunk may hold for a comb of c bases: every k-mer of the image lies inside the chunk's 2048 bases
__host__ __device__ inline u32 minz_entries(u32 c) { return 2049u - c < MINZ_ENTRIES ? 2049u - c : MINZ_ENTRIES; }
// window starts per chunk, a multiple of 64 (ws = k-mers a window holds)
__host__ __device__ inline u32 minz_chunk(u32 c, u32 ws) { return (minz_entries(c) - (ws - 1u)) / 64u * 64u; }

__global__ __launch_bounds__(256) void depth_kernel(const TaxNode *__restrict__ nodes, u32 n, u32 *__restrict__ depth)
{
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 x = (u64)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += stride) {
        u32 d = 0;
        if (nodes[x].flags & NODE_CHAIN_OK) {
            u32 t = (u32)x;
            for (u32 step = 0; step < n; ++step) {               // (a chain that reaches a root is shorter than the taxonomy)
                ++d;
                const u32 pr = nodes[t].parent;
                if (pr == 0) break;
                if (pr >= n) { d = 0; break; }
                t = pr;
            }
        }
        depth[x] = d;
    }
}

// SCORE 0 (BNS_MINIMIZE_DEPTH): aux = depth[id], one word per taxonomy node.  SCORE 1 (BNS_MINIMIZE_FEWEST): aux = the genome counts of
// bns_fewest.hpp, one word per bucket of F.
template <bool SPACED, int SCORE>
__global__ __launch_bounds__(64) void minimize_kernel(ClassifyParams p, u32 w, const u64 *__restrict__ fkeys, const u32 *__restrict__ fvals,
                                                      u64 f_nb, const u32 *__restrict__ aux, u64 *__restrict__ mkeys,
                                                      u32 *__restrict__ mvals, u64 m_nb, unsigned long long *cnt)
{
    __shared__ u64 s_sc[MINZ_ENTRIES];
    __shared__ u64 s_el[MINZ_ENTRIES];
    const int lane = lane_id();
    const u32 rdesc = SPACED ? run_desc(p) : 0u;
    const u64 wave = blockIdx.x, n_waves = gridDim.x;
    const u32 k = p.k, c = p.c;
    const u32 ws = w - c + 1u;                                    // (the host hands in w >= c)
    const u64 chunk_k = minz_chunk(c, ws);
    const u64 fmask = f_nb - 1, mmask = m_nb - 1;
    const u64 mlimit = m_nb < BUILD_MAX_CHAIN ? m_nb : BUILD_MAX_CHAIN;
    u32 inserted = 0;
    u64 lookups = 0;
    bool missing = false;
    u64 before = 0;                                               // chunks of the sequences before r: chunk g belongs to wave g % n_waves
    for (u64 r = 0; r < p.n_units; ++r) {
        const u64 o = p.offsets[r];
        const u64 Lg = p.offsets[r + 1] - o;
        const u64 wb = (o >> 5) + r;
        const u64 n_words = (Lg + 31u) >> 5;
        const u64 nk = Lg >= w ? Lg - w + 1u : 0u;                // windows of the sequence
        const u64 n_chunks = (nk + chunk_k - 1) / chunk_k;
        const u64 first = (wave + n_waves - before % n_waves) % n_waves;
        before += n_chunks;
        for (u64 ch = first; ch < n_chunks; ch += n_waves) {
            if (__atomic_load_n(&cnt[1], __ATOMIC_RELAXED)) break;                 // M filled up: the host grows it and comes again
            const u64 j0 = ch * chunk_k;
            const u64 wi = (j0 >> 5) + (u64)lane;
            const u64 W = wi < n_words ? p.words[wb + wi] : 0ULL;
            const u32 M = wi < n_words ? p.nmask[wb + wi] : 0xFFFFFFFFu;
            const u32 n_win = (nk - j0) < chunk_k ? (u32)(nk - j0) : (u32)chunk_k;
            const u32 n_ent = n_win + ws - 1u;                    // <= minz_entries(c): the last one ends inside the sequence
            // ---- fill: one lookup per position
            for (u32 rd = 0; rd * 64u < n_ent; ++rd) {
                const u32 e = rd * 64u + (u32)lane;
                u64 kmer;
                bool valid;
                if (SPACED) valid = p.n_runs ? extract_spaced_runs(W, M, rd, p, rdesc, kmer) : extract_spaced(W, M, rd, k, rdesc, kmer);
                else        valid = extract_unspaced(W, M, rd, k, kmer);
                valid = valid && e < n_ent;
                if (!SPACED && p.canon) kmer = canonical(kmer, k);
                u64 score = ~0ULL;
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
                        const u32 v = fvals[i];
                        if (SCORE == 0) {
                            const u32 d = v < p.n_nodes ? aux[v] : 0u;
                            score = ((u64)(0xFFFFFFFFu - d) << 32) | v;
                        } else {
                            score = ((u64)aux[i] << 32) | v;     // FMencode(genomes that hold it, taxid): fewer genomes first
                        }
                    } else { missing = true; valid = false; }
                }
                lookups += (u64)__popcll(ballot64(valid));
                s_sc[e] = score;
                s_el[e] = valid ? kmer : ~0ULL;
            }
            __builtin_amdgcn_wave_barrier();
            // ---- sweep: the minimum of every window, repeats skipped, the rest into M
            for (u32 rd = 0; rd * 64u < n_win; ++rd) {
                const u32 pw = rd * 64u + (u32)lane;
                const bool on = pw < n_win;
                const u32 at = on ? pw : 0u;
                u64 bs = s_sc[at], be = s_el[at];
                for (u32 i = 1; i < ws; ++i) {
                    const u64 sc = s_sc[at + i], x = s_el[at + i];
                    const bool lt = sc < bs || (sc == bs && x < be);
                    bs = lt ? sc : bs; be = lt ? x : be;
                }
                const u64 prev = ((u64)dpp<DPP_WAVE_SHR1>((u32)(be >> 32)) << 32) | dpp<DPP_WAVE_SHR1>((u32)be);
                if (on && be != ~0ULL && (lane == 0 || prev != be)) {
                    u64 i = wang64(be) & mmask, step = 0;
                    for (;;) {
                        const u64 old = atomicCAS((unsigned long long *)&mkeys[i], (unsigned long long)BUILD_EMPTY, (unsigned long long)be);
                        if (old == BUILD_EMPTY) { ++inserted; mvals[i] = (u32)bs; break; }
                        if (old == be) break;
                        i = (i + (++step)) & mmask;
                        if (step >= mlimit) { atomicExch(&cnt[1], 1ULL); break; }
                        if ((step & 63u) == 0 && __atomic_load_n(&cnt[1], __ATOMIC_RELAXED)) break;
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();                      // (the next chunk's fill writes what this sweep read)
        }
    }
    for (int off = 32; off >= 1; off >>= 1) inserted += (u32)__shfl_xor((int)inserted, off);
    const bool any_missing = ballot64(missing) != 0ULL;
    if (lane == 0) {
        if (inserted) atomicAdd(&cnt[0], (unsigned long long)inserted);
        if (lookups) atomicAdd(&cnt[2], (unsigned long long)lookups);
        if (any_missing) atomicExch(&cnt[3], 1ULL);
    }
}

}  // namespace bns

namespace {

int minimize_begin(bns_ctx *ctx, u32 w, u64 hint, int score)
{
    BuildSession *s;
    int rc = build_session(ctx, &s, "bns_build_minimize_begin");
    if (rc != BNS_OK) return rc;
    if (score != BNS_MINIMIZE_DEPTH && score != BNS_MINIMIZE_FEWEST) return fail(ctx, BNS_ERR_ARG, "bns_build_minimize_begin_score: score must be BNS_MINIMIZE_DEPTH or BNS_MINIMIZE_FEWEST");
    if (s->finished) return fail(ctx, BNS_ERR_STATE, "bns_build_minimize_begin after bns_build_finish");
    if (s->minimizing) return fail(ctx, BNS_ERR_STATE, "bns_build_minimize_begin called twice");
    if (ctx->win > ctx->c) return fail(ctx, BNS_ERR_STATE, "bns_build_minimize_begin needs a session that scored every k-mer: bns_set_window is beyond the comb");
    if (score == BNS_MINIMIZE_FEWEST && !s->counting) return fail(ctx, BNS_ERR_STATE, "bns_build_minimize_begin_score: BNS_MINIMIZE_FEWEST needs the genome counts (bns_build_count_begin, bns_build_count_add)");
    if (w > ctx->c) {
        if (w > 1920u) return fail(ctx, BNS_ERR_ARG, "window of more than 1920 bases is not supported (a wavefront works on 2048-base chunks)");
        if (w - ctx->c + 1 > 1024u) return fail(ctx, BNS_ERR_ARG, "window of more than 1024 k-mers is not supported");
    }
    if (hint > (1ULL << 40)) return fail(ctx, BNS_ERR_TABLE, "n_buckets_hint beyond 2^40");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    u32 *depth = nullptr;
    if (score == BNS_MINIMIZE_DEPTH) {
        HIPCHK(ctx, hipMalloc((void **)&depth, (size_t)ctx->n_nodes * 4));
        hipLaunchKernelGGL(depth_kernel, dim3(grid_for(ctx, ctx->n_nodes, 256)), dim3(256), 0, st, (const TaxNode *)ctx->nodes, ctx->n_nodes, depth);
    }
    u64 nb = 4;
    while (nb < hint) nb <<= 1;
    u64 *mk; u32 *mv;
    if ((rc = build_alloc_table(ctx, nb, &mk, &mv, st)) != BNS_OK) { (void)hipStreamSynchronize(st); if (depth) (void)hipFree(depth); return rc; }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        if (depth) (void)hipFree(depth);
        (void)hipFree(mk); (void)hipFree(mv);
        ctx->err = std::string("bns_build_minimize_begin: ") + hipGetErrorString(e);
        return BNS_ERR_HIP;
    }
    s->f_keys = s->keys; s->f_vals = s->vals; s->f_nb = s->nb; s->f_n_keys = s->n_keys;
    s->keys = mk; s->vals = mv; s->nb = nb; s->n_keys = 0;
    s->depth = depth;
    s->min_score = score;
    s->min_w = w > ctx->c ? w : ctx->c;
    s->minimizing = true;
    return BNS_OK;
}

int minimize_add(bns_ctx *ctx, const char *d_bases, const u64 *d_offsets, u64 n_seqs, u64 total_bases, void *stream)
{
    BuildSession *s;
    int rc = build_session(ctx, &s, "bns_build_minimize_add");
    if (rc != BNS_OK) return rc;
    if (s->finished) return fail(ctx, BNS_ERR_STATE, "bns_build_minimize_add after bns_build_finish");
    if (!s->minimizing) return fail(ctx, BNS_ERR_STATE, "bns_build_minimize_add before bns_build_minimize_begin");
    if (n_seqs == 0) { ++s->m_batches; return BNS_OK; }
    if (!d_offsets) return BNS_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = stream ? (hipStream_t)stream : ctx->stream;
    if (st != ctx->stream) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = pack_reads_dust(ctx, d_bases, d_offsets, n_seqs, total_bases, st)) != BNS_OK) return rc;
    unsigned long long *d_cnt = ((SmallLayout *)ctx->small.p)->load_cnt;
    ClassifyParams p;
    fill_params(ctx, p);
    p.offsets = d_offsets; p.n_units = n_seqs; p.nmates = 1;
    const unsigned grid = (unsigned)ctx->n_cu * 5;                // one wavefront a block, 31 KiB of LDS each: five to a CU
    const auto t_add = std::chrono::steady_clock::now();
    s->failed = true;                                            // until the batch is in
    for (;;) {
        HIPCHK(ctx, hipMemsetAsync(d_cnt, 0, 32, st));
        const bool fewest = s->min_score == BNS_MINIMIZE_FEWEST;
        const u32 *aux = fewest ? s->g_count : s->depth;
        auto kern = ctx->spaced ? (fewest ? minimize_kernel<true, 1> : minimize_kernel<true, 0>)
                                : (fewest ? minimize_kernel<false, 1> : minimize_kernel<false, 0>);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64), 0, st, p, s->min_w, (const u64 *)s->f_keys, (const u32 *)s->f_vals, s->f_nb, aux, s->keys,
                           s->vals, s->nb, d_cnt);
        HIPCHK(ctx, hipGetLastError());
        unsigned long long h_cnt[4] = {0, 0, 0, 0};
        HIPCHK(ctx, hipMemcpyAsync(h_cnt, d_cnt, 32, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        s->n_keys += h_cnt[0];
        s->m_lookups += h_cnt[2];
        if (h_cnt[3]) return fail(ctx, BNS_ERR_TABLE, "bns_build_minimize_add: a sequence of this batch was not part of the scored build (a k-mer of it is not in the table of all k-mers)");
        if (!h_cnt[1] && s->n_keys <= build_upper(s->nb)) break;
        // M does not hold the batch: double it (a key that went in stays in, with its value) and apply the same batch again
        do {
            if (s->nb >= (1ULL << 40)) return fail(ctx, BNS_ERR_TABLE, "build session: table beyond 2^40 buckets");
            if ((rc = build_rehash(ctx, s, s->nb << 1, st)) != BNS_OK) return rc;
            ++s->m_grows;
        } while (s->n_keys > build_upper(s->nb));
    }
    s->failed = false;
    ++s->m_batches;
    s->s_min += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_add).count();
    return BNS_OK;
}

int minimize_stats(const bns_ctx *ctx, u64 *out6)
{
    if (!ctx || !out6) return BNS_ERR_ARG;
    const BuildSession *s = ctx->build;
    if (!s || !s->minimizing) return BNS_ERR_STATE;
    out6[0] = s->m_batches; out6[1] = s->m_grows; out6[2] = s->f_n_keys; out6[3] = s->n_keys; out6[4] = s->m_lookups;
    out6[5] = (u64)(s->s_min * 1e6);
    return BNS_OK;
}

}  // namespace
