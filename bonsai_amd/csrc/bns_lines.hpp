// bns_lines.hpp -- Kraken output lines assembled on the device for bns_classify_text (gfx950, wave64).  Included by bns_ingest.hip behind
// its scan helpers (block_excl_scan, lookback, shfl_xor64: one scan idiom for the whole text path).
//
// Replaces: append_kraken_classification (classifier.h:112-129) with append_taxa_runs / append_counts (classifier.h:45-70) and the
// kt_for fan-out that formats a chunk (classifier.h:269-287), for units whose name, length, result and hit runs are in HBM already:
//
//     ('C' | 'U') '\t' name '\t' dec(taxon) '\t' dec(l_seq) '\t' [ "M:" dec(missing) '\t' ] [ "A:" dec(ambig) '\t' ]
//     taxon == 0: "0:0\n"      else: per run ( 'U' | 'A' | dec(tax) ) ':' dec(len) '\t', the last '\t' a '\n'
//
// name and l_seq are the first mate's; a unit is printed when emit_all or taxon != 0 (classifier.h:239), others take no bytes.
//
//   lines_len_kernel    a unit per thread, blocks numbered by a ticket: the length of every unit's line (its runs summed by its own lane
//                       when they are few, by the whole wavefront -- lanes striding over the runs, a wave reduction -- when they are
//                       many), then the exclusive prefix over the batch (block scan + decoupled look-back) -> line_off[u], and the
//                       batch's bytes added to the cursor by one lane
//   lines_write_kernel  one wavefront per group of LINES_GROUP consecutive units, whose lines are one contiguous stretch of the output:
//                       tokens are made lane-parallel (the four fixed fields and the first 60 runs in one pass, 64 runs a pass after
//                       that; a wave prefix of the token widths places them), staged in an LDS tile of the wavefront's and stored as
//                       aligned dwords; only the bytes that share a dword with a neighbouring group go out as bytes
#pragma once

namespace bns {
namespace ingest {

constexpr u32 LINES_GROUP = 16;                 // units per wavefront of lines_write_kernel (hit_runs_kernel's group)
constexpr u32 LINES_OWN_RUNS = 16;              // lines_len_kernel: up to this many runs a lane sums alone
constexpr u32 LINES_TILE = 3072;                // bytes of LDS per wavefront (12 KiB per block: no bound on occupancy at 8 blocks per CU)
constexpr u32 LINES_TOKEN = 22;                 // dec(u32) ':' dec(u32) and a separator
constexpr u32 LINES_STEP = 64u * LINES_TOKEN;   // the most one pass appends to the tile
constexpr u32 LINES_NAME_STEP = 1024;
constexpr u32 LINES_FIXED = 4;                  // lanes of the first pass that hold the fixed fields: taxon, l_seq, M:, A:
static_assert(LINES_STEP + 4 <= LINES_TILE && LINES_NAME_STEP + 4 <= LINES_TILE, "a pass must fit behind what a flush leaves");

struct LinesArgs {
    const u32 *taxon, *missing, *ambig;         // per unit
    const u32 *seq_len, *name_off;              // per record of the batch (name_off: n + 1 entries, offsets of the call)
    const char *names; u32 name_base;           // names + (name_off[R] - name_base)
    const u64 *run_start; const u32 *n_runs, *run_tax, *run_len;     // run_tax[run_start[u] + i]
    u64 n_units; u32 nmates, emit_all;
    u64 *line_off;                              // n_units + 1: where unit u's line starts among the call's lines
    u64 base;                                   // bytes of the batches in front
    u64 *state; u32 *ticket;                    // look-back words (one per 256 units) and the ticket counter, zeroed in front of the launch
    unsigned long long *cursor;                 // += the batch's bytes
    char *lines; u64 cap;                       // lines_write_kernel: the batch's bytes (offset line_off[u] - base), room in bytes
};

__device__ __forceinline__ u32 dec_width(u32 x)
{
    return 1u + (x >= 10u) + (x >= 100u) + (x >= 1000u) + (x >= 10000u) + (x >= 100000u) + (x >= 1000000u) + (x >= 10000000u) +
           (x >= 100000000u) + (x >= 1000000000u);
}
__device__ __forceinline__ u32 run_width(u32 tax, u32 len) { return ((tax == 0u || tax == 0xFFFFFFFFu) ? 1u : dec_width(tax)) + 2u + dec_width(len); }
__device__ __forceinline__ u32 count_width(u32 c) { return c ? 3u + dec_width(c) : 0u; }
__device__ __forceinline__ bool line_printed(u32 taxon, u32 emit_all) { return emit_all || taxon != 0u; }

__global__ __launch_bounds__(256) void lines_len_kernel(LinesArgs a)
{
    __shared__ u32 s_b;
    __shared__ u64 s_pre, lds4[4];
    const u32 lane = threadIdx.x & 63u;
    const u64 n = a.n_units;
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) s_b = atomicAdd(a.ticket, 1u);
        __syncthreads();
        const u32 b = s_b;
        if ((u64)b * 256u >= n) return;
        const u64 u = (u64)b * 256u + threadIdx.x;
        u64 len = 0, rs = 0;
        u32 nr = 0;
        if (u < n) {
            const u32 t = a.taxon[u];
            if (line_printed(t, a.emit_all)) {
                const u64 R = u * a.nmates;
                len = 2u + (a.name_off[R + 1] - a.name_off[R]) + 1u + dec_width(t) + 1u + dec_width(a.seq_len[R]) + 1u +
                      count_width(a.missing[u]) + count_width(a.ambig[u]);
                if (!t) len += 4u;
                else { nr = a.n_runs[u]; rs = a.run_start[u]; }
            }
        }
        if (nr <= LINES_OWN_RUNS) for (u32 i = 0; i < nr; ++i) len += run_width(a.run_tax[rs + i], a.run_len[rs + i]);
        // units with many runs (long reads: thousands), one after the other by the whole wavefront
        for (u64 big = __ballot(nr > LINES_OWN_RUNS); big; big &= big - 1) {
            const int j = __builtin_ctzll(big);
            const u32 nj = (u32)__shfl((int)nr, j);
            const u64 rj = ((u64)(u32)__shfl((int)(rs >> 32), j) << 32) | (u32)__shfl((int)(u32)rs, j);
            u64 sum = 0;
            for (u32 i = lane; i < nj; i += 64u) sum += run_width(a.run_tax[rj + i], a.run_len[rj + i]);
#pragma unroll
            for (int off = 32; off; off >>= 1) sum += shfl_xor64(sum, off);
            if ((int)lane == j) len += sum;
        }
        u64 total;
        const u64 ex = block_excl_scan(len, total, lds4);
        const u64 pre = lookback(a.state, b, total, &s_pre) + ex;
        if (u < n) a.line_off[u] = a.base + pre;
        if (u == n - 1) a.line_off[n] = a.base + pre + len;
        if (threadIdx.x == 0 && total) atomicAdd(a.cursor, (unsigned long long)total);
    }
}

// what the lanes of one wavefront have written to its tile is read by other lanes of it
__device__ __forceinline__ void lines_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The wavefront's tile: byte i of it is byte gbase + i of the batch's lines (gbase a multiple of 4), `fill` bytes are there; the first
// `head` bytes (0-3, in front of the group's first line) are a neighbour's.  Whole dwords leave as dwords; the group's first dword when
// it is shared, and -- at the end of the group -- the bytes behind the last whole dword, leave byte by byte.  Nothing at or behind cap.
struct LinesTile { u32 fill, head; u64 gbase; };
__device__ __forceinline__ void lines_flush(u32 *tile, LinesTile &t, char *__restrict__ out, u64 cap, bool final, u32 lane)
{
    lines_wave_sync();
    const u32 ndw = t.fill >> 2, rem = t.fill & 3u;
    for (u32 k = lane; k < ndw; k += 64u) {
        const u32 v = tile[k];
        const u64 g = t.gbase + 4ull * k;
        if (g + 4u > cap) continue;
        if (k == 0 && t.head) { for (u32 i = t.head; i < 4u; ++i) out[g + i] = (char)(v >> (8u * i)); }
        else *reinterpret_cast<u32 *>(out + g) = v;
    }
    const u32 last = tile[ndw < LINES_TILE / 4u ? ndw : 0u];
    if (final) {
        if (lane == 0 && rem) {
            const u64 g = t.gbase + 4ull * ndw;
            for (u32 i = ndw ? 0u : t.head; i < rem; ++i) if (g + i < cap) out[g + i] = (char)(last >> (8u * i));
        }
        return;
    }
    lines_wave_sync();
    if (ndw) {
        if (lane == 0) tile[0] = last;
        t.gbase += 4ull * ndw; t.fill = rem; t.head = 0;
    }
    lines_wave_sync();
}
__device__ __forceinline__ void lines_reserve(u32 *tile, LinesTile &t, u32 bytes, char *__restrict__ out, u64 cap, u32 lane)
{
    if (t.fill + bytes > LINES_TILE) lines_flush(tile, t, out, cap, false, lane);
}

__device__ __forceinline__ u8 *put_dec(u8 *p, u32 x)
{
    const u32 w = dec_width(x);
    for (u32 i = w; i; --i) { p[i - 1u] = (u8)('0' + x % 10u); x /= 10u; }
    return p + w;
}

__global__ __launch_bounds__(256) void lines_write_kernel(LinesArgs a)
{
    __shared__ u32 s_tile[4][LINES_TILE / 4u];
    const u32 lane = threadIdx.x & 63u;
    u32 *tile = s_tile[threadIdx.x >> 6];
    u8 *tb = reinterpret_cast<u8 *>(tile);
    const u64 n_waves = (u64)gridDim.x * 4, n_groups = (a.n_units + LINES_GROUP - 1) / LINES_GROUP;
    for (u64 g = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups; g += n_waves) {
        const u64 u0 = g * LINES_GROUP;
        const u32 nu = (u32)(a.n_units - u0 < LINES_GROUP ? a.n_units - u0 : LINES_GROUP);
        const u64 gstart = a.line_off[u0] - a.base, gend = a.line_off[u0 + nu] - a.base;
        if (gend == gstart) continue;
        LinesTile t;
        t.gbase = gstart & ~3ull; t.head = (u32)(gstart & 3u); t.fill = t.head;
        for (u32 j = 0; j < nu; ++j) {
            const u64 u = u0 + j;
            const u32 taxon = a.taxon[u];
            if (!line_printed(taxon, a.emit_all)) continue;
            const u64 R = u * a.nmates;
            const u32 noff = a.name_off[R], nlen = a.name_off[R + 1] - noff;
            const char *__restrict__ name = a.names + (u32)(noff - a.name_base);
            // 'C' / 'U', the name
            lines_reserve(tile, t, 2u, a.lines, a.cap, lane);
            if (lane == 0) { tb[t.fill] = taxon ? 'C' : 'U'; tb[t.fill + 1u] = '\t'; }
            t.fill += 2u;
            for (u32 c0 = 0; c0 < nlen; c0 += LINES_NAME_STEP) {
                const u32 cn = nlen - c0 < LINES_NAME_STEP ? nlen - c0 : LINES_NAME_STEP;
                lines_reserve(tile, t, cn, a.lines, a.cap, lane);
                for (u32 i = lane; i < cn; i += 64u) tb[t.fill + i] = (u8)name[c0 + i];
                t.fill += cn;
            }
            lines_reserve(tile, t, 1u, a.lines, a.cap, lane);
            if (lane == 0) tb[t.fill] = '\t';
            t.fill += 1u;
            // tokens: '\t' taxon '\t' l_seq '\t' M: A: in the first lanes of the first pass, runs (or "0:0") behind them
            const u32 missing = a.missing[u], ambig = a.ambig[u], l_seq = a.seq_len[R];
            const u32 nr = taxon ? a.n_runs[u] : 0u;
            const u64 rs = taxon ? a.run_start[u] : 0ull;
            const u32 last_fixed = ambig ? 3u : (missing ? 2u : 1u);
            for (u32 r0 = 0, first = 1;; first = 0) {
                // lane's token: [chr | dec(x)] [':' dec(y)] sep
                bool on = false, has_y = false;
                u32 chr = 0, x = 0, y = 0, sep = '\t';
                const u32 fx = first ? LINES_FIXED : 0u;
                if (first && lane < LINES_FIXED) {
                    if (lane == 0) { on = true; x = taxon; }
                    else if (lane == 1) { on = true; x = l_seq; }
                    else if (lane == 2) { on = missing != 0; chr = 'M'; has_y = true; y = missing; }
                    else { on = ambig != 0; chr = 'A'; has_y = true; y = ambig; }
                    if (taxon && !nr && lane == last_fixed) sep = '\n';      // (no run to end the line: the last separator does, as w[-1] = '\n' would)
                } else if (!taxon) {
                    if (first && lane == LINES_FIXED) { on = true; has_y = true; sep = '\n'; }      // "0:0\n"
                } else {
                    const u32 r = r0 + lane - fx;
                    if (r < nr) {
                        on = true; has_y = true;
                        const u32 tx = a.run_tax[rs + r];
                        y = a.run_len[rs + r];
                        if (tx == 0u) chr = 'U'; else if (tx == 0xFFFFFFFFu) chr = 'A'; else x = tx;
                        if (r == nr - 1u) sep = '\n';
                    }
                }
                const u32 w = on ? (chr ? 1u : dec_width(x)) + (has_y ? 1u + dec_width(y) : 0u) + 1u : 0u;
                u32 incl = w;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) { const u32 v = (u32)__shfl_up((int)incl, off); if (lane >= (u32)off) incl += v; }
                const u32 step = (u32)__shfl((int)incl, 63);
                lines_reserve(tile, t, step, a.lines, a.cap, lane);
                if (on) {
                    u8 *p = tb + t.fill + (incl - w);
                    if (chr) *p++ = (u8)chr; else p = put_dec(p, x);
                    if (has_y) { *p++ = ':'; p = put_dec(p, y); }
                    *p = (u8)sep;
                }
                t.fill += step;
                r0 += 64u - fx;
                if (r0 >= nr) break;
            }
        }
        lines_flush(tile, t, a.lines, a.cap, true, lane);
        lines_wave_sync();                                       // (the next group's first bytes go where this flush still reads)
    }
}

}  // namespace ingest
}  // namespace bns
