// bns_inspect.hpp -- the per-taxon key counts of the loaded table behind bns_table_tally (gfx950, wave64).
//
// One streaming walk per layout; every present key is counted exactly once, its value t going to tally_bin(t):
//   inspect_khash_kernel   one lane per khash slot: the slot's flag pair (0 = present; empty and deleted slots do not count) and vals[]
//   inspect_slots_kernel   one lane per 16-byte Slot of a bucket table (BUCKET; the overflow table of MINBUCKET): occ decides, never
//                          the key (key 0 is a legal key)
//   inspect_minb_kernel    one quad per 128-byte bucket, home and spill-only buckets alike: the lanes fetch the four 16-byte pieces of
//                          the line's UPPER half (keys[8..9] | vals[0..3] | vals[4..7] | vals[8..9], header, S) -- the walk needs
//                          vals[] and the header word only.  Occupancy is the header's bits 8-17, never the key (unused slots hold
//                          ~0, which an uncanonical k = 32 db may hold as a key).  A bucket whose count byte is MINB_N_IN_OVF has
//                          had its keys moved to the overflow table by minbucket_place_kernel, which cleared keys[] and vals[] and
//                          left the occupancy bits 0 (it sets them only where it found a multiplier): the walk by occupancy counts
//                          nothing there, and inspect_slots_kernel counts those keys in the overflow table -- once.
// Combining: a lane first merges equal values among its own (a bucket holds runs of equal values on a db of window minimizers);
// one vote per value slot then takes the wavefront's first lane's bin out with ONE LDS add for all lanes that hold it (an LCA-heavy
// db puts a large share of its keys on a few high nodes; tally_kernel's full match loop would take one round per distinct bin,
// and table values are as varied as the db); the rest go to the workgroup's LDS hash of bns_tally.hpp one by one.  The LDS counters
// are 32-bit: a workgroup flushes to the 64-bit HBM counters after flush_rounds <= INSPECT_FLUSH_ROUNDS rounds of at most 16 keys per lane.
//
// No reference counterpart: the reference never asks what its map holds per taxon.
#pragma once
#include "bns_tally.hpp"

namespace bns {

constexpr u32 INSPECT_MINB_UNROLL = 4;                  // buckets a quad of the clustered walk has in flight
// rounds of a workgroup between two flushes of its LDS counters (the kernels' flush_rounds argument; at most this): x TALLY_BLOCK lanes
// x 4 keys x 4 buckets = 2^30 keys.  No table that fits in HBM makes a workgroup of a full grid run that many rounds (2048 workgroups
// would need 2^39 buckets), so the host passes a small number under BNS_DBG_INSPECT_TINY, where tests run the mid-walk flush.
constexpr u32 INSPECT_FLUSH_ROUNDS = 1u << 18;
static_assert((u64)INSPECT_FLUSH_ROUNDS * TALLY_BLOCK * 4u * INSPECT_MINB_UNROLL < (1ULL << 32), "a workgroup's LDS counters are u32");

struct InspectLds {
    u32 key[TALLY_SLOTS];
    u32 cnt[TALLY_SLOTS];
};

__device__ __forceinline__ void inspect_lds_clear(InspectLds &s)
{
    for (u32 i = threadIdx.x; i < TALLY_SLOTS; i += TALLY_BLOCK) { s.key[i] = TALLY_EMPTY; s.cnt[i] = 0u; }
    __syncthreads();
}

// every lane of the workgroup comes here together; the hash is empty again afterwards
__device__ __forceinline__ void inspect_lds_flush(InspectLds &s, unsigned long long *__restrict__ direct)
{
    __syncthreads();
    for (u32 i = threadIdx.x; i < TALLY_SLOTS; i += TALLY_BLOCK) {
        const u32 k = s.key[i];
        if (k != TALLY_EMPTY) atomicAdd(&direct[k], (unsigned long long)s.cnt[i]);
        s.key[i] = TALLY_EMPTY; s.cnt[i] = 0u;
    }
    __syncthreads();
}

// tally_bin with the node's flags word already in a register (nodes[t].flags for 0 < t < n, anything otherwise): the same three cases
__device__ __forceinline__ u32 tally_bin_loaded(u32 n, u32 t, u32 flags)
{
    return t == 0u ? 0u : (t < n && (flags & NODE_CHAIN_OK)) ? t : n;
}

// c keys of bin `bin` (c == 0: this lane has none); every lane of the wavefront runs this together.  The bins come in computed: a
// tally_bin() is a gather from the node array, and a walk that waited for one per add would run at the latency of those, not at the
// table's bandwidth -- the callers issue theirs together, before the first add.
__device__ __forceinline__ void inspect_add(InspectLds &s, u32 bin, u32 c, unsigned long long *__restrict__ direct)
{
    const u64 have = __ballot(c != 0u);
    if (!have) return;
    const int leader = __ffsll((long long)have) - 1;
    const u32 b0 = (u32)__shfl((int)bin, leader);
    const bool same = c != 0u && bin == b0;
    u32 sum = same ? c : 0u;                                                  // the leader's bin: one add for the whole wavefront
    for (int off = 32; off >= 1; off >>= 1) sum += (u32)__shfl_xor((int)sum, off);
    const bool lead = lane_id() == leader;
    const u32 add = lead ? sum : same ? 0u : c;                               // (one call site: the probe loop is inlined and unrolled)
    if (add) tally_lds_add(s.key, s.cnt, lead ? b0 : bin, add, direct, 0);
}

__global__ __launch_bounds__(TALLY_BLOCK) void inspect_khash_kernel(const u32 *__restrict__ flags, const u32 *__restrict__ vals, u64 n_buckets,
                                                                    const TaxNode *__restrict__ nodes, u32 n,
                                                                    unsigned long long *__restrict__ direct, u32 flush_rounds)
{
    __shared__ InspectLds s;
    inspect_lds_clear(s);
    const u64 stride = (u64)gridDim.x * TALLY_BLOCK;
    u32 rounds = 0;
    for (u64 base = (u64)blockIdx.x * TALLY_BLOCK; base < n_buckets; base += stride) {      // (uniform: every lane runs every round)
        const u64 i = base + threadIdx.x;
        const bool present = i < n_buckets && ((flags[i >> 4] >> ((i & 0xfu) << 1)) & 3u) == 0u;
        const u32 bin = present ? tally_bin(nodes, n, vals[i]) : TALLY_EMPTY;
        inspect_add(s, bin, present ? 1u : 0u, direct);
        if (++rounds == flush_rounds) { inspect_lds_flush(s, direct); rounds = 0; }
    }
    inspect_lds_flush(s, direct);
}

__global__ __launch_bounds__(TALLY_BLOCK) void inspect_slots_kernel(const Slot *__restrict__ slots, u64 n_slots, const TaxNode *__restrict__ nodes, u32 n,
                                                                    unsigned long long *__restrict__ direct, u32 flush_rounds)
{
    __shared__ InspectLds s;
    inspect_lds_clear(s);
    const u64 stride = (u64)gridDim.x * TALLY_BLOCK;
    u32 rounds = 0;
    for (u64 base = (u64)blockIdx.x * TALLY_BLOCK; base < n_slots; base += stride) {
        const u64 i = base + threadIdx.x;
        uint2 vo = make_uint2(0u, 0u);                                       // {val, occ}
        if (i < n_slots) vo = *reinterpret_cast<const uint2 *>(reinterpret_cast<const char *>(slots + i) + 8);
        inspect_add(s, vo.y ? tally_bin(nodes, n, vo.x) : TALLY_EMPTY, vo.y ? 1u : 0u, direct);
        if (++rounds == flush_rounds) { inspect_lds_flush(s, direct); rounds = 0; }
    }
    inspect_lds_flush(s, direct);
}

// WHOLE: the quad's lanes fetch the line's lower half as well (the A/B of "upper 64 bytes against whole lines"; same counts).
// A round is INSPECT_MINB_UNROLL buckets per quad, their loads issued together: most buckets of a table at its default load are empty
// and cost one ballot each, so what a wavefront has in flight decides how fast the table streams.
template <bool WHOLE>
__global__ __launch_bounds__(TALLY_BLOCK) void inspect_minb_kernel(const MinBucket *__restrict__ mb, u64 n_bucket, const TaxNode *__restrict__ nodes, u32 n,
                                                                   unsigned long long *__restrict__ direct, u32 flush_rounds)
{
    __shared__ InspectLds s;
    inspect_lds_clear(s);
    constexpr u32 U = INSPECT_MINB_UNROLL, PER = TALLY_BLOCK / 4;            // PER buckets per workgroup and load, U loads per round
    const u64 stride = (u64)gridDim.x * PER * U;
    const u32 q = threadIdx.x & 3u;
    const int lane = lane_id();
    u32 rounds = 0;
    for (u64 base = (u64)blockIdx.x * PER * U; base < n_bucket; base += stride) {           // (uniform: every lane runs every round)
        uint4 v[U];
        u32 keep = 0u;
#pragma unroll
        for (u32 u = 0; u < U; ++u) {
            const u64 b = base + u * PER + (threadIdx.x >> 2);
            v[u] = make_uint4(0u, 0u, 0u, 0u);                               // (past the end: header 0, nothing occupied)
            if (b < n_bucket) {
                const uint4 *line = reinterpret_cast<const uint4 *>(mb + b);
                v[u] = line[4 + q];
                if (WHOLE) { const uint4 lo = line[q]; keep ^= lo.x ^ lo.y ^ lo.z ^ lo.w; }
            }
        }
        if (WHOLE) asm volatile("" ::"v"(keep));                             // (the lower half is fetched, not used)
        u32 bin[U][4], c[U][4], nf[U][4];
#pragma unroll
        for (u32 u = 0; u < U; ++u) {
            const u32 hdr = (u32)__shfl((int)v[u].z, lane | 3);              // header word: third dword of the quad's last piece
            const u32 occ = (hdr >> 8) & 0x3FFu;
            // this lane's slots: q = 1: 0-3, q = 2: 4-7, q = 3: 8-9 (its z, w are the header and S), q = 0: none (keys[8..9])
            const u32 mine = q == 0u ? 0u : q == 3u ? ((occ >> 8) & 3u) : ((occ >> ((q - 1u) * 4u)) & 0xFu);
            const u32 t[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int j = 0; j < 4; ++j) c[u][j] = (mine >> j) & 1u;
#pragma unroll
            for (int j = 0; j < 4; ++j)                                      // equal values of one lane: counted at the first of them
#pragma unroll
                for (int i = j + 1; i < 4; ++i)
                    if (c[u][j] && c[u][i] && t[i] == t[j]) { c[u][j] += c[u][i]; c[u][i] = 0u; }
#pragma unroll
            for (int j = 0; j < 4; ++j) {                                    // (the round's gathers, issued together: no branch around them)
                bin[u][j] = t[j];
                nf[u][j] = nodes[(c[u][j] && t[j] < n) ? t[j] : 0u].flags;   // (node 0 exists: n >= 2)
            }
        }
#pragma unroll
        for (u32 u = 0; u < U; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) bin[u][j] = c[u][j] ? tally_bin_loaded(n, bin[u][j], nf[u][j]) : TALLY_EMPTY;
#pragma unroll
        for (u32 u = 0; u < U; ++u) {
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {                                    // (rolled, the operands by selects: one copy of inspect_add per bucket)
                const u32 bj = j == 0 ? bin[u][0] : j == 1 ? bin[u][1] : j == 2 ? bin[u][2] : bin[u][3];
                const u32 cj = j == 0 ? c[u][0] : j == 1 ? c[u][1] : j == 2 ? c[u][2] : c[u][3];
                inspect_add(s, bj, cj, direct);
            }
        }
        if (++rounds == flush_rounds) { inspect_lds_flush(s, direct); rounds = 0; }
    }
    inspect_lds_flush(s, direct);
}

}  // namespace bns
