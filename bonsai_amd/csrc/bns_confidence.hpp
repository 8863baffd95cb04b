// bns_confidence.hpp -- the confidence threshold behind bns_set_confidence / `bonsai classify -t` (gfx950, wave64).
//
//   confidence_kernel   per unit, after classify (and its overflow kernel), before unpack: T = the resolved taxon, H = the unit's ordered
//                       hit stream, Q = |H| + missing, R = ceil(num * Q / den) exactly.  T becomes the first of T, parent(T), ... whose
//                       clade (hits h == A or inside A's Euler interval) holds >= R hits; 0 when the walk passes a root first.  T stays
//                       when R = 0 or T is not a node whose chain reaches a root (tally_bin's bin n, 0xFFFFFFFF included).
//
// One wavefront per group of CONF_GROUP units: the records, R and T's node are read lane-parallel (one unit per lane), units that need
// no hits (T stays, or |H| < R: the result is 0) are settled there.  The others run one after another over the whole wavefront: each
// hit's node is read once (its tin kept in registers for the first CONF_CACHED x 64 hits), and every step of the walk is one node load
// plus a compare and a ballot per 64 hits.  The answer is T itself for nearly every unit, so the walk rarely takes a step.
// No reference counterpart: Kraken 2's --confidence (its ResolveTree loop), restated as defined behaviour in DESIGN.md.
#pragma once
#include "bns_device.hpp"

namespace bns {

constexpr u32 CONF_GROUP = 16;        // units per wavefront
constexpr u32 CONF_CACHED = 4;        // blocks of 64 hits whose tin stays in registers across the steps of a walk

// ceil(num * q / den) without overflow (num <= den, so the result is <= q)
__device__ __forceinline__ u64 conf_required(u64 num, u64 den, u64 q)
{
    if ((num >> 31) == 0 && (q >> 32) == 0) {
        const u64 p = num * q;
        return p / den + (p % den != 0 ? 1u : 0u);
    }
    u64 rem = __umul64hi(num, q), lo = num * q, quo = 0;         // rem < den: the quotient fits in 64 bits
    for (int b = 63; b >= 0; --b) {
        const bool top = (rem >> 63) != 0;
        rem = (rem << 1) | ((lo >> b) & 1u);
        quo <<= 1;
        if (top || rem >= den) { rem -= den; quo |= 1u; }
    }
    return quo + (rem != 0 ? 1u : 0u);
}

// A's clade holds hit h: h == A, or h lies in A's subtree.  tin_a >= 1 for A on a chain that reaches a root; a hit that is no node of
// the forest has tin 0, so the one test covers both.
__device__ __forceinline__ bool conf_in_clade(u32 tin_h, u32 tin_a, u32 tout_a) { return tin_a <= tin_h && tin_h < tout_a; }

// records[u].x rewritten in place for u < n_units; hits of unit u: hits[offsets[u * nmates]], records[u].w of them (hit_runs_kernel's
// indexing).  num > 0, num <= den (the launch site only launches it then).
__global__ __launch_bounds__(256) void confidence_kernel(uint4 *__restrict__ records, const u64 *__restrict__ offsets, u32 nmates,
                                                         const u32 *__restrict__ hits, u64 n_units, const TaxNode *__restrict__ nodes, u32 n_nodes,
                                                         u64 num, u64 den)
{
    const u32 lane = (u32)lane_id();
    const u64 n_waves = (u64)gridDim.x * 4;
    const u64 n_groups = (n_units + CONF_GROUP - 1) / CONF_GROUP;
    for (u64 g = (u64)blockIdx.x * 4 + (threadIdx.x >> 6); g < n_groups; g += n_waves) {
        const u64 u0 = g * CONF_GROUP;
        const u32 nu = (u32)(n_units - u0 < CONF_GROUP ? n_units - u0 : CONF_GROUP);
        // lane j < nu: unit u0 + j
        u32 taxon = 0, n_hits = 0, tin = 0, tout = 0, parent = 0;
        u64 R = 0, hb = 0;
        bool walk = false;
        if (lane < nu) {
            const uint4 rec = records[u0 + lane];
            taxon = rec.x; n_hits = rec.w;
            R = conf_required(num, den, (u64)rec.y + rec.w);
            if (R && taxon) {
                const TaxNode nt = load_node(nodes, n_nodes, taxon);
                if (nt.flags & NODE_CHAIN_OK) {
                    if ((u64)n_hits < R) records[u0 + lane].x = 0u;          // no clade can hold more hits than there are
                    else { walk = true; tin = nt.tin; tout = nt.tout; parent = nt.parent; hb = offsets[(u0 + lane) * nmates]; }
                }
            }
        }
        u64 todo = __ballot(walk);
        while (todo) {                                               // (wave-uniform)
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const u32 *h = hits + readlane64(hb, j);
            const u32 nh = readlane(n_hits, j);
            const u64 need = readlane64(R, j);
            u32 a = readlane(taxon, j), tin_a = readlane(tin, j), tout_a = readlane(tout, j), par_a = readlane(parent, j);
            u32 ct[CONF_CACHED];
#pragma unroll
            for (u32 c = 0; c < CONF_CACHED; ++c) {
                const u32 i = c * 64u + lane;
                ct[c] = i < nh ? load_node(nodes, n_nodes, h[i]).tin : 0u;
            }
            u32 result = 0;
            for (u32 step = 0; step < n_nodes; ++step) {             // (a chain that reaches a root is shorter than the taxonomy)
                u64 cnt = 0;
#pragma unroll
                for (u32 c = 0; c < CONF_CACHED; ++c) cnt += (u64)__popcll(__ballot(conf_in_clade(ct[c], tin_a, tout_a)));
                for (u32 i0 = CONF_CACHED * 64u; i0 < nh && cnt < need; i0 += 64u) {
                    const u32 i = i0 + lane;
                    const u32 t = i < nh ? load_node(nodes, n_nodes, h[i]).tin : 0u;
                    cnt += (u64)__popcll(__ballot(conf_in_clade(t, tin_a, tout_a)));
                }
                if (cnt >= need) { result = a; break; }
                if (par_a == 0u) break;                              // passed the root: unclassified
                const TaxNode np = load_node(nodes, n_nodes, par_a);
                a = par_a; tin_a = np.tin; tout_a = np.tout; par_a = np.parent;
            }
            if (lane == 0) records[u0 + (u32)j].x = result;
        }
    }
}

}  // namespace bns
