"""The table loads whose plan tests/golden/table_plan_parent.json pins: what a load of the golden db decides (bucket count,
minimizer, identity, window, fill) for every combination of layout, resident / streamed arrays, the three request setters, the
fill debug bits and a contiguous or spaced encoder.  One list for tools/make_table_plan_golden.py, which wrote the file from the
loader as it was before the plan moved into csrc/bns_table_plan.hpp, and for the GPU test that holds today's loader against it."""
import itertools

import bonsai_amd
from classify_forms import SPACED_GAPS

DBG_GROUP_FILL, DBG_PLAIN_FILL, DBG_SPACED_NOCLUSTER = 0x20, 0x10, 0x200
DBG_STREAMED = 0x1000 | (11 << 16)                       # BNS_DBG_STREAM_LOAD, chunks of 2^11 slots
FIELDS = ("buckets", "m", "identity_bits", "span", "group_fill", "n_keys", "main_bytes")
# spilled_keys / overflow_keys are left out: the arrival-order fill places keys in the order its atomics land

LAYOUTS = (bonsai_amd.LAYOUT_BUCKET, bonsai_amd.LAYOUT_MINBUCKET)
ENCODERS = ("contiguous", "spaced", "spaced_nocluster")


def groups():
    """(layout, streamed, encoder): one context serves the 36 cases of a group"""
    return list(itertools.product(LAYOUTS, (False, True), ENCODERS))


def group_cases():
    """(buckets, span, identity, fill bits) of a group's cases"""
    return list(itertools.product((0, 2000, 30011), (0, 15), (0, 52), (0, DBG_GROUP_FILL, DBG_PLAIN_FILL)))


def case_id(layout, streamed, enc, buckets, span, identity, fill):
    return "layout=%d,streamed=%d,enc=%s,buckets=%d,span=%d,identity=%d,dbg_fill=0x%x" % (layout, int(streamed), enc, buckets, span, identity, fill)


def load_group(CL, layout, streamed, enc):
    """-> {case id: {field: value}} of one group, every case a fresh bns_load_table on one context"""
    out = {}
    ctx = bonsai_amd.Context(0)
    try:
        k = int(CL["k"])
        ctx.set_encoder(k, None if enc == "contiguous" else list(SPACED_GAPS), canonicalize=True)
        for buckets, span, identity, fill in group_cases():
            ctx.debug_set(fill | (DBG_STREAMED if streamed else 0) | (DBG_SPACED_NOCLUSTER if enc == "spaced_nocluster" else 0))
            ctx.set_table_buckets(buckets)
            ctx.set_minimizer_span(span)
            ctx.set_minimizer_identity(identity)
            ctx.load_table(int(CL["db_hdr"][0]), CL["db_flags"], CL["db_keys_arr"], CL["db_vals_arr"], layout=layout)
            got = dict(ctx.table_geometry())
            got.update(ctx.table_stats())
            out[case_id(layout, streamed, enc, buckets, span, identity, fill)] = {f: int(got[f]) for f in FIELDS}
    finally:
        ctx.close()
    return out
