"""Every compiled form of classify_kernel and classify_overflow_kernel against the oracle, with proof that it ran.

The matrix is classify_forms.cases(): one case per form and mate count (tests/test_classify_forms_built.py holds that set
against the built library).  A case loads its table the way its form needs -- the window and the minimizer identity asked for,
the cooperative overflow lookup forced over a crowded table with real keys in its overflow table --, classifies the read set
of classify_forms.read_set() through the ASCII or the packed entry point, and compares taxon, missing, ambig, n_hits and the
ordered hit stream of EVERY unit with the oracle.  Then it asks the library which kernel it launched
(Context.last_classify_form()) and holds that against the restated dispatch rule: a dispatch that drifts to a generic kernel
keeps every parity assertion green and fails here.  Last, the case must have reached what it is for: most units classified,
hits, missing and ambiguous k-mers all present, a strict window minimum at every window position and every carried ring entry
(the host restatement in classify_forms), units in the overflow kernel where that is the form under test."""
import numpy as np
import pytest

import classify_forms as F
import synth

pytestmark = pytest.mark.gpu

_EXPECT = {}


def reads_of(oracle, c, w, span):
    return F.many_taxa_reads(w) if c.world == "many" else F.read_set(w, span)


def expectation(oracle, c, w, span):
    """reads, their concatenation and the oracle's answers for the case's (world, window, mate count); shared by the cases
    that differ in the kernel form only"""
    key = (c.k, c.canon, c.gaps, c.world, span, c.paired)
    if key not in _EXPECT:
        reads = reads_of(oracle, c, w, span)
        bases, offsets = synth.concat(reads)
        gaps = list(c.gaps) if c.gaps is not None else None
        exp = oracle.classify_batch(w.table, w.tax, w.k, bases, offsets, paired=c.paired, gaps=gaps, canon=c.canon, spaced_intended=True)
        inc = 2 if c.paired else 1
        hits = []
        for u in range(len(reads) // inc):
            s2 = reads[u * inc + 1].tobytes() if c.paired else None
            hits.append(oracle.classify_seq(w.table, w.tax, w.k, reads[u * inc].tobytes(), s2, gaps=gaps, canon=c.canon, spaced_intended=True)[3])
        _EXPECT[key] = (reads, bases, offsets, exp, hits)
    return _EXPECT[key]


@pytest.mark.parametrize("c", F.cases(), ids=F.case_id)
def test_form_against_oracle(gpu_ctx, oracle, c):
    import bonsai_amd
    ctx = gpu_ctx
    w = F.world(oracle, c.k, c.canon, c.gaps, c.world)
    n_keys = int(w.table.header()[1])
    m_exp, bits_exp = F.case_table(c)
    dbg = F.case_dbg(c)
    clustered_contig = c.layout == 2 and c.gaps is None
    ctx.set_encoder(c.k, list(c.gaps) if c.gaps is not None else None, canonicalize=c.canon)
    try:
        ctx.debug_set(dbg)
        if clustered_contig:
            ctx.set_minimizer_span(c.span)
            ctx.set_minimizer_identity(c.identity)
        if c.ovc == "on":
            ctx.set_table_buckets(max(16, n_keys * 10 // 80))           # 10 slots a bucket: 80 % full
        ctx.load_table(w.n_buckets, w.flags, w.keys, w.vals, layout=c.layout)
        ctx.load_taxonomy(w.parent)
        geo = ctx.table_geometry()
        if m_exp is not None:
            assert geo["m"] == m_exp
        assert geo["identity_bits"] == bits_exp
        if c.ovc == "on":
            assert geo["overflow_keys"] > 0
        span = c.k - geo["m"] if clustered_contig else 0

        reads, bases, offsets, exp, exp_hits = expectation(oracle, c, w, span)
        if c.packed:
            words, bw, bm = bonsai_amd.pack_reads(bases, offsets, threads=2)
            got = ctx.classify_packed(words, bw, bm, offsets, paired=c.paired, want_hits=True)
        else:
            got = ctx.classify(bases, offsets, paired=c.paired, want_hits=True)
        form = ctx.last_classify_form()

        # ---- the oracle's answers, every unit
        for key in ("taxon", "missing", "ambig", "n_hits"):
            bad = np.flatnonzero(got[key] != exp[key])
            assert bad.size == 0, "%s differs at units %s: got %s, expected %s" % (key, bad[:8], got[key][bad[:8]], exp[key][bad[:8]])
        assert len(got["hits"]) == len(exp_hits)
        for u, (a, b) in enumerate(zip(got["hits"], exp_hits)):
            assert np.array_equal(a, b), "hit stream of unit %d" % u

        # ---- the kernel that ran
        heavy = F.ovf_heavy(dbg, geo["overflow_keys"], n_keys)
        assert form["kernel"] == F.expected_form(c.k, c.canon, c.gaps, c.layout, geo["m"], geo["identity_bits"], heavy, c.packed, c.paired)
        assert form["kernel"] == F.case_forms(c)[0]                      # ... which is the form the case is in the matrix for
        n_units = len(reads) // (2 if c.paired else 1)
        assert 1 <= form["chunk"] <= 31 and 1 <= form["grid"] <= (n_units + form["chunk"] - 1) // form["chunk"]

        # ---- the case reached what it is for
        assert (got["taxon"] != 0).mean() > 0.5
        assert int(got["n_hits"].sum()) > 0 and int(got["missing"].sum()) > 0 and int(got["ambig"].sum()) > 0
        if c.world == "many":
            over = sum(1 for h in exp_hits if np.unique(h).size > F.LDS_CAP)
            assert over > 0 and form["overflow_units"] == over
            assert form["overflow_kernel"] == F.expected_overflow_form(c.gaps, c.layout, geo["identity_bits"], c.packed)
            assert 1 <= form["overflow_grid"] <= over
        else:
            assert form["overflow_kernel"] is None and form["overflow_units"] == 0
            assert any(r.size > 4096 for r in reads) and any(reads[i].size != reads[i + 1].size for i in range(0, len(reads), 2))
            if span:
                at, carried = F.window_coverage(reads, c.k, geo["m"])
                assert at.all() and carried.all()
    finally:
        ctx.debug_set(0)
        ctx.set_minimizer_span(0)
        ctx.set_minimizer_identity(0)
        ctx.set_table_buckets(0)
