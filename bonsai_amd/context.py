"""Host-side mirror of the reference's classify objects over the C ABI.

Context bundles what bin/bonsai.cpp:149-157 builds before process_dataset: the Database's khash
(database.h:33-56), the Spacer/Encoder (classifier.h:155-166) and the parent map (util.h:766-785).
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from . import _lib
from ._lib import BonsaiAmdError, u8p, u16p, u32p, u64p, vp


def _p(a, t):
    return a.ctypes.data_as(t)


def concat_reads(seqs):
    """list of bytes/str -> (uint8 bases, uint64 offsets[n+1])"""
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    offsets = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offsets[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    bases = np.frombuffer(b"".join(bs), dtype=np.uint8).copy() if bs else np.zeros(0, dtype=np.uint8)
    return bases, offsets


def pack_reads(bases, offsets, threads=1):
    """bns_pack_reads (host only, no GPU needed): ASCII batch -> (words uint64, bad_word uint64, bad_mask uint32): the 2-bit image
    the classify kernel works on and the sparse list of words that hold a base other than A/C/G/T"""
    L = _lib.load()
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = offsets.size - 1
    words = np.zeros(int(L.bns_packed_words(int(offsets[-1]) if n >= 0 else 0, n)), dtype=np.uint64)
    cap = 1024
    while True:
        bw = np.zeros(cap, dtype=np.uint64); bm = np.zeros(cap, dtype=np.uint32); nb = C.c_uint64()
        rc = L.bns_pack_reads(bases.ctypes.data, _p(offsets, u64p), n, _p(words, u64p), _p(bw, u64p), _p(bm, u32p), cap,
                              C.cast(C.byref(nb), u64p), int(threads))
        if rc == 0:
            return words, bw[:nb.value].copy(), bm[:nb.value].copy()
        if nb.value <= cap:
            raise BonsaiAmdError("bns_pack_reads: %s" % L.bns_strerror(rc).decode())
        cap = int(nb.value)


def pack_reads_qual(seqs, quals, min_quality, threads=1):
    """bns_pack_reads_qual_ptrs (host only): reads (a list of bytes) and their quality strings (bytes of the read's length, or None: a
    read without quality; quals itself may be None) -> (words, bad_word, bad_mask, offsets): pack_reads' image with every base whose
    quality byte is below 33 + min_quality flagged like an invalid base, its code bits 0"""
    L = _lib.load()
    seqs = [bytes(s) for s in seqs]
    n = len(seqs)
    if quals is not None:
        quals = [None if q is None else bytes(q) for q in quals]
        if len(quals) != n or any(q is not None and len(q) != len(s) for s, q in zip(seqs, quals)):
            raise ValueError("pack_reads_qual: one quality string (or None) per read, as long as the read")
    sp = (C.c_char_p * max(1, n))(*seqs)
    qp = (C.c_char_p * max(1, n))(*quals) if quals is not None else None
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    offsets = np.zeros(n + 1, dtype=np.uint64)
    words = np.zeros(int(L.bns_packed_words(int(lens.sum()), n)), dtype=np.uint64)
    cap = 1024
    while True:
        bw = np.zeros(cap, dtype=np.uint64); bm = np.zeros(cap, dtype=np.uint32); nb = C.c_uint64()
        rc = L.bns_pack_reads_qual_ptrs(C.cast(sp, vp), C.cast(qp, vp) if qp is not None else None, _p(lens, u32p), n, int(min_quality),
                                        _p(offsets, u64p), _p(words, u64p), _p(bw, u64p), _p(bm, u32p), cap, C.cast(C.byref(nb), u64p), int(threads))
        if rc == 0:
            return words, bw[:nb.value].copy(), bm[:nb.value].copy(), offsets
        if nb.value <= cap:
            raise BonsaiAmdError("bns_pack_reads_qual_ptrs: %s" % L.bns_strerror(rc).decode())
        cap = int(nb.value)


def confidence_fraction(threshold):
    """a confidence threshold (int, str, Fraction or float; a float goes through its shortest repr: 0.1 is 1/10) -> (num, den) in
    lowest terms, what bns_set_confidence takes; ValueError outside [0, 1], and when a term does not fit the C ABI's uint64_t"""
    if isinstance(threshold, bool):
        raise ValueError("confidence threshold must be a number in [0, 1], not %r" % (threshold,))
    if isinstance(threshold, float):
        threshold = str(threshold)
    try:
        f = Fraction(threshold)
    except (TypeError, ValueError, ZeroDivisionError):
        raise ValueError("confidence threshold must be a number in [0, 1], not %r" % (threshold,)) from None
    if not 0 <= f <= 1:
        raise ValueError("confidence threshold must lie in [0, 1], not %s" % f)
    if f.denominator >= 1 << 64:                         # (num <= den) ctypes would pass the terms mod 2^64: another threshold
        raise ValueError("confidence threshold %s: num and den in lowest terms must be below 2^64" % f)
    return f.numerator, f.denominator


class Context:
    def __init__(self, device=0):
        self.L = _lib.load()
        h = vp()
        rc = self.L.bns_create(device, C.byref(h))
        if rc != 0:
            raise BonsaiAmdError("bns_create(%d): %s" % (device, self.L.bns_strerror(rc).decode()))
        self.h = h
        self.k = None

    def close(self):
        if getattr(self, "h", None):
            self.L.bns_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise BonsaiAmdError("%s: %s (%s)" % (what, self.L.bns_strerror(rc).decode(),
                                                   self.L.bns_last_error(self.h).decode()))

    # ---- configuration
    def set_encoder(self, k, gaps=None, canonicalize=True, spaced_intended=True):
        g = None
        gp = None
        if gaps is not None:
            g = np.ascontiguousarray(gaps, dtype=np.uint16)
            if g.size != k - 1:
                raise ValueError("gaps must have k-1 entries")
            gp = _p(g, u16p)
        self._chk(self.L.bns_set_encoder(self.h, k, gp, int(canonicalize), int(spaced_intended)), "bns_set_encoder")
        self.k = k

    def set_window(self, w, score=_lib.SCORE_LEX):
        """Spacer window + score for minimizer selection (encode / build only; classify is always w = k)."""
        self._chk(self.L.bns_set_window(self.h, w, score), "bns_set_window")

    def set_bucket_slots_log2(self, lg):
        self._chk(self.L.bns_set_bucket_slots_log2(self.h, lg), "bns_set_bucket_slots_log2")

    def set_table_buckets(self, n):
        """clustered table: exact number of home buckets (0 = sized from the key count)"""
        self._chk(self.L.bns_set_table_buckets(self.h, n), "bns_set_table_buckets")

    def set_minimizer_identity(self, bits):
        """clustered table: 32 / 52-bit minimizer identity, 0 = chosen from the key count"""
        self._chk(self.L.bns_set_minimizer_identity(self.h, bits), "bns_set_minimizer_identity")

    def set_table_fill(self, mode):
        """clustered table: 0 = the loader decides, 1 = keys in arrival order, 2 = group-aware fill"""
        self._chk(self.L.bns_set_table_fill(self.h, mode), "bns_set_table_fill")

    def table_geometry(self):
        g = (C.c_uint64 * 8)()
        self._chk(self.L.bns_table_geometry(self.h, g), "bns_table_geometry")
        return {"buckets": g[0], "m": g[1], "identity_bits": g[2], "spilled_keys": g[3], "span": g[4], "overflow_keys": g[5], "group_fill": g[6]}

    def table_warning(self):
        return self.L.bns_table_warning(self.h).decode()

    # debug_set bit: classify_kernel takes a wavefront's work counter by its index & 7 instead of its XCD number, so that a grid of
    # two workgroups (debug_claim_waves(8)) reaches all eight counters and goes from a dry one to the next; same results
    DBG_SHARD_BY_WAVE = 0x200000

    def debug_set(self, bits):
        """test / profiling switches (BNS_DBG_* in bns_api.hip, bns_table_plan.hpp and bns_classify_plan.hpp); not part of the public header"""
        self._chk(self.L.bns_debug_set(self.h, bits), "bns_debug_set")

    def debug_claim_waves(self, waves):
        """bns_debug_set_claim_waves (a test aid, not part of the public header): classify_kernel's claims are sized for `waves`
        resident wavefronts (a multiple of 4) and its grid capped at waves / 4 workgroups; 0 = the device's own"""
        self._chk(self.L.bns_debug_set_claim_waves(self.h, int(waves)), "bns_debug_set_claim_waves")

    def last_classify_form(self):
        """bns_debug_last_classify_form (a test aid, not part of the public header): what the last classify call of this context
        launched.  "kernel": (SPACED, LAYOUT, KT, NM, SPAN, OVC, WIDE, PACKED) of the classify_kernel instantiation (None before the
        first call); "overflow_kernel": (SPACED, LAYOUT, WIDE, PACKED) of the classify_overflow_kernel one, None when no unit went
        there; "overflow_units" / "overflow_grid"; "chunk" (units per claim) and "grid" of classify_kernel."""
        w = np.zeros(18, dtype=np.uint32)
        n = self.L.bns_debug_last_classify_form(self.h, _p(w, u32p), w.size)
        if n != w.size:
            raise BonsaiAmdError("bns_debug_last_classify_form: %d words" % n)
        v = [int(x) for x in w]
        return {"kernel": tuple(v[1:9]) if v[0] else None, "overflow_kernel": tuple(v[10:14]) if v[9] else None,
                "overflow_units": v[14], "overflow_grid": v[15], "chunk": v[16], "grid": v[17]}

    def load_table(self, n_buckets, flags, keys, vals, layout=_lib.LAYOUT_MINBUCKET):
        flags = np.ascontiguousarray(flags, dtype=np.uint32)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        vals = np.ascontiguousarray(vals, dtype=np.uint32)
        if keys.size != n_buckets or vals.size != n_buckets or flags.size != max(1, n_buckets >> 4):
            raise ValueError("khash array sizes do not match n_buckets")
        self._chk(self.L.bns_load_table(self.h, n_buckets, _p(flags, u32p), _p(keys, u64p), _p(vals, u32p), layout),
                  "bns_load_table")

    def load_table_device(self, n_buckets, d_flags, d_keys, d_vals, layout=_lib.LAYOUT_MINBUCKET, stream=None):
        self._chk(self.L.bns_load_table_device(self.h, n_buckets, d_flags, d_keys, d_vals, layout, stream),
                  "bns_load_table_device")

    def table_info(self):
        nk = C.c_uint64(); nb = C.c_uint64(); ly = C.c_int()
        self._chk(self.L.bns_table_info(self.h, C.byref(nk), C.byref(nb), C.byref(ly)), "bns_table_info")
        return {"n_keys": nk.value, "device_bytes": nb.value, "layout": ly.value}

    def table_stats(self):
        st = (C.c_uint64 * 4)()
        self._chk(self.L.bns_table_stats(self.h, st), "bns_table_stats")
        return {"n_keys": st[0], "n_overflow_keys": st[1], "main_bytes": st[2], "overflow_bytes": st[3]}

    def set_minimizer_span(self, span):
        """clustered table, contiguous seeds: minimizer window k - m; 0 = chosen from the db at load, 8 / 11 / 15 fix it"""
        self._chk(self.L.bns_set_minimizer_span(self.h, span), "bns_set_minimizer_span")

    def table_minimizer(self):
        m = C.c_uint32(); sp = C.c_uint64()
        self._chk(self.L.bns_table_minimizer(self.h, C.byref(m), C.byref(sp)), "bns_table_minimizer")
        return {"m": m.value, "spilled_keys": sp.value}

    def load_taxonomy(self, parent):
        parent = np.ascontiguousarray(parent, dtype=np.uint32)
        self._chk(self.L.bns_load_taxonomy(self.h, _p(parent, u32p), parent.size), "bns_load_taxonomy")
        self._n_tax = int(parent.size)

    def tally_enable(self, on=True):
        """bns_tally_enable: count every unit the classify calls report per taxon bin (0 unclassified, n not in the taxonomy)"""
        self._chk(self.L.bns_tally_enable(self.h, int(bool(on))), "bns_tally_enable")

    def tally(self, reset=False):
        """bns_tally_read -> (direct, clade): uint64 arrays of n + 1 entries (n = the size of the parent array loaded)"""
        n = getattr(self, "_n_tax", 0)
        direct = np.zeros(n + 1, dtype=np.uint64)
        clade = np.zeros(n + 1, dtype=np.uint64)
        self._chk(self.L.bns_tally_read(self.h, _p(direct, u64p), _p(clade, u64p), n + 1, int(bool(reset))), "bns_tally_read")
        return direct, clade

    def table_tally(self):
        """bns_table_tally -> (direct, clade): the keys of the loaded table per taxon bin (tally_enable's bins, by the key's value) and
        per clade, uint64 arrays of n + 1 entries.  Every context of a multi-GPU load returns the whole answer: do not add them up."""
        n = getattr(self, "_n_tax", 0)
        direct = np.zeros(n + 1, dtype=np.uint64)
        clade = np.zeros(n + 1, dtype=np.uint64)
        self._chk(self.L.bns_table_tally(self.h, _p(direct, u64p), _p(clade, u64p), n + 1), "bns_table_tally")
        return direct, clade

    def set_confidence(self, threshold):
        """bns_set_confidence: every classify call walks its taxa up to the first ancestor whose clade holds ceil(threshold * Q) of a
        unit's Q probed k-mers (0 when none does); threshold 0 turns it off.  Needs a loaded taxonomy (unless 0)."""
        num, den = confidence_fraction(threshold)
        self._chk(self.L.bns_set_confidence(self.h, num, den), "bns_set_confidence")

    def set_min_hit_groups(self, n):
        """bns_set_min_hit_groups: every classify call leaves a unit unclassified unless at least n DISTINCT keys of it (all mates
        together) are found in the table; n in [0, 64], 0 turns it off.  Applied behind set_confidence's walk; only the taxon changes."""
        self._chk(self.L.bns_set_min_hit_groups(self.h, int(n)), "bns_set_min_hit_groups")

    def sketch_enable(self, max_taxa=65536):
        """bns_sketch_enable: a HyperLogLog sketch (4096 one-byte registers) of the distinct k-mers every classify call looks up, per
        taxon bin, for up to max_taxa bins; 0 frees them and turns it off.  Needs a loaded taxonomy (unless 0)."""
        self._chk(self.L.bns_sketch_enable(self.h, int(max_taxa)), "bns_sketch_enable")

    def sketch(self, reset=False):
        """bns_sketch_read -> (bins uint32[s] ascending, registers uint8[s, 4096], n_dropped_bins)"""
        s = C.c_uint32(); dropped = C.c_uint32()
        self._chk(self.L.bns_sketch_read(self.h, None, None, 0, C.byref(s), C.byref(dropped), 0), "bns_sketch_read")
        bins = np.zeros(s.value, dtype=np.uint32)
        regs = np.zeros((s.value, 4096), dtype=np.uint8)
        self._chk(self.L.bns_sketch_read(self.h, _p(bins, u32p), regs.ctypes.data_as(C.c_void_p), s.value, C.byref(s), C.byref(dropped),
                                         int(bool(reset))), "bns_sketch_read")
        return bins, regs, int(dropped.value)

    def set_min_base_quality(self, q):
        """bns_set_min_base_quality: classify_text() treats every base whose Phred+33 quality byte is below 33 + q like an 'N'
        (q in [0, 93]; 0 turns it off).  FASTA records are untouched."""
        self._chk(self.L.bns_set_min_base_quality(self.h, int(q)), "bns_set_min_base_quality")

    def set_dust(self, window=64, level=20):
        """bns_set_dust: every classify and build call masks low-complexity sequence (symmetric DUST over the packed image: window in
        [8, 64] bases, level in [1, 1000]) before it looks anything up; a masked base counts like an 'N'.  window 0 turns it off."""
        self._chk(self.L.bns_set_dust(self.h, int(window), int(level)), "bns_set_dust")

    def dust_mask(self, bases, offsets):
        """bns_dust_mask -> one bool array per sequence: the bases the current set_dust() masks (those of N's are not set)"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        flags = np.zeros(int(self.L.bns_packed_words(int(offsets[-1]), n)), dtype=np.uint32)
        self._chk(self.L.bns_dust_mask(self.h, bases.ctypes.data if bases.size else None, _p(offsets, u64p), n, _p(flags, u32p)), "bns_dust_mask")
        out = []
        for s in range(n):
            o = int(offsets[s]); ln = int(offsets[s + 1]) - o
            w = flags[(o >> 5) + s:(o >> 5) + s + ((ln + 31) >> 5)]
            bits = np.unpackbits(w.astype(">u4").view(np.uint8)) if w.size else np.zeros(0, dtype=np.uint8)
            out.append(bits[:ln].astype(bool))
        return out

    # ---- hot path (host buffers)
    def classify(self, bases, offsets, paired=False, want_hits=False):
        """classify_seqs (classifier.h:269-287) over one batch; returns dict of per-unit arrays."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_reads = offsets.size - 1
        n_units = n_reads // (2 if paired else 1)
        taxon = np.zeros(n_units, dtype=np.uint32)
        missing = np.zeros(n_units, dtype=np.uint32)
        ambig = np.zeros(n_units, dtype=np.uint32)
        n_hits = np.zeros(n_units, dtype=np.uint32)
        hits = np.zeros(int(offsets[-1]) if want_hits else 0, dtype=np.uint32)
        self._chk(self.L.bns_classify_batch(self.h, bases.ctypes.data, _p(offsets, u64p), n_reads, int(paired),
                                            _p(taxon, u32p), _p(missing, u32p), _p(ambig, u32p), _p(n_hits, u32p),
                                            _p(hits, u32p) if want_hits else None), "bns_classify_batch")
        out = {"taxon": taxon, "missing": missing, "ambig": ambig, "n_hits": n_hits}
        if want_hits:
            inc = 2 if paired else 1
            out["hits"] = [hits[int(offsets[u * inc]):int(offsets[u * inc]) + int(n_hits[u])].copy()
                           for u in range(n_units)]
        return out

    def classify_packed(self, words, bad_word, bad_mask, offsets, paired=False, want_hits=False):
        """classify() over a batch already packed by pack_reads(): same results, 40 instead of 150 bytes per 150-bp read uploaded"""
        words = np.ascontiguousarray(words, dtype=np.uint64)
        bad_word = np.ascontiguousarray(bad_word, dtype=np.uint64); bad_mask = np.ascontiguousarray(bad_mask, dtype=np.uint32)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_reads = offsets.size - 1
        n_units = n_reads // (2 if paired else 1)
        taxon = np.zeros(n_units, dtype=np.uint32); missing = np.zeros(n_units, dtype=np.uint32)
        ambig = np.zeros(n_units, dtype=np.uint32); n_hits = np.zeros(n_units, dtype=np.uint32)
        hits = np.zeros(int(offsets[-1]) if want_hits else 0, dtype=np.uint32)
        self._chk(self.L.bns_classify_batch_packed(self.h, _p(words, u64p), _p(bad_word, u64p) if bad_word.size else None,
                                                   _p(bad_mask, u32p) if bad_mask.size else None, bad_word.size, _p(offsets, u64p), n_reads,
                                                   int(paired), _p(taxon, u32p), _p(missing, u32p), _p(ambig, u32p), _p(n_hits, u32p),
                                                   _p(hits, u32p) if want_hits else None), "bns_classify_batch_packed")
        out = {"taxon": taxon, "missing": missing, "ambig": ambig, "n_hits": n_hits}
        if want_hits:
            inc = 2 if paired else 1
            out["hits"] = [hits[int(offsets[u * inc]):int(offsets[u * inc]) + int(n_hits[u])].copy() for u in range(n_units)]
        return out

    def classify_packed_device(self, d_words, d_nmask, d_offsets, n_reads, total_bases, max_read_len, paired, d_taxon,
                               d_missing=None, d_ambig=None, d_n_hits=None, d_hits=None, stream=None):
        self._chk(self.L.bns_classify_batch_packed_device(self.h, d_words, d_nmask, d_offsets, n_reads, total_bases, max_read_len,
                                                          int(paired), d_taxon, d_missing, d_ambig, d_n_hits, d_hits, stream),
                  "bns_classify_batch_packed_device")

    def classify_runs(self, bases, offsets, paired=False):
        """classify() with the hit stream run-length encoded on the device: out["runs"][u] = (taxids, lengths)."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_reads = offsets.size - 1
        n_units = n_reads // (2 if paired else 1)
        taxon = np.zeros(n_units, dtype=np.uint32)
        missing = np.zeros(n_units, dtype=np.uint32)
        ambig = np.zeros(n_units, dtype=np.uint32)
        n_hits = np.zeros(n_units, dtype=np.uint32)
        run_start = np.zeros(n_units, dtype=np.uint64)
        n_runs = np.zeros(n_units, dtype=np.uint32)
        rt = u32p(); rl = u32p(); tot = C.c_uint64()
        self._chk(self.L.bns_classify_batch_runs(self.h, bases.ctypes.data, _p(offsets, u64p), n_reads, int(paired),
                                                 _p(taxon, u32p), _p(missing, u32p), _p(ambig, u32p), _p(n_hits, u32p),
                                                 _p(run_start, u64p), _p(n_runs, u32p), C.byref(rt), C.byref(rl),
                                                 C.cast(C.byref(tot), u64p)), "bns_classify_batch_runs")
        n = int(tot.value)
        tax = np.ctypeslib.as_array(rt, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
        ln = np.ctypeslib.as_array(rl, shape=(n,)).copy() if n else np.zeros(0, np.uint32)
        runs = [(tax[int(s):int(s) + int(c)], ln[int(s):int(s) + int(c)]) for s, c in zip(run_start, n_runs)]
        return {"taxon": taxon, "missing": missing, "ambig": ambig, "n_hits": n_hits, "runs": runs, "n_runs_total": n}

    def classify_text(self, texts, final=True, limit=None, trim_readno=False, parse_only=False, want_runs=False, want_words=False,
                      cap_records=None, names_cap=None, device_ptrs=None, runs_cap=None, defer=False, between=None,
                      want_lines=False, emit_all=True, lines_cap=None):
        """bns_classify_text: FASTA / FASTQ TEXT (bytes, or a pair of bytes: mates) parsed, packed and classified on the device.
        device_ptrs = [(ptr, n_bytes), ...]: the text is already in HBM.  -> dict with n_records, consumed, status, why, per-unit
        results, per-record seq_len / rec_pos / names, runs as classify_runs() gives them, the packed words when asked for.
        defer: the call in two halves (BNS_TEXT_DEFER, then bns_text_finish; `between()` runs in between) -- "first_half" in the result is
        what the first half reported.
        want_lines: the units' Kraken lines, assembled on the device: "lines" (bytes), "line_off" (uint64, n_units + 1: unit u's line is
        lines[line_off[u]:line_off[u + 1]], empty when it is not printed), "lines_bytes".  emit_all: unclassified units are printed too
        (`classify -a`); lines_cap: room in bytes (default: ample)."""
        if isinstance(texts, (bytes, bytearray, memoryview, np.ndarray)):
            texts = [texts]
        bufs = [np.frombuffer(bytes(t), dtype=np.uint8) if not isinstance(t, np.ndarray) else np.ascontiguousarray(t, dtype=np.uint8) for t in texts]
        ns = len(device_ptrs) if device_ptrs is not None else len(bufs)
        if device_ptrs is not None:
            ptrs = (vp * ns)(*[vp(int(p)) for p, _ in device_ptrs])
            sizes = np.array([n for _, n in device_ptrs], dtype=np.uint64)
        else:
            ptrs = (vp * ns)(*[vp(b.ctypes.data if b.size else 0) for b in bufs])
            sizes = np.array([b.size for b in bufs], dtype=np.uint64)
        cap = int(cap_records) if cap_records is not None else int(sizes.sum()) // 2 + 16
        ncap = int(names_cap) if names_cap is not None else int(sizes.sum()) + 16
        nu_cap = cap
        a = {"taxon": np.zeros(nu_cap, np.uint32), "missing": np.zeros(nu_cap, np.uint32), "ambig": np.zeros(nu_cap, np.uint32),
             "n_hits": np.zeros(nu_cap, np.uint32), "seq_len": np.zeros(cap, np.uint32), "rec_pos": np.zeros(cap, np.uint64),
             "name_off": np.zeros(cap + 1, np.uint32), "names": np.zeros(ncap, np.uint8)}
        o = _lib.TextOut()
        for k in ("taxon", "missing", "ambig", "n_hits", "seq_len", "rec_pos", "name_off", "names"):
            setattr(o, k, a[k].ctypes.data)
        o.names_cap = ncap
        if want_runs:
            a["run_start"] = np.zeros(nu_cap, np.uint64); a["n_runs"] = np.zeros(nu_cap, np.uint32)
            o.run_start = a["run_start"].ctypes.data; o.n_runs = a["n_runs"].ctypes.data
        if want_runs and runs_cap is not None:                 # the caller's own run arrays instead of the context's
            a["run_tax"] = np.zeros(max(1, int(runs_cap)), np.uint32); a["run_len"] = np.zeros(max(1, int(runs_cap)), np.uint32)
            o.run_tax = a["run_tax"].ctypes.data; o.run_len = a["run_len"].ctypes.data; o.runs_cap = int(runs_cap)
        if want_words:
            nw = int(sizes.sum()) // 32 + cap + 2
            a["words"] = np.zeros(nw, np.uint64); a["nmask"] = np.zeros(nw, np.uint32)
            o.words = a["words"].ctypes.data; o.nmask = a["nmask"].ctypes.data
        if want_lines:
            lcap = int(lines_cap) if lines_cap is not None else 24 * int(sizes.sum()) + 128 * cap + 64
            a["lines"] = np.zeros(max(1, lcap), np.uint8); a["line_off"] = np.zeros(nu_cap + 1, np.uint64)
            o.lines = a["lines"].ctypes.data; o.lines_cap = lcap; o.line_off = a["line_off"].ctypes.data
            o.lines_flags = _lib.LINES_ALL if emit_all else 0
        info = _lib.TextInfo()
        flags = (_lib.TEXT_FINAL if final else 0) | (_lib.TEXT_TRIM_READNO if trim_readno else 0) | (_lib.TEXT_PARSE_ONLY if parse_only else 0) | \
                (_lib.TEXT_DEVICE if device_ptrs is not None else 0) | (_lib.TEXT_DEFER if defer else 0)
        lim = int(limit) if limit is not None else 0xFFFFFFFFFFFFFFFF
        self._chk(self.L.bns_classify_text(self.h, ptrs, _p(sizes, u64p), ns, lim, flags, cap, C.byref(o), C.byref(info)), "bns_classify_text")
        first_half = None
        if defer:
            first_half = {"n_records": int(info.n_records), "consumed": [int(info.consumed[i]) for i in range(ns)], "status": int(info.status),
                          "total_bases": int(info.total_bases), "names_bytes": int(info.names_bytes)}
            if between is not None:
                between()
            info = _lib.TextInfo()
            self._chk(self.L.bns_text_finish(self.h, C.byref(info)), "bns_text_finish")
        n = int(info.n_records)
        nu = n // ns
        names = a["names"].tobytes()
        res = {"n_records": n, "consumed": [int(info.consumed[i]) for i in range(ns)], "status": int(info.status), "why": int(info.why),
               "total_bases": int(info.total_bases), "n_slices": int(info.n_slices), "n_launches": int(info.n_launches), "ms_parse": float(info.ms_parse), "ms_classify": float(info.ms_classify),
               "seq_len": a["seq_len"][:n].copy(), "rec_pos": a["rec_pos"][:n].copy(),
               "names": [names[int(a["name_off"][r]):int(a["name_off"][r + 1])] for r in range(n)]}
        if not parse_only:
            for k in ("taxon", "missing", "ambig", "n_hits"):
                res[k] = a[k][:nu].copy()
            if want_runs:
                nt = int(info.n_runs_total)
                if runs_cap is not None:
                    tax, ln = a["run_tax"][:nt].copy(), a["run_len"][:nt].copy()
                else:
                    tax = np.ctypeslib.as_array(info.run_tax, shape=(nt,)).copy() if nt else np.zeros(0, np.uint32)
                    ln = np.ctypeslib.as_array(info.run_len, shape=(nt,)).copy() if nt else np.zeros(0, np.uint32)
                res["runs"] = [(tax[int(s):int(s) + int(c)], ln[int(s):int(s) + int(c)]) for s, c in zip(a["run_start"][:nu], a["n_runs"][:nu])]
            if want_lines:
                nb = int(info.lines_bytes)
                res["lines"] = a["lines"][:nb].tobytes(); res["line_off"] = a["line_off"][:nu + 1].copy(); res["lines_bytes"] = nb
                res["ms_lines"] = float(info.ms_lines)
        if want_words:
            nw = int(self.L.bns_packed_words(int(info.total_bases), n))
            res["words"] = a["words"][:nw].copy(); res["nmask"] = a["nmask"][:nw].copy()
        if first_half is not None:
            res["first_half"] = first_half
        return res

    def encode(self, bases, offsets):
        """Encoder::for_each over a batch (encoder.h:415-442): list of uint64 arrays, one per read."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_reads = offsets.size - 1
        kmers = np.zeros(max(1, int(offsets[-1])), dtype=np.uint64)
        n_k = np.zeros(n_reads, dtype=np.uint32)
        self._chk(self.L.bns_encode_batch(self.h, bases.ctypes.data, _p(offsets, u64p), n_reads, _p(kmers, u64p),
                                          _p(n_k, u32p)), "bns_encode_batch")
        return [kmers[int(offsets[r]):int(offsets[r]) + int(n_k[r])].copy() for r in range(n_reads)]

    def _hashes(self, name, bases, offsets, args, tables, n_tables, words=1, per=1):
        """The hashers' call `name`(h, bases, offsets, n, *args, *tables, out, counts): one array per sequence, (n,) uint64 or
        (n, words).  words = u64 per value and per table entry, per = entries per base of the output buffer, tables = n_tables
        character tables of 256 entries, or None."""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = offsets.size - 1
        out = np.zeros(max(1, words * per * int(offsets[-1])), dtype=np.uint64)
        cnt = np.zeros(n, dtype=np.uint32)
        tabs = [] if tables is None else [np.ascontiguousarray(t, dtype=np.uint64).reshape(-1) for t in tables]
        assert len(tabs) in (0, n_tables) and all(t.size == 256 * words for t in tabs)
        self._chk(getattr(self.L, name)(self.h, bases.ctypes.data, _p(offsets, u64p), n, *args, *([_p(t, u64p) for t in tabs] or [None] * n_tables),
                                        _p(out, u64p), _p(cnt, u32p)), name)
        vals = (out[words * per * int(offsets[r]):words * (per * int(offsets[r]) + int(cnt[r]))] for r in range(n))
        return [(v if words == 1 else v.reshape(-1, words)).copy() for v in vals]

    def rolling_hash(self, bases, offsets, k, canon=False, tables=None, w=0):
        """RollingHasher<u64>::for_each_hash over a batch (encoder.h:644-865): list of uint64 arrays.  w > k: with a window
        (minimizers of the hash stream by lex_score; the canonical path queues both strands' hashes).
        tables = (fwd[256], rc[256]) character tables, None = the default-seed tables (parity unpinned)."""
        return self._hashes("bns_rolling_hash_windowed_batch", bases, offsets, (k, int(canon), int(w)), tables, 2, 1, 2 if (w > k and canon) else 1)

    def rolling_hash128(self, bases, offsets, k, canon=False, tables=None, w=0):
        """RollingHasher<__uint128_t>::for_each_hash (w > k: with a window of w - k + 1 values): list of (n, 2) uint64 arrays
        [lo, hi], one per sequence.  tables = (fwd, rc), each 256 x (lo, hi) u64; None = the default-seed tables."""
        return self._hashes("bns_rolling_hash128_windowed_batch", bases, offsets, (k, int(canon), int(w)), tables, 2, 2, 2 if (w > k and canon) else 1)

    def for_each_hash(self, bases, offsets, k=0, canon=-1, table=None):
        """Encoder::for_each_hash over a batch (encoder.h:355-394, ntHash): list of uint64 arrays, one per sequence.
        k = 0: the encoder's k; canon = -1: the encoder's flag; table = 256 seeds in make_nthash_lut's geometry (None: published)."""
        return self._hashes("bns_for_each_hash_batch", bases, offsets, (int(k), int(canon)), None if table is None else (table,), 1)

    def probe(self, kmers):
        """kh_get over a batch (khash64.h:250-263): (vals, found)."""
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64)
        vals = np.zeros(kmers.size, dtype=np.uint32)
        found = np.zeros(kmers.size, dtype=np.uint8)
        self._chk(self.L.bns_probe(self.h, _p(kmers, u64p), kmers.size, _p(vals, u32p), _p(found, u8p)), "bns_probe")
        return vals, found

    def resolve(self, keys, counts, starts):
        """resolve_tree (util.h:831-869) over a batch of insertion-ordered counters."""
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        counts = np.ascontiguousarray(counts, dtype=np.uint16)
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        n_units = starts.size - 1
        taxon = np.zeros(n_units, dtype=np.uint32)
        self._chk(self.L.bns_resolve_batch(self.h, _p(keys, u32p), _p(counts, u16p), _p(starts, u64p), n_units,
                                           _p(taxon, u32p)), "bns_resolve_batch")
        return taxon

    # ---- device-pointer entry points (ints are raw device addresses, e.g. torch.Tensor.data_ptr())
    def classify_device(self, d_bases, d_offsets, n_reads, total_bases, max_read_len, paired, d_taxon,
                        d_missing=None, d_ambig=None, d_n_hits=None, d_hits=None, stream=None):
        self._chk(self.L.bns_classify_batch_device(self.h, d_bases, d_offsets, n_reads, total_bases, max_read_len,
                                                   int(paired), d_taxon, d_missing, d_ambig, d_n_hits, d_hits, stream),
                  "bns_classify_batch_device")

    def probe_device(self, d_kmers, n, d_vals, d_found=None, stream=None):
        self._chk(self.L.bns_probe_device(self.h, d_kmers, n, d_vals, d_found, stream), "bns_probe_device")

    def encode_device(self, d_bases, d_offsets, n_reads, total_bases, d_kmers, d_n_kmers, stream=None):
        """bns_encode_batch_device: read r's k-mers (minimizers under set_window) at d_kmers[offsets[r]:] (total_bases uint64), their
        number in d_n_kmers[r] (uint32).  Queued on the stream: wait for it before reading."""
        self._chk(self.L.bns_encode_batch_device(self.h, d_bases, d_offsets, n_reads, total_bases, d_kmers, d_n_kmers, stream),
                  "bns_encode_batch_device")

    def build_table_device(self, d_bases, d_offsets, n_genomes, total_bases, d_taxid, n_buckets, d_flags, d_keys,
                           d_vals, stream=None):
        hdr = np.zeros(4, dtype=np.uint64)
        self._chk(self.L.bns_build_table_device(self.h, d_bases, d_offsets, n_genomes, total_bases, d_taxid, n_buckets,
                                                d_flags, d_keys, d_vals, _p(hdr, u64p), stream), "bns_build_table_device")
        return hdr

    # ---- build session: a table that persists in the context, grows, and can start from an existing khash table
    def build_begin(self, n_buckets=0):
        """opens a session with max(4, n_buckets rounded up to a power of two) empty buckets"""
        self._chk(self.L.bns_build_begin(self.h, int(n_buckets)), "bns_build_begin")

    def build_seed(self, n_buckets, flags, keys, vals):
        """the present slots of a khash table (host arrays as load_table takes them); once, before the first build_add"""
        flags = np.ascontiguousarray(flags, dtype=np.uint32)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        vals = np.ascontiguousarray(vals, dtype=np.uint32)
        if flags.size < max(1, (int(n_buckets) + 15) >> 4) or keys.size < n_buckets or vals.size < n_buckets:
            raise ValueError("flags / keys / vals are shorter than n_buckets asks")
        self._chk(self.L.bns_build_seed(self.h, int(n_buckets), _p(flags, u32p), _p(keys, u64p), _p(vals, u32p)), "bns_build_seed")

    def build_add(self, d_bases, d_offsets, n_seqs, total_bases, d_taxid, stream=None):
        """one batch of whole sequences (device arrays, as build_table_device takes them); the table grows as it must"""
        self._chk(self.L.bns_build_add(self.h, d_bases, d_offsets, n_seqs, total_bases, d_taxid, stream), "bns_build_add")

    def build_stats(self, timing=False):
        """{batches, grows, seeded, keys} of the open session (+ add_s / grow_s with timing=True: wall seconds inside build_add, and
        the part of them spent growing)"""
        out = np.zeros(6, dtype=np.uint64)
        self._chk(self.L.bns_build_stats(self.h, _p(out, u64p)), "bns_build_stats")
        d = dict(zip(("batches", "grows", "seeded", "keys"), (int(x) for x in out[:4])))
        if timing:
            d["add_s"], d["grow_s"] = float(out[4]) * 1e-6, float(out[5]) * 1e-6
        return d

    def build_finish(self):
        """compacts, writes the flags and returns hdr, flags, keys, vals (numpy; hdr = n_buckets, n_occupied, size, upper_bound).
        The session stays open (build_stats still answers) until build_end."""
        hdr = np.zeros(4, dtype=np.uint64)
        self._chk(self.L.bns_build_finish(self.h, _p(hdr, u64p)), "bns_build_finish")
        nb = int(hdr[0])
        flags = np.zeros(max(1, nb >> 4), dtype=np.uint32); keys = np.zeros(nb, dtype=np.uint64); vals = np.zeros(nb, dtype=np.uint32)
        self._chk(self.L.bns_build_export(self.h, _p(flags, u32p), _p(keys, u64p), _p(vals, u32p)), "bns_build_export")
        return hdr, flags, keys, vals

    def build_end(self):
        self._chk(self.L.bns_build_end(self.h), "bns_build_end")

    # ---- taxonomic-depth minimizers: the session's table of all k-mers (F) thinned to the deepest-LCA k-mer of every window (M)
    def build_minimize_begin(self, w, n_buckets=0, score="depth"):
        """freezes F (build_add / build_seed are refused from here on) and opens M with max(4, n_buckets rounded up to a power of
        two) buckets; build_finish / build_end then act on M.  score: "depth" (the deepest LCA of every window) or "fewest" (the
        k-mer the fewest genomes hold: needs build_count_begin / build_count_add); an integer is handed to the library as it is"""
        if score == "depth":
            self._chk(self.L.bns_build_minimize_begin(self.h, int(w), int(n_buckets)), "bns_build_minimize_begin")
            return
        code = {"fewest": 1}.get(score, score)
        if isinstance(code, str):
            raise ValueError('score must be "depth" or "fewest"')
        self._chk(self.L.bns_build_minimize_begin_score(self.h, int(w), int(n_buckets), int(code)), "bns_build_minimize_begin_score")

    def build_minimize_add(self, d_bases, d_offsets, n_seqs, total_bases, stream=None):
        """one batch of the sequences F was built from (device arrays, as build_add takes them, without taxids)"""
        self._chk(self.L.bns_build_minimize_add(self.h, d_bases, d_offsets, n_seqs, total_bases, stream), "bns_build_minimize_add")

    def build_minimize_stats(self):
        """{batches, grows, scored_keys (in F), keys (in M), lookups (positions looked up in F), add_s}"""
        out = np.zeros(6, dtype=np.uint64)
        self._chk(self.L.bns_build_minimize_stats(self.h, _p(out, u64p)), "bns_build_minimize_stats")
        d = dict(zip(("batches", "grows", "scored_keys", "keys", "lookups"), (int(x) for x in out[:5])))
        d["add_s"] = float(out[5]) * 1e-6
        return d

    # ---- fewest-genome minimizers: per k-mer of F, the number of distinct genome ids among the sequences that hold it
    def build_count_begin(self):
        """freezes F and gives every bucket of it a zeroed count (8 more bytes a bucket until build_end)"""
        self._chk(self.L.bns_build_count_begin(self.h), "bns_build_count_begin")

    def build_count_add(self, d_bases, d_offsets, n_seqs, total_bases, genome_ids, stream=None):
        """one batch of the sequences F was built from (device arrays, as build_minimize_add takes them) and, on the HOST, the genome
        id of every sequence: non-decreasing within the call and from one call to the next, none 0xFFFFFFFF"""
        ids = np.asarray(genome_ids)
        if ids.size != int(n_seqs):
            raise ValueError("one genome id per sequence")
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) > 0xFFFFFFFF):
            raise ValueError("genome ids are uint32")
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        self._chk(self.L.bns_build_count_add(self.h, d_bases, d_offsets, int(n_seqs), int(total_bases), _p(ids, u32p), stream), "bns_build_count_add")

    def build_count(self, keys):
        """uint32 array: for every key (as the encoder emits it) the number of distinct genomes counted so far, 0 for a key F does not hold"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros(keys.size, dtype=np.uint32)
        self._chk(self.L.bns_build_count_get(self.h, _p(keys, u64p), keys.size, _p(out, u32p)), "bns_build_count_get")
        return out

    def build_count_stats(self):
        """{batches, launches (runs of one genome id), genomes (distinct ids seen), lookups, largest (count), add_s}"""
        out = np.zeros(6, dtype=np.uint64)
        self._chk(self.L.bns_build_count_stats(self.h, _p(out, u64p)), "bns_build_count_stats")
        d = dict(zip(("batches", "launches", "genomes", "lookups", "largest"), (int(x) for x in out[:5])))
        d["add_s"] = float(out[5]) * 1e-6
        return d

    # ---- window session: every window of window_len bases of every sequence, called as classify calls a read
    def windows_begin(self, window_len, pair_cap=1 << 20, confidence=0):
        """opens a session; needs table, encoder and taxonomy, and no confidence threshold on the context.  confidence (what
        set_confidence takes) is the session's own threshold: every window is called as classify calls it as a read under
        set_confidence(confidence); 0: none"""
        num, den = confidence_fraction(confidence)
        self._chk(self.L.bns_windows_begin_conf(self.h, int(window_len), int(pair_cap), num, den), "bns_windows_begin_conf")

    def windows_add(self, d_bases, d_offsets, n_seqs, total_bases, d_taxid, d_taxon=None, stream=None):
        """one batch of whole sequences (device arrays, as build_add takes them).  d_taxon (total_bases uint32, or None): the call of
        the window that starts at each base, 0xFFFFFFFF where none does.  Queued on the stream: sync() before reading d_taxon."""
        self._chk(self.L.bns_windows_add(self.h, d_bases, d_offsets, n_seqs, total_bases, d_taxid, d_taxon, stream), "bns_windows_add")

    def windows(self, reset=False):
        """bns_windows_read -> (seq_taxid uint32[n], called uint32[n], count uint64[n], n_dropped), ascending by (seq_taxid, called)"""
        n = C.c_uint64(); dropped = C.c_uint64()
        self._chk(self.L.bns_windows_read(self.h, None, None, None, 0, C.byref(n), C.byref(dropped), 0), "bns_windows_read")
        seq = np.zeros(n.value, dtype=np.uint32); called = np.zeros(n.value, dtype=np.uint32); count = np.zeros(n.value, dtype=np.uint64)
        self._chk(self.L.bns_windows_read(self.h, _p(seq, u32p), _p(called, u32p), _p(count, u64p), n.value, C.byref(n), C.byref(dropped),
                                          int(bool(reset))), "bns_windows_read")
        return seq, called, count, int(dropped.value)

    def windows_timing(self):
        """bns_windows_timing -> ({"pack_ms", "lookup_ms", "vote_ms"} summed over the adds since the last call, n_adds); the session
        must have begun with set_timing(True)"""
        ms = (C.c_double * 3)(); n = C.c_uint64()
        self._chk(self.L.bns_windows_timing(self.h, ms, C.byref(n)), "bns_windows_timing")
        return {"pack_ms": ms[0], "lookup_ms": ms[1], "vote_ms": ms[2]}, int(n.value)

    def windows_end(self):
        self._chk(self.L.bns_windows_end(self.h), "bns_windows_end")

    def classify_windows(self, bases, offsets, taxids, window_len, pair_cap=1 << 20, confidence=0):
        """host arrays through one session of its own (confidence: the session's threshold, as windows_begin takes it)
        -> (d_taxon image uint32[total_bases], (seq_taxid, called, count, n_dropped))"""
        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        taxids = np.ascontiguousarray(taxids, dtype=np.uint32)
        n_seqs, total = offsets.size - 1, int(offsets[-1])
        if taxids.size != n_seqs or bases.size < total:
            raise ValueError("one taxid per sequence, and the bases the offsets name")
        taxon = np.zeros(total, dtype=np.uint32)
        bufs = []
        self.windows_begin(window_len, pair_cap, confidence)
        try:
            for a in (bases[:total], offsets, taxids):
                bufs.append(self.dev_alloc(a.nbytes + 8))           # (the bases are read up to 8 bytes past the end)
                if a.nbytes:
                    self.dev_upload(bufs[-1], a)
            bufs.append(self.dev_alloc(taxon.nbytes + 8))
            self.windows_add(bufs[0], bufs[1], n_seqs, total, bufs[2], bufs[3])
            self.sync()
            if total:
                self.dev_download(bufs[3], taxon)
            return taxon, self.windows()
        finally:
            self.windows_end()
            for p in bufs:
                self.dev_free(p)

    def set_timing(self, on=True):
        self._chk(self.L.bns_set_timing(self.h, int(on)), "bns_set_timing")

    def last_kernel_ms(self):
        return float(self.L.bns_last_kernel_ms(self.h))

    def timing_summary(self):
        """(sum_ms, count) of the dominant-kernel launches since the last summary."""
        s = C.c_double(); n = C.c_int()
        self._chk(self.L.bns_timing_summary(self.h, C.byref(s), C.byref(n)), "bns_timing_summary")
        return s.value, n.value

    # ---- raw device buffers for hosts without a HIP binding
    def dev_alloc(self, nbytes):
        p = vp()
        self._chk(self.L.bns_dev_alloc(self.h, nbytes, C.byref(p)), "bns_dev_alloc")
        return p.value

    def dev_free(self, ptr):
        self._chk(self.L.bns_dev_free(self.h, ptr), "bns_dev_free")

    def dev_upload(self, dst, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self.L.bns_dev_upload(self.h, dst, arr.ctypes.data, arr.nbytes), "bns_dev_upload")

    def dev_download(self, src, arr):
        self._chk(self.L.bns_dev_download(self.h, arr.ctypes.data, src, arr.nbytes), "bns_dev_download")

    def dev_copy_from(self, dst, other, src, nbytes):
        """bns_dev_copy_peer: nbytes from `src` in the device memory of context `other` to `dst` in this context's (one device or two)"""
        self._chk(self.L.bns_dev_copy_peer(self.h, dst, other.h, src, nbytes), "bns_dev_copy_peer")

    def sync(self):
        self._chk(self.L.bns_dev_sync(self.h), "bns_dev_sync")
