"""The bns_classify_text calls that tests/golden/text_plan_parent.json pins: 600 simulated reads of the 5000-base synth world as
FASTQ text (about 150 KB), taken through every way a call's plan can come out -- one slice, 8 KiB slices, 8 KiB slices and a
batch per 64 records; one file or a pair; host text, an upload prefetched and entered at an offset, device text at an aligned and
an unaligned pointer; the call in two halves; run and line arrays that are too small (the roll-back); a text cut inside its last
record; a record longer than a window.  One list for the recorder, which wrote the file from bns_classify_text as it stood before
its plan moved into csrc/bns_text_plan.hpp, and for tests/test_gpu_text_plan.py, which holds today's against it."""
import ctypes as C
import zlib

import numpy as np

import bonsai_amd
import synth

DBGS = (0, 0x4000, 0x4040)                                  # BNS_DBG_SLICE_8K, and BNS_DBG_BATCH_TINY with it
KINDS = ("one", "pair", "prefetched", "device0", "device37", "defer", "runs_cap", "lines_cap", "cut", "long_record")
FIELDS = ("status", "why", "n_records", "consumed", "total_bases", "names_bytes", "n_slices", "n_launches", "n_runs_total", "lines_bytes",
          "crc_taxon", "crc_seq_len", "crc_rec_pos", "crc_names", "crc_lines", "first_half")


def cases():
    return [(kind, dbg) for kind in KINDS for dbg in DBGS]


def case_id(kind, dbg):
    return "%s,dbg=0x%x" % (kind, dbg)


def fastq_of(reads, mate=1):
    return b"".join(b"@read%d/%d\n" % (i, mate) + r.tobytes() + b"\n+\n" + b"I" * r.size + b"\n" for i, r in enumerate(reads))


def make_context(oracle):
    """-> (context with the world's table and taxonomy, {name: text})"""
    w = synth.make_world(oracle, seed=21, k=31, genome_len=5000)
    c = bonsai_amd.Context(0)
    c.set_encoder(31, None, canonicalize=True)
    c.load_table(w.n_buckets, w.flags, w.keys, w.vals)
    c.load_taxonomy(w.parent)
    reads = synth.simulate_reads(np.random.default_rng(17), w.genomes, 600, length=120)
    long_read = synth.rand_seq(np.random.default_rng(18), 20000)
    docs = {"one": fastq_of(reads), "mate2": fastq_of([r[:90 + i % 7] for i, r in enumerate(reads[::-1])], mate=2),
            "long": fastq_of(reads[:300] + [long_read] + reads[300:])}
    return c, docs


def crc(a):
    return zlib.crc32(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def fields_of(res):
    """the pinned fields of one classify_text() result"""
    runs, half = res.get("runs", []), res.get("first_half")
    return {"status": res["status"], "why": res["why"], "n_records": res["n_records"], "consumed": list(res["consumed"]),
            "total_bases": res["total_bases"], "names_bytes": sum(len(n) for n in res["names"]),
            "n_slices": res["n_slices"], "n_launches": res["n_launches"], "n_runs_total": sum(len(t) for t, _ in runs),
            "lines_bytes": res.get("lines_bytes", 0),
            "crc_taxon": crc(res["taxon"]), "crc_seq_len": crc(res["seq_len"]), "crc_rec_pos": crc(res["rec_pos"]),
            "crc_names": crc(b"\0".join(res["names"])), "crc_lines": crc(res.get("lines", b"")),
            # (a call in two halves: what the first half reported)
            "first_half": [half[k] for k in ("n_records", "consumed", "status", "total_bases", "names_bytes")] if half else None}


def run_case(c, docs, kind, dbg):
    """-> the pinned fields of every call the case makes, in order"""
    doc = docs["one"]
    c.debug_set(dbg)
    try:
        if kind == "one":
            calls = [c.classify_text(doc, trim_readno=True, want_runs=True, want_lines=True)]
        elif kind == "pair":
            calls = [c.classify_text([doc, docs["mate2"]], trim_readno=True, want_lines=True)]
        elif kind == "prefetched":
            # one upload of the whole text; the first call enters it behind the 200th record and stops at a limit, the second takes the rest
            buf = np.frombuffer(doc, dtype=np.uint8).copy()
            off = doc.index(b"@read200/")
            ptrs, sizes = (C.c_void_p * 1)(buf.ctypes.data), np.array([buf.size], dtype=np.uint64)
            c._chk(c.L.bns_text_prefetch(c.h, ptrs, sizes.ctypes.data_as(C.POINTER(C.c_uint64)), 1), "bns_text_prefetch")
            first = c.classify_text(buf[off:], trim_readno=True, want_runs=True, limit=40000)
            calls = [first, c.classify_text(buf[off + first["consumed"][0]:], trim_readno=True, want_runs=True)]
        elif kind in ("device0", "device37"):
            shift = 37 if kind == "device37" else 0
            ptr = c.dev_alloc(len(doc) + 512)
            try:
                c.dev_upload(ptr + shift, np.frombuffer(doc, dtype=np.uint8))
                calls = [c.classify_text([], trim_readno=True, want_lines=True, device_ptrs=[(ptr + shift, len(doc))])]
            finally:
                c.dev_free(ptr)
        elif kind == "defer":
            calls = [c.classify_text(doc, trim_readno=True, want_runs=True, defer=True)]
        elif kind == "runs_cap":
            calls = [c.classify_text(doc, trim_readno=True, want_runs=True, runs_cap=300)]
        elif kind == "lines_cap":
            calls = [c.classify_text(doc, trim_readno=True, want_lines=True, lines_cap=9000)]
        elif kind == "cut":
            calls = [c.classify_text(doc[:len(doc) - 37], final=False, trim_readno=True, want_runs=True)]
        elif kind == "long_record":
            calls = [c.classify_text(docs["long"], trim_readno=True)]
        else:
            raise ValueError(kind)
    finally:
        c.debug_set(0)
    return [fields_of(r) for r in calls]
