"""CPU tier of the crafted DEFLATE streams (tests/deflate_craft.py): legal streams that zlib's encoder never writes, and illegal ones
with a known answer.  zlib's inflater is the reference of every one; the lane decoder's host build (with and without its direct
tables) and the host's parallel gzip reader (csrc/host/pgzip.*) are what is tested.  The device's decoders get the same bytes in
tests/test_gpu_deflate_craft.py."""
import collections
import ctypes as C
import gzip
import os
import subprocess
import zlib

import numpy as np
import pytest

import deflate_craft as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_BGZF = {"blocks/stored_65535"}          # (65535 stored bytes and a header are more than a BGZF member holds)


@pytest.fixture(scope="module")
def cat():
    return dc.catalogue()


@pytest.fixture(scope="module")
def host_forms(tmp_path_factory):
    """{form: run(comp, out_len) -> (status, text, crc)}: both host builds of the lane decoder, a canary behind out[0, out_len)"""
    so = str(tmp_path_factory.mktemp("inf2") / "libinf_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "helpers", "inflate_harness.cpp"),
                    "-o", so], check=True)
    lib = C.CDLL(so)
    forms = {}
    for form in ("inf_host", "inf_host_nolut"):
        fn = getattr(lib, form)
        fn.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]

        def run(comp, n, fn=fn):
            buf = (C.c_ubyte * (n + 256))()
            C.memset(buf, 0xC5, n + 256)
            on, crc = C.c_uint32(), C.c_uint32()
            st = fn(comp, len(comp), buf, n, C.byref(on), C.byref(crc))
            raw = bytes(buf)
            assert raw[n:] == b"\xC5" * 256, "written behind out[0, out_len)"
            assert on.value <= n
            return st, raw[:on.value], crc.value
        forms[form] = run
    return forms


def test_zlib_inflates_every_case_to_its_text(cat):
    assert 25 <= len(cat) < 100 and len({n for n, _, _ in cat}) == len(cat)
    for name, text, raw in cat:
        assert zlib.decompress(raw, -15) == text, name
        assert gzip.decompress(dc.gzip_member(raw, text)) == text, name
        assert gzip.decompress(dc.gzip_member(raw, text, name=b"reads.fq")) == text, name
        if name in NOT_BGZF:
            continue
        assert len(text) <= dc.BGZF_TEXT, name
        m = dc.bgzf_member(raw, text)
        assert gzip.decompress(m + dc.BGZF_EOF) == text and int.from_bytes(m[16:18], "little") == len(m) - 1, name


def test_the_simulator_agrees_with_zlib():
    """expand() is what gives a case its text: checked on its own against zlib, overlapping matches of every distance class included"""
    rng = np.random.default_rng(12)
    toks = dc.random_tokens(rng, 70000, list(range(256)) + list(range(257, 286)), list(range(30)), p_match=0.3, run=(1, 40))
    w = dc.Writer()
    w.fixed(toks, final=True)
    assert zlib.decompress(w.getvalue(), -15) == bytes(dc.expand(toks))
    assert w.census["matches"] > 500 and w.census["dist_lt_len"] > 20


def test_code_helpers():
    for n in list(range(2, 40)) + [286]:
        assert dc.kraft(dc.flat(range(n))) == 32768
    part = {0: 1, 5: 3, 9: 15}
    full = dc.complete(part, range(20, 40))
    assert dc.kraft(full) == 32768 and all(full[s] == l for s, l in part.items()) and max(full.values()) == 15
    assert sorted(dc.ladder(list(range(16))).values()) == list(range(1, 15)) + [15, 15]
    # the canonical codes of RFC 1951 3.2.2's example: lengths (3, 3, 3, 3, 3, 2, 4, 4) -> 010 011 100 101 110 00 1110 1111
    codes = dc.canonical(dict(enumerate((3, 3, 3, 3, 3, 2, 4, 4))))
    assert [format(c, "0%db" % l)[::-1] for c, l in (codes[i] for i in range(8))] == ["010", "011", "100", "101", "110", "00", "1110", "1111"]
    for n in range(3, 259):
        assert dc.token_len(dc.match(n, 1)) == n
    assert dc.token_len(dc.match(258, 1, alt258=True)) == 258 and dc.match(258, 1, alt258=True)[0] == 284
    for d in (1, 4, 5, 24576, 24577, 32506, 32507, 32768):
        assert dc.token_dist(dc.match(3, d)) == d


def test_the_catalogue_holds_its_edge_cases():
    """the census the writer took while it wrote: none of the shapes the catalogue is there for may quietly go"""
    per = dc.catalogue_census()
    total = collections.Counter()
    for c in per.values():
        for k, v in c.items():
            total[k] = max(total[k], v) if k == "longest_run_of_matches" else total[k] + v
    for k in ("ll_deep", "d_deep", "eob_deep", "dist_gt_32506", "dist_32768", "len258_sym285", "len258_sym284", "stored", "fixed", "dynamic",
              "repeat_across_boundary", "empty_blocks"):
        assert total[k] > 0, k
    for n in range(3, 259):
        assert total["len:%d" % n] > 0, n
    for s in range(257, 286):
        assert total["lsym:%d" % s] > 0 and per["fixed/every_symbol"]["lsym:%d" % s] > 0, s
    for ds in range(30):
        for x in ("zeros", "ones"):
            assert per["every_distance"]["dsym:%d:%s" % (ds, x)] > 0 and per["fixed/every_symbol"]["dsym:%d:%s" % (ds, x)] > 0, (ds, x)
    for lo in ("fwd", "rev"):
        for do in ("fwd", "rev"):
            c = per["deep/ll_%s/d_%s" % (lo, do)]
            assert c["ll_deep"] > 300 and c["d_deep"] > 100 and c["eob_deep"] == 2 and c["len258_sym284"] > 0 and c["len258_sym285"] > 0, (lo, do, c)
            assert c["dsym:29:ones"] > 0 and c["dist_32768"] > 0 and c["ll_codes:16"] == 2 and c["dist_codes:16"] == 2
    assert per["straddle_900_1300"]["dist_900_1300"] >= 200
    assert per["dense_len3"]["longest_run_of_matches"] >= 70 and per["dense_len3"]["len:3"] >= 200
    assert per["dense_len258"]["longest_run_of_matches"] >= 70 and per["dense_len258"]["len258_sym285"] >= 200
    assert per["header/one_distance_code"]["dist_codes:1"] == 1 and per["header/one_distance_code"]["matches"] > 0
    assert per["header/no_distance_code"]["dist_codes:0"] == 1 and per["header/30_distance_codes"]["dist_codes:30"] == 1
    assert per["header/286_codes"]["ll_codes:286"] == 2 and per["header/two_symbol_code"]["ll_codes:2"] == 1
    assert per["header/repeat_across_boundary"]["repeat_across_boundary"] >= 2
    assert per["blocks/empty"]["empty_blocks"] >= 4 and per["blocks/100_one_symbol"]["one_symbol_blocks"] == 100
    assert all(per["blocks/stored_at_8_alignments"]["stored_behind_bit:%d" % b] == 2 for b in range(8)) and per["overlapping"]["dist_lt_len"] >= 30
    assert per["distance_is_position"]["matches"] == 6


def test_lane_decoder_host_build_with_and_without_direct_tables(cat, host_forms):
    for name, text, raw in cat:
        for form, run in host_forms.items():
            st, got, crc = run(raw, len(text))
            assert st == 0 and len(got) == len(text) and got == text and crc == (zlib.crc32(text) & 0xFFFFFFFF), (name, form, st)


def test_illegal_streams_have_their_status(host_forms):
    bad = dc.illegal()
    assert len(bad) == 15 and sorted({s for _, _, s in bad}) == [1, 2, 3, 4, 5]
    for name, raw, status in bad:
        with pytest.raises(zlib.error):
            zlib.decompress(raw, -15)
        for form, run in host_forms.items():
            assert run(raw, 64)[0] == status, (name, form)


def test_the_one_stream_cases_are_zlibs_and_under_8_to_1():
    """what tests/test_gpu_deflate_craft.py sends through bns_inflate_stream_device: checked here, where no device is needed"""
    for name in dc.STREAM_CASES:
        text, gz, census = dc.stream_case(name)
        assert gzip.decompress(gz) == text and 1000000 <= len(text) <= 2000000 and len(text) < 8 * len(gz), name
        if census:
            assert census["dist_32768"] > 20 or name == "one_distance_code", name
    c = dc.stream_case("deep")[2]
    assert c["ll_deep"] > 50000 and c["d_deep"] > 2000 and c["dist_codes:16"] == c["dynamic"] > 20
    c = dc.stream_case("openers")[2]
    assert c["dist_32768"] >= c["dynamic"] - 4 > 40                   # (every block behind the first 32 KiB opens with one)
    c = dc.stream_case("one_distance_code")[2]
    assert c["dist_codes:1"] == c["dynamic"] > 20
    c = dc.stream_case("stored_between")[2]
    assert all(c["stored_behind_bit:%d" % b] > 0 for b in range(8))
    assert dc.stream_case("stored_holds_gz")[2]["stored"] >= 10


# ---- the host's parallel gzip reader ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostio():
    from bonsai_amd.build import build_device_library
    build_device_library()
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bonsai_amd", "csrc", "host")], check=True)
    from bonsai_amd import hostio
    return hostio


def pgzip_files():
    """{tag: (plain text, gzip file)}: FASTQ of about 300 KB whose sequence lines come again 32768 bytes on, encoded from the text"""
    rng = np.random.default_rng(41)
    text = dc.fastq_periodic(rng, 1200)
    out = {}
    for tag, kw in (("deep", dict(deep=True)), ("opener", dict(opener=True, block=(5000, 9000))), ("small_blocks", dict(block=(300, 1500))),
                    ("stored_between", dict(stored_every=2, block=(2000, 5000), stored=(1, 700)))):
        raw, census = dc.craft_stream(text, rng, **kw)
        assert census["dist_32768"] > 1000 and (tag != "deep" or (census["ll_deep"] > 10000 and census["d_deep"] > 1000))
        assert tag != "stored_between" or census["stored"] > 20
        out[tag] = (text, dc.gzip_member(raw, text))
    cut = [0, 100003, 100003, 100259, len(text)]                   # several members: an empty one and a small one among them
    blob = b""
    for i in range(4):
        part = text[cut[i]:cut[i + 1]]
        raw, _ = dc.craft_stream(part, rng, deep=i == 3, opener=i == 0) if part else (b"\x03\x00", None)
        blob += dc.gzip_member(raw, part, name=b"part" if i == 2 else None)
    out["members"] = (text, blob)
    # gzip in stored blocks: a FASTA file one of whose records carries a complete FASTQ .gz -- real block headers, none of them a
    # boundary of the outer stream
    inner = gzip.compress(dc.fastq_periodic(np.random.default_rng(42), 1500)[17:], 6)
    fa = lambda a, b: b"".join(b">s%d\n" % i + bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 70)) + b"\n" for i in range(a, b))
    head, blobrec, tail = fa(0, 900), b">blob\n" + inner + b"\n", fa(900, 1800)
    outer = head + blobrec + tail
    w = dc.Writer()
    for p in range(0, len(head), 9000):
        dc.auto_block(w, dc.text_tokens(outer, p, min(p + 9000, len(head)), rng), extra_d=(0, 1))
    p = len(head)
    while p < len(head) + len(blobrec):
        n = min(len(head) + len(blobrec) - p, int(rng.integers(20000, 65536)))
        w.stored(outer[p:p + n])
        p += n
    for p in range(len(head) + len(blobrec), len(outer), 9000):
        q = min(p + 9000, len(outer))
        dc.auto_block(w, dc.text_tokens(outer, p, q, rng), final=q == len(outer), extra_d=(0, 1))
    assert len(inner) > 100000 and w.census["stored"] >= 2
    out["gz_in_stored"] = (outer, dc.gzip_member(w.getvalue(), outer))
    return out


def test_pgzip_reads_crafted_streams(hostio, tmp_path, monkeypatch):
    """chunks that search for headers in deep-coded blocks, blocks that open with a match 32768 back, tiny blocks, stored blocks at odd
    bits, several members -- and stored blocks full of block headers that are none of this stream's: the records are the plain text's"""
    monkeypatch.setenv("BNS_GZ_THREADS", "3")
    want = {}
    for tag, (text, blob) in pgzip_files().items():
        assert gzip.decompress(blob) == text, tag
        if id(text) not in want:
            plain = tmp_path / ("%s.txt" % tag)
            plain.write_bytes(text)
            want[id(text)] = hostio.read_fastx(str(plain))[0]
            assert len(want[id(text)]) >= 1200 and want[id(text)][-1][0] in (b"r0001199", b"s1799")      # (parsed to the end)
        p = tmp_path / ("%s.gz" % tag)
        p.write_bytes(blob)
        for chunk_bytes in (4096, 20000, 1 << 20):
            monkeypatch.setenv("BNS_PGZ_CHUNK", str(chunk_bytes))
            got, _ = hostio.read_fastx(str(p), chunk_size=1 << 18, block_bytes=0 if chunk_bytes != 20000 else 70000)
            assert got == want[id(text)], (tag, chunk_bytes)
        monkeypatch.setenv("BNS_NO_PGZ", "1")
        got, _ = hostio.read_fastx(str(p), chunk_size=1 << 18)
        assert got == want[id(text)], (tag, "one zlib stream")
        monkeypatch.delenv("BNS_NO_PGZ")
