"""GPU tier of the crafted DEFLATE streams (tests/deflate_craft.py): the three device decoders -- a member per lane with and without
the direct tables, a member per wavefront, and the wavefront decoder's mid-stream form behind bns_inflate_stream_device -- on legal
streams that zlib's encoder never writes, and on illegal ones whose status the host build has shown (tests/test_deflate_craft.py).
zlib's inflater is the reference of every text."""
import os
import subprocess
import zlib

import numpy as np
import pytest

import deflate_craft as dc
from test_gpu_cli import BIN, files  # noqa: F401  (the module's fixture: the world of the CLI tests)
from test_inflate import FORMS, gpu_gunzip, gpu_inflate, gz_ctx, inflater  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cat():
    c = dc.catalogue()
    for name, text, raw in c:
        assert zlib.decompress(raw, -15) == text, name
    return c


def check(cases, texts, crc, status):
    for i, ((name, text, _), t, cr, st) in enumerate(zip(cases, texts, crc, status)):
        assert st == 0 and t == text and int(cr) == (zlib.crc32(text) & 0xFFFFFFFF), (i, name, int(st))


@pytest.mark.parametrize("form,lut", FORMS)
def test_catalogue_as_members(inflater, monkeypatch, cat, form, lut):
    """the whole catalogue in one call (a few dozen members: few busy lanes, few wavefronts), and repeated to more than 4096 members"""
    monkeypatch.setenv("BNS_INFLATE_LUT", lut)
    monkeypatch.setenv("BNS_INFLATE_FORM", form)
    lib, h = inflater
    check(cat, *gpu_inflate(lib, h, [r for _, _, r in cat], [len(t) for _, t, _ in cat]))
    for n in (1, 2, 4, 8):                                          # 1 / 2 / 4 / 8 busy lanes
        some = [cat[(5 * n + i) % len(cat)] for i in range(n)]
        check(some, *gpu_inflate(lib, h, [r for _, _, r in some], [len(t) for _, t, _ in some]))
    reps = 4096 // len(cat) + 1
    many = [cat[(i * 7) % len(cat)] for i in range(reps * len(cat))]      # (7 and the catalogue's size: every case, neighbours that change)
    assert len(many) > 4096 and {n for n, _, _ in many} == {n for n, _, _ in cat}
    check(many, *gpu_inflate(lib, h, [r for _, _, r in many], [len(t) for _, t, _ in many]))


@pytest.mark.parametrize("form,lut", FORMS)
def test_illegal_members_among_good_ones(inflater, monkeypatch, cat, form, lut):
    """every crafted illegal stream reports the status of the host build and hurts nobody beside it"""
    monkeypatch.setenv("BNS_INFLATE_LUT", lut)
    monkeypatch.setenv("BNS_INFLATE_FORM", form)
    lib, h = inflater
    bad = dc.illegal()
    good = [c for c in cat if len(c[1]) <= 8000]
    assert len(bad) == 15 and len(good) >= 15
    sent, want = [], []
    for i in range(200):
        if i % 13 == 5:
            name, raw, status = bad[(i // 13) % len(bad)]
            sent.append((raw, 64))
            want.append((name, None, status))
        else:
            name, text, raw = good[i % len(good)]
            sent.append((raw, len(text)))
            want.append((name, text, 0))
    assert {w[0] for w in want if w[1] is None} == {b[0] for b in bad}
    texts, crc, status = gpu_inflate(lib, h, [s[0] for s in sent], [s[1] for s in sent])
    for i, (name, text, st) in enumerate(want):
        assert int(status[i]) == st, (i, name, int(status[i]))
        if text is not None:
            assert texts[i] == text and int(crc[i]) == (zlib.crc32(text) & 0xFFFFFFFF), (i, name)


@pytest.mark.parametrize("name", dc.STREAM_CASES)
def test_one_gzip_stream_on_the_device(inflater, gz_ctx, monkeypatch, name):
    """crafted gzip files through bns_inflate_stream_device with chunks of 4 KiB: whole, in pieces of 70000 compressed bytes, and with
    room for 1 MiB of text a call -- the text is zlib's, every call moves on, CRC-32 and ISIZE of every member hold (gpu_gunzip)"""
    monkeypatch.setenv("BNS_GZ_CHUNK_KB", "4")
    lib, h = inflater
    text, gz, _ = dc.stream_case(name)
    stats = []
    assert gpu_gunzip(lib, h, gz_ctx, gz, stats=stats) == text
    print(name, "whole file: (chunks, chained, stop_why, status, text bytes) per call:", stats)
    if name == "deep":
        assert stats[0][0] > 8 and stats[0][1] > 8                # the headers of deep-coded blocks are found, and the chunks chain
    assert gpu_gunzip(lib, h, gz_ctx, gz, piece=70000) == text
    assert gpu_gunzip(lib, h, gz_ctx, gz, text_cap=1 << 20) == text


def periodic_fastq(reads, reps=8):
    """FASTQ of the world's reads in groups of exactly 32768 bytes that differ in one digit of their names: 32768 back lies the same text"""
    groups = []
    for rep in range(reps):
        recs, total, i = [], 0, 0
        rec = lambda i, pad: b"@m%d_%03d/1 c%s\n%s\n+\n%s\n" % (rep, i, b"x" * pad, reads[i % 300].tobytes(), (b"@>+I" * reads[i % 300].size)[:reads[i % 300].size])
        while total + len(rec(i, 0)) <= 32768 - 700:
            recs.append(rec(i, 0))
            total += len(recs[-1])
            i += 1
        pad = 32768 - total - len(rec(i, 0))
        assert pad >= 0
        groups.append(b"".join(recs) + rec(i, pad))
        assert len(groups[-1]) == 32768
    return b"".join(groups)


def test_cli_reads_crafted_gzip_and_bgzf(files, tmp_path):
    """`bonsai classify -a` on a crafted .fq.gz and a crafted BGZF file (deep codes, blocks that open with a match 32768 back): byte for
    byte the output of the plain file, on the device's inflate paths and on the host's"""
    def cli(path, **env):
        e = dict(os.environ, BNS_CLI_TIMING="1")
        e.update({k: str(v) for k, v in env.items()})
        p = subprocess.run([BIN, "classify", "-a", files["db"], files["nodes"], path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=e)
        assert p.returncode == 0, p.stderr.decode()
        return p.stdout, p.stderr.decode()

    rng = np.random.default_rng(61)
    text = periodic_fastq(files["reads"])
    plain = str(tmp_path / "c.fq")
    open(plain, "wb").write(text)
    want, _ = cli(plain, BNS_TEXT_GPU=0)
    assert want.count(b"\n") == text.count(b"\n") // 4
    raw, census = dc.craft_stream(text, rng, deep=True, opener=True, block=(9000, 30000))
    assert census["dist_32768"] > 100 and census["ll_deep"] > 10000 and census["d_deep"] > 100
    gz = str(tmp_path / "c.fq.gz")
    open(gz, "wb").write(dc.gzip_member(raw, text))
    members = []
    for a in range(0, len(text), dc.BGZF_TEXT):
        part = text[a:a + dc.BGZF_TEXT]
        raw, census = dc.craft_stream(part, rng, deep=True, opener=True, block=(33000, 33000))
        assert census["dist_32768"] > 10 or len(part) < 40000
        members.append(dc.bgzf_member(raw, part))
    bgz = str(tmp_path / "c_bgzf.fq.gz")
    open(bgz, "wb").write(b"".join(members) + dc.BGZF_EOF)
    for path, envs in ((gz, ({}, {"BNS_GZ_CHUNK_KB": 4}, {"BNS_GZ_GPU": 0}, {"BNS_TEXT_GPU": 0})),
                       (bgz, ({}, {"BNS_BGZF_GPU": 1}, {"BNS_BGZF_GPU": 0}, {"BNS_TEXT_GPU": 0, "BNS_BGZF_GPU": 0}))):
        for env in envs:
            out, err = cli(path, **env)
            print(os.path.basename(path), env, [l for l in err.splitlines() if "on the device" in l or "on the GPU" in l or "host parser" in l or "gave up" in l])
            assert out == want, (path, env)
