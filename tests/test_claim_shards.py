"""classify_kernel's eight work counters (bonsai_amd/csrc/bns_claims.hpp, claim_shard_global), on the host: the header is
compiled with tests/helpers/claim_shards_harness.cpp, which plays the counters and draws from them the way the kernel does.

A draw d from counter x stands for global claim 8 d + x of the tiling that tests/test_claim_schedule.py checks for one counter.
Whatever the order in which the eight counters are drawn dry -- round-robin, one shard drained before the others are touched, a
seeded random order, or the kernel's own loop with its wavefronts taking turns at random -- the static claims and the claims of all
eight shards tile [0, n_units) exactly once, no claim is larger than a full one, a shard that was past the end once never hands out a
claim again, and eight dry shards mean that every unit has been given to somebody.  At 2^32 - 2^22 - 1 units and 8192 wavefronts the
draws past the end (one per wavefront and shard) must not wrap the 32-bit base."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

import claims_lib as CL

FULL = CL.FULL
WAVES = (4, 8, 8192)
BIG = 2 ** 32 - 2 ** 22 - 1
WHY = {1: "the claims do not tile [0, n_units)", 2: "an empty claim or one larger than a full one", 3: "a unit dealt out twice",
       4: "a shard that was past the end handed out a claim again", 5: "eight dry shards, and units nobody was given",
       6: "a small batch with a dynamic part", 7: "a wavefront drew more often than once per dry shard"}
_DIR = tempfile.TemporaryDirectory(prefix="bns_claim_shards_")


@pytest.fixture(scope="module")
def H():
    so = os.path.join(_DIR.name, "libclaimshards.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Werror",
                    os.path.join(CL.ROOT, "tests", "helpers", "claim_shards_harness.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.shards_drain.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64]
    L.shards_drain.restype = C.c_int
    L.shards_waves.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]
    L.shards_waves.restype = C.c_int
    return L


def sizes(W):
    """1 .. a few thousand, every size around which the deal changes shape, and the sizes at which 0, 3, 8 and 200 dynamic claims
    (and one unit either way: a cut last claim) follow the static part"""
    S = CL.stagger_total(W)
    ns = set(range(1, 3200 if W <= 8 else 400))
    for b in (30 * W, 31 * W, S, 64 * W) + tuple(S + k * FULL for k in (1, 3, 7, 8, 9, 16, 200)):
        ns |= {b + d for d in range(-2, 3) if b + d > 0}
    return sorted(ns)


def check(rc, what, n, W):
    assert rc == 0, "%s, n_units %d, %d wavefronts: %s" % (what, n, W, WHY.get(rc, rc))


@pytest.mark.parametrize("W", WAVES)
def test_drain_orders(H, W):
    checked = 0
    for n in sizes(W):
        check(H.shards_drain(n, W // 4, FULL, 0, 0, 3, 0), "round-robin", n, W)
        check(H.shards_drain(n, W // 4, FULL, 1, n % 8, 3, 0), "shard %d drained first" % (n % 8), n, W)
        check(H.shards_drain(n, W // 4, FULL, 2, 0, 3, 1400 + n), "random order", n, W)
        checked += 1
    assert checked > 300


@pytest.mark.parametrize("W", WAVES)
def test_wavefront_loop(H, W):
    """the kernel's loop: home shards by wavefront index (the debug bit) and by workgroup (an XCD each); every draw past the end
    stays within the 2^22 units the batch size leaves below 2^32"""
    over = C.c_uint64()
    most = 0
    for n in sizes(W)[:: 1 if W <= 8 else 7]:
        for by_wave in (1, 0):
            check(H.shards_waves(n, W // 4, FULL, by_wave, 99 + n, C.byref(over)), "wavefront loop", n, W)
            assert over.value < 2 ** 22
            most = max(most, over.value)
    assert most >= (8 * (W - 1) + 1) * FULL                  # every wavefront saw every shard dry: W draws past the end on each


@pytest.mark.parametrize("W", WAVES)
def test_largest_batch(H, W):
    over = C.c_uint64()
    check(H.shards_drain(BIG, W // 4, FULL, 0, 0, W, 0), "round-robin", BIG, W)
    check(H.shards_drain(BIG, W // 4, FULL, 1, 5, W, 0), "shard 5 drained first", BIG, W)
    check(H.shards_waves(BIG, W // 4, FULL, 0, 7, C.byref(over)), "wavefront loop", BIG, W)
    assert (8 * (W - 1) + 1) * FULL <= over.value <= 8 * W * FULL < 2 ** 22

