"""The classify_kernel / classify_overflow_kernel instantiations compiled into bonsai_amd/lib/libbonsai_amd.so are exactly the
forms the dispatch rule can reach (classify_forms.image()), and exactly the forms the GPU-tier matrix runs
(classify_forms.cases()).  Nothing is compiled that the rule cannot reach; nothing reachable is missing from the matrix.  No
allow-list: an instantiation that turns out unreachable is made reachable or deleted.

Where the names come from.  Both places hold on a library built by hipcc 7 for gfx950, and both are read here with the small
ELF reader below (no llvm tool, no demangler):
  * the gfx950 code object inside the host library's .hip_fatbin section -- an uncompressed clang offload bundle -- carries one
    `<mangled name>.kd` kernel descriptor per instantiation in its symbol table.  This is the compiled device code itself and
    the set the assertions are made on;
  * the host symbol table carries one OBJECT symbol (the kernel handle the launch stub registers) per instantiation under the
    same mangled name; it must list the same set.
The template arguments are the Itanium-mangled literals after `classify_kernelI` (Lb0E, Li31E, ...), read with a regular
expression.

Also here, because it needs no device: the read set of the GPU-tier matrix puts a strict window minimum at every window
position, and at every carried ring entry in a later round, for every (k, m) of the matrix."""
import os
import re
import struct

import numpy as np
import pytest

import classify_forms as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "bonsai_amd", "lib", "libbonsai_amd.so")


# ---- a small ELF64 little-endian symbol reader -----------------------------------------------------------------------------
def elf_sections(d):
    assert d[:4] == b"\x7fELF" and d[4] == 2 and d[5] == 1, "not a little-endian ELF64 image"
    shoff, = struct.unpack_from("<Q", d, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", d, 0x3A)
    secs = []
    for i in range(shnum):
        name, typ, _flags, _addr, off, size, link, _info, _align, entsize = struct.unpack_from("<IIQQQQIIQQ", d, shoff + i * shentsize)
        secs.append({"name_off": name, "type": typ, "off": off, "size": size, "link": link, "entsize": entsize})
    strs = secs[shstrndx]
    for s in secs:
        a = strs["off"] + s["name_off"]
        s["name"] = d[a:d.index(b"\0", a)].decode()
    return secs


def elf_symbols(d):
    """[(name, type)] of every entry of .symtab and .dynsym (type: 1 OBJECT, 2 FUNC, ...)"""
    out = []
    secs = elf_sections(d)
    for s in secs:
        if s["type"] not in (2, 11):                     # SHT_SYMTAB, SHT_DYNSYM
            continue
        st = secs[s["link"]]
        for i in range(s["size"] // 24):
            name, info = struct.unpack_from("<IB", d, s["off"] + 24 * i)
            a = st["off"] + name
            out.append((d[a:d.index(b"\0", a)].decode(), info & 15))
    return out


BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def device_code_objects(d):
    """the gfx950 ELF images of the clang offload bundles in .hip_fatbin (one bundle per translation unit)"""
    fat = [s for s in elf_sections(d) if s["name"] == ".hip_fatbin"]
    assert len(fat) == 1
    base, end = fat[0]["off"], fat[0]["off"] + fat[0]["size"]
    out = []
    at = d.find(BUNDLE_MAGIC, base, end)
    assert at == base, "the fat binary does not start with an uncompressed offload bundle"
    while at >= 0:
        n, = struct.unpack_from("<Q", d, at + len(BUNDLE_MAGIC))
        p = at + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", d, p)
            triple = d[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                out.append(d[at + off:at + off + size])
        at = d.find(BUNDLE_MAGIC, at + 1, end)
    return out


ARG = r"L([bi])(n?\d+)E"
KERNEL_RE = re.compile(r"^_ZN3bns(\d+)(classify_kernel|classify_overflow_kernel)I((?:%s)+)EEv" % ARG)


def parse_instantiation(sym):
    """mangled name -> (kernel, tuple of template arguments as ints), None for any other symbol"""
    m = KERNEL_RE.match(sym)
    if not m or int(m.group(1)) != len(m.group(2)):
        return None
    args = tuple(-int(v[1:]) if v.startswith("n") else int(v) for _, v in re.findall(ARG, m.group(3)))
    return m.group(2), args


def instantiations(names):
    got = {"classify_kernel": set(), "classify_overflow_kernel": set()}
    for n in names:
        p = parse_instantiation(n)
        if p:
            got[p[0]].add(p[1])
    return got


@pytest.fixture(scope="module")
def built():
    from bonsai_amd.build import build_device_library
    build_device_library()
    d = open(SO, "rb").read()
    host = instantiations(n for n, typ in elf_symbols(d) if typ == 1)
    dev_names = []
    for co in device_code_objects(d):
        dev_names += [n[:-3] for n, typ in elf_symbols(co) if n.endswith(".kd") and typ == 1]
    return {"host": host, "device": instantiations(dev_names)}


def test_mangled_names_parse():
    assert parse_instantiation("_ZN3bns15classify_kernelILb0ELi2ELi31ELi1ELi15ELb0ELb1ELb0EEEvNS_14ClassifyParamsE") == \
        ("classify_kernel", (0, 2, 31, 1, 15, 0, 1, 0))
    assert parse_instantiation("_ZN3bns24classify_overflow_kernelILb1ELi0ELb0ELb1EEEvNS_14ClassifyParamsEPjm") == \
        ("classify_overflow_kernel", (1, 0, 0, 1))
    assert parse_instantiation("_ZN3bns30__device_stub__classify_kernelILb0ELi2ELi31ELi1ELi8ELb1ELb0ELb0EEEvNS_14ClassifyParamsE") is None
    assert parse_instantiation("_ZN3bns13encode_kernelILb0EEEvNS_14ClassifyParamsEPmPj") is None


def test_compiled_instantiations_are_the_image_of_the_rule(built):
    kern, ovf = F.image()
    dev = built["device"]
    print("compiled for gfx950: %d classify_kernel and %d classify_overflow_kernel instantiations; the rule reaches %d and %d"
          % (len(dev["classify_kernel"]), len(dev["classify_overflow_kernel"]), len(kern), len(ovf)))
    assert len(dev["classify_kernel"]) > 0 and len(dev["classify_overflow_kernel"]) > 0
    assert dev["classify_kernel"] - kern == set(), "compiled, but no call can reach it"
    assert kern - dev["classify_kernel"] == set(), "reachable, but not compiled"
    assert dev["classify_overflow_kernel"] == ovf
    assert built["host"] == dev                          # the host side's kernel handles name the same set


def test_matrix_runs_every_form():
    kern, ovf = F.image()
    cs = F.cases()
    assert len(set(cs)) == len(cs) and len({F.case_id(c) for c in cs}) == len(cs)
    forms = [F.case_forms(c) for c in cs]
    ran = {f for f, _ in forms}
    print("%d cases over %d classify_kernel forms" % (len(cs), len(ran)))
    assert kern - ran == set(), "no case of the matrix runs this form"
    assert ran - kern == set()
    # a form with the mates per unit in it has one case per mate count; the others are run single AND paired
    for f in sorted(kern):
        mates = {c.paired for c, (g, _) in zip(cs, forms) if g == f}
        assert mates == ({f[3] == 2} if f[2] else {False, True}), f
    ovf_ran = {o for c, (_, o) in zip(cs, forms) if c.world == "many"}
    assert ovf_ran == ovf
    for o in sorted(ovf):
        assert {c.paired for c, (_, g) in zip(cs, forms) if c.world == "many" and g == o} == {False, True}, o


def test_rule_examples():
    """the rule at the places the issue names: same m, same kernel; what falls back, and to what"""
    E = F.expected_form
    assert E(25, True, None, 2, 19, 32, False, False, False) == (0, 2, 25, 1, 6, 0, 0, 0)
    assert F.minimizer_len(25, 11) == F.minimizer_len(25, 8) == 19 and F.minimizer_len(25, 15) == 16
    assert [F.minimizer_len(32, s) for s in F.SPANS] == [17, 21, 24] and [F.minimizer_len(31, s) for s in F.SPANS] == [16, 20, 23]
    assert [F.minimizer_len(21, s) for s in F.SPANS] == [16, 19, 19] and [F.minimizer_len(27, s) for s in F.SPANS] == [16, 19, 19]
    assert F.minimizer_len(19, 8) == 19 and F.minimizer_len(16, 15) == 16 and F.minimizer_len(17, 15) == 16
    assert E(31, True, None, 2, 16, 52, True, False, True) == (0, 2, 31, 2, 15, 1, 1, 0)
    assert E(31, True, None, 2, 16, 32, False, True, True) == (0, 2, 31, 2, 15, 0, 0, 1)
    assert E(31, True, None, 2, 16, 32, True, True, True) == (0, 2, 0, 0, 8, 0, 0, 1)        # packed + OVC: generic
    assert E(31, True, None, 2, 16, 52, False, True, False) == (0, 2, 0, 0, 8, 0, 1, 1)      # packed + wide: generic wide
    assert E(27, True, None, 2, 16, 52, False, False, False) == (0, 2, 0, 0, 8, 0, 1, 0)
    assert E(27, True, None, 2, 16, 32, True, False, False) == (0, 2, 0, 0, 8, 0, 0, 0)
    assert E(25, False, None, 2, 19, 32, False, False, False) == (0, 2, 0, 0, 8, 0, 0, 0)    # not canonical: generic
    assert E(31, True, None, 1, 0, 0, False, False, False) == (0, 1, 0, 0, 8, 0, 0, 0)
    assert E(31, True, F.SPACED_GAPS, 2, 14, 32, True, True, True) == (1, 2, 0, 0, 8, 0, 0, 1)
    assert E(24, True, None, 2, 16, 32, False, False, True) == (0, 2, 0, 0, 8, 0, 0, 0)
    with pytest.raises(ValueError):
        E(31, True, None, 2, 19, 32, False, False, False)


def test_vectorised_window_agrees_with_kmer_buckets():
    """window_minima (numpy, what the coverage condition is computed with) against kmer_buckets (the plain restatement): the
    bucket of the window minimum it finds is the bucket kmer_buckets gives, N bases and both m-mer paths (m <= 16, m > 16)"""
    rng = np.random.default_rng(3)
    import synth
    for k, m in ((31, 16), (31, 23), (21, 19), (25, 16), (32, 17), (20, 19)):
        seq = synth.mutate(rng, synth.rand_seq(rng, 300), 0.0, 0.01)
        seq[40:60] = ord("A")
        ref = F.kmer_buckets(seq, k, m, 1 << 20)
        valid, pos, _ = F.window_minima(seq, k, m)
        h = F.mmer_hashes(seq, m)
        assert len(ref) == valid.size and [b is not None for b in ref] == list(valid)
        for j in np.flatnonzero(valid):
            x = (int(h[j + pos[j]]) * 0x9E3779B1) & F.M32
            x ^= x >> 15
            assert (int("{:032b}".format(x)[::-1], 2) << 20) >> 32 == ref[j]


def matrix_windows():
    return sorted({(c.k, c.canon, F.case_table(c)[0]) for c in F.cases()
                   if c.world == "std" and c.gaps is None and c.layout == 2 and F.case_table(c)[0] < c.k})


@pytest.mark.parametrize("k,canon,m", matrix_windows(), ids=lambda v: str(v))
def test_read_set_reaches_every_window_entry(oracle, k, canon, m):
    """A window minimum computed wrongly at ONE position of the unrolled read-back, or one carried ring entry lost between
    rounds, shows only if some k-mer's minimum sits there alone."""
    w = F.world(oracle, k, canon, None)
    reads = F.read_set(w, k - m)
    at, carried = F.window_coverage(reads, k, m)
    assert at.all(), np.flatnonzero(~at)
    assert carried.all(), np.flatnonzero(~carried)
    nk = {r.size - k + 1 for r in reads}
    assert {1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, k - m, k - m + 1} <= nk and {-k + 1, 0} <= nk
    assert any(r.size > 4096 for r in reads) and any(2048 < r.size <= 4096 for r in reads)
    assert len(reads) % 2 == 0 and any(reads[i].size != reads[i + 1].size for i in range(0, len(reads), 2))   # mates of unequal length
