"""The per-taxon tally on the device (bns_tally_enable / bns_tally_read: tally_kernel, clade_kernel) and the taxon report of
`bonsai classify -R` built on it: the Python API against np.bincount and a DFS over the synthetic taxonomy, and the CLI's report
against one restated here from the oracle's per-read taxa -- every input form, several contexts, taxa outside the taxonomy."""
import gzip
import os
import subprocess
from collections import Counter, defaultdict

import numpy as np
import pytest

import bonsai_amd
import synth
from bonsai_amd import _lib
from test_gpu_cli import BIN, files  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

RANKS = {1: "no rank", 2: "superkingdom", 3: "superkingdom", 11: "phylum", 12: "phylum", 21: "phylum", 101: "genus", 102: "genus",
         111: "genus", 201: "genus", 1001: "species", 1002: "species", 1003: "species", 1004: "species", 2001: "species", 2002: "strain"}
NAMES = {1: "root", 2: "Alpha", 3: "Beta", 11: "Alpha one", 101: "Genus a", 1001: "Species a1", 2002: "Strain b"}
LETTER = {"superkingdom": "D", "domain": "D", "kingdom": "K", "phylum": "P", "class": "C", "order": "O", "family": "F", "genus": "G",
          "species": "S"}


def expected_report(taxa, pairs=synth.TAX_PAIRS, ranks=None, names=None):
    """the report as the -R spec states it, from the units' taxa and the (child, parent) pairs of nodes.dmp"""
    ranks, names = ranks or {}, names or {}
    par = {c: (0 if c == 1 else p) for c, p in pairs}
    n = max(max(par), max(par.values())) + 1

    def chain_ok(v):
        seen = set()
        while v in par and v not in seen:
            seen.add(v)
            if par[v] == 0:
                return True
            v = par[v]
        return False

    direct = Counter(0 if t == 0 else (t if t < n and chain_ok(t) else n) for t in (int(x) for x in taxa))
    kids = defaultdict(list)
    for c, p in par.items():
        if p != 0 and chain_ok(c):
            kids[p].append(c)
    clade = {}

    def total_of(v):
        clade[v] = direct[v] + sum(total_of(k) for k in kids[v])
        return clade[v]

    roots = sorted(c for c, p in par.items() if p == 0)
    for r in roots:
        total_of(r)
    total = len(taxa)
    out = []

    def line(c, d, code, tid, depth, name):
        out.append("%6.2f\t%d\t%d\t%s\t%d\t%s%s\n" % (100.0 * c / total, c, d, code, tid, "  " * depth, name))

    if direct[0]:
        line(direct[0], direct[0], "U", 0, 0, "unclassified")

    def walk(v, depth, base, steps):
        own = "R" if v == 1 else LETTER.get(ranks.get(v, "no rank"), "")
        if own:
            base, steps = own, 0
        elif base:
            steps += 1
        line(clade[v], direct[v], base + (str(steps) if steps else "") if base else "-", v, depth, names.get(v, str(v)))
        for k in sorted((k for k in kids[v] if clade[k]), key=lambda k: (-clade[k], k)):
            walk(k, depth + 1, base, steps)

    for r in roots:
        if clade[r]:
            walk(r, 0, "", 0)
    if direct[n]:
        line(direct[n], direct[n], "-", 4294967295, 0, "(not in taxonomy)")
    return "".join(out)


def subtree_sums(direct):
    """clade[] by a DFS over synth.TAX_PAIRS (bins 0 and n as they are)"""
    kids = defaultdict(list)
    for c, p in synth.TAX_PAIRS:
        if c != 1:
            kids[p].append(c)
    clade = direct.copy()

    def dfs(v):
        s = int(direct[v]) + sum(dfs(k) for k in kids[v])
        clade[v] = s
        return s
    dfs(1)
    return clade


def fastq(reads, prefix=b"r", eol=b"\n"):
    return b"".join(b"@%s%d%s%s%s+%s%s%s" % (prefix, i, eol, r.tobytes(), eol, eol, b"I" * r.size, eol) for i, r in enumerate(reads))


def test_tally_python_api(gpu_ctx, small_world):
    w, c = small_world, gpu_ctx
    c.set_encoder(31, None, canonicalize=True)
    c.load_table(w.n_buckets, w.flags, w.keys, w.vals)
    c.load_taxonomy(w.parent)
    n = w.parent.size
    with pytest.raises(bonsai_amd.BonsaiAmdError):
        c.tally()                                                   # not enabled yet
    c.tally_enable()
    try:
        rng = np.random.default_rng(5)
        taxa = []
        for b in range(3):
            reads = synth.simulate_reads(rng, w.genomes, 400 + 100 * b, var_len=True, n_rate=0.003)
            bases, offsets = synth.concat(reads)
            taxa.append(c.classify(bases, offsets)["taxon"])
            taxa.append(c.classify(bases, offsets, paired=True)["taxon"])
            words, bw, bm = bonsai_amd.pack_reads(bases, offsets)
            taxa.append(c.classify_packed(words, bw, bm, offsets)["taxon"])
            taxa.append(c.classify_runs(bases, offsets)["taxon"])
            doc = fastq(reads)
            got = c.classify_text(doc, final=True)
            assert got["n_records"] == len(reads)
            taxa.append(got["taxon"])
            half = len(reads) // 2
            pair = c.classify_text([fastq(reads[:half]), fastq(reads[half:2 * half])], final=True, defer=True)
            assert pair["n_records"] == 2 * half
            taxa.append(pair["taxon"])
        all_taxa = np.concatenate(taxa)
        direct, clade = c.tally()
        assert direct.dtype == np.uint64 and direct.size == n + 1
        assert np.array_equal(direct, np.bincount(all_taxa, minlength=n + 1).astype(np.uint64))
        assert direct[n] == 0 and direct[0] > 0 and direct[1:n].sum() > 0
        assert np.array_equal(clade, subtree_sums(direct))
        assert clade[1] == all_taxa.size - direct[0]
        # reset: the counts read, then zeroed
        d2, _ = c.tally(reset=True)
        assert np.array_equal(d2, direct)
        d3, c3 = c.tally()
        assert not d3.any() and not c3.any()
        # text calls whose run arrays fill up end early (BNS_TEXT_CAP) and hand the batch back: it is counted once, when it is taken
        reads = synth.simulate_reads(rng, w.genomes, 3000)
        doc = fastq(reads)
        exp = c.classify(*synth.concat(reads))["taxon"]
        c.tally(reset=True)
        c.debug_set(0x4040)                                         # (many pieces, a classify launch per >= 64 records)
        try:
            pos, done, cap, capped = 0, 0, 400, 0
            while pos < len(doc):
                part = c.classify_text(doc[pos:], final=True, want_runs=True, runs_cap=cap)
                capped += part["status"] == _lib.TEXT_CAP
                assert np.array_equal(part["taxon"], exp[done:done + part["n_records"]])
                done += part["n_records"]; pos += part["consumed"][0]
                if part["n_records"] == 0:
                    cap *= 2
        finally:
            c.debug_set(0)
        assert done == len(reads) and capped > 2
        d4, _ = c.tally()
        assert np.array_equal(d4, np.bincount(exp, minlength=n + 1).astype(np.uint64))
        # a new taxonomy starts the tally again
        c.load_taxonomy(w.parent)
        assert not c.tally()[0].any()
    finally:
        c.tally_enable(False)


@pytest.fixture(scope="module")
def rep(files, oracle, tmp_path_factory):
    d = tmp_path_factory.mktemp("report")
    nodes, names = str(d / "nodes.dmp"), str(d / "names.dmp")
    with open(nodes, "w") as f:
        for ch, p in synth.TAX_PAIRS:
            f.write("%d\t|\t%d\t|\t%s\t|\t\t|\n" % (ch, p, RANKS[ch]))
    with open(names, "w") as f:
        for t, nm in NAMES.items():
            f.write("%d\t|\t%s\t|\t\t|\tscientific name\t|\n" % (t, nm))
            f.write("%d\t|\t%s synonym\t|\t\t|\tsynonym\t|\n" % (t, nm))
    w, reads = files["w"], files["reads"]
    tax1 = [oracle.classify_seq(w.table, w.tax, 31, r.tobytes())[0] for r in reads[:300]]
    tax_pair = [oracle.classify_seq(w.table, w.tax, 31, reads[i].tobytes(), reads[300 + i].tobytes())[0] for i in range(300)]
    return {"dir": d, "nodes": nodes, "names": names, "tax1": tax1, "tax_pair": tax_pair}


def run_both(opts, inputs, files, rep, tmp_path, tag, names=True, stdin=None, env=None):
    """the same run without and with -R: stdout and the -b file must not change; -> (report text, taxa of the -b file, stderr)"""
    e = dict(os.environ, **(env or {}))
    report = str(tmp_path / (tag + ".report"))
    outs = []
    for with_r in (False, True):
        tb = str(tmp_path / ("%s_%d.bin" % (tag, with_r)))
        extra = (["-R", report] + (["-n", rep["names"]] if names else [])) if with_r else []
        p = subprocess.run([BIN, "classify", "-b", tb] + extra + opts + [files["db"], rep["nodes"]] + inputs,
                           input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=e)
        assert p.returncode == 0, p.stderr.decode()
        outs.append((p.stdout, open(tb, "rb").read(), p.stderr.decode()))
    assert outs[0][0] == outs[1][0], tag
    assert outs[0][1] == outs[1][1], tag
    return open(report).read(), np.frombuffer(outs[1][1], dtype="<u4"), outs[1][2]


def test_report_input_forms(files, rep, tmp_path):
    tax1, names = rep["tax1"], NAMES
    want = expected_report(tax1, ranks=RANKS, names=names)
    assert "\tunclassified\n" in want and "\tG\t101\t" in want and "\tG1\t2002\t" in want           # (a strain right under a genus)
    r1 = files["r1"]
    text = open(r1, "rb").read()
    forms = {}
    crlf = str(tmp_path / "crlf.fq"); open(crlf, "wb").write(text.replace(b"\n", b"\r\n")); forms["crlf"] = crlf
    bg = str(tmp_path / "r1.bgzf.gz"); synth.write_bgzf(bg, text, member_sizes=[5000, 700]); forms["bgzf"] = bg
    gz = str(tmp_path / "r1.gz")
    with gzip.open(gz, "wb") as f:
        f.write(text)
    forms["gzip"] = gz
    pk = str(tmp_path / "r1.bnsp")
    p = subprocess.run([BIN, "pack", "-o", pk, "-c", "20000", r1], stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    forms["bnsp"] = pk
    got, tb, _ = run_both(["-a"], [r1], files, rep, tmp_path, "plain")
    assert tb.tolist() == tax1 and got == want
    for tag, path in forms.items():
        got, tb, _ = run_both(["-a"], [path], files, rep, tmp_path, tag)
        assert tb.tolist() == tax1 and got == want, tag
    # -K (no lines), names left out: every taxon is its id
    got, _, _ = run_both(["-K"], [r1], files, rep, tmp_path, "noname", names=False)
    assert got == expected_report(tax1, ranks=RANKS)
    # a pipe: the host reader
    got, tb, _ = run_both(["-a"], ["/dev/stdin"], files, rep, tmp_path, "pipe", stdin=text)
    assert tb.tolist() == tax1 and got == want
    # multi-line FASTA
    got, tb, _ = run_both(["-a"], [files["fa"]], files, rep, tmp_path, "fasta")
    assert got == expected_report(tax1[:50], ranks=RANKS, names=names)
    # a pair of files (one of them gzip): one unit per pair
    got, tb, _ = run_both(["-a"], [r1, files["r2"]], files, rep, tmp_path, "pair")
    assert tb.tolist() == rep["tax_pair"] and got == expected_report(rep["tax_pair"], ranks=RANKS, names=names)


def test_report_handback_and_contexts(files, rep, tmp_path):
    reads = files["reads"]
    tax1 = rep["tax1"]
    good = fastq(reads[:200], b"g")
    stray = b"stray text\n" + fastq(reads[200:260], b"s")
    hb = str(tmp_path / "handback.fq"); open(hb, "wb").write(good + stray + good)
    got, tb, err = run_both(["-a", "-c", "20000"], [hb], files, rep, tmp_path, "handback", env={"BNS_CLI_TIMING": "1", "BNS_TEXT_BLOCK_BYTES": "5000"})
    assert "host parser takes the rest" in err
    want_taxa = tax1[:200] + tax1[200:260] + tax1[:200]
    assert tb.tolist() == want_taxa and got == expected_report(want_taxa, ranks=RANKS, names=NAMES)
    # two contexts (one device twice): one tally each, summed -- plain text blocks, and the host path's chunks
    big = str(tmp_path / "big.fq")
    open(big, "wb").write(b"".join(fastq(reads[:300], b"m%d_" % k) for k in range(8)))
    want = expected_report(tax1 * 8, ranks=RANKS, names=NAMES)
    for tag, env in (("g_text", {"BNS_TEXT_BLOCK_BYTES": "40000"}), ("g_host", {"BNS_TEXT_GPU": "0"})):
        got, tb, _ = run_both(["-a", "-g", "0,0", "-c", "20000"], [big], files, rep, tmp_path, tag, env=env)
        assert tb.tolist() == tax1 * 8 and got == want, tag


def test_report_taxa_outside_the_taxonomy(files, rep, tmp_path):
    """db values that are no key of nodes.dmp (one below n, one above), and a nodes.dmp whose chain breaks: (not in taxonomy)"""
    from bonsai_amd import hostio
    d = hostio.read_db(files["db"])
    vals = d["vals"].copy()
    vals[vals == 1003] = 1500                                      # < n = 2003, not a key
    vals[vals == 1004] = 7777                                      # >= n
    assert (vals == 1500).any() and (vals == 7777).any()
    db2 = str(tmp_path / "odd.db")
    hostio.write_db(db2, 31, 31, d["gaps"], [d["n_buckets"], d["n_occupied"], d["size"], d["upper_bound"]], d["flags"], d["keys"], vals)
    broken = str(tmp_path / "broken.dmp")
    pairs_broken = [(ch, p) for ch, p in synth.TAX_PAIRS if ch != 201]     # 2001 and 2002 hang below an id that is not a key
    with open(broken, "w") as f:
        for ch, p in pairs_broken:
            f.write("%d\t|\t%d\t|\t%s\t|\t\t|\n" % (ch, p, RANKS[ch]))
    for db, nodes, pairs, tag in ((db2, rep["nodes"], synth.TAX_PAIRS, "odd_db"), (files["db"], broken, pairs_broken, "broken_chain")):
        for devs in ("0", "0,0"):
            r = str(tmp_path / ("%s_%s.report" % (tag, devs)))
            tb = str(tmp_path / ("%s_%s.bin" % (tag, devs)))
            p = subprocess.run([BIN, "classify", "-K", "-g", devs, "-c", "20000", "-b", tb, "-R", r, "-n", rep["names"], db, nodes, files["r1"]],
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
            assert p.returncode == 0, p.stderr.decode()
            taxa = np.fromfile(tb, dtype="<u4")
            got = open(r).read()
            assert got == expected_report(taxa.tolist(), pairs=pairs, ranks=RANKS, names=NAMES), (tag, devs)
            last = got.splitlines()[-1].split("\t")
            assert last[3:] == ["-", "4294967295", "(not in taxonomy)"] and int(last[1]) > 0, (tag, devs)
