#!/usr/bin/env python3
"""The fixed synthetic genome set of profiles/build_stream.txt: N genomes of 26 contigs x 100 kb (2.6 Mb each, lines of 80), under a
taxonomy root -> 16 genera -> N species.  A genome is its genus' ancestor with 1 % of the bases substituted, so genomes of a genus
share most of their minimizers (values fold to the genus) and genera share none.  Seeded: the same bytes on every machine.

    python tools/build_stream_set.py OUTDIR [N=256]
writes OUTDIR/g000.fna .., OUTDIR/nodes.dmp, OUTDIR/nameidmap.txt and OUTDIR/paths.txt (for `bonsai build -F`)."""
import os
import sys

import numpy as np

CONTIGS, CONTIG_LEN, GENERA, SUBST = 26, 100000, 16, 0.01


def main():
    out = sys.argv[1]
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    os.makedirs(out, exist_ok=True)
    rng = np.random.default_rng(20240917)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    L = CONTIGS * CONTIG_LEN
    ancestors = [rng.integers(0, 4, size=L, dtype=np.uint8) for _ in range(GENERA)]
    with open(os.path.join(out, "nodes.dmp"), "w") as f:
        f.write("1\t|\t1\t|\tno rank\t|\t\t|\n")
        for g in range(GENERA):
            f.write("%d\t|\t1\t|\tgenus\t|\t\t|\n" % (10 + g))
        for i in range(n):
            f.write("%d\t|\t%d\t|\tspecies\t|\t\t|\n" % (1000 + i, 10 + i % GENERA))
    paths = []
    with open(os.path.join(out, "nameidmap.txt"), "w") as nm:
        for i in range(n):
            codes = ancestors[i % GENERA].copy()
            at = rng.integers(0, L, size=int(L * SUBST))
            codes[at] = (codes[at] + rng.integers(1, 4, size=at.size, dtype=np.uint8)) & 3
            text = acgt[codes].reshape(CONTIGS, CONTIG_LEN // 80, 80)
            lines = np.concatenate([text, np.full((CONTIGS, CONTIG_LEN // 80, 1), 10, dtype=np.uint8)], axis=2)
            p = os.path.join(out, "g%03d.fna" % i)
            with open(p, "wb") as f:
                for c in range(CONTIGS):
                    f.write(b">SYN_%06d.1%s synthetic contig %d\n" % (i, b"" if c == 0 else b"_%d" % (c + 1), c + 1))
                    f.write(lines[c].tobytes())
            nm.write("SYN_%06d.1\t%d\n" % (i, 1000 + i))
            paths.append(p)
    with open(os.path.join(out, "paths.txt"), "w") as f:
        f.write("\n".join(paths) + "\n")
    print("%d genomes, %d bases each, in %s" % (n, L, out))


if __name__ == "__main__":
    main()
