#!/usr/bin/env python3
"""Writes tests/golden/table_plan_parent.json: what a table load of the golden db decides in every case of
tests/table_plan_cases.py.  Run on a GPU from the commit whose loader is to be pinned; the committed file came from the last
commit before the decisions moved into csrc/bns_table_plan.hpp.  Every case is loaded twice: a field that differs between the
two runs is not a function of the request alone and is dropped (and named on stdout).

    python tools/make_table_plan_golden.py [out.json]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import table_plan_cases as T   # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "table_plan_parent.json")
    CL = np.load(os.path.join(ROOT, "tests", "golden", "classify_ref.npz"))
    runs = []
    for _ in range(2):
        cases = {}
        for layout, streamed, enc in T.groups():
            cases.update(T.load_group(CL, layout, streamed, enc))
        runs.append(cases)
    unstable = sorted({f for cid in runs[0] for f in T.FIELDS if runs[0][cid][f] != runs[1][cid][f]})
    for f in unstable:
        print("dropped (differs between two runs):", f)
    fields = [f for f in T.FIELDS if f not in unstable]
    doc = {"fields": fields, "cases": {cid: [v[f] for f in fields] for cid, v in runs[0].items()}}
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote %s: %d cases, fields %s" % (out, len(doc["cases"]), ",".join(fields)))


if __name__ == "__main__":
    main()
