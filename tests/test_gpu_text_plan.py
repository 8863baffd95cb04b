"""bns_classify_text against tests/golden/text_plan_parent.json: the calls of tests/text_plan_cases.py, recorded (twice, only what
agreed was kept: everything did) from the entry point as it was before its plan moved into csrc/bns_text_plan.hpp.  Status, why,
where each stream stopped, how many slices and classify launches the call made, run and line totals and a CRC of every result
array: what a call decides shows in them, whatever path it takes."""
import json
import os

import pytest

import text_plan_cases as T

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLD, "text_plan_parent.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def ctx_docs(oracle):
    c, docs = T.make_context(oracle)
    yield c, docs
    c.close()


@pytest.mark.parametrize("kind,dbg", T.cases(), ids=[T.case_id(*c) for c in T.cases()])
def test_text_call_is_the_parents(ctx_docs, pinned, kind, dbg):
    c, docs = ctx_docs
    got = T.run_case(c, docs, kind, dbg)
    want = pinned["cases"][T.case_id(kind, dbg)]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        bad = {f: (g[f], w[f]) for f in w if g[f] != w[f]}
        assert not bad, "call %d differs (got, pinned): %s" % (i, bad)
