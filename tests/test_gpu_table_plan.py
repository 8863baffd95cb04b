"""What a table load of the golden db decides, against tests/golden/table_plan_parent.json: the same cases (tests/table_plan_cases.py)
recorded by tools/make_table_plan_golden.py from the loader as it was before its decisions moved into csrc/bns_table_plan.hpp.
Bucket count, minimizer length, identity, window, fill, key count and table bytes are functions of the request and of counts that
do not depend on the order atomics land in; spilled / overflow keys are not pinned."""
import json
import os

import numpy as np
import pytest

import table_plan_cases as T

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def CL():
    return np.load(os.path.join(GOLD, "classify_ref.npz"))


@pytest.fixture(scope="module")
def pinned():
    with open(os.path.join(GOLD, "table_plan_parent.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("layout,streamed,enc", T.groups())
def test_table_plan_is_the_parents(CL, pinned, layout, streamed, enc):
    got = T.load_group(CL, layout, streamed, enc)
    assert len(got) == 36
    bad = {cid: (v, pinned["cases"][cid]) for cid, v in got.items() if [v[f] for f in pinned["fields"]] != pinned["cases"][cid]}
    assert not bad, "%d of %d cases differ (got, pinned): %s" % (len(bad), len(got), sorted(bad.items())[:3])
