"""bns_set_min_hit_groups on a caller's stream: the scenario of tests/test_gpu_caller_stream.py (late input A over a poison P on a busy
stream of the caller's, tests/stream_lib.py) with the filter on.  The pack of the ASCII input and hit_groups_kernel must run on the
caller's stream behind the classify kernel: a step anywhere else reads P's bases, or P's records."""
import numpy as np
import pytest

import hit_groups_ref as HG
from test_gpu_caller_stream import LAYOUT_MINBUCKET, READ_LEN, check_units, classify_call, env, expect_classify  # noqa: F401  (env: the module's fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("paired", [False, True], ids=["single", "paired"])
def test_classify_device_min_hit_groups(env, paired):  # noqa: F811
    e, b, w, c = env, env.batch, env.w, env.ctx
    e.table(LAYOUT_MINBUCKET)
    exp = expect_classify(e.oracle, w, "A", e.reads_a, paired)
    g, found = HG.groups_of(e.oracle, w.table, e.reads_a, paired, 31)
    assert found.tolist() == exp["n_hits"].tolist()
    # N = the median G of the classified units (at most 64): about half of them fall below it
    n = int(min(64, np.median(g[exp["taxon"] != 0])))
    taxon = HG.apply(exp["taxon"], g, n)
    changed = int((taxon != exp["taxon"]).sum())
    assert n >= 2 and changed >= len(g) // 10 and np.count_nonzero(taxon) >= len(g) // 10
    # the poison's own answer differs: a pass that saw P's image would show
    exp_p = expect_classify(e.oracle, w, "P", e.reads_p, paired)
    g_p, _ = HG.groups_of(e.oracle, w.table, e.reads_p, paired, 31)
    assert float((HG.apply(exp_p["taxon"], g_p, n) != taxon).mean()) >= 0.5
    c.set_min_hit_groups(n)
    try:
        outs = b.outs(e, paired)
        call = classify_call(e, b, paired, READ_LEN, outs)
        e.late.warm(b.fills, outs, call)
        got = e.late.run(b.fills, outs, call)
        check_units(got, exp, b.offsets, 2 if paired else 1, taxon=taxon)
        if not paired:
            assert e.late.busy_at_return                                 # (no read-back: the whole call was queued inside the delay)
    finally:
        c.set_min_hit_groups(0)
        e.torch.cuda.synchronize()
