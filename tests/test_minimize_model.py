"""CPU tier of taxonomic-depth minimizer selection: the model the GPU tests compare against (tests/minimize_model.py) encodes as the
oracle does, and the committed edge world holds what those tests rely on -- windows whose k-mers differ in depth, selected keys a
Lex build would not keep, and score ties that only the k-mer value breaks."""
import numpy as np
import pytest

import build_cases as bc
import minimize_model as mm

# (name, k, gaps, w, canon): the forms of tests/test_gpu_build_minimize.py
FORMS = (
    ("k31-w50-canon", 31, None, 50, True),
    ("k31-w50-forward", 31, None, 50, False),
    ("k32-w40-canon", 32, None, 40, True),
    ("k21-w84", 21, None, 84, True),
    ("k21-w85", 21, None, 85, True),
    ("k31-w1031", 31, None, 1031, True),
    ("spaced-half-w50", 31, bc.G_HALF, 50, True),
    ("spaced-long-w80", 31, bc.G_LONG, 80, True),
    ("k31-w31", 31, None, 31, True),
)
BY_NAME = {f[0]: f for f in FORMS}


def world_of(oracle, form):
    _, k, gaps, w, _ = form
    return bc.make_edge_world(oracle, bc.SEED, mm.comb_of(k, gaps), w)


@pytest.mark.parametrize("name", [f[0] for f in FORMS])
def test_model_encodes_as_the_oracle(oracle, name):
    """the model's valid k-mers of every sequence, in order, are the oracle's unwindowed stream"""
    form = BY_NAME[name]
    _, k, gaps, w, canon = form
    wld = world_of(oracle, form)
    n = 0
    for i, s in enumerate(wld.seqs):
        km, ok = mm.position_kmers(s, k, gaps, canon)
        exp = oracle.encode(s, k, gaps=list(gaps) if gaps is not None else None, canon=canon, spaced_intended=True)
        assert np.array_equal(km[ok], exp), (name, i, len(s))
        n += int(ok.sum())
    assert n > 100000


def test_depths_are_the_chain_lengths(oracle):
    wld = bc.make_edge_world(oracle, bc.SEED, 31, 50)
    d = mm.depths(wld.parent)
    assert d[1] == 1 and len(d) == bc.N_NODES
    for t, dep in wld.depth.items():                     # (build_cases counts edges: the root is 0 there)
        assert d[t] == dep + 1
    assert max(d.values()) >= bc.CHAIN + 1
    # an id whose chain leaves the taxonomy has no depth, nor has anything below it
    par = np.full(12, mm.ABSENT, dtype=np.uint32)
    par[1] = 0; par[2] = 1; par[3] = 2; par[5] = 4; par[6] = 5; par[7] = 11
    assert mm.depths(par) == {1: 1, 2: 2, 3: 3, 5: 0, 6: 0, 7: 0}


def test_edge_world_exercises_the_rule(oracle):
    """comb 31, w 50: what the GPU tests rely on is in the committed world"""
    wld = bc.make_edge_world(oracle, bc.SEED, 31, 50)
    ks, vs, F, depth = mm.expected(oracle, wld, 31, 50)
    stats = {}
    M = mm.select(F, depth, wld.seqs, 31, 50, stats=stats)
    assert np.array_equal(mm.sorted_pairs(M)[0], ks)
    lex_keys, _, _ = bc.expected(oracle, wld, bc.BY_NAME["w50-lex-canon"])
    not_in_lex = int((~np.isin(ks, lex_keys)).sum())
    print("windows %d, mixed %d, ties %d, valid positions %d; %d keys selected of %d scored, %d of them not in the Lex db (%d keys)"
          % (stats["windows"], stats["mixed"], stats["ties"], stats["valid"], ks.size, len(F), not_in_lex, lex_keys.size))
    assert stats["mixed"] >= 1000
    assert not_in_lex >= 1000
    assert stats["ties"] * 2 > stats["windows"]
    # every value is F's, the LCA over all sequences
    assert all(F[k] == v for k, v in zip(ks.tolist(), vs.tolist()))


def test_w_at_most_the_comb_selects_everything(oracle):
    wld = bc.make_edge_world(oracle, bc.SEED, 31, 31)
    ks, vs, F, _ = mm.expected(oracle, wld, 31, 31)
    fk, fv = mm.sorted_pairs(F)
    assert np.array_equal(ks, fk) and np.array_equal(vs, fv)


def test_window_minima_against_brute_force():
    rng = np.random.default_rng(7)
    for ws in (1, 2, 5, 20, 64):
        ent = [None if rng.random() < 0.3 else (int(rng.integers(0, 4)), int(rng.integers(0, 50))) for _ in range(200)]
        got = list(mm.window_minima(ent, ws))
        exp = []
        for p in range(len(ent) - ws + 1):
            held = [e for e in ent[p:p + ws] if e is not None]
            exp.append(min(held) if held else None)
        assert got == exp
