"""CPU: mg_plan_beam's resample rule restated in numpy -- select (which slots survive a boundary and which survivor
each loser becomes) and lineage (the action sequence that ends in every slot) -- with known answers on hand-made values,
and the refusals of the binding and the Python wrappers that need no device.  tests/test_beam.py compares the device
with these two functions.
"""
import ctypes

import numpy as np
import pytest

import magical_amd
from magical_amd import native


def select(values, survivors):
    """parents i32[K, n] of values f64[K, n]: per env the `survivors` slots with the highest value survive, the lower k
    first among equal values, and are their own parents; loser j, in ascending k, gets survivor j mod survivors, in
    ascending k"""
    values = np.asarray(values, dtype=np.float64)
    K, n = values.shape
    parents = np.empty((K, n), dtype=np.int32)
    for e in range(n):
        ranked = sorted(range(K), key=lambda k: (-values[k, e], k))
        surv = sorted(ranked[:survivors])
        losers = [k for k in range(K) if k not in surv]
        parents[surv, e] = surv
        for j, k in enumerate(losers):
            parents[k, e] = surv[j % survivors]
    return parents


def lineage(actions, parents, seg):
    """plans u8[H, K, n]: slot k applies its own actions in every segment, and at boundary d (after step (d + 1) * seg)
    takes over the history of parents[d][k]"""
    actions = np.asarray(actions)
    H, K, n = actions.shape
    plans = actions.copy()
    e = np.arange(n)[None, :]
    for d in range(len(parents)):
        h1 = (d + 1) * seg
        plans[:h1] = plans[:h1][:, np.asarray(parents[d], dtype=np.int64), e]
    return plans


def col(*v):
    return np.array(v, dtype=np.float64)[:, None]


def test_tie_across_the_boundary_keeps_the_lower_slot():
    # ranked: slot 3 (0.9), then slots 1 and 4 tied at 0.5: slot 1 survives, 4 does not
    p = select(col(0.1, 0.5, 0.2, 0.9, 0.5), 2)
    assert p[:, 0].tolist() == [1, 1, 3, 3, 1]   # losers 0, 2, 4 <- survivors 1, 3, 1
    # -0.0 and 0.0 are one value
    assert select(col(-0.0, 0.0, 1.0), 2)[:, 0].tolist() == [0, 0, 2]


def test_all_equal_values_keep_the_first_slots():
    p = select(np.zeros((7, 3)), 3)
    for e in range(3):
        assert p[:, e].tolist() == [0, 1, 2, 0, 1, 2, 0]


def test_every_slot_survives():
    v = np.random.RandomState(0).rand(6, 4)
    assert np.array_equal(select(v, 6), np.arange(6, dtype=np.int32)[:, None].repeat(4, axis=1))


def test_one_survivor_fills_every_slot():
    v = np.array([[0.1, 0.7], [0.9, 0.7], [0.3, 0.2]])
    assert select(v, 1).tolist() == [[1, 0], [1, 0], [1, 0]]


def test_envs_are_independent_and_parents_are_survivors():
    v = np.random.RandomState(1).randint(0, 3, (9, 5)).astype(np.float64)   # many ties
    p = select(v, 4)
    for e in range(5):
        surv = sorted(set(p[:, e].tolist()))
        assert len(surv) == 4 and all(p[s, e] == s for s in surv)
        assert min(v[s, e] for s in surv) >= max([v[k, e] for k in range(9) if k not in surv])
        assert np.array_equal(select(v[:, e:e + 1], 4)[:, 0], p[:, e])


def test_lineage():
    H, K, n, seg = 5, 3, 2, 2
    a = np.arange(H * K * n, dtype=np.uint8).reshape(H, K, n)
    ident = np.arange(K, dtype=np.int32)[:, None].repeat(n, axis=1)
    assert np.array_equal(lineage(a, [ident, ident], seg), a)
    assert np.array_equal(lineage(a, [], seg), a)
    p0 = np.array([[0, 1], [0, 1], [2, 1]], dtype=np.int32)   # env 0: slot 1 <- 0; env 1: slots 0, 2 <- 1
    p1 = np.array([[2, 0], [1, 1], [2, 2]], dtype=np.int32)   # env 0: slot 0 <- 2; env 1: unchanged
    got = lineage(a, [p0, p1], seg)
    assert np.array_equal(got[4], a[4])                        # the last segment is every slot's own
    assert got[:2, 1, 0].tolist() == a[:2, 0, 0].tolist() and got[2:, 1, 0].tolist() == a[2:, 1, 0].tolist()
    assert got[:4, 0, 0].tolist() == a[:4, 2, 0].tolist()      # slot 0 took slot 2's whole history at boundary 1
    assert got[:2, 2, 1].tolist() == a[:2, 1, 1].tolist() and got[2:, 2, 1].tolist() == a[2:, 2, 1].tolist()


def test_binding_declares_the_call():
    lib = native.load()
    assert [f for f, _ in native.mg_plan_beam_out._fields_] == ["best", "best_value", "first_action", "best_plan", "values",
                                                                "steps", "errors", "depth_values", "parents"]
    assert len(lib.mg_plan_beam.argtypes) == 10
    # refused on the host, before any GPU call: nothing is launched for a null handle
    assert lib.mg_plan_beam(None, None, None, 4, 2, 2, 1, None, None, None) == -22
    assert b"mg_plan_beam" in lib.mg_last_error()


def test_policy_refuses_bad_arguments_without_an_env():
    ok = dict(horizon=8, candidates=4, seg=2, survivors=2)
    p = magical_amd.BeamPolicy(None, **ok)
    assert (p.horizon, p.candidates, p.seg, p.survivors, p.repeat, p.t) == (8, 4, 2, 2, 1, 0)
    for bad in (dict(horizon=0), dict(candidates=0), dict(seg=0), dict(seg=9), dict(survivors=0), dict(survivors=5),
                dict(repeat=0), dict(objective=3)):
        with pytest.raises(ValueError):
            magical_amd.BeamPolicy(None, **dict(ok, **bad))
    assert magical_amd.BeamPolicy(None, objective="peak", **ok).objective == magical_amd.Objective("peak")
