"""CPU: the host side of the rollout objectives (mg_lookahead_obj / mg_plan_obj / mg_plan_cem_obj) -- the definitions of
RETURN and PEAK restated in numpy and pinned by hand-worked cases, the header's new structs against the binding, the
Objective value type, and how the policies and the single env pass an objective on.

`objective_values` is the reference tests/test_objective.py holds the kernel to, bit for bit: numpy float64 scalar
arithmetic is one rounded IEEE double operation per operator, in the order the header states them.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import magical_amd
from magical_amd import envs, native, planning
from magical_amd.pipeline import PipelinedVecEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# the definition in numpy
def objective_values(s, r, done_n, gamma, tail):
    """s = [s_0 .. s_n], r = [r_1 .. r_n] -> (G, P, kp) of one rollout, as include/magical_sim.h defines them"""
    s, r = np.asarray(s, dtype=np.float64), np.asarray(r, dtype=np.float64)
    n = len(r)
    assert len(s) == n + 1
    gamma, tail = np.float64(gamma), np.float64(tail)
    g = np.float64(1.0)
    G, P, kp = np.float64(0.0), s[0], 0
    for k in range(1, n + 1):
        G = G + g * r[k - 1]        # g_{k-1} * r_k
        g = g * gamma               # g_k
        v = g * s[k]
        if v > P:
            P, kp = v, k
    if not (n >= 1 and done_n):
        G = G + (g * tail) * s[n]
    return float(G), float(P), int(kp)


def test_hand_worked_return_and_peak():
    # n = 0: nothing simulated.  G is the tail term alone, P the entry score
    assert objective_values([0.25], [], False, 0.5, 0.0) == (0.0, 0.25, 0)
    assert objective_values([0.25], [], False, 0.5, 2.0) == (0.5, 0.25, 0)
    assert objective_values([0.25], [], True, 0.5, 2.0) == (0.5, 0.25, 0)   # done_n means nothing without a step
    # gamma = 1, no termination: rewards 0.5, 0.25, 1.0; the tail adds tail * s_3
    s, r = [0.0, 0.5, 0.75, 0.25], [0.5, 0.25, 1.0]
    assert objective_values(s, r, False, 1.0, 0.0) == (1.75, 0.75, 2)
    assert objective_values(s, r, False, 1.0, 1.0) == (2.0, 0.75, 2)
    # gamma = 0.5 (every product exact): G = 0.5 + 0.5 * 0.25 + 0.25 * 1.0 = 0.875, tail: + (0.125 * 2) * 0.25;
    # v = 0.25, 0.1875, 0.03125: the peak moves to the earlier step
    assert objective_values(s, r, False, 0.5, 0.0) == (0.875, 0.25, 1)
    assert objective_values(s, r, False, 0.5, 2.0) == (0.9375, 0.25, 1)
    # termination at k = n: the terminal reward is the score there and no tail is added
    s, r = [0.0, 0.0, 0.5], [0.0, 0.5]
    assert objective_values(s, r, True, 1.0, 1.0) == (0.5, 0.5, 2)
    assert objective_values(s, r, True, 0.5, 8.0) == (0.25, 0.125, 2)
    # a sparse env that is not done pays nothing: tail = 1, gamma = 1 is s_n itself
    assert objective_values(s, [0.0, 0.0], False, 1.0, 1.0) == (0.5, 0.5, 2)
    # ties in PEAK go to the earliest k -- the entry state included
    assert objective_values([0.5, 1.0, 0.0, 1.0], [0, 0, 0], False, 1.0, 0.0)[1:] == (1.0, 1)
    assert objective_values([1.0, 1.0, 1.0], [0, 0], False, 1.0, 0.0)[1:] == (1.0, 0)
    assert objective_values([0.0, 0.0, 0.0], [0, 0], False, 0.5, 0.0)[1:] == (0.0, 0)
    # a negative dense reward: G may be negative, P never is (scores lie in [0, 1])
    assert objective_values([0.0, 0.0], [-0.25], False, 1.0, 0.0) == (-0.25, 0.0, 0)


def test_sequential_products_not_powers():
    """g_k is the running product, rounded at every step: 0.9 ** 3 differs from 0.9 * 0.9 * 0.9 in the last place"""
    g = np.float64(0.9) * np.float64(0.9) * np.float64(0.9)
    G, P, kp = objective_values([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0], False, 0.9, 1.0)
    assert P == float(g) and kp == 3 and G == float((g * np.float64(1.0)) * np.float64(1.0))


# ---------------------------------------------------------------------------------------------------------------------
# header and binding
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "magical_sim.h")).read(), flags=re.S)


def _structs(src):
    return {name: [" ".join(d.split()) for d in body.split(";") if d.strip()]
            for body, name in re.findall(r"typedef struct \{(.*?)\}\s*(\w+);", src, flags=re.S)}


def test_header_declares_the_structs_and_calls():
    src = _header()
    st = _structs(src)
    assert st["mg_objective"] == ["int32_t kind", "int32_t reserved", "double gamma", "double tail"]
    assert st["mg_objective_out"] == ["double *value", "double *peak", "int32_t *peak_step", "double *score_trace",
                                      "double *reward_trace"]
    kinds = re.search(r"enum \{ MG_OBJ_FINAL = (\d), MG_OBJ_RETURN = (\d), MG_OBJ_PEAK = (\d) \};", src)
    assert kinds and [int(x) for x in kinds.groups()] == [native.OBJ_FINAL, native.OBJ_RETURN, native.OBJ_PEAK] == [0, 1, 2]
    args = lambda fn: [" ".join(a.split()) for a in re.search(r"int %s\((.*?)\);" % fn, src, flags=re.S).group(1).split(",")]  # noqa: E731
    assert args("mg_lookahead_obj") == ["mg_sim *sim", "const uint8_t *actions_dev", "int32_t H",
                                        "const mg_objective *objective", "const mg_lookahead_out *out",
                                        "const mg_objective_out *obj_out", "void *stream"]
    assert args("mg_plan_obj") == ["mg_sim *sim", "const uint8_t *actions_dev", "int32_t H", "int32_t K",
                                   "const mg_objective *objective", "const mg_plan_out *out", "void *stream"]
    # mg_plan_cem's arguments with the objective in front of the outputs
    base, obj = args("mg_plan_cem"), args("mg_plan_cem_obj")
    assert obj == base[:-2] + ["const mg_objective *objective"] + base[-2:]
    # additions only: the calls the objectives build on are declared as they were
    assert args("mg_lookahead") == ["mg_sim *sim", "const uint8_t *actions_dev", "int32_t H", "const mg_lookahead_out *out",
                                    "void *stream"]


def test_struct_layouts_match_the_header():
    """mg_objective: two i32 then two f64, no padding, 24 bytes; mg_objective_out: five pointers"""
    o = native.mg_objective
    assert [(f, t) for f, t in o._fields_] == [("kind", ctypes.c_int32), ("reserved", ctypes.c_int32),
                                               ("gamma", ctypes.c_double), ("tail", ctypes.c_double)]
    assert ctypes.sizeof(o) == 24 and (o.kind.offset, o.reserved.offset, o.gamma.offset, o.tail.offset) == (0, 4, 8, 16)
    oo = native.mg_objective_out
    assert [f for f, _ in oo._fields_] == ["value", "peak", "peak_step", "score_trace", "reward_trace"]
    assert all(t is ctypes.c_void_p for _, t in oo._fields_)
    assert ctypes.sizeof(oo) == 5 * ctypes.sizeof(ctypes.c_void_p)


def test_binding_declares_the_calls():
    for fn in ("mg_lookahead_obj", "mg_plan_obj", "mg_plan_cem_obj"):
        assert fn in native.EXPORTS
    lib = native.load()
    vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
    f = lib.mg_lookahead_obj
    assert f.argtypes[:3] == [vp, vp, i32] and f.argtypes[6] is vp and len(f.argtypes) == 7 and f.restype is i32
    assert [a._type_ for a in f.argtypes[3:6]] == [native.mg_objective, native.mg_lookahead_out, native.mg_objective_out]
    f = lib.mg_plan_obj
    assert f.argtypes[:4] == [vp, vp, i32, i32] and f.argtypes[6] is vp and len(f.argtypes) == 7 and f.restype is i32
    assert [a._type_ for a in f.argtypes[4:6]] == [native.mg_objective, native.mg_plan_out]
    f, base = lib.mg_plan_cem_obj, lib.mg_plan_cem
    assert f.argtypes[:12] == base.argtypes[:12] == [vp, vp, vp] + [i32] * 7 + [u64, u64]
    assert f.argtypes[12]._type_ is native.mg_objective and f.argtypes[13:] == base.argtypes[12:] and f.restype is i32
    # refused on the host, before any GPU call: a null objective, and each invalid one, with a null sim
    assert lib.mg_lookahead_obj(None, None, 1, None, None, None, None) == -22 and b"objective" in lib.mg_last_error()
    assert lib.mg_plan_obj(None, None, 1, 1, None, None, None) == -22
    assert lib.mg_plan_cem_obj(None, None, None, 0, 1, 1, 1, 1, 1, 1, 0, 0, None, None, None) == -22
    for bad, word in INVALID:
        o = native.mg_objective(**dict(dict(kind=1, reserved=0, gamma=1.0, tail=0.0), **bad))
        assert lib.mg_lookahead_obj(None, None, 1, ctypes.byref(o), None, None, None) == -22, bad
        assert word in lib.mg_last_error(), (bad, lib.mg_last_error())
    ok = native.mg_objective(kind=2, reserved=0, gamma=1.0, tail=0.0)
    assert lib.mg_lookahead_obj(None, None, 1, ctypes.byref(ok), None, None, None) == -22
    assert b"null sim" in lib.mg_last_error()   # a valid objective: refused for what mg_lookahead refuses


# what the C ABI refuses in an objective (tests/test_objective.py sends the same list to a live sim)
INVALID = [({"kind": -1}, b"kind"), ({"kind": 3}, b"kind"), ({"reserved": 1}, b"reserved"),
           ({"gamma": 0.0}, b"gamma"), ({"gamma": -0.5}, b"gamma"), ({"gamma": 1.0000001}, b"gamma"),
           ({"gamma": float("nan")}, b"gamma"), ({"gamma": float("inf")}, b"gamma"),
           ({"tail": -1.0}, b"tail"), ({"tail": float("inf")}, b"tail"), ({"tail": float("nan")}, b"tail")]


# ---------------------------------------------------------------------------------------------------------------------
# the Python surface
def test_objective_value_type():
    assert magical_amd.Objective is planning.Objective and "Objective" in magical_amd.__all__
    o = magical_amd.Objective()
    assert (o.kind, o.gamma, o.tail, o.kind_id) == ("final", 1.0, 0.0, 0)
    p = magical_amd.Objective("peak", gamma=0.9)
    assert (p.kind, p.gamma, p.tail, p.kind_id) == ("peak", 0.9, 0.0, 2)
    assert magical_amd.Objective("return", 1, 1).kind_id == 1
    assert p == magical_amd.Objective(kind="peak", gamma=0.9, tail=0.0) and p != o and hash(p) == hash(magical_amd.Objective("peak", 0.9))
    assert "peak" in repr(p) and "0.9" in repr(p)
    with pytest.raises(AttributeError):
        p.gamma = 0.5
    for kw in [dict(kind="best"), dict(kind=1), dict(kind=None), dict(gamma=0.0), dict(gamma=-0.1), dict(gamma=1.5),
               dict(gamma=float("nan")), dict(gamma="x"), dict(gamma=None), dict(tail=-1.0), dict(tail=float("inf")),
               dict(tail=float("nan"))]:
        with pytest.raises(ValueError):
            magical_amd.Objective(**kw)
    assert planning.as_objective(None, "f") is None and planning.as_objective(p, "f") is p
    assert planning.as_objective("return", "f") == magical_amd.Objective("return")
    for bad in (1, 0.9, ("peak", 0.9), "best"):
        with pytest.raises(ValueError):
            planning.as_objective(bad, "f")


def test_every_surface_takes_the_objective():
    import inspect
    for cls in (envs.VecMagicalEnv, PipelinedVecEnv, envs.MagicalEnv):
        for fn in ("lookahead", "plan", "plan_cem"):
            p = inspect.signature(getattr(cls, fn)).parameters
            assert "objective" in p and p["objective"].default is None, (cls.__name__, fn)
        p = inspect.signature(cls.lookahead).parameters
        assert "trace" in p and p["trace"].default is False, cls.__name__
    for cls in (planning.ShootingPolicy, planning.CEMPolicy):
        p = inspect.signature(cls.__init__).parameters
        assert p["objective"].default is None, cls.__name__


class StubEnv:
    """records how the policies call plan / plan_cem"""
    num_envs = 3

    def __init__(self):
        self.calls = []

    def sample_plans(self, H, K, repeat=1, key=42, step=0, out=None):
        return torch.ones((H, K, self.num_envs), dtype=torch.uint8)

    def plan(self, actions, details=False, **kw):
        self.calls.append(("plan", kw))
        return {"best": torch.zeros(self.num_envs, dtype=torch.int32), "first_action": actions[0, 0]}

    def plan_cem(self, H, K, iters, elites, alpha=1, repeat=1, key=42, step=0, weights=None, details=False, **kw):
        self.calls.append(("plan_cem", kw))
        return {"first_action": torch.ones(self.num_envs, dtype=torch.uint8),
                "weights": torch.ones((H, 18, self.num_envs), dtype=torch.int16).view(torch.uint16)}


def test_policies_pass_the_objective_on():
    env, o = StubEnv(), magical_amd.Objective("peak", 0.9)
    planning.ShootingPolicy(env, 4, 3)()
    planning.ShootingPolicy(env, 4, 3, objective=o)()
    planning.ShootingPolicy(env, 4, 3, objective="return")()
    planning.CEMPolicy(env, 4, 3, 2, 1)()
    planning.CEMPolicy(env, 4, 3, 2, 1, objective=o)()
    # without an objective the policies call plan() / plan_cem() exactly as they did
    assert env.calls == [("plan", {}), ("plan", {"objective": o}), ("plan", {"objective": magical_amd.Objective("return")}),
                         ("plan_cem", {}), ("plan_cem", {"objective": o})]
    with pytest.raises(ValueError):
        planning.ShootingPolicy(env, 4, 3, objective=0.9)
    with pytest.raises(ValueError):
        planning.CEMPolicy(env, 4, 3, 2, 1, objective=2)
