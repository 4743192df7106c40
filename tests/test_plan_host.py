"""CPU: the host side of mg_plan / mg_plan_sample -- header, ctypes binding, build units, ShootingPolicy's counter
arithmetic, plan()'s shape checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import magical_amd
from magical_amd import build, envs, native, planning

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("best", "int32_t"), ("best_score", "double"), ("first_action", "uint8_t"), ("scores", "double"),
          ("steps", "int32_t"), ("errors", "int32_t")]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "magical_sim.h")).read(), flags=re.S)


def test_header_declares_the_calls_the_outputs_and_the_cap():
    src = _header()
    body = {name: b for b, name in re.findall(r"typedef struct \{(.*?)\}\s*(\w+);", src, flags=re.S)}["mg_plan_out"]
    decls = [re.match(r"(\w+)\s*\*\s*(\w+)$", d.strip()).groups() for d in body.split(";") if d.strip()]
    assert [(n, t) for t, n in decls] == FIELDS
    args = lambda fn: [" ".join(a.split()) for a in re.search(r"int %s\((.*?)\);" % fn, src, flags=re.S).group(1).split(",")]  # noqa: E731
    assert args("mg_plan") == ["mg_sim *sim", "const uint8_t *actions_dev", "int32_t H", "int32_t K",
                               "const mg_plan_out *out", "void *stream"]
    assert args("mg_plan_sample") == ["mg_sim *sim", "uint8_t *actions_dev", "int32_t H", "int32_t K", "int32_t repeat",
                                      "uint64_t key", "uint64_t step", "void *stream"]
    cap = re.search(r"#define\s+MG_PLAN_MAX_ROLLOUTS\s+(\d+)", src)
    assert cap and int(cap.group(1)) == 262144 == native.PLAN_MAX_ROLLOUTS


def test_binding_matches_the_header():
    assert "mg_plan" in native.EXPORTS and "mg_plan_sample" in native.EXPORTS
    assert [f for f, _ in native.mg_plan_out._fields_] == [f for f, _ in FIELDS]
    assert all(t is ctypes.c_void_p for _, t in native.mg_plan_out._fields_)
    assert ctypes.sizeof(native.mg_plan_out) == 6 * ctypes.sizeof(ctypes.c_void_p)
    lib = native.load()
    vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
    fn = lib.mg_plan
    assert fn.argtypes[:4] == [vp, vp, i32, i32] and fn.argtypes[5] is vp and len(fn.argtypes) == 6
    assert fn.argtypes[4]._type_ is native.mg_plan_out and fn.restype is i32
    assert lib.mg_plan_sample.argtypes == [vp, vp, i32, i32, i32, u64, u64, vp] and lib.mg_plan_sample.restype is i32
    # refused on the host, before any GPU call: nothing is launched for a null handle
    assert fn(None, None, 1, 1, None, None) == -22 and lib.mg_last_error() != b""
    assert lib.mg_plan_sample(None, None, 1, 1, 1, 0, 0, None) == -22


def test_build_lists_the_plan_unit():
    assert "mg_plan.hip" in build.UNITS
    for h in build.UNITS["mg_plan.hip"]:
        assert os.path.exists(os.path.join(build.CSRC, h)), h
    assert {"mg_plan.h", "mg_philox.h"} <= set(build.UNITS["mg_plan.hip"]) and {"mg_plan.h", "mg_philox.h"} <= set(build.UNITS["mg_sim.hip"])
    assert sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip")) == sorted(build.UNITS)
    # the rollouts are the lookahead kernel as it is: the plan unit defines no rollout kernel of its own
    src = open(os.path.join(build.CSRC, "mg_plan.hip")).read()
    assert "mg_stepk.h" not in src and "mg_lookahead.h" not in src


class StubEnv:
    """records sample_plans / plan calls; candidate k's first action for every env is k + 1, the best is always the last"""
    num_envs = 3

    def __init__(self):
        self.calls = []

    def sample_plans(self, H, K, repeat=1, key=42, step=0, out=None):
        self.calls.append(("sample", H, K, repeat, key, step))
        return torch.arange(1, K + 1, dtype=torch.uint8)[None, :, None].expand(H, K, self.num_envs)

    def plan(self, actions, details=False):
        self.calls.append(("plan", tuple(actions.shape)))
        return {"best": torch.full((self.num_envs,), actions.shape[1] - 1, dtype=torch.int32), "first_action": actions[0, -1]}


@pytest.mark.parametrize("H,K,repeat,J", [(6, 4, 2, 3), (7, 5, 2, 4), (5, 3, 1, 5), (3, 2, 8, 1)])
def test_shooting_policy_counter_arithmetic(H, K, repeat, J):
    """decision t draws from counter t * K * ceil(H / repeat) on: consecutive decisions use disjoint counter ranges"""
    assert magical_amd.ShootingPolicy is planning.ShootingPolicy and "ShootingPolicy" in magical_amd.__all__
    env = StubEnv()
    policy = planning.ShootingPolicy(env, horizon=H, candidates=K, repeat=repeat, key=9)
    for t in range(3):
        act = policy({"allo": None})
        assert act.tolist() == [K] * env.num_envs
        assert env.calls[-2:] == [("sample", H, K, repeat, 9, t * K * J), ("plan", (H, K, env.num_envs))]
        assert planning.plan_step(t, H, K, repeat) == t * K * J
    policy.reset()
    policy()
    assert env.calls[-2] == ("sample", H, K, repeat, 9, 0)
    with pytest.raises(ValueError):
        planning.ShootingPolicy(env, horizon=0, candidates=K)
    with pytest.raises(ValueError):
        planning.ShootingPolicy(env, horizon=H, candidates=K, repeat=0)


def test_plan_shape_checks():
    a = envs.plan_actions(np.ones((4, 3, 13), dtype=np.int64), 13)
    assert a.shape == (4, 3, 13) and a.dtype == torch.uint8
    assert envs.plan_actions(torch.ones((3, 13)), 13).shape == (1, 3, 13)     # [K, N]: H = 1
    assert envs.plan_actions(torch.ones((0, 3, 13)), 13).shape == (0, 3, 13)  # H = 0: score the current states
    for bad in [(4, 3, 12), (13,), (2, 4, 3, 13), (4, 0, 13)]:
        with pytest.raises(ValueError):
            envs.plan_actions(torch.zeros(bad, dtype=torch.uint8), 13)
    with pytest.raises(ValueError):   # K * N above MG_PLAN_MAX_ROLLOUTS
        envs.plan_actions(torch.zeros((1, 2049, 128), dtype=torch.uint8), 128)
    assert hasattr(envs.VecMagicalEnv, "plan") and hasattr(envs.VecMagicalEnv, "sample_plans")
    assert hasattr(envs.MagicalEnv, "plan")
    from magical_amd.pipeline import PipelinedVecEnv
    assert hasattr(PipelinedVecEnv, "plan") and hasattr(PipelinedVecEnv, "sample_plans")
