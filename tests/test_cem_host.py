"""CPU: the host side of mg_plan_cem -- header, ctypes binding, build units, CEMPolicy's counter arithmetic and warm
start, and the numpy restatement of the definition (Philox4x32-10, the weighted draw D, the candidates of an
iteration, the elites and the refit) that tests/test_cem.py compares the device with, checked here on hand-worked
cases."""
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
          ("steps", "int32_t"), ("errors", "int32_t"), ("iter_best", "double")]
M32 = np.uint64(0xffffffff)


# ---------------------------------------------------------------------------------------------------------------------
# the definition in numpy
def philox_word(key, counter, e):
    """first output word of Philox4x32-10 for key (k lo, k hi) and counter (c lo, c hi, e, 0); counter and e broadcast"""
    c = np.asarray(counter, dtype=np.uint64)
    c0, c1 = c & M32, c >> np.uint64(32)
    c2 = np.asarray(e, dtype=np.uint64) + np.zeros_like(c0)
    c0, c1 = c0 + np.zeros_like(c2), c1 + np.zeros_like(c2)
    c3 = np.zeros_like(c2)
    k0, k1 = np.uint64(int(key) & 0xffffffff), np.uint64((int(key) >> 32) & 0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0


def pick(w, word):
    """w: [18, n] weights, word: [n] -> the action of each env: the smallest a whose cumulative weight exceeds word % T"""
    w = np.asarray(w, dtype=np.int64).copy()
    w[:, w.sum(axis=0) == 0] = 1
    r = np.asarray(word, dtype=np.int64) % w.sum(axis=0)
    return np.argmax(np.cumsum(w, axis=0) > r, axis=0).astype(np.uint8)   # (argmax: the first True)


def draw(w, key, counter, n):
    return pick(w, philox_word(key, counter, np.arange(n)))


def candidates(w, H, K, repeat, key, step, i, prev=None, prev_best=None):
    """u8[H, K, n] of iteration i from the weights w [J, 18, n]; from iteration 1 on candidate 0 is the incumbent"""
    J, n = -(-H // repeat), w.shape[2]
    out = np.zeros((H, K, n), dtype=np.uint8)
    for h in range(H):
        for k in range(K):
            out[h, k] = draw(w[h // repeat], key, step + (i * K + k) * J + h // repeat, n)
    if i > 0:
        out[:, 0] = prev[:, prev_best, np.arange(n)]
    return out


def elites_of(scores, E):
    """[E, n]: the E candidates of every env with the highest scores, the lower k first among equal scores"""
    return np.argsort(-np.asarray(scores, dtype=np.float64), axis=0, kind="stable")[:E]


def refit(cand, scores, E, alpha, repeat):
    H, K, n = cand.shape
    J = -(-H // repeat)
    el = elites_of(scores, E)
    w = np.full((J, 18, n), alpha, dtype=np.int64)
    for j in range(J):
        acts = cand[j * repeat][el, np.arange(n)]   # [E, n]
        for a in range(18):
            w[j, a] += (acts == a).sum(axis=0)
    return w.astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "magical_sim.h")).read(), flags=re.S)


def test_header_declares_the_call_and_the_outputs():
    src = _header()
    body = {name: b for b, name in re.findall(r"typedef struct \{(.*?)\}\s*(\w+);", src, flags=re.S)}["mg_plan_cem_out"]
    decls = [re.match(r"(\w+)\s*\*\s*(\w+)$", d.strip()).groups() for d in body.split(";") if d.strip()]
    assert [(n, t) for t, n in decls] == FIELDS
    args = [" ".join(a.split()) for a in re.search(r"int mg_plan_cem\((.*?)\);", src, flags=re.S).group(1).split(",")]
    assert args == ["mg_sim *sim", "uint8_t *actions_dev", "uint16_t *weights_dev", "int32_t warm", "int32_t H",
                    "int32_t K", "int32_t iters", "int32_t elites", "int32_t alpha", "int32_t repeat", "uint64_t key",
                    "uint64_t step", "const mg_plan_cem_out *out", "void *stream"]


def test_binding_matches_the_header():
    assert "mg_plan_cem" in native.EXPORTS
    assert [f for f, _ in native.mg_plan_cem_out._fields_] == [f for f, _ in FIELDS]
    assert all(t is ctypes.c_void_p for _, t in native.mg_plan_cem_out._fields_)
    assert ctypes.sizeof(native.mg_plan_cem_out) == 7 * ctypes.sizeof(ctypes.c_void_p)
    lib = native.load()
    vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
    fn = lib.mg_plan_cem
    assert fn.argtypes[:12] == [vp, vp, vp] + [i32] * 7 + [u64, u64] and fn.argtypes[13] is vp and len(fn.argtypes) == 14
    assert fn.argtypes[12]._type_ is native.mg_plan_cem_out and fn.restype is i32
    # refused on the host, before any GPU call: nothing is launched for a null handle
    assert fn(None, None, None, 0, 1, 1, 1, 1, 1, 1, 0, 0, None, None) == -22
    assert b"mg_plan_cem" in lib.mg_last_error()


def test_build_lists_the_cem_unit():
    assert "mg_cem.hip" in build.UNITS
    for h in build.UNITS["mg_cem.hip"]:
        assert os.path.exists(os.path.join(build.CSRC, h)), h
    assert {"mg_cem.h", "mg_philox.h", "mg_sim.h"} <= set(build.UNITS["mg_cem.hip"])   # mg_plan_cem lives in the unit
    assert sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip")) == sorted(build.UNITS)
    # the rollouts are the lookahead kernel as it is: the unit defines no rollout kernel of its own
    src = open(os.path.join(build.CSRC, "mg_cem.hip")).read()
    assert "mg_stepk.h" not in src and "mg_lookahead.h" not in src
    philox = open(os.path.join(build.CSRC, "mg_philox.h")).read()
    assert "philox_word" in philox and "philox_word(key, step, e) % 18u" in philox


def test_python_surface():
    assert hasattr(envs.VecMagicalEnv, "plan_cem") and hasattr(envs.MagicalEnv, "plan_cem")
    from magical_amd.pipeline import PipelinedVecEnv
    assert hasattr(PipelinedVecEnv, "plan_cem")
    assert magical_amd.CEMPolicy is planning.CEMPolicy and magical_amd.cem_step is planning.cem_step
    assert "CEMPolicy" in magical_amd.__all__ and "cem_step" in magical_amd.__all__


@pytest.mark.parametrize("H,K,iters,repeat,J", [(6, 4, 3, 2, 3), (7, 5, 3, 2, 4), (5, 3, 1, 1, 5), (3, 2, 4, 8, 1)])
def test_cem_step_arithmetic(H, K, iters, repeat, J):
    for t in range(4):
        assert planning.cem_step(t, H, K, iters, repeat) == t * iters * K * J
    # a decision's last counter is below the next decision's first
    last = planning.cem_step(1, H, K, iters, repeat) + ((iters - 1) * K + K - 1) * J + (H - 1) // repeat
    assert last == planning.cem_step(2, H, K, iters, repeat) - 1


class StubEnv:
    """records plan_cem calls; the weights it returns: slot j holds j + 10 * (the call's number) everywhere"""
    num_envs = 2

    def __init__(self):
        self.calls, self.given = [], []

    def plan_cem(self, H, K, iters, elites, alpha=1, repeat=1, key=42, step=0, weights=None, details=False):
        self.calls.append((H, K, iters, elites, alpha, repeat, key, step))
        self.given.append(None if weights is None else weights.clone())
        J = -(-H // repeat)
        w = (torch.arange(J, dtype=torch.int16)[:, None, None] + 10 * len(self.calls)).expand(J, 18, self.num_envs)
        return {"first_action": torch.full((self.num_envs,), len(self.calls), dtype=torch.uint8),
                "weights": w.contiguous().view(torch.uint16)}


@pytest.mark.parametrize("H,K,iters,repeat,J", [(6, 4, 3, 2, 3), (7, 5, 2, 2, 4), (5, 3, 1, 1, 5)])
def test_cem_policy_takes_disjoint_counters(H, K, iters, repeat, J):
    env = StubEnv()
    policy = planning.CEMPolicy(env, horizon=H, candidates=K, iters=iters, elites=2, alpha=3, repeat=repeat, key=9)
    for t in range(3):
        act = policy({"allo": None})
        assert act.tolist() == [t + 1] * env.num_envs
        assert env.calls[-1] == (H, K, iters, 2, 3, repeat, 9, t * iters * K * J)
        assert env.given[-1] is None   # no warm start unless asked for
    policy.reset()
    policy()
    assert env.calls[-1][-1] == 0


def test_cem_policy_warm_start_shift():
    w = torch.arange(3 * 18 * 2, dtype=torch.int16).reshape(3, 18, 2).view(torch.uint16)   # hand-made: all distinct
    s = planning.shift_weights(w)
    assert s.dtype == torch.uint16 and s.shape == w.shape
    assert np.array_equal(s[:2].numpy(), w[1:].numpy()) and np.array_equal(s[2].numpy(), np.ones((18, 2), dtype=np.uint16))
    assert np.array_equal(w.numpy().ravel(), np.arange(108, dtype=np.uint16))   # the input is left as it was
    env = StubEnv()
    policy = planning.CEMPolicy(env, horizon=3, candidates=4, iters=2, elites=2, warm_start=True)
    for t in range(3):
        policy()
    assert env.given[0] is None
    for t in (1, 2):   # decision t starts from decision t - 1's weights (slots 10t, 10t + 1, 10t + 2), shifted
        g = env.given[t].numpy()
        assert g.shape == (3, 18, 2)
        assert (g[0] == 10 * t + 1).all() and (g[1] == 10 * t + 2).all() and (g[2] == 1).all()
    policy.reset()
    assert policy.weights is None and policy.t == 0
    policy()
    assert env.given[-1] is None and env.calls[-1][-1] == 0


def test_cem_policy_refuses_bad_arguments():
    env = StubEnv()
    ok = dict(horizon=4, candidates=4, iters=2, elites=2)
    planning.CEMPolicy(env, **ok)
    for bad in [dict(horizon=0), dict(candidates=0), dict(iters=0), dict(elites=0), dict(elites=5), dict(repeat=0),
                dict(alpha=-1), dict(repeat=2, warm_start=True)]:
        with pytest.raises(ValueError):
            planning.CEMPolicy(env, **dict(ok, **bad))
    planning.CEMPolicy(env, **dict(ok, repeat=1, warm_start=True))


def test_philox_reference():
    # the Random123 known answer for the all-zero counter and key
    assert int(philox_word(0, 0, 0)) == 0x6627e8d5
    # broadcasting: a vector of envs at one counter = the scalar calls
    e = np.arange(5)
    got = philox_word(0x1234567887654321, (1 << 33) + 7, e)
    assert [int(x) for x in got] == [int(philox_word(0x1234567887654321, (1 << 33) + 7, int(k))) for k in e]
    assert len(set(int(x) for x in got)) == 5


def test_draw_at_uniform_weights_is_word_mod_18():
    n = 13
    for key, c in [(42, 0), (7, 100), (9, (1 << 33) + 5)]:
        word = philox_word(key, c, np.arange(n))
        assert np.array_equal(draw(np.ones((18, n)), key, c, n), (word % np.uint64(18)).astype(np.uint8))
        # T == 0 draws as if all weights were 1
        assert np.array_equal(draw(np.zeros((18, n)), key, c, n), (word % np.uint64(18)).astype(np.uint8))


def test_pick_hand_worked():
    w = np.zeros((18, 1), dtype=np.int64)
    w[3], w[4] = 2, 1          # T = 3: r = 0, 1 -> action 3; r = 2 -> action 4
    assert [int(pick(w, [r])[0]) for r in (0, 1, 2, 3, 4, 5, 302)] == [3, 3, 4, 3, 3, 4, 4]
    w[0], w[17] = 1, 5         # cumulative 1, 3, 4, 9: T = 9
    assert [int(pick(w, [r])[0]) for r in range(9)] == [0, 3, 3, 4, 17, 17, 17, 17, 17]
    # alpha = 0: an action of weight 0 is never drawn
    n = 64
    w = np.zeros((18, n), dtype=np.int64)
    w[3], w[4] = 2, 1
    seen = set()
    for c in range(40):
        seen |= set(draw(w, 5, c, n).tolist())
    assert seen == {3, 4}


def test_refit_hand_worked():
    # one env, K = 5, E = 3: scores 0.5, 1.0, 0.5, 0.5, 0.2 -- the tie at 0.5 straddles the elite boundary, and the
    # lower k wins it: the elites are k = 1, 0, 2, not 3
    scores = np.array([[0.5], [1.0], [0.5], [0.5], [0.2]])
    assert elites_of(scores, 3)[:, 0].tolist() == [1, 0, 2]
    cand = np.zeros((3, 5, 1), dtype=np.uint8)   # H = 3, repeat = 2: slots at rows 0 and 2
    cand[0, :, 0] = [3, 4, 3, 7, 7]
    cand[1, :, 0] = [3, 4, 3, 7, 7]
    cand[2, :, 0] = [9, 9, 0, 9, 9]
    w = refit(cand, scores, 3, 1, 2)
    assert w.shape == (2, 18, 1) and w.dtype == np.uint16
    want0, want1 = [1] * 18, [1] * 18
    want0[3], want0[4] = 3, 2
    want1[9], want1[0] = 3, 2
    assert w[0, :, 0].tolist() == want0 and w[1, :, 0].tolist() == want1
    w0 = refit(cand, scores, 3, 0, 2)
    assert w0[0, :, 0].sum() == 3 and w0[0, 7, 0] == 0 and w0[0, 3, 0] == 2
    # -0.0 and 0.0 are one score: the lower k first
    assert elites_of(np.array([[0.0], [-0.0], [0.0]]), 2)[:, 0].tolist() == [0, 1]
    assert elites_of(np.array([[-0.0], [0.0], [-1.0]]), 2)[:, 0].tolist() == [0, 1]


def test_candidates_hand_worked():
    H, K, repeat, key, step, n = 5, 3, 2, 11, 40, 4
    J = 3
    c0 = candidates(np.ones((J, 18, n)), H, K, repeat, key, step, 0)
    for h in range(H):
        for k in range(K):   # what mg_plan_sample is documented to write
            want = philox_word(key, step + k * J + h // repeat, np.arange(n)) % np.uint64(18)
            assert np.array_equal(c0[h, k], want.astype(np.uint8))
    best = np.array([2, 0, 1, 2])
    c1 = candidates(np.ones((J, 18, n)), H, K, repeat, key, step, 1, c0, best)
    assert np.array_equal(c1[:, 0], c0[:, best, np.arange(n)])           # the incumbent, unchanged
    want = philox_word(key, step + (K + 1) * J + 2, np.arange(n)) % np.uint64(18)
    assert np.array_equal(c1[4, 1], want.astype(np.uint8))               # iteration 1 draws K * J counters further on
