"""GPU: mg_plan_beam (VecMagicalEnv.plan_beam, PipelinedVecEnv.plan_beam, MagicalEnv.plan_beam, BeamPolicy).

Every comparison is bit-exact.  The reference is the definition restated in numpy (tests/test_beam_host.py: select and
lineage) around the existing API: the values after every segment must be what plan(details=True) -- which
tests/test_plan.py pins to lookahead and stepping -- gives for the lineages' action prefixes, the parents what select
gives for those values, the plans what lineage gives for those parents.  Warm-up is test_plan's (test_lookahead's
script, seed 7, 20 steps); the candidates are sample_plans' with key 42, step 0.

How the key of the first test was checked: NOT with the C oracle on the CPU, which the case was meant to be chosen with
(as tests/test_cem.py's was), but on the device with the host loop over plan() alone -- sample_plans, plan() of every
segment's prefixes, select and lineage in numpy, no call of plan_beam.  For MoveToCorner at H = 7, seg = 3, K = 5,
survivors = 2 that run has, for key 42, slots whose parent is another slot, envs with equal values on both sides of the
survivor boundary, and slots whose final plan differs from their own action column; the test asserts all three.
"""
import ctypes

import numpy as np
import pytest
import torch

import magical_amd
from magical_amd import Objective
from magical_amd import envs as mg_envs
from magical_amd import native
from magical_amd.pipeline import PipelinedVecEnv
from test_beam_host import lineage, select
from test_lookahead import CLUSTER, CORNER, FAR, FORMS, N, REGION, W, make, same, step_out, warm
from test_plan import warm_script

KEYS = ["best", "best_value", "first_action", "plan", "plans", "values", "steps", "errors", "depth_values", "parents"]


def check(env, acts, seg, B, objective=None, ctx=None):
    """plan_beam(acts) of env against the definition; returns the result as numpy arrays"""
    kw = {} if objective is None else {"objective": objective}
    H, K, n = acts.shape
    D = -(-H // seg)
    res = env.plan_beam(acts, seg, B, details=True, **kw)
    assert list(res) == KEYS
    got = {k: v.cpu().numpy() for k, v in res.items()}
    assert got["plans"].shape == (H, K, n) and got["depth_values"].shape == (D, K, n)
    assert got["parents"].shape == (D - 1, K, n) and got["parents"].dtype == np.int32
    a = acts.cpu().numpy()
    # the values after every segment = plan() of the lineages' prefixes, the parents = select of those values
    for d in range(D):
        h1 = min(H, (d + 1) * seg)
        prefix = lineage(a[:h1], got["parents"][:d], seg)
        ref = env.plan(torch.from_numpy(prefix), details=True, **kw)
        assert np.array_equal(got["depth_values"][d], ref["scores"].cpu().numpy()), (ctx, "depth_values", d)
        if d < D - 1:
            assert np.array_equal(got["parents"][d], select(got["depth_values"][d], B)), (ctx, "parents", d)
    assert np.array_equal(got["plans"], lineage(a, got["parents"], seg)), (ctx, "plans")
    # one long rollout of every final plan
    ref = env.plan(res["plans"], details=True, **kw)
    for k, r in (("values", "scores"), ("steps", "steps"), ("errors", "errors")):
        assert torch.equal(res[k], ref[r]), (ctx, k)
    assert np.array_equal(got["values"], got["depth_values"][-1]), ctx
    best = got["values"].argmax(axis=0)   # the first occurrence of the maximum: the lowest k
    idx = np.arange(n)
    assert np.array_equal(got["best"], best.astype(np.int32)), ctx
    assert np.array_equal(got["best_value"], got["values"][best, idx]), ctx
    assert np.array_equal(got["first_action"], got["plans"][0, best, idx]), ctx
    assert np.array_equal(got["plan"], got["plans"][:, best, idx]), ctx
    plain = env.plan_beam(acts, seg, B, **kw)
    assert list(plain) == KEYS[:4]
    same(plain, {k: res[k] for k in KEYS[:4]}, (ctx, "plain"))
    return got


def boundary_tie(got, B):
    ranked = -np.sort(-got["depth_values"][:-1], axis=1)
    return bool((ranked[:, B - 1] == ranked[:, B]).any())


@pytest.mark.gpu
def test_lineage_equals_one_long_rollout():
    """MoveToCorner, 13 envs, H = 7 in segments of 3, 3 and 1, K = 5, 2 survivors, on a run that exercises the rules"""
    H, K, seg, B = 7, 5, 3, 2
    a = warm(make(CORNER), warm_script())
    acts = a.sample_plans(H, K, key=42, step=0)
    got = check(a, acts, seg, B)
    assert (got["parents"] != np.arange(K, dtype=np.int32)[None, :, None]).any(), "no slot was resampled"
    assert boundary_tie(got, B), "no env with equal values on both sides of the survivor boundary"
    assert (got["plans"] != acts.cpu().numpy()).any(), "every slot's plan is its own action column"
    assert np.array_equal(got["steps"], np.full((K, N), H, dtype=np.int32))
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,n,pair", FORMS)
def test_every_compiled_form(name, env, n, pair, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a = warm(make(name, n), warm_script(n))
    assert a.step_form()[:2] == pair
    check(a, a.sample_plans(5, 5, key=42, step=0), 2, 2, ctx=name)
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [REGION, CORNER])
def test_wide_and_ragged(name):
    """K = 70: more than one wavefront of slots and no multiple of 64; 9 survivors"""
    a = warm(make(name), warm_script())
    got = check(a, a.sample_plans(4, 70, key=42, step=0), 2, 9, ctx=name)
    if name == REGION:   # binary scores: the rank rule alone picks the survivors of an all-tied env
        v = got["depth_values"][0]
        flat = v.min(axis=0) == v.max(axis=0)
        assert flat.any(), "no env with all-equal values"
        e = int(np.argmax(flat))
        assert got["parents"][0][:, e].tolist() == [k if k < 9 else (k - 9) % 9 for k in range(70)]
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 16])
def test_env_counts(n):
    """16 envs: every slot's columns start on a word boundary, the packed path of the 1- and 2-byte rows (13 is the
    element path); 1 env"""
    a = warm(make(CORNER, n), warm_script(n))
    got = check(a, a.sample_plans(5, 5, key=42, step=0), 2, 2, ctx=n)
    if n == 16:
        assert (got["parents"] != np.arange(5, dtype=np.int32)[None, :, None]).any()
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("objective", [None, Objective("return", gamma=0.9, tail=0.5)])
def test_degenerate_ends_are_plan(objective):
    kw = {} if objective is None else {"objective": objective}
    H, K = 7, 5
    a = warm(make(CORNER), warm_script())
    acts = a.sample_plans(H, K, key=42, step=0)
    want = a.plan(acts, details=True, **kw)
    for seg, B in ((3, K), (H, 2)):
        got = a.plan_beam(acts, seg, B, details=True, **kw)
        assert torch.equal(got["plans"], acts), (seg, B)
        for k, r in (("best", "best"), ("best_value", "best_score"), ("first_action", "first_action"),
                     ("values", "scores"), ("steps", "steps"), ("errors", "errors")):
            assert torch.equal(got[k], want[r]), (seg, B, k)
        ident = torch.arange(K, dtype=torch.int32, device="cuda")[None, :, None].expand(got["parents"].shape)
        assert torch.equal(got["parents"], ident), (seg, B)
    a.close()


OBJECTIVES = [None, Objective("return", gamma=0.9, tail=0.5), Objective("peak", gamma=0.95)]


@pytest.mark.gpu
@pytest.mark.parametrize("objective", OBJECTIVES, ids=["final", "return", "peak"])
@pytest.mark.parametrize("left", [4, 2, FAR - W], ids=["ends-in-segment-1", "ends-in-segment-0", "no-end"])
def test_objectives_and_episode_end(objective, left):
    """a debug-reward sim whose episodes end `left` steps from the warmed-up state: in the second segment, in the first,
    or never.  The values, steps and errors are those of plan(plans), and the later segments simulate nothing"""
    H, K, seg, B = 7, 5, 3, 2
    a = warm(make(CORNER, L=W + left, debug_reward=True), warm_script())
    got = check(a, a.sample_plans(H, K, key=42, step=0), seg, B, objective, ctx=left)
    assert np.array_equal(got["steps"], np.full((K, N), min(H, left), dtype=np.int32))
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["window", "no_auto_reset"])
def test_sim_is_untouched(mode):
    """a twin that never planned steps to the same bytes, across an episode's end"""
    kw = dict(window=(mode == "window"), auto_reset=(mode != "no_auto_reset"))
    acts = warm_script()
    a, c = (warm(make(CORNER, L=W + 3, **kw), acts) for _ in range(2))
    a.plan_beam(a.sample_plans(7, 5, key=42, step=0), 3, 2, details=True, objective=Objective("peak", gamma=0.95))
    a.plan_beam(a.sample_plans(4, 70, key=42, step=0), 2, 9)
    for t in range(W, W + 4):
        same(step_out(a, acts[t]), step_out(c, acts[t]), t)
    a.close(), c.close()


@pytest.mark.gpu
def test_refusals_launch_nothing():
    a = warm(make(REGION), warm_script())
    big = make(REGION, 128)
    lib = native.load()
    H, K, D = 7, 3, 3
    c = a.sample_plans(H, K, key=42, step=0)
    i32, f64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float64, device="cuda")
    bufs = dict(best=torch.full((N,), -7, **i32), best_value=torch.full((N,), -7.0, **f64),
                first_action=torch.full((N,), 99, dtype=torch.uint8, device="cuda"),
                best_plan=torch.full((H, N), 99, dtype=torch.uint8, device="cuda"),
                values=torch.full((K, N), -7.0, **f64), steps=torch.full((K, N), -7, **i32),
                errors=torch.full((K, N), -7, **i32), depth_values=torch.full((D, K, N), -7.0, **f64),
                parents=torch.full((D - 1, K, N), -7, **i32))
    plans = torch.full((H, K, N), 99, dtype=torch.uint8, device="cuda")
    keep = {k: v.clone() for k, v in bufs.items()}
    out = native.mg_plan_beam_out(**{k: v.data_ptr() for k, v in bufs.items()})
    nobest = native.mg_plan_beam_out(**{k: v.data_ptr() for k, v in bufs.items() if k != "best"})
    ap, pp, st, o = ctypes.c_void_p(c.data_ptr()), ctypes.c_void_p(plans.data_ptr()), a._stream(), ctypes.byref(out)

    def refused(rc):
        assert rc == -22 and lib.mg_last_error() != b""

    def obj(kind=1, reserved=0, gamma=0.9, tail=0.5):
        return ctypes.byref(native.mg_objective(kind=kind, reserved=reserved, gamma=gamma, tail=tail))

    refused(lib.mg_plan_beam(None, ap, pp, H, K, 3, 2, None, o, st))
    refused(lib.mg_plan_beam(a.handle, None, pp, H, K, 3, 2, None, o, st))
    refused(lib.mg_plan_beam(a.handle, ap, None, H, K, 3, 2, None, o, st))
    refused(lib.mg_plan_beam(a.handle, ap, pp, H, K, 3, 2, None, None, st))
    refused(lib.mg_plan_beam(a.handle, ap, pp, H, K, 3, 2, None, ctypes.byref(nobest), st))
    refused(lib.mg_plan_beam(a.handle, ap, pp, 0, K, 1, 2, None, o, st))           # H = 0
    refused(lib.mg_plan_beam(a.handle, ap, pp, 4097, K, 3, 2, None, o, st))
    refused(lib.mg_plan_beam(a.handle, ap, pp, H, 0, 3, 1, None, o, st))           # K = 0
    refused(lib.mg_plan_beam(a.handle, ap, pp, H, 4097, 3, 2, None, o, st))
    refused(lib.mg_plan_beam(big.handle, ap, pp, H, 2049, 3, 2, None, o, big._stream()))   # K * N > MG_PLAN_MAX_ROLLOUTS
    refused(lib.mg_plan_beam(a.handle, ap, pp, H, K, 0, 2, None, o, st))           # seg
    refused(lib.mg_plan_beam(a.handle, ap, pp, H, K, H + 1, 2, None, o, st))
    refused(lib.mg_plan_beam(a.handle, ap, pp, H, K, 3, 0, None, o, st))           # survivors
    refused(lib.mg_plan_beam(a.handle, ap, pp, H, K, 3, K + 1, None, o, st))
    refused(lib.mg_plan_beam(a.handle, ap, pp, H, K, 3, 2, obj(kind=3), o, st))    # the objective
    refused(lib.mg_plan_beam(a.handle, ap, pp, H, K, 3, 2, obj(reserved=1), o, st))
    refused(lib.mg_plan_beam(a.handle, ap, pp, H, K, 3, 2, obj(gamma=0.0), o, st))
    refused(lib.mg_plan_beam(a.handle, ap, pp, H, K, 3, 2, obj(tail=-1.0), o, st))
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert torch.equal(v, keep[k]), k
    assert bool((plans == 99).all())
    for bad in (dict(seg=0), dict(seg=H + 1), dict(survivors=0), dict(survivors=K + 1)):
        with pytest.raises(ValueError):
            a.plan_beam(c, **dict(dict(seg=3, survivors=2), **bad))
    with pytest.raises(ValueError):
        a.plan_beam(torch.zeros((0, K, N), dtype=torch.uint8), 1, 1)
    with pytest.raises(ValueError):
        a.plan_beam(torch.zeros((2, K, N + 1), dtype=torch.uint8), 1, 1)
    with pytest.raises(ValueError):
        a.plan_beam(c, 3, 2, objective=3)
    assert lib.mg_plan_beam(a.handle, ap, pp, H, K, 3, 2, None, o, st) == 0
    torch.cuda.synchronize()
    assert not torch.equal(bufs["best"], keep["best"]) and not bool((plans == 99).any())
    check(a, c, 3, 2)   # and the sim plans as if nothing had happened
    a.close(), big.close()


@pytest.mark.gpu
def test_pool_env_and_single_env():
    H, K, seg, B = 7, 5, 3, 2
    acts = warm_script()
    vec = warm(make(REGION), acts)
    pool = PipelinedVecEnv(REGION, N, chunks=3, base_seed=1000, max_episode_steps=FAR)
    pool.reset()
    for t in range(W):
        pool.step(acts[t])
    c = vec.sample_plans(H, K, key=42, step=0)
    got, want = pool.plan_beam(c, seg, B, details=True), vec.plan_beam(c, seg, B, details=True)
    assert list(got) == list(want) == KEYS
    same(got, want, "pool")   # per-env results: chunking changes nothing
    pool.close(), vec.close()
    env = mg_envs.MagicalEnv(CORNER, seed=5)
    with pytest.raises(RuntimeError):
        env.plan_beam([[1, 2]], 1, 1)
    env.reset()
    for t in range(W):
        env.step(1)
    one = env._vec   # the one-env vec env behind it
    seqs = one.sample_plans(8, 6, key=3, step=0)
    plan, best_value, values = env.plan_beam(seqs[:, :, 0].cpu().numpy(), 2, 2)
    want = one.plan_beam(seqs, 2, 2, details=True)
    assert plan.dtype == np.uint8 and plan.tolist() == want["plan"][:, 0].tolist()
    assert best_value == float(want["best_value"][0]) and values.tolist() == want["values"][:, 0].tolist()
    env.close()


@pytest.mark.gpu
def test_beam_policy():
    """the policy's actions = first_action of an explicit sample_plans + plan_beam with the documented step"""
    H, K, seg, B, rep, key = 6, 4, 2, 2, 2, 5
    o = Objective("return", gamma=0.9, tail=0.5)
    env = magical_amd.make_vec("MoveToCorner-Demo-LoRes4E-v0", N, base_seed=1000, debug_reward=True)
    policy = magical_amd.BeamPolicy(env, horizon=H, candidates=K, seg=seg, survivors=B, repeat=rep, key=key, objective=o)
    obs, taken = env.reset(), []
    for t in range(3):
        want = env.plan_beam(env.sample_plans(H, K, repeat=rep, key=key, step=magical_amd.plan_step(t, H, K, rep)), seg, B,
                             objective=o)
        act = policy(obs)
        assert act.shape == (N,) and act.dtype == torch.uint8
        assert torch.equal(act, want["first_action"]) and torch.equal(policy.last["plan"], want["plan"]), t
        taken.append(act.clone())
        obs, _, _, _ = env.step(act)
    assert policy.t == 3 and len(torch.unique(torch.stack(taken))) > 1
    policy.reset()
    assert policy.t == 0
    env.close()
