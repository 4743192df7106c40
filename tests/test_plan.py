"""GPU: mg_plan / mg_plan_sample (VecMagicalEnv.plan / sample_plans, PipelinedVecEnv, MagicalEnv.plan, ShootingPolicy).

Every comparison is bit-exact (torch.equal).  Candidate k of a plan must be what lookahead() gives for the action column
actions[:, k] on the same sim (tests/test_lookahead.py pins lookahead to stepped twins, the parity suite pins stepping
to the oracle); one test compares with stepped twins directly.  13 envs x 3 candidates = 39 rollouts: at 8 and 16
envs per workgroup the last workgroup is partial and workgroups mix candidates of different envs, and 13 is odd, so
candidates 1 and 2 start off a 4-byte boundary in the 1- and 2-byte state rows (the fan-out's element-wise stores);
the 4-env chunks of the pool test and the 1-env x 5 cases cover its packed stores.  Warm-up and candidate 0 are
test_lookahead's script (seed 7), candidates 1.. the same generator with seeds 8..: chosen with the C oracle on the CPU
so that MoveToCorner's scores after 7 steps have envs with a tied maximum (0.0 / 1.0 in every candidate) and envs whose
best candidate is not candidate 0.
"""
import ctypes

import numpy as np
import pytest
import torch

import magical_amd
from magical_amd import envs as mg_envs
from magical_amd import native
from magical_amd.pipeline import PipelinedVecEnv
from test_lookahead import CLUSTER, CORNER, FAR, FORMS, MATCH, N, REGION, W, make, same, script, step_out, warm

HMAX = 40


def warm_script(n=N):
    return script(W + HMAX, n)


def cands(H, K, n=N):
    """[H, K, n] candidates: candidate k = steps W .. W + H of script seed 7 + k (candidate 0 continues the warm-up)"""
    return torch.stack([script(W + HMAX, n, seed=7 + k)[W:W + H] for k in range(K)], dim=1).contiguous()


def plan_vs_lookahead(env, a, ctx=None):
    """plan(a) of env with scores, steps and errors of every candidate equal to the lookahead of its column, and the
    reduction equal to the host's; returns (the result, whether any rollout ended with live arbiters)"""
    res = env.plan(a, details=True)
    live = False
    for k in range(a.shape[1]):
        la = env.lookahead(a[:, k], bodies=True)
        assert torch.equal(res["scores"][k], la["score"]), (ctx, k)
        assert torch.equal(res["steps"][k], la["steps"]), (ctx, k)
        assert torch.equal(res["errors"][k], la["errors"]), (ctx, k)
        live = live or bool((la["counts"][:, 3] > 0).any())
    check_reduction(res, a, ctx)
    return res, live


def check_reduction(res, a, ctx=None):
    scores = res["scores"].cpu().numpy()
    best = scores.argmax(axis=0)   # the first occurrence of the maximum: the lowest k
    idx = np.arange(scores.shape[1])
    assert np.array_equal(res["best"].cpu().numpy(), best.astype(np.int32)), ctx
    assert np.array_equal(res["best_score"].cpu().numpy(), scores[best, idx]), ctx
    if a.shape[0] > 0:
        assert np.array_equal(res["first_action"].cpu().numpy(), a[0].cpu().numpy()[best, idx]), ctx
    return scores, best


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,n,pair", FORMS)
def test_bit_identical_to_lookahead(name, env, n, pair, monkeypatch):
    """every compiled (form, envs per workgroup) pair, H = 7 and 40: candidate k = lookahead of its action column, with
    live arbiters at the horizon in some rollout"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    K = 3 if n == N else 5
    a = warm(make(name, n), warm_script(n))
    assert a.step_form()[:2] == pair
    for H in (7, HMAX):
        res, live = plan_vs_lookahead(a, cands(H, K, n), H)
        assert torch.equal(res["steps"], torch.full((K, n), H, dtype=torch.int32, device="cuda"))
        assert live, ("no live arbiter: the case exercises no contact", H)
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [REGION, CLUSTER])
def test_equals_stepped_twins(name):
    """without lookahead in between: candidate k's score = score() of a twin stepped through actions[:, k]"""
    H, K = 7, 3
    acts, c = warm_script(), cands(7, 3)
    a = warm(make(name), acts)
    res = a.plan(c, details=True)
    for k in range(K):
        b = warm(make(name, auto_reset=False), acts)
        for h in range(H):
            b.step(c[h, k])
        assert torch.equal(res["scores"][k], b.score()), k
        assert torch.equal(res["errors"][k], b.errors()), k
        b.close()
    a.close()


@pytest.mark.gpu
def test_reduction_ties_and_non_trivial_maxima():
    """best / best_score / first_action = numpy's argmax along k and gathers, on inputs that have envs with a tied
    maximum and envs whose best candidate is not 0 (asserted); K = 1; H = 0"""
    a = warm(make(CORNER), warm_script())
    c = cands(7, 3)
    res = a.plan(c, details=True)
    scores, best = check_reduction(res, c)
    tied = (scores == scores.max(axis=0)).sum(axis=0) > 1
    assert tied.any(), "no env with a tied maximum: the tie rule is not exercised"
    assert (best != 0).any(), "every env's best candidate is 0: a kernel that always answers 0 would pass"
    assert len(np.unique(scores)) > 3   # MoveToCorner's score is graded, not binary
    plain = a.plan(c)
    assert list(plain) == ["best", "best_score", "first_action"]
    for key in plain:
        assert torch.equal(plain[key], res[key]), key
    # K = 1: the only candidate
    one, _ = plan_vs_lookahead(a, c[:, 1:2])
    assert torch.equal(one["best"], torch.zeros(N, dtype=torch.int32, device="cuda"))
    assert torch.equal(one["scores"][0], res["scores"][1]) and torch.equal(one["first_action"], c[0, 1])
    # H = 0: the current state, K times
    zero = a.plan(torch.empty((0, 3, N), dtype=torch.uint8), details=True)
    now = a.score()
    for k in range(3):
        assert torch.equal(zero["scores"][k], now), k
    assert torch.equal(zero["best"], torch.zeros(N, dtype=torch.int32, device="cuda"))
    assert torch.equal(zero["best_score"], now)
    assert torch.equal(zero["steps"], torch.zeros((3, N), dtype=torch.int32, device="cuda"))
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", [(REGION, {}), (CORNER, {"MG_STEP_BLK": "16"}), (CLUSTER, {})],
                         ids=["region-5/8", "corner-6/16", "cluster-4"])
def test_per_env_horizons(name, env, monkeypatch):
    """envs 3 steps from their episode's end, envs with none left and envs that run all H, in one batch"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L, H, K = 60, 8, 3
    a = warm(make(name, L=L), warm_script())
    left = torch.tensor([(3, 0, H)[e % 3] for e in range(N)])
    a.set_episode_steps(torch.where(left == H, torch.full((N,), W), L - left))
    res, _ = plan_vs_lookahead(a, cands(H, K))
    assert torch.equal(res["steps"].cpu(), left.to(torch.int32)[None].expand(K, N))
    a.close()


@pytest.mark.gpu
def test_sim_is_untouched():
    """a many-block task with the next-layout shadow, episodes of 9 steps with staggered phases: after plan() and
    sample_plans() the following steps, across auto-resets, give the bytes of a twin that never planned; a lookahead
    gives what it gave before the plan"""
    name, L = "MatchRegions-TestAll-LoResStack-v0", 9
    acts = warm_script()
    sims = [make(name, L=L), make(name, L=L)]
    for s in sims:
        s.reset()
        s.set_episode_steps(torch.arange(N) % L)
        for t in range(6):
            s.step(acts[t])
    a, c = sims
    before = (a.bodies(), a.errors(), a.arbiters(), a.lookahead(acts[6:13], bodies=True))
    res = a.plan(cands(7, 3), details=True)
    assert 1 <= int(res["steps"].min()) < 7
    a.sample_plans(5, 3, repeat=2, key=11, step=3)
    after = (a.bodies(), a.errors(), a.arbiters(), a.lookahead(acts[6:13], bodies=True))
    assert torch.equal(before[0][0], after[0][0]) and torch.equal(before[0][1], after[0][1])
    assert torch.equal(before[1], after[1])
    assert torch.equal(before[2][0], after[2][0]) and torch.equal(before[2][1].view(torch.int64), after[2][1].view(torch.int64))
    same(after[3], before[3], "lookahead after plan")
    resets = 0
    for t in range(6, 12):
        if t == 9:
            a.plan(cands(4, 2))   # again, between auto-reset steps
        ga, gc = step_out(a, acts[t]), step_out(c, acts[t])
        same(ga, gc, t)
        resets += int(gc["done"].sum())
    assert resets > 0
    a.close(), c.close()


@pytest.mark.gpu
def test_pool_growth():
    """K = 2, then 5 (the fan pool is re-allocated), then 2 again (the larger pool, partly used) on one sim"""
    a = warm(make(REGION), warm_script())
    first = None
    for K in (2, 5, 2):
        res, _ = plan_vs_lookahead(a, cands(7, K), K)
        if first is None:
            first = res
    same(res, first, "K = 2 again")
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["window", "frames_only", "unwrapped", "no_auto_reset"])
def test_modes(mode):
    """window rings, frames_only outputs, the unwrapped surface, auto_reset=False: the plain env's numbers"""
    acts, c = warm_script(), cands(7, 3)
    name = "MoveToRegion-Demo-v0" if mode == "unwrapped" else REGION
    a = make(name, window=(mode == "window"), auto_reset=(mode != "no_auto_reset"))
    if mode == "frames_only":
        a.bind_outputs(a.output_buffers(), frames_only=True)
    warm(a, acts)
    b = warm(make(REGION), acts)
    got, _ = plan_vs_lookahead(a, c, mode)
    same(got, b.plan(c, details=True), mode)
    a.close(), b.close()


@pytest.mark.gpu
def test_sampler_is_the_action_generator():
    a = make(REGION)
    for H, K, repeat, key, step in [(5, 3, 2, 42, 100), (5, 3, 1, 7, 0), (4, 2, 3, 9, (1 << 33) + 5)]:
        J = -(-H // repeat)
        got = a.sample_plans(H, K, repeat=repeat, key=key, step=step)
        assert got.shape == (H, K, N) and got.dtype == torch.uint8 and int(got.max()) < 18
        for h in range(H):
            for k in range(K):
                assert torch.equal(got[h, k], a.random_actions(step + k * J + h // repeat, key)), (H, repeat, h, k)
    assert J == 2 and torch.equal(got[0], got[2]) and not torch.equal(got[0], got[3])   # held for 3 steps
    out = torch.full((5, 3, N), 99, dtype=torch.uint8, device="cuda")
    assert a.sample_plans(5, 3, repeat=2, key=42, step=100, out=out) is out
    assert torch.equal(out, a.sample_plans(5, 3, repeat=2, key=42, step=100))
    assert a.sample_plans(0, 3).shape == (0, 3, N)
    a.close()


@pytest.mark.gpu
def test_refusals_launch_nothing():
    a = warm(make(REGION), warm_script())
    big = make(REGION, 128)
    lib = native.load()
    c = cands(7, 3)
    i32 = dict(dtype=torch.int32, device="cuda")
    bufs = dict(best=torch.full((N,), -7, **i32), best_score=torch.full((N,), -7.0, dtype=torch.float64, device="cuda"),
                first_action=torch.full((N,), 99, dtype=torch.uint8, device="cuda"),
                scores=torch.full((3, N), -7.0, dtype=torch.float64, device="cuda"),
                steps=torch.full((3, N), -7, **i32), errors=torch.full((3, N), -7, **i32))
    keep = {k: v.clone() for k, v in bufs.items()}
    out = native.mg_plan_out(**{k: v.data_ptr() for k, v in bufs.items()})
    nobest = native.mg_plan_out(**{k: v.data_ptr() for k, v in bufs.items() if k != "best"})
    samp = torch.full((7, 3, N), 99, dtype=torch.uint8, device="cuda")
    ap, sp, st, o = ctypes.c_void_p(c.data_ptr()), ctypes.c_void_p(samp.data_ptr()), a._stream(), ctypes.byref(out)

    def refused(rc):
        assert rc == -22 and lib.mg_last_error() != b""

    refused(lib.mg_plan(a.handle, ap, 7, 0, o, st))                        # K = 0
    refused(lib.mg_plan(a.handle, ap, 7, 4097, o, st))
    refused(lib.mg_plan(big.handle, ap, 7, 2049, o, big._stream()))        # K * N = 262272 > MG_PLAN_MAX_ROLLOUTS
    refused(lib.mg_plan(a.handle, ap, -1, 3, o, st))
    refused(lib.mg_plan(a.handle, ap, 4097, 3, o, st))
    refused(lib.mg_plan(a.handle, ap, 7, 3, ctypes.byref(nobest), st))     # null best
    refused(lib.mg_plan(a.handle, ap, 7, 3, None, st))
    refused(lib.mg_plan(None, ap, 7, 3, o, st))
    refused(lib.mg_plan(a.handle, None, 7, 3, o, st))                      # null actions with H > 0
    refused(lib.mg_plan_sample(a.handle, sp, 7, 3, 0, 42, 0, st))          # repeat = 0
    refused(lib.mg_plan_sample(a.handle, sp, 7, 0, 1, 42, 0, st))
    refused(lib.mg_plan_sample(a.handle, sp, 4097, 3, 1, 42, 0, st))
    refused(lib.mg_plan_sample(big.handle, sp, 7, 2049, 1, 42, 0, big._stream()))
    refused(lib.mg_plan_sample(a.handle, None, 7, 3, 1, 42, 0, st))
    refused(lib.mg_plan_sample(None, sp, 7, 3, 1, 42, 0, st))
    assert lib.mg_plan_sample(a.handle, sp, 0, 3, 1, 42, 0, st) == 0       # H = 0: a no-op
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert torch.equal(v, keep[k]), k
    assert bool((samp == 99).all())
    with pytest.raises(ValueError):
        a.plan(torch.zeros((2, 3, N + 1), dtype=torch.uint8))
    with pytest.raises(ValueError):
        a.plan(torch.zeros((2, 0, N), dtype=torch.uint8))
    with pytest.raises(native.NativeError):
        a.plan(torch.zeros((4097, 1, N), dtype=torch.uint8))
    with pytest.raises(native.NativeError):
        a.sample_plans(7, 3, repeat=0)
    assert lib.mg_plan(a.handle, None, 0, 3, o, st) == 0                   # H = 0: no actions needed
    plan_vs_lookahead(a, c)                                                # and the sim plans as if nothing had happened
    a.close(), big.close()


@pytest.mark.gpu
def test_pool_env_and_single_env():
    H, K = 7, 3
    acts, c = warm_script(), cands(7, 3)
    vec = warm(make(REGION), acts)
    pool = PipelinedVecEnv(REGION, N, chunks=3, base_seed=1000, max_episode_steps=FAR)
    assert pool.bounds == [0, 4, 8, 13]
    pool.reset()
    for t in range(W):
        pool.step(acts[t])
    got, want = pool.plan(c, details=True), vec.plan(c, details=True)
    assert list(got) == list(want)
    same(got, want, "pool")
    assert got["scores"].shape == (K, N) and got["best"].shape == (N,)
    # the pool's sampler follows its random_actions (chunk k: key + k, envs numbered from 0)
    sp = pool.sample_plans(5, K, repeat=2, key=42, step=9)
    for h in range(5):
        for k in range(K):
            assert torch.equal(sp[h, k], pool.random_actions(9 + k * 3 + h // 2, 42)), (h, k)
    pool.close(), vec.close()
    env = mg_envs.MagicalEnv(CORNER, seed=5)
    with pytest.raises(RuntimeError):
        env.plan([[1, 2]])
    env.reset()
    for t in range(W):
        env.step(1)
    seqs = np.array([[1] * 12, [3] * 12, [1] * 6 + [7] * 6, [1] * 12]).T   # [H, K]
    best, best_score, scores = env.plan(seqs)
    want = [env.lookahead(seqs[:, k])[0] for k in range(4)]
    assert scores.dtype == np.float64 and scores.tolist() == want
    assert best == int(np.argmax(want)) and best_score == want[best] and scores[0] == scores[3]
    env.close()


@pytest.mark.gpu
def test_shooting_policy():
    """the policy's actions = first_action of an explicit sample_plans + plan with the documented step; two runs with
    the same key are identical"""
    H, K, rep, key = 6, 4, 2, 5
    runs = []
    for run in range(2):
        env = magical_amd.make_vec("MoveToCorner-Demo-LoRes4E-v0", N, base_seed=1000, debug_reward=True)
        policy = magical_amd.ShootingPolicy(env, horizon=H, candidates=K, repeat=rep, key=key)
        obs, taken = env.reset(), []
        for t in range(3):
            if run == 0:
                want = env.plan(env.sample_plans(H, K, repeat=rep, key=key, step=t * K * 3))
            act = policy(obs)
            assert act.shape == (N,) and act.dtype == torch.uint8
            if run == 0:
                assert torch.equal(act, want["first_action"]), t
                assert torch.equal(policy.last["best"], want["best"])
            taken.append(act.clone())
            obs, _, _, _ = env.step(act)
        runs.append(torch.stack(taken))
        policy.reset()
        assert policy.t == 0
        env.close()
    assert torch.equal(runs[0], runs[1])
    assert len(torch.unique(runs[0])) > 1
