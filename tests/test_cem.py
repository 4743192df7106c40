"""GPU: mg_plan_cem (VecMagicalEnv.plan_cem, PipelinedVecEnv.plan_cem, MagicalEnv.plan_cem, CEMPolicy).

Every comparison is bit-exact.  The reference is the definition restated in numpy (tests/test_cem_host.py: Philox, the
weighted draw, the incumbent rule, the elites with their tie rule, the refit) looped over the existing API: every
iteration's candidates go through plan(details=True), which tests/test_plan.py pins to lookahead and stepping.
Warm-up is test_plan's (test_lookahead's script, seed 7, 20 steps).  The key of the first test (42, step 0) was
checked on the CPU before any GPU run, with the C oracle in place of plan(): 13 oracle envs of the same seeds, warmed
up with the same script and stepped through every candidate of the numpy loop with the episode length set to end at
the horizon, so that the last step reports the score.  For MoveToCorner at H = 7, K = 5, repeat = 2, iters = 3,
elites = 2 that run has envs whose second and third ranked scores are equal (3 envs score 0.0 in every candidate), envs
whose best candidate of iteration 0 is not candidate 0, and envs whose best score rises between iterations; keys 1..5
have them too.  The same run for MoveToRegion at H = 3, K = 70 gives one score for all 70 candidates in every env
(the wide case is all ties there), which is why MoveToCorner, with some 390 distinct scores, runs that shape as well.
"""
import ctypes

import numpy as np
import pytest
import torch

import magical_amd
from magical_amd import envs as mg_envs
from magical_amd import native
from magical_amd.pipeline import PipelinedVecEnv
from test_cem_host import candidates, elites_of, refit
from test_lookahead import CORNER, FAR, FORMS, N, REGION, W, make, same, step_out, warm
from test_plan import warm_script

KEYS = ("actions", "scores", "steps", "errors", "best", "best_score", "first_action", "plan", "iter_best", "weights")


def host_cem(env, H, K, iters, elites, alpha=1, repeat=1, key=42, step=0, weights=None):
    """the definition as a loop over plan(): numpy arrays under plan_cem's names, plus 'history': every iteration's
    (candidates, scores, best)"""
    n, J = env.num_envs, -(-H // repeat)
    w = np.ones((J, 18, n), dtype=np.uint16) if weights is None else np.array(weights, dtype=np.uint16)
    cand = best = None
    iter_best, history = [], []
    for i in range(iters):
        cand = candidates(w, H, K, repeat, key, step, i, cand, best)
        res = {k: v.cpu().numpy() for k, v in env.plan(torch.from_numpy(cand), details=True).items()}
        best = res["best"].astype(np.int64)
        iter_best.append(res["best_score"])
        history.append((cand, res["scores"], best))
        w = refit(cand, res["scores"], elites, alpha, repeat)
    out = dict(res, actions=cand, plan=cand[:, best, np.arange(n)], iter_best=np.array(iter_best), weights=w)
    out["history"] = history
    return out


def agree(got, want, ctx=None, keys=KEYS):
    for k in keys:
        g = got[k].cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (ctx, k, g.dtype, g.shape)
        assert np.array_equal(g, want[k]), (ctx, k)


def dev_weights(w):
    return torch.from_numpy(np.ascontiguousarray(w).view(np.int16)).cuda().view(torch.uint16)


@pytest.mark.gpu
def test_equals_the_host_loop():
    """MoveToCorner, 13 envs, H = 7 with repeat = 2 (4 slots, the last of one row), K = 5, 3 iterations, 2 elites: every
    output equals the host loop's, on a run that has a tie across the elite boundary, a best candidate other than 0
    in iteration 0 and an improvement between iterations (see the module docstring for how it was chosen)"""
    H, K, rep, iters, E = 7, 5, 2, 3, 2
    a = warm(make(CORNER), warm_script())
    got = a.plan_cem(H, K, iters, E, alpha=1, repeat=rep, key=42, step=0, details=True)
    assert list(got) == ["best", "best_score", "first_action", "plan", "weights", "iter_best", "actions", "scores",
                         "steps", "errors"]
    want = host_cem(a, H, K, iters, E, alpha=1, repeat=rep, key=42, step=0)
    agree(got, want)
    assert got["weights"].shape == (4, 18, N) and got["weights"].dtype == torch.uint16
    assert got["plan"].shape == (H, N) and got["iter_best"].shape == (iters, N)
    tie = False
    for cand, scores, best in want["history"]:
        ranked = -np.sort(-scores, axis=0)
        tie = tie or bool((ranked[E - 1] == ranked[E]).any())
    assert tie, "no env with equal scores on both sides of the elite boundary: the tie rule is not exercised"
    assert (want["history"][0][2] != 0).any(), "every env's best candidate of iteration 0 is candidate 0"
    ib = want["iter_best"]
    assert (ib[1:] > ib[:-1]).any(), "no env improves between iterations"
    totals = got["weights"].cpu().numpy().astype(np.int64).sum(axis=1)
    assert totals.min() == 18 + E == totals.max()
    plain = a.plan_cem(H, K, iters, E, alpha=1, repeat=rep, key=42, step=0)
    assert list(plain) == ["best", "best_score", "first_action", "plan", "weights", "iter_best"]
    agree(plain, want, "plain", list(plain))
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [REGION, CORNER])
def test_wide_k(name):
    """K = 70: more than one wavefront of candidates and no multiple of 64; 9 elites, alpha = 0 (weights with zeros).
    MoveToRegion's scores are binary: an env whose 70 scores are all equal exists (asserted), and the rank rule alone
    picks its elites (k < 9); MoveToCorner's are graded"""
    H, K, iters, E = 3, 70, 2, 9
    a = warm(make(name), warm_script())
    got = a.plan_cem(H, K, iters, E, alpha=0, key=42, step=0, details=True)
    want = host_cem(a, H, K, iters, E, alpha=0, key=42, step=0)
    agree(got, want, name)
    flat = [bool((s.min(axis=0) == s.max(axis=0)).any()) for _, s, _ in want["history"]]
    if name == REGION:
        assert all(flat), "no env with all-equal scores"
        s = want["history"][-1][1]
        e = int(np.argmax(s.min(axis=0) == s.max(axis=0)))
        assert elites_of(s, E)[:, e].tolist() == list(range(E))
    else:
        assert len(np.unique(want["scores"])) > 50
    w = got["weights"].cpu().numpy().astype(np.int64)
    assert w.min() == 0 and w.sum(axis=1).min() == E == w.sum(axis=1).max()
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rep", [1, 2])
def test_one_iteration_is_sample_plans_and_plan(rep):
    H, K, key, step = 7, 5, 9, (1 << 33) + 5
    a = warm(make(CORNER), warm_script())
    got = a.plan_cem(H, K, 1, 2, repeat=rep, key=key, step=step, details=True)
    acts = a.sample_plans(H, K, repeat=rep, key=key, step=step)
    assert torch.equal(got["actions"], acts)
    ref = a.plan(acts, details=True)
    for k in ref:
        assert torch.equal(got[k], ref[k]), k
    assert torch.equal(got["iter_best"][0], ref["best_score"])
    assert torch.equal(got["plan"], acts[:, ref["best"].long(), torch.arange(N, device="cuda")])
    w = refit(acts.cpu().numpy(), ref["scores"].cpu().numpy(), 2, 1, rep)
    assert np.array_equal(got["weights"].cpu().numpy(), w)
    a.close()


@pytest.mark.gpu
def test_incumbent():
    a = warm(make(CORNER), warm_script())
    res = a.plan_cem(7, 5, 4, 2, repeat=2, key=3, details=True)
    ib = res["iter_best"]
    assert bool((ib[1:] >= ib[:-1]).all()) and bool((ib[1:] > ib[:-1]).any())
    assert torch.equal(ib[-1], res["best_score"])
    two = a.plan_cem(7, 5, 2, 2, repeat=2, key=3, details=True)
    assert torch.equal(two["scores"][0], two["iter_best"][0])   # candidate 0 of iteration 1 is iteration 0's best
    assert torch.equal(two["iter_best"], ib[:2])                # and a longer call starts as the shorter one does
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,n,pair", FORMS)
def test_forms(name, env, n, pair, monkeypatch):
    """every compiled (form, envs per workgroup) pair, 2 iterations"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    K = 3 if n == N else 5
    a = warm(make(name, n), warm_script(n))
    assert a.step_form()[:2] == pair
    got = a.plan_cem(7, K, 2, 2, repeat=2, key=5, step=11, details=True)
    agree(got, host_cem(a, 7, K, 2, 2, repeat=2, key=5, step=11), name)
    a.close()


@pytest.mark.gpu
def test_warm_start():
    """iters = 1 + 1 with the weights handed over = the host's draw from them; zero-total weights draw uniformly"""
    H, K, E, rep, key, step = 7, 5, 2, 2, 42, 100
    J = 4
    a = warm(make(CORNER), warm_script())
    first = a.plan_cem(H, K, 1, E, repeat=rep, key=key, step=step, details=True)
    w1 = first["weights"].cpu().numpy()
    w = dev_weights(w1)
    second = a.plan_cem(H, K, 1, E, repeat=rep, key=key, step=step + K * J, weights=w, details=True)
    assert second["weights"] is w   # updated in place
    assert np.array_equal(second["actions"].cpu().numpy(), candidates(w1, H, K, rep, key, step + K * J, 0))
    agree(second, host_cem(a, H, K, 1, E, repeat=rep, key=key, step=step + K * J, weights=w1), "second")
    assert not np.array_equal(second["actions"].cpu().numpy(), a.sample_plans(H, K, rep, key, step + K * J).cpu().numpy())
    # alpha = 0 weights (zeros in them), and slot 1 of env 2 emptied altogether: T = 0 draws as all ones
    z = a.plan_cem(H, K, 1, E, alpha=0, repeat=rep, key=key, step=step)["weights"].cpu().numpy()
    z[1, :, 2] = 0
    third = a.plan_cem(H, K, 2, E, alpha=0, repeat=rep, key=key, step=7, weights=dev_weights(z), details=True)
    agree(third, host_cem(a, H, K, 2, E, alpha=0, repeat=rep, key=key, step=7, weights=z), "third")
    with pytest.raises(ValueError):
        a.plan_cem(H, K, 1, E, repeat=rep, weights=torch.empty((J, 18, N + 1), dtype=torch.uint16, device="cuda"))
    with pytest.raises(ValueError):
        a.plan_cem(H, K, 1, E, repeat=rep, weights=torch.ones((J, 18, N), dtype=torch.int16, device="cuda"))
    with pytest.raises(ValueError):
        a.plan_cem(H, 0, 1, E)
    a.close()


@pytest.mark.gpu
def test_cem_policy_warm_start():
    """CEMPolicy(warm_start=True) over 3 decisions = its host restatement on a twin: cem_step counters, the weights
    shifted one slot with the last slot all ones; two runs with the same key are identical"""
    H, K, iters, E, key = 4, 5, 2, 2, 5
    a = magical_amd.make_vec(CORNER, N, base_seed=1000, debug_reward=True)
    b = magical_amd.make_vec(CORNER, N, base_seed=1000, debug_reward=True)
    policy = magical_amd.CEMPolicy(a, horizon=H, candidates=K, iters=iters, elites=E, key=key, warm_start=True)
    obs, _ = a.reset(), b.reset()
    w, taken = None, []
    for t in range(3):
        act = policy(obs)
        assert act.shape == (N,) and act.dtype == torch.uint8
        want = host_cem(b, H, K, iters, E, key=key, step=t * iters * K * H, weights=w)
        agree(policy.last, want, t, ["best", "best_score", "first_action", "plan", "iter_best", "weights"])
        assert np.array_equal(act.cpu().numpy(), want["first_action"])
        w = np.concatenate([want["weights"][1:], np.ones((1, 18, N), dtype=np.uint16)])
        assert np.array_equal(policy.weights.cpu().numpy(), w)
        taken.append(act.clone())
        obs, _, _, _ = a.step(act)
        b.step(act)
    policy.reset()
    assert policy.t == 0 and policy.weights is None
    assert len(torch.unique(torch.stack(taken))) > 1
    a.close(), b.close()


@pytest.mark.gpu
def test_sim_is_untouched():
    """a many-block task with the next-layout shadow, episodes of 9 steps with staggered phases: after plan_cem() the
    following steps, across auto-resets, give the bytes of a twin that never planned; then the same with window rings"""
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
    res = a.plan_cem(7, 3, 2, 2, repeat=2, key=11, step=3, details=True)
    assert 1 <= int(res["steps"].min()) < 7
    after = (a.bodies(), a.errors(), a.arbiters(), a.lookahead(acts[6:13], bodies=True))
    assert torch.equal(before[0][0], after[0][0]) and torch.equal(before[0][1], after[0][1])
    assert torch.equal(before[1], after[1])
    assert torch.equal(before[2][0], after[2][0]) and torch.equal(before[2][1].view(torch.int64), after[2][1].view(torch.int64))
    same(after[3], before[3], "lookahead after plan_cem")
    resets = 0
    for t in range(6, 12):
        if t == 9:
            a.plan_cem(4, 2, 2, 1)   # again, between auto-reset steps
        ga, gc = step_out(a, acts[t]), step_out(c, acts[t])
        same(ga, gc, t)
        resets += int(gc["done"].sum())
    assert resets > 0
    a.close(), c.close()
    a, c = make(REGION, L=L, window=True), make(REGION, L=L, window=True)
    for s in (a, c):
        s.reset()
        s.set_episode_steps(torch.arange(N) % L)
    plain = make(REGION, L=L)
    plain.reset()
    plain.set_episode_steps(torch.arange(N) % L)
    resets = 0
    for t in range(8):
        if t in (3, 6):
            got = a.plan_cem(5, 3, 2, 2, key=4, step=t, details=True)
            agree(got, host_cem(plain, 5, 3, 2, 2, key=4, step=t), ("window", t))
        ga, gc = step_out(a, acts[t]), step_out(c, acts[t])
        same(ga, gc, ("window", t))
        plain.step(acts[t])
        resets += int(gc["done"].sum())
    assert resets > 0
    a.close(), c.close(), plain.close()


@pytest.mark.gpu
def test_refusals_launch_nothing():
    H, K, J = 7, 3, 4
    a = warm(make(REGION), warm_script())
    big = make(REGION, 128)
    lib = native.load()
    i32, f64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float64, device="cuda")
    bufs = dict(best=torch.full((N,), -7, **i32), best_score=torch.full((N,), -7.0, **f64),
                first_action=torch.full((N,), 99, dtype=torch.uint8, device="cuda"),
                scores=torch.full((K, N), -7.0, **f64), steps=torch.full((K, N), -7, **i32),
                errors=torch.full((K, N), -7, **i32), iter_best=torch.full((2, N), -7.0, **f64))
    acts = torch.full((H, K, N), 99, dtype=torch.uint8, device="cuda")
    wts = torch.full((J, 18, N), 777, dtype=torch.int16, device="cuda")
    keep = {k: v.clone() for k, v in bufs.items()}
    out = native.mg_plan_cem_out(**{k: v.data_ptr() for k, v in bufs.items()})
    nobest = native.mg_plan_cem_out(**{k: v.data_ptr() for k, v in bufs.items() if k != "best"})
    ap, wp, st, o = ctypes.c_void_p(acts.data_ptr()), ctypes.c_void_p(wts.data_ptr()), a._stream(), ctypes.byref(out)

    def call(sim=a, actions=ap, weights=wp, warm=0, H=H, K=K, iters=2, elites=2, alpha=1, repeat=2, out=o):
        return lib.mg_plan_cem(sim.handle if sim is not None else None, actions, weights, warm, H, K, iters, elites,
                               alpha, repeat, 42, 0, out, st if sim is not big else big._stream())

    def refused(rc, word):
        assert rc == -22 and word in lib.mg_last_error().decode(), (word, lib.mg_last_error())

    refused(call(H=0), "H")
    refused(call(H=4097), "H")
    refused(call(K=0), "K")
    refused(call(K=4097), "K")
    refused(call(sim=big, K=2049), "K * num_envs")      # 262272 > MG_PLAN_MAX_ROLLOUTS
    refused(call(iters=0), "iters")
    refused(call(iters=65), "iters")
    refused(call(elites=0), "elites")
    refused(call(elites=K + 1), "elites")
    refused(call(alpha=-1), "alpha")
    refused(call(alpha=1025), "alpha")
    refused(call(repeat=0), "repeat")
    refused(call(warm=2), "warm")
    refused(call(sim=None), "null")
    refused(call(actions=None), "actions_dev")
    refused(call(weights=None), "weights_dev")
    refused(call(out=None), "out")
    refused(call(out=ctypes.byref(nobest)), "out->best")
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert torch.equal(v, keep[k]), k
    assert bool((acts == 99).all()) and bool((wts == 777).all())
    with pytest.raises(native.NativeError):
        a.plan_cem(H, K, 65, 2)
    with pytest.raises(native.NativeError):
        a.plan_cem(H, K, 2, K + 1)
    # and the sim plans as if nothing had happened, at the ranges' ends too
    agree(a.plan_cem(H, K, 2, K, alpha=1024, repeat=2, details=True), host_cem(a, H, K, 2, K, alpha=1024, repeat=2))
    assert call() == 0
    torch.cuda.synchronize()
    assert int(acts.max()) < 18 and int(wts.min()) >= 1 and not torch.equal(bufs["best_score"], keep["best_score"])
    assert torch.equal(bufs["best_score"], bufs["iter_best"][1])
    a.close(), big.close()


@pytest.mark.gpu
def test_pool_env_and_single_env():
    H, K, iters, E, rep, key, step = 7, 3, 2, 2, 2, 42, 9
    acts = warm_script()
    pool = PipelinedVecEnv(REGION, N, chunks=3, base_seed=1000, max_episode_steps=FAR)
    assert pool.bounds == [0, 4, 8, 13]
    pool.reset()
    for t in range(W):
        pool.step(acts[t])
    got = pool.plan_cem(H, K, iters, E, repeat=rep, key=key, step=step, details=True)
    assert got["actions"].shape == (H, K, N) and got["weights"].shape == (4, 18, N) and got["iter_best"].shape == (iters, N)
    b = pool.bounds
    for c, sim in enumerate(pool.sims):
        want = sim.plan_cem(H, K, iters, E, repeat=rep, key=key + c, step=step, details=True)
        assert list(got) == list(want)
        for k, v in want.items():
            g = got[k][..., b[c]:b[c + 1]]
            assert g.shape == v.shape and np.array_equal(g.cpu().numpy(), v.cpu().numpy()), (c, k)
    # a warm start through the pool: updated in place, equal to the chunks' own
    w = got["weights"].view(torch.int16).clone().view(torch.uint16)
    again = pool.plan_cem(H, K, 1, E, repeat=rep, key=key, step=step + 50, weights=w)
    assert again["weights"] is w
    for c, sim in enumerate(pool.sims):
        wc = got["weights"].view(torch.int16)[:, :, b[c]:b[c + 1]].contiguous().view(torch.uint16)
        want = sim.plan_cem(H, K, 1, E, repeat=rep, key=key + c, step=step + 50, weights=wc)
        assert np.array_equal(w[:, :, b[c]:b[c + 1]].cpu().numpy(), wc.cpu().numpy()), c
        assert torch.equal(again["best_score"][b[c]:b[c + 1]], want["best_score"]), c
    pool.close()
    env = mg_envs.MagicalEnv(CORNER, seed=5)
    with pytest.raises(RuntimeError):
        env.plan_cem(6, 4, 2, 2)
    env.reset()
    for t in range(W):
        env.step(1)
    plan, best_score, iter_best = env.plan_cem(6, 4, 3, 2, repeat=2, key=8, step=1)
    want = env._vec.plan_cem(6, 4, 3, 2, repeat=2, key=8, step=1)
    assert plan.dtype == np.uint8 and plan.shape == (6,) and iter_best.dtype == np.float64 and iter_best.shape == (3,)
    assert np.array_equal(plan, want["plan"][:, 0].cpu().numpy()) and best_score == float(want["best_score"][0])
    assert np.array_equal(iter_best, want["iter_best"][:, 0].cpu().numpy())
    assert env.lookahead(plan)[0] == best_score
    env.close()
