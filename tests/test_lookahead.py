"""GPU: mg_lookahead (VecMagicalEnv.lookahead / score, PipelinedVecEnv.lookahead, MagicalEnv.score).

Every comparison is bit-exact (torch.equal) against twins of the same name and seeds that are stepped through the same
actions with mg_step, which the parity suite pins to the oracle.  13 envs: at 8 envs per workgroup the last workgroup
has 5 real and 3 shadow envs, at 16 one workgroup has 13 real and 3 shadow ones; plus 1-env cases.  The action script
(forward-biased, seed 7) and the 20 warm-up steps were chosen on the CPU with the C oracle so that after 1, 7 and 40
further steps some of the 13 envs have live arbiters in every task used here: warm-start state crosses the H-loop.
"""
import ctypes

import numpy as np
import pytest
import torch

from magical_amd import envs as mg_envs
from magical_amd import native
from magical_amd.pipeline import PipelinedVecEnv

N, W, FAR = 13, 20, 1000   # envs, warm-up steps, an episode length no test reaches
HS = (1, 7, 40)

REGION, CORNER = "MoveToRegion-Demo-LoRes4E-v0", "MoveToCorner-Demo-LoRes4E-v0"
CLUSTER, MATCH = "ClusterColour-Demo-LoResStack-v0", "MatchRegions-TestAll-LoRes4E-v0"


def script(steps, n=N, seed=7):
    """[steps, n] actions: 70% forward with open fingers (action 1), the rest uniform"""
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 18, (steps, n))
    a[rs.rand(steps, n) < 0.7] = 1
    return torch.as_tensor(a.astype(np.uint8)).cuda()


def make(name, n=N, L=FAR, **kw):
    return mg_envs.VecMagicalEnv(name, n, base_seed=1000, max_episode_steps=L, **kw)


def warm(env, acts, steps=W):
    env.reset()
    for t in range(steps):
        env.step(acts[t])
    return env


def twins(name, count, acts, n=N, L=FAR, **kw):
    """`count` warmed-up sims in the same state; all but the first keep their terminal state (auto_reset=False)"""
    return [warm(make(name, n, L, **(kw if k == 0 else dict(kw, auto_reset=False))), acts) for k in range(count)]


def step_out(env, a):
    obs, rew, done, info = env.step(a)
    out = {"obs." + k: v.clone() for k, v in obs.items()}
    out.update(reward=rew.clone(), done=done.clone(), eval_score=info["eval_score"].clone())
    out["bodies"], out["counts"] = env.bodies()
    return out


def same(got, want, ctx):
    for k, w in want.items():
        assert torch.equal(got[k], w), (ctx, k)


# name, env vars set before the sim is created, envs, the (form, envs per workgroup) it must run
FORMS = [(REGION, {}, N, (5, 8)), (REGION, {"MG_STEP_BLK": "16"}, N, (5, 16)),
         (CORNER, {}, N, (6, 8)), (CORNER, {"MG_STEP_BLK": "16"}, N, (6, 16)),
         (CLUSTER, {}, N, (4, 1)), (MATCH, {}, N, (4, 1)),
         (MATCH, {"MG_STEP_VARIANT": "0"}, N, (0, 64)), (CORNER, {"MG_STEP_VARIANT": "0", "MG_STEP_BLK0": "8"}, N, (0, 8)),
         (REGION, {}, 1, (5, 8)), (CLUSTER, {}, 1, (4, 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,n,pair", FORMS)
def test_bit_identical_to_stepping(name, env, n, pair, monkeypatch):
    """bodies and counts after a lookahead of H actions = those of a twin stepped through them, for every compiled form
    (1, 7 and 40 steps from the same state: the lookahead leaves it alone), with live arbiters at every horizon"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    acts = script(W + max(HS), n)
    a, b = twins(name, 2, acts, n)
    assert a.step_form()[:2] == pair
    done = 0
    for H in HS:
        la = a.lookahead(acts[W:W + H], bodies=True)
        for t in range(done, H):
            b.step(acts[W + t])
        done = H
        bodies, counts = b.bodies()
        assert torch.equal(la["bodies"], bodies) and torch.equal(la["counts"], counts), H
        assert torch.equal(la["steps"], torch.full((n,), H, dtype=torch.int32, device="cuda"))
        assert torch.equal(la["errors"], b.errors())
        assert bool((counts[:, 3] > 0).any()), ("no live arbiter: the case exercises no contact", H)
    a.close(), b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 65, 70])
@pytest.mark.parametrize("name", [REGION, CLUSTER])
def test_ragged_env_counts_and_separate_pools(name, n):
    """The scratch copy is mg_plan's fan-out with one candidate.  Env counts that are no multiple of 4 (the last lane's
    packed 1- and 2-byte words would run past the last env) or of 64: a lookahead of 3 actions = a twin stepped through
    them, the sim's state dumps before = after.  Then lookahead, plan (2 candidates, its own pool), lookahead on the
    same sim: what a sim that only ever looked ahead returns, and the next step of both is the same."""
    H, W0 = 3, 6
    acts = script(W0 + H + 1, n)
    a, b, c = (warm(make(name, n, **kw), acts, W0) for kw in ({}, {"auto_reset": False}, {}))
    before = (a.bodies(), a.errors(), a.arbiters())
    la = a.lookahead(acts[W0:W0 + H], bodies=True)
    after = (a.bodies(), a.errors(), a.arbiters())
    assert torch.equal(before[0][0], after[0][0]) and torch.equal(before[0][1], after[0][1])
    assert torch.equal(before[1], after[1])
    assert torch.equal(before[2][0], after[2][0]) and torch.equal(before[2][1].view(torch.int64), after[2][1].view(torch.int64))
    for t in range(H):
        b.step(acts[W0 + t])
    bodies, counts = b.bodies()
    assert torch.equal(la["bodies"], bodies) and torch.equal(la["counts"], counts)
    assert torch.equal(la["steps"], torch.full((n,), H, dtype=torch.int32, device="cuda"))
    assert torch.equal(la["errors"], b.errors())
    cands = torch.stack([acts[W0:W0 + H], acts[W0 + 1:W0 + H + 1]], dim=1)   # [H, 2, n]
    plan = a.plan(cands, details=True)
    assert torch.equal(plan["scores"][0], la["score"])   # candidate 0 is the lookahead's sequence
    again = a.lookahead(acts[W0:W0 + H], bodies=True)
    only = [c.lookahead(acts[W0:W0 + H], bodies=True) for _ in range(2)]
    same(la, only[0], "first"), same(again, only[1], "after a plan")
    same(step_out(a, acts[W0 + H]), step_out(c, acts[W0 + H]), "next step")
    a.close(), b.close(), c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,L", [(REGION, FAR), (CORNER, FAR), ("MatchRegions-TestAll-LoResStack-v0", 9),
                                    ("PickAndPlace-Demo-LoRes4E-v0", 9)])
def test_sim_is_untouched(name, L):
    """state dumps before = after; the following steps (L = 9, phases staggered: across auto-resets, from the next-layout
    shadow for the many-block tasks) give the bytes of a twin that never looked ahead"""
    acts = script(W + 12)
    sims = [make(name, L=L), make(name, L=L)]
    for s in sims:
        s.reset()
        if L != FAR:
            s.set_episode_steps(torch.arange(N) % L)
        for t in range(6):
            s.step(acts[t])
    a, c = sims
    before = (a.bodies(), a.errors(), a.arbiters())
    la = a.lookahead(acts[6:13])
    assert int(la["steps"].min()) >= 1 and (L == FAR or int(la["steps"].min()) < 7)
    after = (a.bodies(), a.errors(), a.arbiters())
    assert torch.equal(before[0][0], after[0][0]) and torch.equal(before[0][1], after[0][1])
    assert torch.equal(before[1], after[1])
    assert torch.equal(before[2][0], after[2][0]) and torch.equal(before[2][1].view(torch.int64), after[2][1].view(torch.int64))
    resets = 0
    for t in range(6, 12):
        if t == 9:
            a.lookahead(acts[0:3])   # again, between auto-reset steps
        ga, gc = step_out(a, acts[t]), step_out(c, acts[t])
        same(ga, gc, t)
        resets += int(gc["done"].sum())
    assert L == FAR or resets > 0
    a.close(), c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", [(REGION, {}), (CORNER, {"MG_STEP_BLK": "16"}), (CLUSTER, {}),
                                      (MATCH, {"MG_STEP_VARIANT": "0"})], ids=["region-5/8", "corner-6/16", "cluster-4", "match-0"])
def test_early_end_and_per_env_horizons(name, env, monkeypatch):
    """envs 3 steps from their episode's end stop there with mg_step's eval_score; in a mixed batch (3 left, 0 left,
    far) every env gets its own horizon, workgroup neighbours of an early-ending env included"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L, H = 60, 8
    acts = script(W + H)
    for mixed in (False, True):
        a, b = twins(name, 2, acts, L=L)
        left = torch.tensor([(3, 0, H)[e % 3] for e in range(N)]) if mixed else torch.full((N,), 3)
        phase = torch.where(left == H, torch.full((N,), W), L - left)   # far envs keep their phase (40 steps left)
        a.set_episode_steps(phase), b.set_episode_steps(phase)
        la = a.lookahead(acts[W:], bodies=True)
        want_b, want_c = b.bodies()
        want_b, want_c = want_b.clone(), want_c.clone()
        score = torch.full((N,), float("nan"), dtype=torch.float64, device="cuda")
        for t in range(H):
            out = step_out(b, acts[W + t])
            at = (left == t + 1).cuda()
            want_b[at], want_c[at] = out["bodies"][at], out["counts"][at]
            ends = at & (left < H).cuda()
            assert bool(out["done"][ends].all())
            score[ends] = out["eval_score"][ends]
        assert torch.equal(la["steps"].cpu(), left.to(torch.int32)), mixed
        assert torch.equal(la["bodies"], want_b) and torch.equal(la["counts"], want_c), mixed
        known = ~torch.isnan(score)
        assert bool(known.any()) and torch.equal(la["score"][known], score[known]), mixed
        a.close(), b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [REGION, CORNER, CLUSTER, MATCH])
def test_mid_episode_score(name):
    """the score of a state that is nowhere near its episode's end = the eval_score of a twin whose episode ends there;
    score() (H = 0) is the same number for the state as it stands"""
    L, H = 60, 7
    acts = script(W + H)
    a, b = warm(make(name), acts), warm(make(name, L=L, auto_reset=False), acts)
    b.set_episode_steps(torch.full((N,), L - H))
    la = a.lookahead(acts[W:])
    for t in range(H):
        out = step_out(b, acts[W + t])
    assert bool(out["done"].all()) and torch.equal(la["steps"], torch.full((N,), H, dtype=torch.int32, device="cuda"))
    assert torch.equal(la["score"], out["eval_score"])
    for t in range(H):
        a.step(acts[W + t])
    assert torch.equal(a.score(), out["eval_score"])
    assert torch.equal(a.lookahead(acts[:0])["steps"], torch.zeros(N, dtype=torch.int32, device="cuda"))
    a.close(), b.close()


@pytest.mark.gpu
def test_single_env_score():
    env = mg_envs.MagicalEnv(CORNER, seed=5)
    with pytest.raises(RuntimeError):
        env.score()
    env.reset()
    acts = [1] * env.max_episode_steps
    ahead, steps = env.lookahead(acts + [1, 1])
    for k, a in enumerate(acts):
        _, _, done, info = env.step(a)
    assert done and steps == len(acts) and ahead == info["eval_score"] == env.score()
    env.close()


@pytest.mark.gpu
def test_broadcast_planning_round_trip():
    """one recorded state broadcast to 13 envs, 13 candidate action sequences: candidate k = a 1-env sim restored from
    the same record and stepped through sequence k"""
    name, H = "MoveToCorner-Demo-LoResStack-v0", 12
    acts = script(W + H)
    pool = warm(make(name), acts)
    snap = pool.snapshot(envs=[0])
    pool.restore(snap, recs=[0] * N)
    la = pool.lookahead(acts[W:], bodies=True)
    assert not torch.equal(la["bodies"][0], la["bodies"][5])   # the candidates differ
    one = make(name, 1, auto_reset=False)
    one.reset()
    for k in (0, 5, 12):
        one.restore(snap)
        for t in range(H):
            one.step(acts[W + t, k:k + 1])
        bodies, counts = one.bodies()
        assert torch.equal(la["bodies"][k], bodies[0]) and torch.equal(la["counts"][k], counts[0]), k
        assert float(la["score"][k]) == float(one.score()[0])
    pool.close(), one.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["window", "frames_only", "unwrapped"])
def test_modes(mode):
    """window rings, frames_only outputs and the unwrapped surface: the same numbers as the plain env's twin"""
    H = 7
    acts = script(W + H)
    name = "MoveToRegion-Demo-v0" if mode == "unwrapped" else REGION
    a = make(name, window=(mode == "window"))
    if mode == "frames_only":
        a.bind_outputs(a.output_buffers(), frames_only=True)
    warm(a, acts)
    b = warm(make(REGION, auto_reset=False), acts)
    la = a.lookahead(acts[W:], bodies=True)
    for t in range(H):
        b.step(acts[W + t])
    bodies, counts = b.bodies()
    assert torch.equal(la["bodies"], bodies) and torch.equal(la["counts"], counts)
    a.close(), b.close()


@pytest.mark.gpu
def test_refusals_launch_nothing():
    acts = script(W + 3)
    a, b = twins(REGION, 2, acts)
    lib = native.load()
    score = torch.zeros(N, dtype=torch.float64, device="cuda")
    out = native.mg_lookahead_out(score=score.data_ptr())
    ap, st = ctypes.c_void_p(acts.data_ptr()), a._stream()
    assert lib.mg_lookahead(a.handle, ap, -1, ctypes.byref(out), st) == -22
    assert lib.mg_lookahead(a.handle, ap, 4097, ctypes.byref(out), st) == -22
    assert lib.mg_lookahead(a.handle, None, 1, ctypes.byref(out), st) == -22
    assert lib.mg_lookahead(a.handle, ap, 1, None, st) == -22
    assert lib.mg_lookahead(None, ap, 1, ctypes.byref(out), st) == -22
    assert lib.mg_lookahead(a.handle, ap, 1, ctypes.byref(native.mg_lookahead_out()), st) == -22   # null score
    with pytest.raises(native.NativeError):
        a.lookahead(torch.zeros((4097, N), dtype=torch.uint8))
    with pytest.raises(ValueError):
        a.lookahead(torch.zeros((2, N + 1), dtype=torch.uint8))
    assert lib.mg_lookahead(a.handle, None, 0, ctypes.byref(out), st) == 0   # H = 0: score only, no actions needed
    for t in range(W, W + 3):
        same(step_out(a, acts[t]), step_out(b, acts[t]), t)
    a.close(), b.close()


@pytest.mark.gpu
def test_pool_matches_batch():
    H = 7
    acts = script(W + H)
    vec = warm(make(REGION), acts)
    pool = PipelinedVecEnv(REGION, N, chunks=3, base_seed=1000, max_episode_steps=FAR)
    assert pool.bounds == [0, 4, 8, 13]
    pool.reset()
    for t in range(W):
        pool.step(acts[t])
    got, want = pool.lookahead(acts[W:], bodies=True), vec.lookahead(acts[W:], bodies=True)
    assert list(got) == list(want)
    same(got, want, "pool")
    assert got["bodies"].shape == (N, 16, 6)
    pool.close(), vec.close()
