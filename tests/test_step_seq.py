"""GPU: mg_step_seq (VecMagicalEnv.step_seq / step_repeat, MagicalEnv.step_seq, PipelinedVecEnv.step_seq, sb3 frame_skip).

Every comparison is bit-exact (torch.equal / byte equality): both sides run the same device functions.  Episodes are
L = 12 env-steps long and a call runs R in {1, 4, 7}; before a call the envs' episode phases are staggered with
set_episode_steps so that a batch holds envs that end at step 1 of the call, at a middle step, exactly at step R, not at
all, and envs already past their end (which take one step, as mg_step's do).  The action script, seeds and warm-up are
tests/test_lookahead.py's, chosen there so that contacts are live inside the loop; the warm-up runs with the episode
counter far below zero so that no episode ends in it.
"""
import numpy as np
import pytest
import torch

from magical_amd import envs as mg_envs
from magical_amd.pipeline import PipelinedVecEnv
from test_lookahead import CLUSTER, CORNER, HS, MATCH, N, REGION, W, script
from test_step_seq_host import seq_done, seq_horizon, seq_reward

L = 12
RS = (1, 4, 7)
GROUPS = ("first", "middle", "last", "none", "past")


def lefts(R, n=N, rot=0):
    """steps left in the episode per env (<= 0: already past its end), and the group of each env.  Env k % n takes
    entry k + rot of: ends at step 1, at a middle step, at step R, past its end by 0 and by 2, then envs that do not
    end (the most: they are the ones whose bodies are compared with the lookahead's)"""
    mid = {1: 1, 4: 2, 7: 3}[R]
    table = [(1, "first"), (mid, "middle" if 1 < mid < R else "first"), (R, "last" if R > 1 else "first"), (0, "past"),
             (-2, "past")] + [(R + 1 + k % (L - R), "none") for k in range(8)]
    pick = [table[(k + rot) % len(table)] for k in range(n)]
    return np.array([p[0] for p in pick]), [p[1] for p in pick]


def groups_possible(R):
    return {"first", "none", "past"} | ({"last"} if R > 1 else set()) | ({"middle"} if R > 2 else set())


def make(name, n=N, **kw):
    return mg_envs.VecMagicalEnv(name, n, base_seed=1000, max_episode_steps=L, **kw)


def warm(env, acts, steps=W):
    env.reset()
    env.set_episode_steps(torch.full((env.num_envs,), -10000))   # no episode ends in the warm-up
    for t in range(steps):
        env.step(acts[t])
    return env


def phase(env, left):
    env.set_episode_steps(torch.as_tensor(L - left))


def f32_bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# name, constructor arguments, env vars set before the sim is created, the (form, envs per workgroup) it must run
PAIRS = [(REGION, {}, {}, (5, 8)), (REGION, {}, {"MG_STEP_BLK": "16"}, (5, 16)),
         (REGION, {}, {"MG_STEP_VARIANT": "0", "MG_STEP_BLK0": "8"}, (0, 8)), (REGION, {}, {"MG_STEP_VARIANT": "0"}, (0, 64)),
         (REGION, {}, {"MG_STEP_VARIANT": "0", "MG_STEP_BLK0": "1"}, (0, 1)),
         (CORNER, {}, {}, (6, 8)), (CORNER, {}, {"MG_STEP_BLK": "16"}, (6, 16)),
         (CORNER, {}, {"MG_STEP_VARIANT": "0", "MG_STEP_BLK0": "8"}, (0, 8)),
         (CORNER, {"debug_reward": True}, {}, (6, 8)), (CORNER, {"debug_reward": True}, {"MG_STEP_BLK": "16"}, (6, 16)),
         (CORNER, {"debug_reward": True}, {"MG_STEP_VARIANT": "0", "MG_STEP_BLK0": "8"}, (0, 8)),
         (CLUSTER, {}, {}, (4, 1)), (CLUSTER, {}, {"MG_STEP_VARIANT": "0", "MG_STEP_BLK0": "8"}, (0, 8)),
         (MATCH, {}, {}, (4, 1)), (MATCH, {}, {"MG_STEP_VARIANT": "0", "MG_STEP_BLK0": "8"}, (0, 8))]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [N, 1])
@pytest.mark.parametrize("name,kw,env,pair", PAIRS)
def test_every_compiled_pair_against_the_lookahead(name, kw, env, pair, n, monkeypatch):
    """steps, the terminal eval_score, the summed reward and, for envs that did not end, the bodies = what a traced
    lookahead of the same actions, taken on the same sim just before the call, reports (it does not mutate).  An env past
    its end is not in the lookahead (0 steps there): it takes one step and is done.  13 envs hold all five groups at once
    (at R = 1 and 4 those that exist); one env goes through them call by call, restored to the warmed state in between."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    acts = script(W + max(HS), n)
    a = warm(make(name, n, **kw), acts)
    assert a.step_form()[:2] == pair
    snap = a.snapshot()
    live = False
    for R in RS:
        seen = set()
        for rot in (range(1) if n > 1 else range(6)):
            left, grp = lefts(R, n, rot)
            seen |= set(grp)
            a.restore(snap)
            phase(a, left)
            chunk = acts[W:W + R]
            la = a.lookahead(chunk, bodies=True, trace=True)
            la = {k: v.clone() for k, v in la.items()}
            obs, rew, done, info = a.step_seq(chunk)
            want_n, want_d = seq_horizon(R, L, L - left), seq_done(R, L, L - left)
            ctx = (R, rot)
            assert np.array_equal(info["steps"].cpu().numpy(), want_n), ctx
            assert np.array_equal(done.cpu().numpy().astype(bool), want_d), ctx
            inla = torch.as_tensor(left >= 1).cuda()   # envs the lookahead simulates
            ended = torch.as_tensor(want_d).cuda()
            assert torch.equal(info["steps"][inla], la["steps"][inla]), ctx
            assert torch.equal(info["eval_score"][ended & inla], la["score"][ended & inla]), ctx
            assert bool((info["eval_score"][~ended] == 0.0).all()), ctx
            want_r = torch.as_tensor(seq_reward(la["reward_trace"].cpu().numpy(), want_n))
            assert torch.equal(f32_bits(rew)[inla.cpu()], f32_bits(want_r)[inla.cpu()]), ctx
            if not a.debug_reward:
                assert torch.equal(rew, info["eval_score"].to(torch.float32)), ctx
            bodies, counts = a.bodies()
            assert torch.equal(bodies[~ended], la["bodies"][~ended]) and torch.equal(counts[~ended], la["counts"][~ended]), ctx
            assert torch.equal(a.errors()[~ended], la["errors"][~ended]), ctx
            live = live or bool((counts[~ended][:, 3] > 0).any())
        assert seen == groups_possible(R), (R, seen)
    assert live or n == 1, "no compared env has a live arbiter at the end of a chunk: the case exercises no contact"
    a.close()


def record(env, out=None):
    obs = env._obs() if out is None else out[0]
    rec = {"allo": obs["allo"].clone(), "ego": obs["ego"].clone(), "done": env.done.clone(),
           "eval_score": env.eval_score.clone(), "reward": env.reward.clone(), "errors": env.errors()}
    rec["bodies"], rec["counts"] = env.bodies()
    rec["arb"], hs = env.arbiters()
    rec["arb_hash"] = hs.view(torch.int64)
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [(REGION, {}), (CORNER, {"debug_reward": True}), (MATCH, {}), (CLUSTER.replace("LoResStack", "LoRes4E"), {}),
                                     (REGION, {"auto_reset": False}), (MATCH, {"auto_reset": False})],
                         ids=["region-fused", "corner-fused-debug", "match-shadow", "cluster-shadow", "region-noreset", "match-noreset"])
def test_against_mg_step(name, kw):
    """three chunks in a row (R = 7, 4, 1); before each, a twin is restored from a snapshot of the env and then stepped R
    times with mg_step.  For env e the twin's record after its step n_e = step_seq's done, eval_score, bodies, arbiters,
    error flags and current allo / ego frames -- for a finished env of an auto-reset sim the post-reset state and the next
    episode's first frame (fused reset, shadow hand-over), for auto_reset=False the terminal state and its frame"""
    acts = script(W + max(HS))
    a, b = warm(make(name, **kw), acts), make(name, **kw)
    b.reset()
    t, resets = W, 0
    for c, R in enumerate((7, 4, 1)):
        left, grp = lefts(R, N, rot=c)
        assert set(grp) == groups_possible(R)
        phase(a, left)
        b.restore(a.snapshot())
        chunk = acts[t:t + R]
        out = a.step_seq(chunk)
        got = record(a, out)
        n_e = seq_horizon(R, L, L - left)
        assert np.array_equal(out[3]["steps"].cpu().numpy(), n_e)
        recs = []
        for h in range(R):
            recs.append(record(b, b.step(chunk[h])))
        for k in range(1, R + 1):
            at = torch.as_tensor(n_e == k).cuda()
            if not bool(at.any()):
                continue
            for key, w in recs[k - 1].items():
                if key == "reward" and a.debug_reward:
                    continue   # the sum of doubles is not the sum of the twin's floats (checked against the lookahead)
                assert torch.equal(got[key][at], w[at]), (R, k, key)
        assert np.array_equal(got["done"].cpu().numpy().astype(bool), seq_done(R, L, L - left))
        resets += int(got["done"].sum())
        t += R
    assert resets > 0
    a.close(), b.close()


def host_stack(hist, frame, fresh):
    """the next [n, 96, 96, 12] stack (oldest frame first): the frame pushed, a fresh env's filled with its frame"""
    new = torch.cat([hist[..., 3:], frame], dim=-1)
    new[fresh] = frame[fresh].repeat(1, 1, 1, 4)
    return new


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", [(REGION, "plain"), (CLUSTER, "plain"), (REGION, "window"), (REGION, "frames_only")])
def test_stacks_hold_the_frames_at_call_boundaries(name, mode, monkeypatch):
    """obs_past (LoRes4E) and both stacks (LoResStack) = a host-built stack of the frames returned at call boundaries, a
    reset env's stack filled with its first frame; the same through a window ring of period 4 (mg_window_start), and
    frames_only outputs = the plain sim's current frames"""
    if mode == "window":
        monkeypatch.setattr(mg_envs, "WINDOW_K", 4)
    stack = "LoResStack" in name
    acts = script(W + max(HS))
    a = make(name, window=(mode == "window"))
    assert a.window_k == (4 if mode == "window" else 0)
    twin = None
    if mode == "frames_only":
        a.bind_outputs(a.output_buffers(), frames_only=True)
        twin = make(name)
        twin.reset()
    obs = a.reset()
    cur = (lambda o: (o["allo"][..., 9:], o["ego"][..., 9:])) if stack else (lambda o: (o["allo"], o["ego"]))
    if mode != "frames_only":
        hist = [f.repeat(1, 1, 1, 4) for f in cur(obs)]
    t, resets = 0, 0
    for c in range(9):
        R = RS[c % 3]
        left, _ = lefts(R, N, rot=c)
        phase(a, left)
        chunk = acts[t:t + R]
        obs, rew, done, info = a.step_seq(chunk)
        resets += int(done.sum())
        if mode == "frames_only":
            phase(twin, left)
            tobs = twin.step_seq(chunk)[0]
            assert obs["allo"].shape == (N, 96, 96, 3) and "past_obs" not in obs
            assert torch.equal(obs["allo"], tobs["allo"]) and torch.equal(obs["ego"], tobs["ego"]), c
        else:
            fr = cur(obs)
            hist = [host_stack(h, f, done) for h, f in zip(hist, fr)]
            if stack:
                assert torch.equal(obs["allo"], hist[0]) and torch.equal(obs["ego"], hist[1]), c
            else:
                assert torch.equal(obs["past_obs"], hist[1]), c
        t += R
    assert resets > 0
    a.close()
    if twin is not None:
        twin.close()


def step_outputs(out, env):
    obs, rew, done, info = out
    res = {"obs." + k: v.clone() for k, v in obs.items()}
    res.update(reward=rew.clone(), done=done.clone(), eval_score=info["eval_score"].clone(), errors=env.errors())
    res["bodies"], res["counts"] = env.bodies()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw", [(REGION, {}), (CORNER, {"debug_reward": True}), (CLUSTER, {}), (MATCH, {"auto_reset": False})],
                         ids=["region", "corner-debug", "cluster", "match-noreset"])
def test_one_step_is_mg_step(name, kw):
    """thirty step_seq calls of R = 1 and thirty mg_step calls on twins, across two episode boundaries: every bound
    output (observation, stacks, reward, done, eval_score) and the bodies are equal at every step"""
    acts = script(30)
    a, b = make(name, **kw), make(name, **kw)
    a.reset(), b.reset()
    stag = torch.arange(N) % L
    a.set_episode_steps(stag), b.set_episode_steps(stag)
    ends = 0
    for t in range(30):
        got, want = step_outputs(a.step_seq(acts[t:t + 1]), a), step_outputs(b.step(acts[t]), b)
        for k, w in want.items():
            assert torch.equal(got[k], w), (t, k)
        assert torch.equal(a.seq_steps, torch.ones(N, dtype=torch.int32, device="cuda"))
        ends += int(want["done"][0])
    assert ends >= 2 or not kw.get("auto_reset", True)
    a.close(), b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [REGION, MATCH], ids=["region-fused", "match-shadow"])
def test_continuation(name):
    """after a chunk the env is where n mg_step calls leave it: a twin restored from its snapshot and the env itself give
    the same bytes over five further steps, and a masked reset of the same envs draws the same layouts (the RNG stream)"""
    acts = script(W + max(HS))
    a, b = warm(make(name), acts), make(name)
    b.reset()
    left, _ = lefts(7)
    phase(a, left)
    a.step_seq(acts[W:W + 7])
    b.restore(a.snapshot())
    for t in range(W + 7, W + 12):
        got, want = step_outputs(a.step(acts[t]), a), step_outputs(b.step(acts[t]), b)
        for k, w in want.items():
            assert torch.equal(got[k], w), (t, k)
    mask = (torch.arange(N) % 3 == 0).cuda()
    oa, ob = a.reset(mask), b.reset(mask)
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    assert torch.equal(a.bodies()[0], b.bodies()[0]) and torch.equal(a.bodies()[1], b.bodies()[1])
    a.close(), b.close()


@pytest.mark.gpu
def test_pool_single_env_and_sb3():
    """PipelinedVecEnv.step_seq in chunks of 4, 4 and 5 envs = the plain env; MagicalEnv.step_seq = env 0 of a vector of
    one; sb3 with frame_skip=4 reports episode lengths in env-steps and returns equal to the summed rewards"""
    acts = script(40)
    vec = make(REGION)
    pool = PipelinedVecEnv(REGION, N, chunks=3, base_seed=1000, max_episode_steps=L)
    assert pool.bounds == [0, 4, 8, 13]
    vec.reset(), pool.reset()
    t = 0
    for c in range(6):
        R = RS[c % 3]
        left, _ = lefts(R, N, rot=c)
        phase(vec, left), pool.set_episode_steps(torch.as_tensor(L - left))
        want = vec.step_seq(acts[t:t + R])
        got = pool.step_seq(acts[t:t + R])
        pool.wait()
        for k in want[0]:
            assert torch.equal(got[0][k], want[0][k]), (c, k)
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), c
        assert torch.equal(got[3]["eval_score"], want[3]["eval_score"]) and torch.equal(got[3]["steps"], want[3]["steps"]), c
        t += R
    pool.close(), vec.close()

    one = mg_envs.VecMagicalEnv(CORNER, 1, seeds=[5], auto_reset=False)
    env = mg_envs.MagicalEnv(CORNER, seed=5)
    with pytest.raises(RuntimeError):
        env.step_seq([1])
    one.reset(), env.reset()
    Lc = env.max_episode_steps
    a1 = (acts[:, 0].cpu().tolist() * (Lc // 40 + 2))[:Lc + 6]
    for lo, hi in ((0, 5), (5, 9), (9, Lc + 6)):   # the last call runs into the episode's end and stops there
        obs, r, d, info = env.step_seq(a1[lo:hi])
        wobs, wr, wd, winfo = one.step_seq(torch.as_tensor(a1[lo:hi], dtype=torch.uint8)[:, None])
        assert info["steps"] == int(winfo["steps"][0]) == min(hi, Lc) - lo
        assert r == float(wr[0]) and d == bool(wd[0]) == (hi >= Lc) and info["eval_score"] == float(winfo["eval_score"][0])
        for k in obs:
            assert np.array_equal(obs[k], wobs[k][0].cpu().numpy()), k
    assert env._episode_steps == Lc
    one.close(), env.close()

    from magical_amd.sb3 import MagicalVecEnv
    n, k = 3, 4
    venv = MagicalVecEnv(CORNER, n, seeds=[21, 22, 23], max_episode_steps=10, debug_reward=True, frame_skip=k)
    ref = mg_envs.VecMagicalEnv(CORNER, n, seeds=[21, 22, 23], max_episode_steps=10, debug_reward=True, auto_reset=False)
    venv.reset(), ref.reset()
    ret, length, episodes = np.zeros(n), np.zeros(n, dtype=np.int64), 0
    for t in range(7):
        a = acts[t, :n].cpu().numpy()
        robs, rrew, rdone, rinfo = ref.step_repeat(a, k)
        terminal = {key: v.cpu().numpy() for key, v in robs.items()}
        steps = rinfo["steps"].cpu().numpy()
        obs, rew, dones, infos = venv.step(a)
        assert steps.tolist() == [k, k, k] if t % 3 < 2 else steps.tolist() == [2, 2, 2]   # 4 + 4 + 2 = 10
        assert np.array_equal(rew, rrew.cpu().numpy()) and np.array_equal(dones, rdone.cpu().numpy())
        ret += rrew.cpu().numpy().astype(np.float64)
        length += steps
        for i in range(n):
            if dones[i]:
                episodes += 1
                assert infos[i]["episode"]["l"] == length[i] == 10
                assert abs(infos[i]["episode"]["r"] - ret[i]) < 1e-5
                for key, v in infos[i]["terminal_observation"].items():
                    assert np.array_equal(v, terminal[key][i]), key   # the frame of the terminal state
        if dones.any():
            assert dones.all()
            ret[:], length[:] = 0.0, 0
            ref.reset()
    assert episodes == 2 * n
    venv.close(), ref.close()
