"""GPU: rollout objectives (mg_lookahead_obj / mg_plan_obj / mg_plan_cem_obj; lookahead / plan / plan_cem with
objective=, trace=True).

Every comparison is bit-exact (torch.equal / np.array_equal).  The traces are held to twins stepped with mg_step
(score() after every step, the reward output), the values to the numpy restatement of the definitions
(tests/test_objective_host.py) applied to the device traces.  13 envs as in tests/test_lookahead.py: at 8 and 16 envs
per workgroup the last workgroup is partial, so shadow lanes take part in the traced kernel's per-step barriers, and the
staggered-horizon cases put envs that end after 1 and 3 steps, envs with no step left and envs that run the whole
horizon into one workgroup.

The rise-and-fall column of test_peak_sees_what_final_misses was chosen on the CPU with the C oracle: from the reset
state of MoveToCorner-Demo (seeds 1000 + e), 4 steps forward and 12 back take envs 2, 4 and 12 towards the corner and
out again (scores 0.23 -> 0.66 -> 0.00, 0.52 -> 1.00 -> 0.22, 0.52 -> 1.00 -> 0.23), while standing still keeps 0.23,
0.51, 0.52.
"""
import ctypes

import numpy as np
import pytest
import torch

from magical_amd import Objective, native
from magical_amd import envs as mg_envs
from magical_amd.pipeline import PipelinedVecEnv
from test_cem_host import candidates, refit
from test_lookahead import CLUSTER, CORNER, FAR, FORMS, N, REGION, W, make, same, script, step_out, twins, warm
from test_objective_host import INVALID, objective_values
from test_plan import cands, check_reduction, warm_script

PICK = "PickAndPlace-Demo-LoRes4E-v0"
RETURNS = [(1.0, 0.0), (1.0, 1.0), (0.9, 0.0), (0.9, 1.0)]
PEAKS = [1.0, 0.9]


def stepped(b, acts, H):
    """the twin stepped through acts[:H]: (scores f64[H, n] after each step, rewards f32[H, n], done u8[H, n])"""
    sc, rw, dn = [], [], []
    for h in range(H):
        _, rew, done, _ = b.step(acts[h])
        sc.append(b.score().clone()), rw.append(rew.clone()), dn.append(done.clone())
    return torch.stack(sc), torch.stack(rw), torch.stack(dn)


def check_values(la, s0, o, done_n, ctx=None):
    """value / peak / peak_step of a lookahead with objective o = the host restatement on its own traces"""
    st, rt = la["score_trace"].cpu().numpy(), la["reward_trace"].cpu().numpy()
    steps, s0 = la["steps"].cpu().numpy(), s0.cpu().numpy()
    value, peak, kp = la["value"].cpu().numpy(), la["peak"].cpu().numpy(), la["peak_step"].cpu().numpy()
    assert kp.dtype == np.int32 and value.dtype == peak.dtype == np.float64
    for e in range(len(steps)):
        n = int(steps[e])
        G, P, k = objective_values([s0[e]] + list(st[:n, e]), rt[:n, e], bool(done_n[e]), o.gamma, o.tail)
        want = {"final": st[n - 1, e] if n else s0[e], "return": G, "peak": P}[o.kind]
        assert value[e] == want, (ctx, o, e, value[e], want)
        assert peak[e] == P and kp[e] == k, (ctx, o, e, peak[e], P, kp[e], k)


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,n,pair", FORMS)
def test_trace_equals_stepping(name, env, n, pair, monkeypatch):
    """every compiled (form, envs per workgroup) pair, H = 7 and 40: row h of the traces = the twin's score() and
    reward after step h + 1, with live arbiters at the horizon; the outputs of the plain call are unchanged; the
    values are the host restatement's"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    acts = script(W + 40, n)
    a, b = twins(name, 2, acts, n)
    assert a.step_form()[:2] == pair
    o = Objective("return", 0.9, 1.0)
    s0 = a.score()
    sc, rw, dn = stepped(b, acts[W:], 40)
    assert not bool(dn.any())
    for H in (7, 40):
        la = a.lookahead(acts[W:W + H], bodies=True, objective=o, trace=True)
        assert list(la) == ["score", "steps", "errors", "bodies", "counts", "value", "peak", "peak_step", "score_trace",
                            "reward_trace"]
        assert la["score_trace"].shape == la["reward_trace"].shape == (H, n)
        assert torch.equal(la["score_trace"], sc[:H]), H
        assert torch.equal(la["reward_trace"].float(), rw[:H]), H
        assert torch.equal(la["score"], sc[H - 1]), H
        same(la, a.lookahead(acts[W:W + H], bodies=True), H)
        assert bool((la["counts"][:, 3] > 0).any()), ("no live arbiter: the case exercises no contact", H)
        check_values(la, s0, o, [False] * n, H)
    bodies, counts = b.bodies()
    assert torch.equal(la["bodies"], bodies) and torch.equal(la["counts"], counts)
    a.close(), b.close()


STAGGER = [(REGION, {}), (CORNER, {"MG_STEP_BLK": "16"}), (CLUSTER, {})]
STAGGER_IDS = ["region-5/8", "corner-6/16", "cluster-4"]
L_, H_ = 60, 8


def staggered(name, count=2, **kw):
    """warmed twins with L = 60 whose envs have 1, 3, 0 and 40 steps left, in turn: (sims, left i64[N], actions [H, N])"""
    acts = script(W + H_)
    sims = twins(name, count, acts, L=L_, **kw)
    left = torch.tensor([(1, 3, 0, L_ - W)[e % 4] for e in range(N)])
    for s in sims:
        s.set_episode_steps(L_ - left)
    return sims, left, acts[W:]


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", STAGGER, ids=STAGGER_IDS)
def test_per_env_horizons(name, env, monkeypatch):
    """envs that end at step 1, at step 3, that have no step left and that run all 8, side by side in a workgroup:
    rows past an env's end hold its final score and reward 0, the terminal step's reward is the terminal score, steps
    are the plain lookahead's"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    (a, b), left, acts = staggered(name)
    n = torch.clamp(left, max=H_)
    s0 = a.score()
    plain = a.lookahead(acts)
    la = a.lookahead(acts, objective=Objective("peak"), trace=True)
    assert torch.equal(la["steps"], plain["steps"]) and torch.equal(la["steps"].cpu(), n.to(torch.int32))
    assert torch.equal(la["score"], plain["score"]) and torch.equal(la["errors"], plain["errors"])
    sc, rw, dn = stepped(b, acts, H_)
    full = torch.cat([s0[None], sc])   # s_0 .. s_H of the twin
    idx = torch.minimum(torch.arange(1, H_ + 1)[:, None], n[None, :]).cuda()   # row h: s_{min(h + 1, n)}
    want_s = full.gather(0, idx)
    live = (torch.arange(H_)[:, None] < n[None, :]).cuda()
    want_r = torch.where(live, rw, torch.zeros_like(rw))
    assert torch.equal(la["score_trace"], want_s)
    assert torch.equal(la["reward_trace"].float(), want_r)
    assert not bool(torch.isnan(la["score_trace"]).any())
    assert torch.equal(la["reward_trace"][~live], torch.zeros(int((~live).sum()), dtype=torch.float64, device="cuda"))
    for e in range(N):
        k = int(left[e])
        if 1 <= k < H_:   # the terminal step pays the terminal score, as mg_step's done step does
            assert bool(dn[k - 1, e]) and float(la["reward_trace"][k - 1, e]) == float(la["score_trace"][k - 1, e]) == float(la["score"][e])
            assert not bool(la["reward_trace"][:k - 1, e].any())
        if k == 0:
            assert float(la["score"][e]) == float(s0[e]) and bool((la["score_trace"][:, e] == s0[e]).all())
    a.close(), b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,env", STAGGER, ids=STAGGER_IDS)
def test_values(name, env, monkeypatch):
    """value, peak and peak_step = the host restatement on the device traces for every (gamma, tail) of the issue, on
    staggered horizons (termination inside the horizon, n = 0, the full horizon); RETURN with gamma = 1, tail = 1 on a
    sim without debug reward and FINAL's value are the score, bit for bit"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    (a,), left, acts = staggered(name, 1)
    done_n = [1 <= int(k) <= H_ for k in left]
    s0 = a.score()
    objs = [Objective("return", g, t) for g, t in RETURNS] + [Objective("peak", g) for g in PEAKS] + [Objective("final", 0.9, 1.0)]
    for o in objs:
        la = a.lookahead(acts, objective=o, trace=True)
        check_values(la, s0, o, done_n, name)
        if o.kind == "final" or (o.kind, o.gamma, o.tail) == ("return", 1.0, 1.0):
            assert torch.equal(la["value"], la["score"]), o
        only = a.lookahead(acts, objective=o)   # without traces: the same values
        assert list(only) == ["score", "steps", "errors", "value", "peak", "peak_step"]
        same(only, {k: la[k] for k in only}, o)
    a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [CORNER, PICK])
def test_dense_reward(name):
    """debug_reward sims: the reward trace is the dense reward of every simulated step (non-zero everywhere), equal to
    the twin's reward output, and RETURN sums it"""
    H = 7
    acts = script(W + H)
    a, b = twins(name, 2, acts, debug_reward=True)
    s0 = a.score()
    o = Objective("return", 0.9, 0.0)
    la = a.lookahead(acts[W:], objective=o, trace=True)
    sc, rw, dn = stepped(b, acts[W:], H)
    assert bool((rw != 0).all()) and bool((la["reward_trace"] != 0).all())
    assert torch.equal(la["reward_trace"].float(), rw) and torch.equal(la["score_trace"], sc)
    check_values(la, s0, o, [False] * N, name)
    assert not torch.equal(la["value"], la["score"])
    a.close(), b.close()


RISE_FALL = [1] * 4 + [2] * 12   # forward, then back (see the module docstring)
RISE_FALL_ENVS = [2, 4, 12]


@pytest.mark.gpu
def test_peak_sees_what_final_misses():
    """a column that crosses its best score mid-horizon and leaves again: PEAK reports when and how high, and in a plan
    against standing still PEAK picks the column where FINAL picks standing still"""
    a = make(CORNER)
    a.reset()
    H = len(RISE_FALL)
    col = torch.tensor(RISE_FALL, dtype=torch.uint8)[:, None].expand(H, N).contiguous().cuda()
    la = a.lookahead(col, objective=Objective("peak"), trace=True)
    tr = la["score_trace"].cpu().numpy()
    for e in RISE_FALL_ENVS:
        kp, n = int(la["peak_step"][e]), int(la["steps"][e])
        assert n == H and 0 < kp < n, (e, kp)
        assert float(la["peak"][e]) > float(la["score"][e]) and float(la["peak"][e]) == tr[kp - 1, e] == tr[:, e].max()
        assert tr[kp - 1, e] > tr[0, e] and tr[kp - 1, e] > tr[-1, e]   # it rises, then falls
    both = torch.stack([torch.zeros_like(col), col], dim=1)   # candidate 0 stays put
    peak = a.plan(both, details=True, objective=Objective("peak"))
    final = a.plan(both, details=True, objective=Objective("final"))
    plain = a.plan(both, details=True)
    for e in RISE_FALL_ENVS:
        assert int(peak["best"][e]) == 1 and float(peak["best_score"][e]) == float(la["peak"][e])
        assert float(final["scores"][0, e]) >= float(final["scores"][1, e]) and int(final["best"][e]) == 0
    same(final, plain, "FINAL is mg_plan")
    a.close()


def host_cem(env, o, H, K, iters, elites, alpha, repeat, key, step):
    """tests/test_cem.py's host loop with plan(objective=o) as the rollout"""
    n, J = env.num_envs, -(-H // repeat)
    w = np.ones((J, 18, n), dtype=np.uint16)
    cand = best = None
    iter_best = []
    for i in range(iters):
        cand = candidates(w, H, K, repeat, key, step, i, cand, best)
        res = {k: v.cpu().numpy() for k, v in env.plan(torch.from_numpy(cand), details=True, objective=o).items()}
        best = res["best"].astype(np.int64)
        iter_best.append(res["best_score"])
        w = refit(cand, res["scores"], elites, alpha, repeat)
    return dict(res, actions=cand, plan=cand[:, best, np.arange(n)], iter_best=np.array(iter_best), weights=w)


@pytest.mark.gpu
@pytest.mark.parametrize("name,pair", [(REGION, (5, 8)), (CLUSTER, (4, 1))])
def test_plan_and_cem(name, pair):
    """candidate k of plan(objective=o) = lookahead(column k, objective=o)['value'], best = numpy's argmax;
    plan_cem(objective=o) = the host loop over plan(objective=o): 13 envs, K = 5, H = 7, 2 iterations"""
    H, K = 7, 5
    a = warm(make(name), warm_script())
    assert a.step_form()[:2] == pair
    c = cands(H, K)
    for o in (Objective("return", 0.9, 1.0), Objective("peak", 0.9)):
        res = a.plan(c, details=True, objective=o)
        for k in range(K):
            la = a.lookahead(c[:, k], objective=o)
            assert torch.equal(res["scores"][k], la["value"]), (o, k)
            assert torch.equal(res["steps"][k], la["steps"]) and torch.equal(res["errors"][k], la["errors"]), (o, k)
        check_reduction(res, c, o)
        short = a.plan(c, objective=o)
        same(short, {k: res[k] for k in short}, o)
        got = a.plan_cem(H, K, 2, 2, alpha=1, repeat=2, key=42, step=0, details=True, objective=o)
        want = host_cem(a, o, H, K, 2, 2, 1, 2, 42, 0)
        for key in ("actions", "scores", "steps", "errors", "best", "best_score", "first_action", "plan", "iter_best", "weights"):
            g = got[key].cpu().numpy()
            assert g.dtype == want[key].dtype and np.array_equal(g, want[key]), (o, key)
    a.close()


@pytest.mark.gpu
def test_untouched_and_identical():
    """after objective calls, lookahead, step and snapshot bytes = those of a twin that never made them; FINAL without
    extra outputs returns lookahead's tensors"""
    H = 7
    acts = script(W + H + 2)
    a, c = (warm(make(REGION), acts) for _ in range(2))
    a.lookahead(acts[W:W + H], objective=Objective("return", 0.9, 1.0), trace=True)
    a.plan(cands(H, 3), objective=Objective("peak", 0.9))
    a.plan_cem(H, 3, 2, 2, objective=Objective("return"))
    want = c.lookahead(acts[W:W + H], bodies=True)
    same(a.lookahead(acts[W:W + H], bodies=True), want, "plain lookahead")
    lib = native.load()
    got = {k: torch.empty_like(v) for k, v in want.items()}
    out = native.mg_lookahead_out(**{k: v.data_ptr() for k, v in got.items()})
    obj = native.mg_objective(kind=native.OBJ_FINAL, reserved=0, gamma=0.5, tail=3.0)
    ap = ctypes.c_void_p(acts[W:W + H].contiguous().data_ptr())
    for oo in (None, ctypes.byref(native.mg_objective_out())):
        for v in got.values():
            v.zero_()
        assert lib.mg_lookahead_obj(a.handle, ap, H, ctypes.byref(obj), ctypes.byref(out), oo, a._stream()) == 0
        same(got, want, "FINAL without outputs")
    # (into zeroed buffers, as tests/test_snapshot.py compares blobs: the padding between a blob's sections is not written)
    blobs = [s.snapshot(out=torch.zeros(s.snapshot_bytes(), dtype=torch.uint8, device="cuda")).tobytes() for s in (a, c)]
    assert blobs[0] == blobs[1]
    for t in range(W + H, W + H + 2):
        same(step_out(a, acts[t]), step_out(c, acts[t]), t)
    a.close(), c.close()


@pytest.mark.gpu
def test_refusals_launch_nothing():
    acts = script(W + 3)
    a, b = twins(REGION, 2, acts)
    for kw in (dict(kind="best"), dict(gamma=0.0), dict(gamma=1.5), dict(tail=-1.0), dict(tail=float("nan"))):
        with pytest.raises(ValueError):
            a.lookahead(acts[W:], objective=Objective(**kw))
    with pytest.raises(ValueError):
        a.plan(cands(3, 2), objective=0.9)
    lib = native.load()
    score = torch.full((N,), -7.0, dtype=torch.float64, device="cuda")
    value = torch.full((N,), -7.0, dtype=torch.float64, device="cuda")
    best = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    lo, oo = native.mg_lookahead_out(score=score.data_ptr()), native.mg_objective_out(value=value.data_ptr())
    po, co = native.mg_plan_out(best=best.data_ptr()), native.mg_plan_cem_out(best=best.data_ptr())
    c = cands(3, 2)
    cw = torch.zeros((3, 18, N), dtype=torch.int16, device="cuda")
    ap, cp, wp, st = ctypes.c_void_p(acts[W:].contiguous().data_ptr()), ctypes.c_void_p(c.data_ptr()), ctypes.c_void_p(cw.data_ptr()), a._stream()
    for bad, _ in INVALID:
        o = native.mg_objective(**dict(dict(kind=1, reserved=0, gamma=1.0, tail=0.0), **bad))
        assert lib.mg_lookahead_obj(a.handle, ap, 3, ctypes.byref(o), ctypes.byref(lo), ctypes.byref(oo), st) == -22, bad
        assert lib.mg_plan_obj(a.handle, cp, 3, 2, ctypes.byref(o), ctypes.byref(po), st) == -22, bad
        assert lib.mg_plan_cem_obj(a.handle, cp, wp, 0, 3, 2, 1, 1, 1, 1, 0, 0, ctypes.byref(o), ctypes.byref(co), st) == -22, bad
    ok = native.mg_objective(kind=2, reserved=0, gamma=0.9, tail=0.0)
    assert lib.mg_lookahead_obj(a.handle, ap, 3, None, ctypes.byref(lo), ctypes.byref(oo), st) == -22   # null objective
    assert lib.mg_lookahead_obj(a.handle, ap, 4097, ctypes.byref(ok), ctypes.byref(lo), ctypes.byref(oo), st) == -22
    assert lib.mg_lookahead_obj(a.handle, None, 3, ctypes.byref(ok), ctypes.byref(lo), ctypes.byref(oo), st) == -22
    assert lib.mg_lookahead_obj(a.handle, ap, 3, ctypes.byref(ok), None, ctypes.byref(oo), st) == -22
    assert lib.mg_plan_obj(a.handle, cp, 3, 0, ctypes.byref(ok), ctypes.byref(po), st) == -22
    assert lib.mg_plan_obj(a.handle, cp, 3, 2, None, ctypes.byref(po), st) == -22
    torch.cuda.synchronize()
    assert bool((score == -7).all()) and bool((value == -7).all()) and bool((best == -7).all())   # nothing was written
    assert lib.mg_lookahead_obj(a.handle, ap, 3, ctypes.byref(ok), ctypes.byref(lo), ctypes.byref(oo), st) == 0
    same(a.lookahead(acts[W:], bodies=True), b.lookahead(acts[W:], bodies=True), "plain call after the refusals")
    torch.cuda.synchronize()
    assert torch.equal(score, b.lookahead(acts[W:])["score"]) and not bool((value == -7).any())
    for t in range(W, W + 3):
        same(step_out(a, acts[t]), step_out(b, acts[t]), t)
    a.close(), b.close()


@pytest.mark.gpu
def test_pool_and_single_env():
    """PipelinedVecEnv (chunks of 4, 4 and 5 envs) and MagicalEnv give the flat sim's results per env"""
    H, K = 7, 3
    acts = script(W + H)
    o = Objective("return", 0.9, 1.0)
    vec = warm(make(REGION), acts)
    pool = PipelinedVecEnv(REGION, N, chunks=3, base_seed=1000, max_episode_steps=FAR)
    assert pool.bounds == [0, 4, 8, 13]
    pool.reset()
    for t in range(W):
        pool.step(acts[t])
    got, want = pool.lookahead(acts[W:], objective=o, trace=True), vec.lookahead(acts[W:], objective=o, trace=True)
    assert list(got) == list(want) and got["score_trace"].shape == (H, N)
    same(got, want, "pool lookahead")
    c = cands(H, K)
    got, want = pool.plan(c, details=True, objective=o), vec.plan(c, details=True, objective=o)
    assert list(got) == list(want)
    same(got, want, "pool plan")
    got = pool.plan_cem(H, K, 2, 2, key=42, objective=o, details=True)
    for k, (sim, lo, hi) in enumerate(zip(pool.sims, pool.bounds, pool.bounds[1:])):
        one = sim.plan_cem(H, K, 2, 2, key=42 + k, objective=o, details=True)
        for key in ("best", "best_score", "iter_best", "scores", "actions"):
            assert torch.equal(got[key][..., lo:hi], one[key]), (k, key)
    pool.close(), vec.close()
    # the single env: seed 1000 is env 0 of a flat sim with base_seed 1000
    env = mg_envs.MagicalEnv(CORNER, seed=1000)
    flat = make(CORNER, 1, L=env.max_episode_steps)
    env.reset(), flat.reset()
    po = Objective("peak")
    res = env.lookahead(RISE_FALL, objective=po, trace=True)
    col = torch.tensor(RISE_FALL, dtype=torch.uint8)[:, None]
    want = flat.lookahead(col, objective=po, trace=True)
    assert res["score"] == float(want["score"][0]) and res["steps"] == int(want["steps"][0]) == len(RISE_FALL)
    assert res["value"] == float(want["value"][0]) == res["peak"] and res["peak_step"] == int(want["peak_step"][0])
    assert np.array_equal(res["score_trace"], want["score_trace"][:, 0].cpu().numpy())
    assert np.array_equal(res["reward_trace"], want["reward_trace"][:, 0].cpu().numpy())
    assert env.lookahead(RISE_FALL) == (res["score"], res["steps"])   # without an objective: the pair, as before
    both = np.stack([np.zeros(len(RISE_FALL), dtype=np.uint8), np.array(RISE_FALL, dtype=np.uint8)], axis=1)
    best, best_score, scores = env.plan(both, objective=po)
    wp = flat.plan(torch.as_tensor(both)[:, :, None], details=True, objective=po)
    assert best == int(wp["best"][0]) and best_score == float(wp["best_score"][0])
    assert np.array_equal(scores, wp["scores"][:, 0].cpu().numpy()) and scores[1] == res["peak"]
    plan, bs, ib = env.plan_cem(5, 4, 2, 2, key=9, objective=po)
    wc = flat.plan_cem(5, 4, 2, 2, key=9, objective=po)
    assert np.array_equal(plan, wc["plan"][:, 0].cpu().numpy()) and bs == float(wc["best_score"][0])
    assert np.array_equal(ib, wc["iter_best"][:, 0].cpu().numpy())
    env.close(), flat.close()
