"""GPU: env state snapshot / restore (mg_snapshot, mg_restore; VecMagicalEnv.snapshot / restore).

Every comparison is bit-exact (torch.equal) against an uninterrupted run of the same simulator, which the parity
suite pins to the oracle.  Shapes: 70 envs (padded row stride 128: one full wavefront and a ragged one) and 1 env;
max_episode_steps = 9 with episode phases staggered 0..8, so some envs auto-reset on the first step after a restore
and every env does within 9; actions from random_actions(step).
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from magical_amd import envs as mg_envs
from magical_amd import native, registry
from magical_amd.snapshot import PoolSnapshot, Snapshot

N, L, T0, T1 = 70, 9, 6, 12   # envs, episode length, steps before the snapshot, steps compared after it


def make(name, n=N, base_seed=1000, **kw):
    return mg_envs.VecMagicalEnv(name, n, base_seed=base_seed, max_episode_steps=L, **kw)


def start(env, acts):
    """reset, stagger the episode phases, run the steps before the snapshot"""
    env.reset()
    env.set_episode_steps(torch.arange(env.num_envs) % L)
    for t in range(T0):
        env.step(acts[t])


def actions(env, steps):
    return [env.random_actions(t).clone() for t in range(steps)]


def state_of(env, obs):
    rec = {"obs." + k: v.clone() for k, v in obs.items()}
    if hasattr(env, "bodies"):
        b, c = env.bodies()
        a, h = env.arbiters()
        rec.update(bodies=b, counts=c, arbiters=a, hashes=h.view(torch.int64))
    rec["errors"] = env.errors().clone()
    return rec


def step_rec(env, a):
    obs, rew, done, info = env.step(a)
    if hasattr(env, "wait"):
        env.wait()
    rec = state_of(env, obs)
    rec.update(reward=rew.clone(), done=done.clone(), eval_score=info["eval_score"].clone())
    return rec


def assert_same(got, want, ctx, rows=None, want_rows=None):
    for k, w in want.items():
        g = got[k]
        if rows is not None:
            g, w = g[rows], w[want_rows if want_rows is not None else rows]
        assert torch.equal(g, w), (ctx, k)


def continuation(env, acts):
    return [step_rec(env, acts[t]) for t in range(T0, T0 + T1)]


NAMES = ["MoveToRegion-Demo-LoRes4E-v0",        # quad form, fused reset, static layer in use
         "MoveToCorner-Demo-LoResStack-v0",     # contacts: warm-started arbiters are live
         "MatchRegions-TestAll-LoResStack-v0",  # cooperative form, next-layout shadow, rejection-sampled layouts
         "PickAndPlace-Demo-LoRes4E-v0",        # target output
         "MoveToRegion-Demo-v0",                # unwrapped 384^2 surface
         "MoveToCorner-Demo-LoRes3EA-v0",       # allo frame + ego ring composed into past_obs
         "MoveToRegion-Demo-LoRes4A-v0",        # allo ring, plain ego frame
         "MoveToRegion-Demo-LoResCHW4E-v0"]     # channels-first views of the same bytes


def _same_sim(name, n):
    env = make(name, n)
    acts = actions(env, T0 + T1)
    start(env, acts)
    obs0 = {k: v for k, v in env._obs().items()}
    at_snap = state_of(env, obs0)
    snap = env.snapshot()
    assert len(snap) == n and snap.blob.numel() == env.snapshot_bytes()
    want = continuation(env, acts)
    assert any(bool(r["done"].any()) for r in want)   # the continuation crosses episode boundaries
    obs = env.restore(snap)
    assert_same(state_of(env, obs), at_snap, "restored")
    got = continuation(env, acts)
    for t, (g, w) in enumerate(zip(got, want)):
        assert_same(g, w, t)
    h = snap.header
    spec = registry.lookup(name)
    assert (h.task, h.rand_flags, h.count) == (spec.task_id, spec.rand_flags, n)
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_continuation_same_sim(name):
    _same_sim(name, N)


@pytest.mark.gpu
def test_continuation_one_env():
    _same_sim("MoveToRegion-Demo-LoRes4E-v0", 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", [("MatchRegions-TestAll-LoResStack-v0", "plain"),
                                          ("MatchRegions-TestAll-LoResStack-v0", "seeded-halves"),
                                          ("MoveToRegion-Demo-LoRes4E-v0", "plain"),
                                          ("MoveToRegion-Demo-LoRes4E-v0", "seeded-halves")])
def test_continuation_fresh_sim_through_host(name, variant, tmp_path):
    """The blob travels through the host and a file into a second simulator with other seeds: the continuation,
    auto-resets included, is the first simulator's -- so the MT19937 streams and the shadow's next layouts travel.
    seeded-halves: after seed() (the next-layout shadow invalid: auto-resets run in place) and restored in two
    calls through envs / recs, so the shadow stays invalid."""
    a = make(name)
    acts = actions(a, T0 + T1)
    start(a, acts)
    snap = a.snapshot()
    at_snap = state_of(a, a._obs())
    want = continuation(a, acts)
    a.close()
    path = str(tmp_path / "snap.pt")
    snap.cpu().save(path)
    loaded = Snapshot.load(path)
    assert loaded.device.type == "cpu" and len(loaded) == N and loaded.header == snap.header
    b = make(name, base_seed=777000)
    b.reset()
    b.step(acts[0])
    dev = loaded.to(b.device)
    if variant == "plain":
        obs = b.restore(dev)
    else:
        b.seed([31337 + i for i in range(N)])
        half = list(range(N // 2))
        rest = list(range(N // 2, N))
        b.restore(dev, envs=rest, recs=rest)
        obs = b.restore(dev, envs=half, recs=half)
    assert_same(state_of(b, obs), at_snap, "restored")
    for t, w in enumerate(want):
        assert_same(step_rec(b, acts[T0 + t]), w, t)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["MatchRegions-TestAll-LoResStack-v0", "MoveToRegion-Demo-LoRes4E-v0"])
def test_subset_and_broadcast(name):
    """One record of env 3 (step 6) broadcast into envs 0, 5 and 69 of a running simulator at step 10: they become
    env 3 at step 6 and, fed env 3's actions, repeat its trajectory and its next auto-reset; every other env stays
    the untouched twin's."""
    src, dst, tw = 3, [0, 5, 69], 4
    a, b = make(name), make(name)
    acts = actions(a, T0 + tw + T1)
    start(a, acts)
    start(b, acts)
    one = a.snapshot(envs=[src])
    assert len(one) == 1 and one.blob.numel() == a.snapshot_bytes(1)
    at_snap = state_of(b, b._obs())
    hist = {}   # the twin's records by step
    for t in range(T0, T0 + tw):
        step_rec(a, acts[t])
        hist[t] = step_rec(b, acts[t])
    obs = a.restore(one, envs=dst, recs=[0, 0, 0])
    others = [e for e in range(N) if e not in dst]
    now = state_of(a, obs)
    for k in now:
        if k.startswith("obs.") or k in ("bodies", "counts", "arbiters", "hashes", "errors"):
            for e in dst:
                assert torch.equal(now[k][e], at_snap[k][src]), ("restored", k, e)
            assert torch.equal(now[k][others], state_of(b, b._obs())[k][others]), ("others at restore", k)
    seen_done = False
    for j in range(T1):
        t = T0 + tw + j
        act = acts[t].clone()
        act[dst] = acts[T0 + j][src]
        got = step_rec(a, act)
        hist[t] = step_rec(b, acts[t])
        assert_same(got, hist[t], ("others", j), rows=others)
        for e in dst:
            assert_same(got, hist[T0 + j], ("broadcast", j, e), rows=e, want_rows=src)
        seen_done = seen_done or bool(got["done"][dst[0]])
    assert seen_done   # the restored envs went through their next auto-reset
    a.close()
    b.close()


@pytest.mark.gpu
def test_refusals_leave_the_state_untouched():
    name = "MoveToRegion-Demo-LoRes4E-v0"
    a, b = make(name), make(name)
    acts = actions(a, T0 + 1)
    start(a, acts)
    start(b, acts)
    good = a.snapshot()
    other_task = make("MoveToCorner-Demo-LoRes4E-v0")
    other_task.reset()
    other_pp = make("MoveToRegion-Demo-LoResStack-v0")
    other_pp.reset()
    bad_magic = Snapshot(good.blob.clone())
    bad_magic.blob[0] ^= 0xFF
    cases = {
        "task": lambda: a.restore(other_task.snapshot()),
        "preproc": lambda: a.restore(other_pp.snapshot()),
        "truncated": lambda: a.restore(Snapshot(good.blob[:good.blob.numel() // 2].clone())),
        "magic": lambda: a.restore(bad_magic),
        "env out of range": lambda: a.restore(good, envs=[N], recs=[0]),
        "negative env": lambda: a.restore(good, envs=[-1], recs=[0]),
        "duplicate destination": lambda: a.restore(good, envs=[1, 1], recs=[0, 0]),
        "record out of range": lambda: a.restore(good, envs=[0], recs=[len(good)]),
        "snapshot env out of range": lambda: a.snapshot(envs=[N]),
    }
    for what, call in cases.items():
        with pytest.raises(native.NativeError):
            call()
            pytest.fail(what)
    # the library's own header check (the Python wrapper refuses a bad magic value before it gets there)
    rc = a.lib.mg_restore(a.handle, ctypes.c_void_p(bad_magic.blob.data_ptr()), None, None, N, a._stream())
    assert rc == -22 and b"magic" in a.lib.mg_last_error()
    # modes whose frame stacks are not in the simulator
    win = make(name, window=True)
    win.reset()
    fo = make(name)
    views = fo.output_buffers()
    fo.bind_outputs({k: views[k] for k in views}, frames_only=True)
    fo.reset()
    for env in (win, fo):
        with pytest.raises(native.NativeError):
            env.snapshot()
        with pytest.raises(native.NativeError):
            env.restore(good)
    assert_same(step_rec(a, acts[T0]), step_rec(b, acts[T0]), "after the refusals")
    for env in (a, b, other_task, other_pp, win, fo):
        env.close()


@pytest.mark.gpu
def test_pool_snapshot(tmp_path):
    """PipelinedVecEnv: 70 envs in 3 ragged chunks; the pool's snapshot continues like the plain batch's run, in
    the pool itself and restored into a batch of the same env order."""
    from magical_amd import pipeline
    name = "MoveToRegion-Demo-LoRes4E-v0"
    seeds = [1000 + i for i in range(N)]
    ref = make(name)
    pool = pipeline.PipelinedVecEnv(name, N, chunks=3, seeds=seeds, max_episode_steps=L)
    sizes = [pool.bounds[k + 1] - pool.bounds[k] for k in range(3)]
    assert sum(sizes) == N and len(set(sizes)) > 1
    acts = actions(ref, T0 + T1)
    start(ref, acts)
    pool.reset()
    pool.set_episode_steps(torch.arange(N) % L)
    for t in range(T0):
        pool.step(acts[t])
    snap = pool.snapshot()
    at_snap = {k: v for k, v in state_of(ref, ref._obs()).items() if k.startswith("obs.") or k == "errors"}
    want = continuation(ref, acts)
    for t in range(T0, T0 + 3):   # move the pool on before putting it back
        pool.step(acts[t])
    obs = pool.restore(snap)
    assert_same(state_of(pool, obs), at_snap, "pool restored")
    for t, w in enumerate(want):
        got = step_rec(pool, acts[T0 + t])
        assert_same(got, {k: w[k] for k in got}, ("pool", t))
    path = str(tmp_path / "pool.pt")
    snap.cpu().save(path)
    loaded = PoolSnapshot.load(path)
    assert loaded.bounds == pool.bounds and len(loaded) == N
    batch = make(name, base_seed=424242)
    batch.reset()
    obs = batch.restore(loaded)
    assert_same(state_of(batch, obs), at_snap, "batch restored")
    for t, w in enumerate(want):
        assert_same(step_rec(batch, acts[T0 + t]), w, ("batch", t))
    pool.close()
    for env in (ref, batch):
        env.close()


@pytest.mark.gpu
def test_single_env_state_round_trip():
    """MagicalEnv.get_state / set_state over an episode boundary: the reset after the restore draws the same layout."""
    import magical_amd
    env = magical_amd.make("MatchRegions-TestAll-LoRes4E-v0", seed=11)
    acts = np.random.RandomState(3).randint(0, 18, 400)
    env.reset()
    for t in range(5):
        obs0, *_ = env.step(acts[t])
    state = env.get_state()
    assert isinstance(state, bytes)

    def run():
        out, t, done = [], 5, False
        while not done and t < 5 + 6:   # a few steps, then an explicit reset (the episode boundary), then a few more
            o, r, done, info = env.step(acts[t])
            out.append((o, r, done, info["eval_score"]))
            t += 1
        out.append((env.reset(), 0.0, False, 0.0))
        for t in range(t, t + 4):
            o, r, done, info = env.step(acts[t])
            out.append((o, r, done, info["eval_score"]))
        return out

    want = run()
    back = env.set_state(state)
    assert all(np.array_equal(back[k], obs0[k]) for k in obs0)
    got = run()
    assert len(got) == len(want)
    for (o1, r1, d1, s1), (o2, r2, d2, s2) in zip(got, want):
        assert all(np.array_equal(o1[k], o2[k]) for k in o2) and (r1, d1, s1) == (r2, d2, s2)
    env.close()


@pytest.mark.gpu
def test_restored_continuation_matches_oracle():
    """A MoveToRegion continuation after a restore equals the CPU oracle's uninterrupted rollout bit for bit."""
    import magical_amd
    import pyoracle as po
    name = "MoveToRegion-Demo-LoRes4E-v0"
    spec = registry.lookup(name)
    n, steps, cut = 2, 12, 6
    vec = magical_amd.make_vec(name, n, seeds=[1000, 1001])
    orc = [po.OracleEnv(spec.task, spec.rand_flags, spec.preproc, spec.max_episode_steps, seed=1000 + i) for i in range(n)]
    vec.reset()
    ref = [o.reset() for o in orc]
    acts = np.random.RandomState(42).randint(0, 18, (steps, n))
    for t in range(steps):
        ref = [orc[i].step(int(acts[t, i]))[0] for i in range(n)]
    for t in range(cut):
        vec.step(torch.as_tensor(acts[t], dtype=torch.uint8))
    snap = vec.snapshot()
    for t in range(cut, steps):
        vec.step(torch.as_tensor(acts[(t * 7) % steps], dtype=torch.uint8))   # wander off
    vec.restore(snap)
    for t in range(cut, steps):
        obs, *_ = vec.step(torch.as_tensor(acts[t], dtype=torch.uint8))
    flat = torch.cat([obs[k].reshape(n, -1) for k in obs], dim=1).cpu().numpy()
    for i in range(n):
        assert np.array_equal(flat[i], ref[i]), i
    vec.close()


@pytest.mark.gpu
def test_blob_format_is_stable():
    """tests/golden/snapshot_blob.bin was written by the library that introduced blob layout version 1 (3 envs of
    MoveToRegion-Demo-v0 -- no preprocessor: state sections only -- 5 steps, envs [2, 0]; make_snapshot_blob.py).  The
    same run writes the same bytes today, and the file restores into a fresh sim that then steps as the recorded one."""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, "snapshot_blob.json")) as f:
        meta = json.load(f)
    want = torch.from_numpy(np.fromfile(os.path.join(golden, "snapshot_blob.bin"), dtype=np.uint8))
    acts = torch.as_tensor(meta["actions"], dtype=torch.uint8)
    envs, t0 = meta["envs"], meta["before"]
    a = mg_envs.VecMagicalEnv(meta["name"], len(meta["seeds"]), seeds=meta["seeds"])
    b = mg_envs.VecMagicalEnv(meta["name"], len(meta["seeds"]), seeds=meta["seeds"])
    a.reset(), b.reset()
    for t in range(t0):
        a.step(acts[t])
    # mg_snapshot does not write the padding that rounds a record's state bytes up to 16: the buffer is zeroed first, as
    # the fixture's was
    got = a.snapshot(envs=envs, out=torch.zeros(want.numel(), dtype=torch.uint8, device="cuda")).blob.cpu()
    assert got.numel() == want.numel()
    assert torch.equal(got, want), ("first differing byte", int((got != want).nonzero()[0]))
    b.restore(Snapshot(want), envs=envs)
    for t in range(t0, t0 + meta["after"]):
        a.step(acts[t]), b.step(acts[t])
        (ba, ca), (bb, cb) = a.bodies(), b.bodies()
        assert torch.equal(ba[envs], bb[envs]) and torch.equal(ca[envs], cb[envs]), t
    a.close(), b.close()
