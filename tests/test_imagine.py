"""GPU: mg_imagine (VecMagicalEnv.imagine, PipelinedVecEnv.imagine, MagicalEnv.imagine).

The reference for every frame is a twin handle that really steps: the same name, seeds and size with auto_reset=False,
brought to the same state and then driven by F step_seq calls of `every` actions.  The twin's observations are pinned to
the oracle by the parity suite.  Every comparison is exact byte equality.  11 envs: two workgroups of the 8-env robot
forms, the last ragged with shadow slots, and eleven waves of the cooperative form; H = 7 with every in {1, 3, 7}
(segments of 3, 3, 1).  A few warm-up steps come first, so that the frame ring holds distinct frames.
"""
import ctypes

import numpy as np
import pytest
import torch

from magical_amd import envs as mg_envs
from magical_amd import native
from magical_amd.pipeline import PipelinedVecEnv
from test_imagine_host import stack_rule
from test_lookahead import CLUSTER, FAR, MATCH, REGION, same, script, step_out

N, H, W0 = 11, 7, 5
EVERY = (1, 3, 7)
CORNER_STACK, REGION_3EA, CORNER_4A = "MoveToCorner-Demo-LoResStack-v0", "MoveToRegion-Demo-LoRes3EA-v0", "MoveToCorner-Demo-LoRes4A-v0"
UNWRAPPED = "MoveToRegion-Demo-v0"


def make(name, n=N, L=FAR, **kw):
    return mg_envs.VecMagicalEnv(name, n, base_seed=1000, max_episode_steps=L, **kw)


def warm(env, acts, steps=W0):
    env.reset()
    for t in range(steps):
        env.step(acts[t])
    return env


def segments(every, h=H):
    return [(k, min(h, k + every)) for k in range(0, h, every)]


def current(obs, key):
    """the view's 3-channel current frame in a step()'s observation (LoResStack: the newest frame of its stack)"""
    v = obs[key]
    return v[..., 9:12] if v.shape[-1] == 12 else v


def drive(twin, snap, acts, every):
    """the twin's observations after each of the F step_seq calls, from the snapshot's state"""
    twin.restore(snap)
    out = []
    for lo, hi in segments(every):
        obs = twin.step_seq(acts[W0 + lo:W0 + hi])[0]
        out.append({k: v.clone() for k, v in obs.items()})
    return out


def by_rule(env, before, plain, stacked):
    """the stacks by tests/test_imagine_host.py's numpy restatement: history from the env's own stacked observation
    `before` (channels 3 .. 11 are its three most recent frames, oldest first, in every stacked layout)"""
    pp = env.spec.preproc
    out = {}
    for key in stacked:
        if stacked[key].shape[-1] != 12:
            continue
        src = "allo" if (key == "allo" or pp == "LoRes4A") else "ego"
        h = before[key].cpu().numpy()
        hist = np.stack([h[..., 3:6], h[..., 6:9], h[..., 9:12]])
        lead = plain["allo"].cpu().numpy() if pp == "LoRes3EA" else None
        out[key] = stack_rule(hist, plain[src].cpu().numpy(), lead)
    return out


# name, the (form, envs per workgroup) it must run, env vars set before the sims are created
CASES = [(REGION, (5, 8), {}), (CORNER_STACK, (6, 8), {}), (CLUSTER, (4, 1), {}), (MATCH, (4, 1), {}),
         (REGION_3EA, (5, 8), {}), (CORNER_4A, (6, 8), {}),
         (MATCH, (4, 1), {"MG_DEBUG_RENDER_RETRY": "2"})]   # every pair handed over twice in the render's class chain


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [0, W0], ids=["after_reset", "mid_episode"])
@pytest.mark.parametrize("name,pair,env", CASES)
def test_frames_and_stacks_equal_the_twins(name, pair, env, steps, monkeypatch):
    """allo, ego and the stacked key of every frame f = what the twin shows after its f+1-th step_seq; the plain frames
    = the twin's current frames; the stacks = the numpy rule on the plain frames and the env's own history.  Right
    after reset() the ring holds the first frame four times; mid-episode it holds distinct frames."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    acts = script(W0 + H, N)
    a, b = warm(make(name), acts, steps), warm(make(name, auto_reset=False), acts, steps)
    assert a.step_form()[:2] == pair
    snap = b.snapshot()
    before = {k: v.clone() for k, v in a._obs().items()}
    for every in EVERY:
        F = len(segments(every))
        stacked, plain = a.imagine(acts[W0:], every, stacks=True), a.imagine(acts[W0:], every)
        assert list(stacked) == list(before) and list(plain) == ["allo", "ego"]
        want = drive(b, snap, acts, every)
        for f in range(F):
            for key in stacked:
                assert stacked[key].shape[0] == F and torch.equal(stacked[key][f], want[f][key]), (every, f, key)
            for key in plain:
                assert tuple(plain[key].shape) == (F, N, 96, 96, 3)
                assert torch.equal(plain[key][f], current(want[f], key)), (every, f, key)
        for key, w in by_rule(a, before, plain, stacked).items():
            assert np.array_equal(stacked[key].cpu().numpy(), w), (every, key, "stack rule")
        if every == 1:   # the rollout moves: the case exercises more than one frame
            assert not torch.equal(plain["ego"][0], plain["ego"][F - 1])
    a.close(), b.close()


LEFT = np.array([2, 5, 30, 2, 30, 5, 30, 30, 2, 30, 5])   # env-steps left in the episode when the call is made


@pytest.mark.gpu
@pytest.mark.parametrize("name", [REGION, CLUSTER, MATCH])
def test_episode_end_inside_the_horizon(name):
    """envs 2 and 5 steps before max_episode_steps stop at their terminal step: frames up to it equal the twin's, later
    frames repeat the terminal frame, steps = the lookahead's; envs far from the end run all 7"""
    L = 50
    acts = script(W0 + H, N)
    a, b = warm(make(name, L=L), acts), warm(make(name, L=L, auto_reset=False), acts)
    for e in (a, b):
        e.set_episode_steps(torch.as_tensor(L - LEFT))
    snap = b.snapshot()
    n = np.minimum(H, LEFT)
    la = a.lookahead(acts[W0:])
    assert np.array_equal(la["steps"].cpu().numpy(), n)
    for every in EVERY:
        segs = segments(every)
        img = a.imagine(acts[W0:], every, details=True)
        assert torch.equal(img["steps"], la["steps"]) and torch.equal(img["score"], la["score"]), every
        want = drive(b, snap, acts, every)
        for f, (lo, hi) in enumerate(segs):
            live = torch.as_tensor(lo < n).cuda()          # the segment starts before the env's terminal step
            last = torch.as_tensor(np.minimum(-(-n // every) - 1, f)).cuda()   # the frame of its terminal state, if passed
            for key in ("allo", "ego"):
                assert torch.equal(img[key][f][live], current(want[f], key)[live]), (every, f, key)
                held = img[key][last, torch.arange(N).cuda()]
                assert torch.equal(img[key][f], held), (every, f, key, "a stopped env repeats its terminal frame")
        if every == 1:   # an env that stopped would have moved on: the twin's frames past its end differ somewhere
            assert not torch.equal(img["ego"][2], img["ego"][H - 1])
    a.close(), b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [REGION, CORNER_STACK, MATCH])
def test_lookahead_outputs_are_the_lookaheads(name):
    """score, steps, bodies, counts and errors of imagine(details=True) are bit for bit lookahead(bodies=True)'s, for
    every segment length, with episodes that end inside the horizon among them"""
    L = 50
    acts = script(W0 + H, N)
    a = warm(make(name, L=L), acts)
    a.set_episode_steps(torch.as_tensor(L - LEFT))
    la = a.lookahead(acts[W0:], bodies=True)
    for every in EVERY + (2,):
        img = a.imagine(acts[W0:], every, details=True)
        same(img, la, every)
    same(a.lookahead(acts[W0:], bodies=True), la, "again")
    a.close()


def blob(env):
    """the env's snapshot bytes, taken into zeroed memory (the blob's alignment padding is never written)"""
    out = torch.zeros(env.snapshot_bytes(), dtype=torch.uint8, device="cuda")
    return env.snapshot(out=out).tobytes()


def raw_state(env):
    out = {k: v.clone() for k, v in env.output_buffers().items()}
    out["bodies"], out["counts"] = env.bodies()
    out["errors"], (out["rng_key"], out["rng_pos"]) = env.errors(), env.rng_state()
    out["rng_key"] = out["rng_key"].view(torch.int32)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", [REGION, CLUSTER, MATCH])
def test_the_sim_is_untouched(name):
    """snapshot bytes and bound outputs before = after; the following steps, across an auto-reset (fused, from the
    next-layout shadow), give the bytes of a twin that never imagined"""
    L = W0 + 2
    acts = script(W0 + H, N)
    a, c = warm(make(name, L=L), acts), warm(make(name, L=L), acts)
    before, rec = raw_state(a), blob(a)
    for every in EVERY:
        a.imagine(acts[W0:], every, stacks=True, details=True)
    assert blob(a) == rec
    same(raw_state(a), before, "after imagine")
    for t in range(W0, W0 + 4):
        got, want = step_out(a, acts[t]), step_out(c, acts[t])
        same(got, want, t)
        if t == W0 + 1:
            assert bool(got["done"].all())   # the auto-reset
        a.imagine(acts[W0:], 3)              # and between the steps
    a.close(), c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["window", "frames_only"])
@pytest.mark.parametrize("name", [REGION, CLUSTER])
def test_plain_frames_in_every_output_mode(name, mode):
    """window rings and frames_only outputs: the plain frames equal the materialised handle's, window_start() and the
    bound buffers are unchanged, the next step is the twin's, and a stack request is refused (no frame history)"""
    acts = script(W0 + H, N)
    a = make(name, window=(mode == "window"))
    if mode == "frames_only":
        a.bind_outputs(a.output_buffers(), frames_only=True)
    b = make(name, window=(mode == "window"))
    if mode == "frames_only":
        b.bind_outputs(b.output_buffers(), frames_only=True)
    m = make(name)
    for e in (a, b, m):
        warm(e, acts)
    keep = [None if r is None else r.clone() for r in a.wring] + [v.clone() for v in a.output_buffers().values()]
    s0 = a.window_start()
    for every in EVERY:
        got, want = a.imagine(acts[W0:], every, details=True), m.imagine(acts[W0:], every, details=True)
        same(got, want, (mode, every))
    assert a.window_start() == s0
    now = [None if r is None else r for r in a.wring] + list(a.output_buffers().values())
    assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(now, keep))
    with pytest.raises(native.NativeError, match="-22"):
        a.imagine(acts[W0:], 1, stacks=True)
    ga, gb = a.step(acts[W0])[0], b.step(acts[W0])[0]
    # (frames_only writes each view's N current frames at the head of its bound buffer; LoResStack's own 12-channel
    # buffers are larger than that and their tails are never written)
    cut = N * 96 * 96 * 3 if mode == "frames_only" else None
    assert all(torch.equal(ga[k].reshape(-1)[:cut], gb[k].reshape(-1)[:cut]) for k in ga)
    a.close(), b.close(), m.close()


@pytest.mark.gpu
def test_refusals_launch_nothing():
    acts = script(W0 + H, N)
    a = warm(make(REGION), acts)
    lib, st, FR = native.load(), a._stream(), 96 * 96 * 3
    ap = ctypes.c_void_p(acts[W0:].contiguous().data_ptr())
    buf = {k: torch.zeros((H, N, 96, 96, c), dtype=torch.uint8, device="cuda")
           for k, c in (("allo", 3), ("ego", 3), ("stack_allo", 12), ("stack_ego", 12))}

    def fr(*keys):
        return ctypes.byref(native.mg_imagine_out(**{k: buf[k].data_ptr() for k in keys}))

    def refused(env, *args):
        rec = blob(env) if env.spec.preproc is not None and not env.window_k and not env.frames_only else None
        errs = env.errors().clone()
        assert lib.mg_imagine(*args) == -22
        torch.cuda.synchronize()
        assert all(int(b.abs().sum()) == 0 for b in buf.values()), "a refused call wrote a frame"
        assert torch.equal(env.errors(), errs)
        assert rec is None or blob(env) == rec

    h = a.handle
    refused(a, None, ap, H, 1, None, fr("ego"), st)
    refused(a, h, None, H, 1, None, fr("ego"), st)
    refused(a, h, ap, H, 1, None, None, st)
    refused(a, h, ap, H, 1, None, fr(), st)                               # all four null
    for bad_h in (0, -1, 4097):
        refused(a, h, ap, bad_h, 1, None, fr("ego"), st)
    for bad_every in (0, -1, H + 1):
        refused(a, h, ap, H, bad_every, None, fr("ego"), st)
    refused(a, h, ap, H, 1, None, fr("allo", "ego", "stack_allo"), st)    # LoRes4E keeps no allo stack
    refused(a, h, ap, H, 1, None, fr("allo", "stack_ego"), st)            # a stack without its plain frames
    four_a, three, raw, win = make(CORNER_4A), make(REGION_3EA), make(UNWRAPPED), make(REGION, window=True)
    fo = make(REGION)
    fo.bind_outputs(fo.output_buffers(), frames_only=True)
    for e in (four_a, three, raw, win, fo):
        warm(e, acts, 1)
    refused(four_a, four_a.handle, ap, H, 1, None, fr("allo", "ego", "stack_ego"), st)   # LoRes4A keeps no ego stack
    refused(three, three.handle, ap, H, 1, None, fr("ego", "stack_ego"), st)             # LoRes3EA's stack needs allo too
    refused(three, three.handle, ap, H, 1, None, fr("allo", "ego", "stack_allo"), st)
    refused(raw, raw.handle, ap, H, 1, None, fr("allo", "ego"), st)                      # preproc 0
    refused(win, win.handle, ap, H, 1, None, fr("ego", "stack_ego"), st)                 # window rings: no history
    refused(fo, fo.handle, ap, H, 1, None, fr("ego", "stack_ego"), st)                   # frames_only: no history
    with pytest.raises(ValueError):
        raw.imagine(acts[W0:])
    # the accepted forms of the same calls do write
    assert lib.mg_imagine(h, ap, H, 1, None, fr("ego"), st) == 0
    assert lib.mg_imagine(three.handle, ap, H, 1, None, fr("allo", "ego", "stack_ego"), st) == 0
    torch.cuda.synchronize()
    assert int(buf["ego"].sum()) > 0 and int(buf["stack_ego"].sum()) > 0
    for e in (a, four_a, three, raw, win, fo):
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [REGION, "MoveToCorner-Demo-LoResCHW4E-v0"])
def test_pool_matches_batch(name):
    acts = script(W0 + H, N)
    vec = warm(make(name), acts)
    pool = PipelinedVecEnv(name, N, chunks=2, base_seed=1000, max_episode_steps=FAR)
    pool.reset()
    for t in range(W0):
        pool.step(acts[t])
    for every in EVERY:
        got = pool.imagine(acts[W0:], every, stacks=True, details=True)
        want = vec.imagine(acts[W0:], every, stacks=True, details=True)
        assert list(got) == list(want)
        same(got, want, every)
    chw = name != REGION
    assert tuple(got["past_obs"].shape) == ((1, N, 12, 96, 96) if chw else (1, N, 96, 96, 12))
    assert tuple(want["ego"].shape) == ((1, N, 3, 96, 96) if chw else (1, N, 96, 96, 3))
    same(pool.imagine(acts[W0:], 3), vec.imagine(acts[W0:], 3), "plain")
    pool.close(), vec.close()


@pytest.mark.gpu
def test_single_env_matches_a_one_env_batch():
    acts = script(W0 + H, 1)
    ids = [int(x) for x in acts[:, 0].cpu()]
    one = mg_envs.MagicalEnv(REGION, seed=1000)
    vec = mg_envs.VecMagicalEnv(REGION, 1, base_seed=1000, auto_reset=False)
    one.reset(), vec.reset()
    for t in range(W0):
        one.step(ids[t]), vec.step(acts[t])
    for every, stacks in ((1, True), (3, True), (7, False)):
        got, want = one.imagine(ids[W0:], every=every, stacks=stacks), vec.imagine(acts[W0:], every, stacks=stacks)
        assert list(got) == list(want)
        for k in got:
            assert isinstance(got[k], np.ndarray) and np.array_equal(got[k], want[k][:, 0].cpu().numpy()), (every, k)
    obs = one.step(ids[W0])[0]
    want = vec.step(acts[W0])[0]
    assert all(np.array_equal(obs[k], want[k][0].cpu().numpy()) for k in obs)
    one.close(), vec.close()
