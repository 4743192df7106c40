"""GPU parity: the HIP path (through the C ABI) against the CPU oracle.

Inputs: env i seeded 1000 + i; actions numpy RandomState(42).randint(0, 18, (T, N))
(SURVEY.md section 8(d)).  Bar: LoRes observations bit-exact, full-resolution
frames bit-exact, body poses equal (tolerance 1e-4 stated by the north star,
asserted at 1e-9 here because both sides share the operation order), rewards,
done flags and eval scores equal.
"""
import numpy as np
import pytest
import torch

import pyoracle as po
import magical_amd
from magical_amd import envs as mg_envs
from magical_amd import registry

CONFIGS = [
    ("MoveToRegion-Demo-LoRes4E-v0", 6, 90),
    ("MoveToCorner-Demo-LoRes4E-v0", 6, 90),
    ("ClusterColour-Demo-LoResStack-v0", 3, 60),
    ("MatchRegions-TestAll-LoRes4E-v0", 4, 130),
]
# SURVEY.md 8(f) F1 tasks: full episodes (scores at done) for the Demo and the most random variant
TASK_CONFIGS = [
    ("MakeLine-Demo-LoRes4E-v0", 3, 185),
    ("MakeLine-TestAll-LoRes4E-v0", 4, 185),
    ("MakeLine-TestCountPlus-LoResStack-v0", 3, 40),
    ("FindDupe-Demo-LoRes4E-v0", 3, 105),
    ("FindDupe-TestAll-LoRes4E-v0", 4, 105),
    ("FindDupe-TestJitter-LoResStack-v0", 3, 30),
    ("FixColour-Demo-LoRes4E-v0", 3, 65),
    ("FixColour-TestAll-LoRes4E-v0", 4, 65),
    ("FixColour-TestJitter-LoRes3EA-v0", 3, 30),
    # the fork's own training configs: train_rl.py:87-92 (PickAndPlace, debug_reward), train_il.py:216
    ("PickAndPlace-Demo-LoResCHW4A-v0", 4, 85),
    ("PickAndPlace-Test-LoRes4A-v0", 3, 85),
    ("PickAndPlace-Demo-v0", 2, 12),
    ("MoveToCorner-Demo-DebugReward-v0", 2, 85),
]
# the other observation preprocessors (benchmarks/__init__.py:51-190): same rollout check
PREPROC_CONFIGS = [
    ("MoveToRegion-Demo-LoRes3EA-v0", 4, 45),
    ("MoveToCorner-TestAll-LoRes4A-v0", 3, 30),
    ("MoveToRegion-TestAll-LoResCHW4E-v0", 3, 30),
    ("MoveToRegion-Demo-LoResCHW4A-v0", 2, 12),
    ("MoveToRegion-TestJitter-v0", 2, 12),
]
POSE_TOL = 1e-9


def oracle_obs_split(spec, flat):
    shapes = mg_envs._obs_shapes(spec)
    out, off = {}, 0
    for k, s in shapes.items():
        n = int(np.prod(s))
        out[k] = flat[off:off + n].reshape(s)
        off += n
    return out


def oracle_env(spec, seed):
    return po.OracleEnv(spec.task, spec.rand_flags, spec.preproc, spec.max_episode_steps, seed=seed)


def with_targets(spec, ref, orc):
    """PickAndPlace observation extras (pick_and_place.py:103-107) as the vec env delivers them:
    float32 [1], [1], [2] (the spaces' dtype, as SB3's DummyVecEnv buffers them)."""
    if spec.task == "PickAndPlace":
        t = orc.target().astype(np.float32)
        ref["target_type"], ref["target_colour"], ref["target_position"] = t[0:1], t[1:2], t[2:4]
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,steps", CONFIGS + PREPROC_CONFIGS + TASK_CONFIGS)
def test_rollout_parity(name, n, steps):
    spec = registry.lookup(name)
    seeds = [1000 + i for i in range(n)]
    vec = magical_amd.make_vec(name, n, seeds=seeds)
    orc = [oracle_env(spec, s) for s in seeds]
    acts = np.random.RandomState(42).randint(0, 18, (steps, n))
    obs = vec.reset()
    ref = [with_targets(spec, oracle_obs_split(spec, o.reset()), o) for o in orc]
    assert list(obs.keys()) == list(vec.observation_space.spaces.keys())
    for k in obs:
        got = obs[k].cpu().numpy()
        for i in range(n):
            assert np.array_equal(got[i], ref[i][k]), f"reset obs {k} env {i}"
    max_pose = 0.0
    for t in range(steps):
        obs, rew, done, info = vec.step(torch.as_tensor(acts[t], dtype=torch.uint8))
        torch.cuda.synchronize()
        got_obs = {k: v.cpu().numpy() for k, v in obs.items()}
        got_rew, got_done = rew.cpu().numpy(), done.cpu().numpy()
        got_score = info["eval_score"].cpu().numpy()
        bodies, counts = vec.bodies()
        bodies = bodies.cpu().numpy()
        for i in range(n):
            o, r, d, s = orc[i].step(int(acts[t, i]))
            assert bool(got_done[i]) == d, f"step {t} env {i} done"
            assert got_score[i] == s and got_rew[i] == np.float32(r), f"step {t} env {i} score {got_score[i]} vs {s}"
            if d:
                o = orc[i].reset()
            else:
                b = orc[i].bodies()
                diff = np.abs(bodies[i, :len(b)] - b).max()
                max_pose = max(max_pose, diff)
                assert diff <= POSE_TOL, f"step {t} env {i} body state diff {diff}"
            ref = with_targets(spec, oracle_obs_split(spec, o), orc[i])
            for k in got_obs:
                assert np.array_equal(got_obs[k][i], ref[k]), f"step {t} env {i} obs {k}"
    assert int(vec.errors().abs().sum().item()) == 0
    vec.close()


# every compiled step-kernel (and render-class) form, forced through the experiment switches read at mg_create
# (MG_STEP_VARIANT: 0 = HBM state (the default for scenes beyond the LDS caps), 5/6 = compile-time
# constraint lists with 4 lanes per env (robot scenes), 4 = LDS with runtime lists, one env per 64-lane
# wavefront (every other scene); MG_STEP_BLK / MG_STEP_BLK0: envs per workgroup).  The robot-scene rows are
# effectively contact-free (45 random steps from reset; live arbiters in 0.16% of MoveToRegion env-steps, DESIGN.md
# section 2): the forms' contact paths are compared with the oracle in tests/test_contact_forms.py
KERNEL_FORMS = [
    ("MoveToRegion-Demo-LoRes4E-v0", 70, 45, {"MG_STEP_VARIANT": "0", "MG_STEP_BLK0": "8"}),
    # 4 lanes per env (16 envs per 64-lane workgroup; 70 envs leave shadow lanes in the last one)
    ("MoveToRegion-Demo-LoRes4E-v0", 70, 45, {"MG_STEP_VARIANT": "5"}),   # 8 envs per workgroup (small grid)
    ("MoveToRegion-Demo-LoRes4E-v0", 70, 45, {"MG_STEP_VARIANT": "5", "MG_STEP_BLK": "16"}),
    ("MoveToCorner-Demo-LoRes4E-v0", 70, 45, {"MG_STEP_VARIANT": "6", "MG_STEP_BLK": "16"}),
    # robot + block scenes at 8 envs per workgroup (8 lanes per env; the default below 16 envs per CU, the
    # pipelined pool's 2048-env chunks): removed in round 4 after a GPU fault, restored in round 5.  The 4-env
    # workgroups (16 lanes per env) were removed in round 6 after an unexplained fault of form 5/4
    # (profiles/r06_blk4)
    ("MoveToCorner-Demo-LoRes4E-v0", 70, 45, {"MG_STEP_VARIANT": "6", "MG_STEP_BLK": "8"}),
    ("MoveToCorner-Demo-LoRes4E-v0", 70, 45, {"MG_STEP_VARIANT": "0", "MG_STEP_BLK0": "1"}),
    ("ClusterColour-Demo-LoResStack-v0", 66, 30, {"MG_STEP_VARIANT": "4"}),
    ("MatchRegions-TestAll-LoRes4E-v0", 66, 30, {"MG_STEP_VARIANT": "4"}),
    ("ClusterShape-TestAll-LoRes4E-v0", 66, 30, {"MG_STEP_VARIANT": "0"}),
    ("MatchRegions-TestAll-LoRes4E-v0", 66, 30, {"MG_STEP_VARIANT": "0"}),
    ("MatchRegions-TestAll-LoRes4E-v0", 66, 30, {"MG_STEP_VARIANT": "0", "MG_STEP_BLK0": "8"}),
    # render classes of the many-block tasks: the first 1 / 2 / 3 classes of the chain (medium-0, medium-1,
    # medium-2) hand every (env, view) on
    ("ClusterColour-TestAll-LoResStack-v0", 66, 30, {"MG_DEBUG_RENDER_RETRY": "1"}),
    ("MatchRegions-TestAll-LoRes4E-v0", 66, 30, {"MG_DEBUG_RENDER_RETRY": "1"}),
    ("ClusterColour-TestAll-LoResStack-v0", 66, 30, {"MG_DEBUG_RENDER_RETRY": "2"}),
    ("MatchRegions-TestAll-LoRes4E-v0", 66, 30, {"MG_DEBUG_RENDER_RETRY": "2"}),
    ("MatchRegions-TestAll-LoRes4E-v0", 66, 30, {"MG_DEBUG_RENDER_RETRY": "3"}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,steps,env", KERNEL_FORMS,
                         ids=[f[0].split("-")[0] + "-" + "-".join(f"{k}{v}" for k, v in f[3].items())
                              for f in KERNEL_FORMS])
def test_step_kernel_forms(name, n, steps, env, monkeypatch):
    """Every step-kernel form gives the oracle's trajectories (a spread of envs across workgroups)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    spec = registry.lookup(name)
    seeds = [300 + i for i in range(n)]
    vec = magical_amd.make_vec(name, n, seeds=seeds)
    pick = sorted({0, 1, 3, 4, 15, 16, 17, 63, 64, n - 1})
    orc = {i: oracle_env(spec, seeds[i]) for i in pick}
    acts = np.random.RandomState(11).randint(0, 18, (steps, n))
    vec.reset()
    for i in pick:
        orc[i].reset()
    for t in range(steps):
        obs, rew, done, info = vec.step(torch.as_tensor(acts[t], dtype=torch.uint8))
        got = {k: v[pick].cpu().numpy() for k, v in obs.items()}
        bodies, _ = vec.bodies()
        bodies = bodies[pick].cpu().numpy()
        for j, i in enumerate(pick):
            o, r, d, s = orc[i].step(int(acts[t, i]))
            if d:
                o = orc[i].reset()
            else:
                b = orc[i].bodies()
                assert np.abs(bodies[j, :len(b)] - b).max() <= POSE_TOL, f"step {t} env {i} bodies"
            ref = oracle_obs_split(spec, o)
            for k in got:
                assert np.array_equal(got[k][j], ref[k]), f"step {t} env {i} obs {k}"
    assert int(vec.errors().abs().sum().item()) == 0
    vec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["MakeLine-TestLayout-v0", "MakeLine-TestCountPlus-v0", "MatchRegions-TestLayout-v0",
                                  "FindDupe-TestLayout-v0", "FindDupe-TestAll-v0", "FixColour-TestLayout-v0",
                                  "FixColour-TestAll-v0",
                                  "ClusterColour-TestLayout-v0", "ClusterShape-TestLayout-v0",
                                  "MoveToRegion-TestLayout-v0", "MoveToCorner-TestAll-v0"])
def test_scores_on_random_layouts(name):
    """Episode length 1: every env is scored on its randomised initial layout (plus one step), so
    the scorers see many non-trivial layouts; GPU eval_score == oracle for all of them."""
    spec = registry.lookup(name)
    n = 512
    seeds = [5000 + i for i in range(n)]
    vec = magical_amd.make_vec(name, n, seeds=seeds, max_episode_steps=1, auto_reset=False)
    vec.reset()
    acts = np.random.RandomState(2).randint(0, 18, n)
    _, rew, done, info = vec.step(torch.as_tensor(acts, dtype=torch.uint8))
    got = info["eval_score"].cpu().numpy()
    errs = vec.errors().cpu().numpy()
    assert bool(done.all())
    ref = np.zeros(n)
    placement = np.zeros(n, dtype=bool)
    for i in range(n):
        o = po.OracleEnv(spec.task, spec.rand_flags, spec.preproc, 1, seed=seeds[i])
        try:
            o.reset()
        except po.PlacementError:  # geom.py:335-336 (e.g. MoveToCorner robot drawn next to a corner)
            placement[i] = True
            continue
        ref[i] = o.step(int(acts[i]))[3]
    assert np.array_equal((errs & 2) != 0, placement)
    ok = ~placement
    assert np.array_equal(got[ok], ref[ok]), np.nonzero(got[ok] != ref[ok])
    assert int(np.abs(errs & ~(2 | 64)).sum()) == 0
    vec.close()
    print(name, "non-zero scores:", int((ref > 0).sum()), "of", n)


def _placements(name, kinds, cols, roles_in_goal, poses, rs, targets=None):
    """Block poses that make the scorers' outcomes vary: blocks dropped into / pulled out of goal
    regions, laid along a line (MakeLine) or gathered by colour (ClusterColour)."""
    goals = [i for i, k in enumerate(kinds) if k == 1]
    blocks = [i for i, k in enumerate(kinds) if k == 3]
    out = {}
    if name.startswith("MakeLine"):
        o, d = rs.uniform(-0.5, 0.5, 2), rs.uniform(-1, 1, 2)
        d /= np.linalg.norm(d)
        for j, b in enumerate(blocks):
            if rs.rand() < 0.85:
                t = (j - 1.5) * rs.uniform(0.3, 0.45)
                out[b] = (*(o + t * d + rs.uniform(-0.12, 0.12, 2)), rs.uniform(-3, 3))
        return out
    if name.startswith("PickAndPlace"):
        tx, ty = targets[2], targets[3]
        for b in blocks:
            if rs.rand() < 0.7:
                out[b] = (tx + rs.uniform(-0.3, 0.3), ty + rs.uniform(-0.3, 0.3), rs.uniform(-3, 3))
        return out
    if name.startswith("Cluster"):
        centre = {c: rs.uniform(-0.6, 0.6, 2) for c in set(cols)}
        for b in blocks:
            if rs.rand() < 0.9:
                out[b] = (*(centre[cols[b]] + rs.uniform(-0.15, 0.15, 2)), rs.uniform(-3, 3))
        return out
    for j, b in enumerate(blocks):
        r = rs.rand()
        if name.startswith("FixColour"):
            g = goals[j] if j < len(goals) else goals[0]
            if roles_in_goal[b] == 2 and r < 0.7:  # the odd block out
                out[b] = (rs.uniform(-0.9, 0.9), rs.uniform(-0.9, 0.9), rs.uniform(-3, 3))
            elif r < 0.2:
                out[b] = (rs.uniform(-0.9, 0.9), rs.uniform(-0.9, 0.9), rs.uniform(-3, 3))
            else:
                continue
            continue
        g = goals[rs.randint(len(goals))]
        want_in = r < (0.7 if roles_in_goal[b] == 1 else 0.15)
        if want_in:
            gx, gy, gh, gw = poses[g]
            out[b] = (gx + rs.uniform(-0.35, 0.35) * gw, gy + rs.uniform(-0.35, 0.35) * gh, rs.uniform(-3, 3))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["FindDupe-Demo-v0", "FindDupe-TestAll-v0", "FixColour-Demo-v0", "FixColour-TestAll-v0",
                                  "MatchRegions-TestAll-v0", "MakeLine-TestAll-v0", "ClusterColour-TestAll-v0",
                                  "ClusterShape-TestAll-v0", "PickAndPlace-Demo-v0", "PickAndPlace-Test-v0"])
def test_scores_with_placed_blocks(name):
    """Blocks are moved (Body.position / angle setters, both sides) into scoring configurations, then
    one step ends the episode: GPU eval_score == oracle on layouts with every score outcome."""
    spec = registry.lookup(name)
    n = 192
    seeds = [7000 + i for i in range(n)]
    vec = magical_amd.make_vec(name, n, seeds=seeds, max_episode_steps=1, auto_reset=False)
    vec.reset()
    acts = np.random.RandomState(4).randint(0, 18, n)
    ref, rref = np.zeros(n), np.zeros(n)
    skip = np.zeros(n, dtype=bool)
    for i in range(n):
        o = po.OracleEnv(spec.task, spec.rand_flags, spec.preproc, 1, seed=seeds[i])
        try:
            o.reset()
        except po.PlacementError:
            skip[i] = True
            continue
        kinds, types, cols, poses = o.entities()
        body0, nb = {}, 0
        for k, kind in enumerate(kinds):  # bodies in entity add order: blocks 1, robot 6, others 0
            body0[k] = nb
            nb += 1 if kind == 3 else 6 if kind == 2 else 0
        roles = {}
        goal = [k for k, kind in enumerate(kinds) if kind == 1]
        for k, kind in enumerate(kinds):  # role proxy from colours: same colour as (its) goal
            if kind == 3:
                roles[k] = 1 if goal and cols[k] == cols[goal[0]] else 2
        if name.startswith("FixColour"):
            blocks = [k for k, kind in enumerate(kinds) if kind == 3]
            roles = {b: (1 if cols[b] == cols[goal[j]] else 2) for j, b in enumerate(blocks)}
        tg = o.target() if spec.task == "PickAndPlace" else None
        for b, (x, y, a) in _placements(name, kinds, cols, roles, poses, np.random.RandomState(i), tg).items():
            o.set_body_pose(body0[b], x, y, a)
            vec.set_body_pose(i, body0[b], x, y, a)
        _, rref[i], _, ref[i] = o.step(int(acts[i]))
    _, rew, done, info = vec.step(torch.as_tensor(acts, dtype=torch.uint8))
    got = info["eval_score"].cpu().numpy()
    assert np.array_equal(rew.cpu().numpy()[~skip], rref[~skip].astype(np.float32))
    errs = vec.errors().cpu().numpy()
    assert np.array_equal((errs & 2) != 0, skip)
    assert np.array_equal(got[~skip], ref[~skip]), np.nonzero(got[~skip] != ref[~skip])
    vals = np.unique(ref[~skip])
    print(name, f"{len(vals)} distinct scores; zero {int((ref[~skip] == 0).sum())}, one {int((ref[~skip] == 1).sum())}")
    assert len(vals) >= 2, "placements produced a single score outcome"
    vec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,retry", [(c[0], 0) for c in CONFIGS] + [("MatchRegions-TestAll-LoRes4E-v0", 1),
                                                                     ("MatchRegions-TestAll-LoRes4E-v0", 2),
                                                                     ("MatchRegions-TestAll-LoRes4E-v0", 3)])
def test_full_resolution_frames(name, retry, monkeypatch):
    if retry:   # the later render classes, through the earlier classes' hand-over
        monkeypatch.setenv("MG_DEBUG_RENDER_RETRY", str(retry))
    spec = registry.lookup(name)
    n = 3
    seeds = [7 + i for i in range(n)]
    vec = magical_amd.make_vec(name, n, seeds=seeds)
    orc = [oracle_env(spec, s) for s in seeds]
    vec.reset()
    for o in orc:
        o.reset()
    acts = np.random.RandomState(3).randint(0, 18, (25, n))
    for t in range(25):
        vec.step(torch.as_tensor(acts[t], dtype=torch.uint8))
        for i in range(n):
            orc[i].step(int(acts[t, i]))
        if t % 8 == 0 or t == 24:
            full = vec.render_full().cpu().numpy()
            for i in range(n):
                a, g = orc[i].render_full()
                assert np.array_equal(full[i, 0], a), f"allo frame step {t} env {i}"
                assert np.array_equal(full[i, 1], g), f"ego frame step {t} env {i}"
    vec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,steps,L", [("MoveToRegion-Demo-LoRes4E-v0", 1, 200, None),
                                            ("MoveToRegion-Demo-LoRes4E-v0", 4096, 205, None),
                                            ("MoveToRegion-Demo-LoRes4E-v0", 4096, 210, 250),
                                            ("MoveToCorner-Demo-LoRes4E-v0", 4096, 85, None),
                                            ("MoveToCorner-Demo-LoRes4E-v0", 4096, 210, 250),
                                            ("ClusterColour-Demo-LoResStack-v0", 64, 255, None),
                                            ("ClusterColour-Demo-LoResStack-v0", 8192, 250, None),
                                            ("MatchRegions-TestAll-LoRes4E-v0", 8192, 125, None)])
def test_full_size_sampled_parity(name, n, steps, L):
    """BASELINE configs at their sizes (C2 4096, C3 4096, C4 8192, C5 8192) plus the C1 plumbing case
    (1 env x 200 steps): every env steps on the GPU, a spread of envs (incl. the first/last lanes of
    64-wide blocks and the last env; every env when n <= 64) is checked against the oracle every step --
    observations bit-exact, body state (p, a, v, w) within POSE_TOL (north star: positions within 1e-4
    over 200 steps), done / eval_score equal.  Episode lengths: MoveToRegion 40, MoveToCorner 80,
    ClusterColour 240, MatchRegions 120 steps, so the default cases cross 5 / 1 / 1 / 1 auto-resets
    (ClusterColour-Demo-LoResStack at step 240, with its frame stacks refilled); L = 250 lifts the
    TimeLimit so MoveToRegion / MoveToCorner run 210 contiguous physics steps with no reset."""
    spec = registry.lookup(name)
    seeds = [1000 + i for i in range(n)]
    vec = magical_amd.make_vec(name, n, seeds=seeds, max_episode_steps=L)
    pick = list(range(n)) if n <= 64 else sorted(i for i in {0, 1, 63, 64, 127, n // 2 + 5, n - 65, n - 1} if 0 <= i < n)
    orc = {i: po.OracleEnv(spec.task, spec.rand_flags, spec.preproc, L or spec.max_episode_steps, seed=seeds[i])
           for i in pick}
    resets = 0
    acts = np.random.RandomState(9).randint(0, 18, (steps, n))
    obs = vec.reset()
    for i in pick:
        ref = oracle_obs_split(spec, orc[i].reset())
        for k in obs:
            assert np.array_equal(obs[k][i].cpu().numpy(), ref[k]), f"reset env {i} {k}"
    for t in range(steps):
        obs, rew, done, info = vec.step(torch.as_tensor(acts[t], dtype=torch.uint8))
        got = {k: v[pick].cpu().numpy() for k, v in obs.items()}
        got_done = done[pick].cpu().numpy()
        got_score = info["eval_score"][pick].cpu().numpy()
        bodies = vec.bodies()[0][pick].cpu().numpy()
        for j, i in enumerate(pick):
            o, r, d, s = orc[i].step(int(acts[t, i]))
            assert bool(got_done[j]) == d and got_score[j] == s, f"step {t} env {i}"
            if d:
                o = orc[i].reset()
                resets += 1
            else:
                b = orc[i].bodies()
                diff = np.abs(bodies[j, :len(b)] - b).max()
                assert diff <= POSE_TOL, f"step {t} env {i} body state diff {diff}"
            ref = oracle_obs_split(spec, o)
            for k in got:
                assert np.array_equal(got[k][j], ref[k]), f"step {t} env {i} obs {k}"
    assert resets == len(pick) * (steps // (L or spec.max_episode_steps))
    assert int(vec.errors().abs().sum().item()) == 0
    vec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,L", [("MoveToRegion-Demo-LoRes4E-v0", 70, 9), ("MoveToRegion-Demo-LoRes4A-v0", 70, 9),
                                      ("ClusterColour-Demo-LoResStack-v0", 66, 9),
                                      ("MoveToCorner-Demo-LoResCHW4E-v0", 40, 7)])
def test_window_stacks_match_materialised(name, n, L):
    """The simulator's window rings (mg_bind_window, make_vec(window=True)): every stacked output, read as the
    strided view of its ring, equals the materialised stack of the default env (and so the oracle's) bit for
    bit over 30 steps -- the ring (K = 8) wraps three times, episodes of L
    steps end in auto-resets that refill the window, and a masked explicit reset at step 15 refills some envs'
    windows while the others keep theirs."""
    seeds = [500 + i for i in range(n)]
    a = magical_amd.make_vec(name, n, seeds=seeds, max_episode_steps=L, window=True)
    b = magical_amd.make_vec(name, n, seeds=seeds, max_episode_steps=L)
    assert a.window_k == 8 and b.window_k == 0
    oa, ob = a.reset(), b.reset()
    stacked = [k for k in oa if oa[k].shape[-1] == 12 or (oa[k].dim() == 4 and oa[k].shape[1] == 12)]
    assert stacked and all(not oa[k].is_contiguous() for k in stacked)
    acts = np.random.RandomState(8).randint(0, 18, (30, n))
    mask = torch.from_numpy((np.random.RandomState(9).rand(n) < 0.3).astype(np.uint8)).cuda()
    for t in range(30):
        for k in ob:
            assert torch.equal(oa[k], ob[k]), (t, k)
        if t == 15:
            oa, ob = a.reset(mask), b.reset(mask)
            for k in ob:
                assert torch.equal(oa[k], ob[k]), ("masked reset", k)
        act = torch.as_tensor(acts[t], dtype=torch.uint8)
        oa, ra, da, ia = a.step(act)
        ob, rb, db, ib = b.step(act)
        assert torch.equal(ra, rb) and torch.equal(da, db)
    for k in ob:
        assert torch.equal(oa[k], ob[k]), k
    assert int(a.errors().abs().sum()) == 0
    a.close()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,steps", [("MoveToRegion-Demo-LoRes4E-v0", 4096, 85),
                                          ("MoveToCorner-Demo-LoRes4E-v0", 4096, 165)])
def test_full_size_pipelined_parity(name, n, steps):
    """The configuration bench.py times for C2 / C3: magical_amd.pipeline.PipelinedVecEnv
    with bench.py's own chunking (pipeline.default_chunks: MoveToRegion 3 chunks of 1360-1376 envs, MoveToCorner 2 of
    2048; the 8-envs-per-workgroup step
    forms 5 / 6 and the auto-reset fused into the step kernel),
    episode phases spread over the envs the oracle does not follow (so every step mixes resetting and running
    envs in a workgroup), against the oracle every step on a spread of envs of every chunk: observations
    bit-exact, body state within POSE_TOL, done / eval_score equal, >= 2 episode boundaries."""
    from magical_amd import pipeline
    spec = registry.lookup(name)
    L = spec.max_episode_steps
    seeds = [1000 + i for i in range(n)]
    chunks = pipeline.default_chunks(spec, n)
    pool = pipeline.PipelinedVecEnv(name, n, chunks=chunks, seeds=seeds)
    assert chunks >= 2 and sum(s.num_envs for s in pool.sims) == n
    pick = {0, 1, 7, 8, 63, 64, n - 9, n - 1}
    for b in pool.bounds[1:-1]:   # both sides of every chunk boundary
        pick |= {b - 1, b, b + 1, b + 9}
    pick = sorted(pick)
    orc = {i: po.OracleEnv(spec.task, spec.rand_flags, spec.preproc, L, seed=seeds[i]) for i in pick}
    obs = pool.reset()
    pool.wait()
    for i in pick:
        ref = oracle_obs_split(spec, orc[i].reset())
        for k in obs:
            assert np.array_equal(obs[k][i].cpu().numpy(), ref[k]), f"reset env {i} {k}"
    phase = np.array([0 if i in orc else (i * 7) % L for i in range(n)], dtype=np.int32)
    pool.set_episode_steps(torch.from_numpy(phase))
    acts = np.random.RandomState(9).randint(0, 18, (steps, n)).astype(np.uint8)
    a_dev = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    resets = 0
    for t in range(steps):
        a_dev.copy_(torch.from_numpy(acts[t]))
        obs, rew, done, info = pool.step(a_dev)
        pool.wait()
        got = {k: v[pick].cpu().numpy() for k, v in obs.items()}
        got_done, got_score = done[pick].cpu().numpy(), info["eval_score"][pick].cpu().numpy()
        bodies = torch.cat([s.bodies()[0] for s in pool.sims])[pick].cpu().numpy()
        for j, i in enumerate(pick):
            o, r, d, s = orc[i].step(int(acts[t, i]))
            assert bool(got_done[j]) == d and got_score[j] == s, f"step {t} env {i}"
            if d:
                o = orc[i].reset()
                resets += 1
            else:
                b = orc[i].bodies()
                diff = np.abs(bodies[j, :len(b)] - b).max()
                assert diff <= POSE_TOL, f"step {t} env {i} body state diff {diff}"
            ref = oracle_obs_split(spec, o)
            for k in got:
                assert np.array_equal(got[k][j], ref[k]), f"step {t} env {i} obs {k}"
    assert resets == len(pick) * (steps // L) and steps // L >= 2
    assert int((pool.errors() != 0).sum()) == 0
    pool.close()


# Auto-reset paths (mg_sim.hip): the next-layout shadow (default for the many-block tasks: the next
# episode's layout is sampled on a side stream while the current one runs, and the auto-reset copies it in)
# and the in-place reset_kernel (default for the robot scenes), each forced both ways with short episodes,
# plus a re-seed and a masked explicit reset while the shadow is live.
RESET_PATHS = [
    ("MatchRegions-TestAll-LoRes4E-v0", 66, 40, 7, {}),
    ("MatchRegions-TestAll-LoRes4E-v0", 66, 40, 7, {"MG_RESET_PREFETCH": "0"}),
    # the shadow -> main copy with several envs per workgroup (the default cap, 2048 workgroups, is above n here)
    ("MatchRegions-TestAll-LoRes4E-v0", 66, 40, 7, {"MG_COPY_WG": "5"}),
    ("ClusterColour-TestAll-LoResStack-v0", 66, 30, 4, {}),
    ("MoveToRegion-Demo-LoRes4E-v0", 70, 45, 5, {"MG_RESET_PREFETCH": "1"}),
    # the robot scenes' auto-reset: fused into the step kernel (default) and as its own launch
    ("MoveToRegion-Demo-LoRes4E-v0", 70, 45, 5, {}),
    ("MoveToCorner-Demo-LoRes4E-v0", 70, 45, 6, {}),
    ("MoveToCorner-Demo-LoRes4E-v0", 70, 45, 6, {"MG_FUSED_RESET": "0"}),
    ("PickAndPlace-Demo-LoResCHW4A-v0", 8, 30, 4, {}),
    ("PickAndPlace-Demo-LoResCHW4A-v0", 8, 30, 4, {"MG_COPY_WG": "3"}),
    ("FindDupe-TestAll-LoRes4E-v0", 66, 30, 1, {}),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,steps,L,env", RESET_PATHS,
                         ids=[f"{f[0].split('-')[0]}-L{f[3]}-" + "-".join(f"{k}{v}" for k, v in f[4].items())
                              for f in RESET_PATHS])
def test_reset_paths(name, n, steps, L, env, monkeypatch):
    """Auto-resets every L steps through either reset path equal the oracle's resets (observations,
    bodies, done / score, PickAndPlace targets, error flags); then the envs are re-seeded, run again, and
    a masked explicit reset is issued mid-episode with auto-reset on."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    spec = registry.lookup(name)
    pick = sorted(i for i in {0, 1, 17, 63, 64, n - 1} if i < n)

    def run(seeds, acts, masked_at=None):
        orc = {i: po.OracleEnv(spec.task, spec.rand_flags, spec.preproc, L, seed=seeds[i]) for i in pick}
        obs = vec.reset()
        for i in pick:
            ref = with_targets(spec, oracle_obs_split(spec, orc[i].reset()), orc[i])
            for k in obs:
                assert np.array_equal(obs[k][i].cpu().numpy(), ref[k]), f"reset env {i} {k}"
        mask = np.zeros(n, dtype=np.uint8)
        mask[pick[1::2]] = 1
        for t in range(acts.shape[0]):
            if t == masked_at:
                obs = vec.reset(torch.as_tensor(mask))
                for i in pick:
                    if mask[i]:
                        ref = with_targets(spec, oracle_obs_split(spec, orc[i].reset()), orc[i])
                        for k in obs:
                            assert np.array_equal(obs[k][i].cpu().numpy(), ref[k]), f"masked reset env {i} {k}"
            obs, rew, done, info = vec.step(torch.as_tensor(acts[t], dtype=torch.uint8))
            got = {k: v[pick].cpu().numpy() for k, v in obs.items()}
            got_done = done[pick].cpu().numpy()
            got_score = info["eval_score"][pick].cpu().numpy()
            bodies = vec.bodies()[0][pick].cpu().numpy()
            for j, i in enumerate(pick):
                o, r, d, sc = orc[i].step(int(acts[t, i]))
                assert bool(got_done[j]) == d and got_score[j] == sc, f"step {t} env {i}"
                if d:
                    o = orc[i].reset()
                else:
                    b = orc[i].bodies()
                    assert np.abs(bodies[j, :len(b)] - b).max() <= POSE_TOL, f"step {t} env {i} bodies"
                ref = with_targets(spec, oracle_obs_split(spec, o), orc[i])
                for k in got:
                    assert np.array_equal(got[k][j], ref[k]), f"step {t} env {i} obs {k}"

    seeds = [700 + i for i in range(n)]
    vec = magical_amd.make_vec(name, n, seeds=seeds, max_episode_steps=L)
    run(seeds, np.random.RandomState(3).randint(0, 18, (steps, n)))
    seeds2 = [9000 + 3 * i for i in range(n)]
    vec.seed(seeds2)
    run(seeds2, np.random.RandomState(4).randint(0, 18, (steps, n)), masked_at=steps // 2 + 1)
    assert int(vec.errors().abs().sum().item()) == 0
    vec.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", [("MoveToRegion-Demo-LoRes4E-v0", 64), ("MoveToCorner-Demo-LoRes4E-v0", 64)])
def test_allo_static_layer_in_use(name, n, monkeypatch):
    """The allocentric static layer (render_kernel: arena + goals rendered once per episode, copied into
    every 4x4 block no body geom reaches) is really used: with its copied blocks poisoned
    (MG_DEBUG_SCACHE=2) the reset frames are still exact and later allo frames carry the poison outside
    the bodies' reach, while the ego view is untouched; with the layer off (=1) every frame equals the
    oracle.  (The default path's parity is every other rollout test.)"""
    spec = registry.lookup(name)
    seeds = [40 + i for i in range(n)]
    acts = np.random.RandomState(8).randint(0, 18, (6, n))
    for mode in ("2", "1"):
        monkeypatch.setenv("MG_DEBUG_SCACHE", mode)
        vec = magical_amd.make_vec(name, n, seeds=seeds)
        orc = [oracle_env(spec, s) for s in seeds]
        obs = vec.reset()
        ref = [oracle_obs_split(spec, o.reset()) for o in orc]
        for i in range(n):
            assert np.array_equal(obs["allo"][i].cpu().numpy(), ref[i]["allo"])
        for t in range(acts.shape[0]):
            obs, _, _, _ = vec.step(torch.as_tensor(acts[t], dtype=torch.uint8))
            allo, ego = obs["allo"].cpu().numpy(), obs["ego"].cpu().numpy()
            ref = [oracle_obs_split(spec, orc[i].step(int(acts[t, i]))[0]) for i in range(n)]
            for i in range(n):
                assert np.array_equal(ego[i], ref[i]["ego"])
                if mode == "1":
                    assert np.array_equal(allo[i], ref[i]["allo"])
                else:
                    poisoned = np.all(allo[i] == 0x55, axis=-1) & np.any(ref[i]["allo"] != 0x55, axis=-1)
                    frac = poisoned.mean()
                    assert frac > 0.3, (t, i, frac)
                    keep = ~np.all(allo[i] == 0x55, axis=-1)
                    assert np.array_equal(allo[i][keep], ref[i]["allo"][keep])
        vec.close()


@pytest.mark.gpu
def test_device_sincos_is_correctly_rounded():
    """The device sin/cos (fast certified path + double-double fallback) equals the oracle's
    correctly rounded sin/cos on 1M arguments, incl. arguments next to multiples of pi/2."""
    import ctypes
    from magical_amd import native
    lib = native.load()
    rs = np.random.RandomState(123)
    x = np.concatenate([rs.uniform(-8, 8, 400000), rs.uniform(-1e-3, 1e-3, 100000),
                        rs.uniform(-40, 40, 400000),
                        (np.arange(-50, 51)[:, None] * (np.pi / 2) + rs.uniform(-1e-9, 1e-9, (101, 990))).ravel()])
    xd = torch.as_tensor(x, dtype=torch.float64, device="cuda")
    s = torch.empty_like(xd)
    c = torch.empty_like(xd)
    native.check(lib.mg_selftest_sincos(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(s.data_ptr()),
                                        ctypes.c_void_p(c.data_ptr()), len(x), None))
    torch.cuda.synchronize()
    s, c = s.cpu().numpy(), c.cpu().numpy()
    L = po.lib()
    ref_s = np.array([L.o_crsin(float(v)) for v in x])
    ref_c = np.array([L.o_crcos(float(v)) for v in x])
    assert np.array_equal(s, ref_s) and np.array_equal(c, ref_c)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["MoveToRegion-Demo-LoRes3EA-v0", "MoveToRegion-Demo-LoRes4E-v0"])
def test_masked_reset(name):
    """reset(mask) resets exactly the masked envs (SB3 VecEnv per-env reset); the
    others keep their state, frame stacks and observations."""
    spec = registry.lookup(name)
    n = 6
    seeds = [50 + i for i in range(n)]
    vec = magical_amd.make_vec(name, n, seeds=seeds, auto_reset=False)
    orc = [oracle_env(spec, s) for s in seeds]
    vec.reset()
    for o in orc:
        o.reset()
    acts = np.random.RandomState(5).randint(0, 18, (12, n))
    mask = np.array([1, 0, 0, 1, 0, 1], dtype=np.uint8)
    for t in range(12):
        if t == 6:
            obs = vec.reset(torch.as_tensor(mask))
            got = {k: v.cpu().numpy() for k, v in obs.items()}
            for i in range(n):
                if mask[i]:
                    ref = oracle_obs_split(spec, orc[i].reset())
                    for k in got:
                        assert np.array_equal(got[k][i], ref[k]), f"masked reset env {i} obs {k}"
        obs, rew, done, info = vec.step(torch.as_tensor(acts[t], dtype=torch.uint8))
        got = {k: v.cpu().numpy() for k, v in obs.items()}
        for i in range(n):
            o, r, d, s = orc[i].step(int(acts[t, i]))
            ref = oracle_obs_split(spec, o)
            for k in got:
                assert np.array_equal(got[k][i], ref[k]), f"step {t} env {i} obs {k}"
    vec.close()


@pytest.mark.gpu
def test_every_registered_name():
    """All 441 registered names (benchmarks/__init__.py:427-1102) run on the GPU: 2 envs, reset + 4
    steps, observations (keys, shapes, values), rewards, done and eval_score equal to the oracle."""
    checked = 0
    for name in registry.ALL_REGISTERED_ENVS:
        spec = registry.lookup(name)
        if spec.task == "PickAndPlace" and spec.preproc == "LoResStack":
            with pytest.raises(ValueError):
                magical_amd.make_vec(name, 2)
            continue
        seeds, orc, refs = [], [], []
        for sd in range(11, 40):  # seeds whose first layout places (PlacementError is covered elsewhere)
            o = oracle_env(spec, sd)
            try:
                first = o.reset()
            except po.PlacementError:
                continue
            seeds.append(sd); orc.append(o); refs.append(with_targets(spec, oracle_obs_split(spec, first), o))
            if len(seeds) == 2:
                break
        vec = magical_amd.make_vec(name, 2, seeds=seeds)
        obs = vec.reset()
        assert list(obs.keys()) == list(vec.observation_space.spaces.keys()), name
        for k, space in vec.observation_space.spaces.items():
            assert tuple(obs[k].shape[1:]) == tuple(space.shape), (name, k)
        acts = np.random.RandomState(1).randint(0, 18, (4, 2))
        for t in range(5):
            for i in range(2):
                for k in obs:
                    assert np.array_equal(obs[k][i].cpu().numpy(), refs[i][k]), (name, t, i, k)
            if t == 4:
                break
            obs, rew, done, info = vec.step(torch.as_tensor(acts[t], dtype=torch.uint8))
            for i in range(2):
                o, r, d, s = orc[i].step(int(acts[t, i]))
                assert rew[i].item() == np.float32(r) and bool(done[i]) == d, (name, t, i)
                refs[i] = with_targets(spec, oracle_obs_split(spec, o), orc[i])
        assert int(vec.errors().abs().sum().item()) == 0, name
        vec.close()
        checked += 1
    assert checked == len(registry.ALL_REGISTERED_ENVS) - 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["PickAndPlace-Demo-LoResCHW4A-v0", "MoveToCorner-Demo-LoRes4E-v0"])
def test_sb3_vec_env(name):
    """SB3 VecEnv adapter (train_rl.py:87-92 DummyVecEnv + Monitor): auto-reset obs = first frame of the
    next episode, info['terminal_observation'] = last frame of the finished one, Monitor episode
    return/length, eval_score in every info; all against oracle episodes."""
    from magical_amd.sb3 import MagicalVecEnv
    spec = registry.lookup(name)
    n, T, L = 3, 13, 5
    seeds = [21, 22, 23]
    venv = MagicalVecEnv(name, n, seeds=seeds, max_episode_steps=L)
    orc = [po.OracleEnv(spec.task, spec.rand_flags, spec.preproc, L, seed=s) for s in seeds]
    obs = venv.reset()
    ref = [with_targets(spec, oracle_obs_split(spec, o.reset()), o) for o in orc]
    ret = np.zeros(n)
    acts = np.random.RandomState(8).randint(0, 18, (T, n))
    for t in range(T):
        for i in range(n):
            for k in obs:
                assert np.array_equal(obs[k][i], ref[i][k]), (t, i, k)
        obs, rew, dones, infos = venv.step(acts[t])
        assert rew.dtype == np.float32 and dones.dtype == bool and len(infos) == n
        for i in range(n):
            o, r, d, s = orc[i].step(int(acts[t, i]))
            ret[i] += np.float32(r)
            assert rew[i] == np.float32(r) and dones[i] == d and infos[i]["eval_score"] == s
            last = with_targets(spec, oracle_obs_split(spec, o), orc[i])
            if d:
                term = infos[i]["terminal_observation"]
                for k in term:
                    assert np.array_equal(term[k], last[k]), (t, i, k)
                assert infos[i]["episode"]["l"] == L and infos[i]["TimeLimit.truncated"] is False
                assert abs(infos[i]["episode"]["r"] - ret[i]) < 1e-5
                ret[i] = 0.0
                ref[i] = with_targets(spec, oracle_obs_split(spec, orc[i].reset()), orc[i])
            else:
                assert "terminal_observation" not in infos[i]
                ref[i] = last
    venv.close()


@pytest.mark.gpu
def test_batched_evaluation_protocol():
    """BatchedEvaluationProtocol: each test variant's n_rollouts episodes run as one GPU batch; every
    score equals the oracle episode driven by the same actions."""
    from magical_amd import evaluation
    n = 6
    recorded = []

    def policy(obs):
        a = torch.as_tensor(np.random.RandomState(len(recorded)).randint(0, 18, n), dtype=torch.uint8).cuda()
        recorded.append(a.cpu().numpy())
        return a

    class Checked(evaluation.BatchedEvaluationProtocol):
        def obtain_scores(self, env_name):
            recorded.clear()
            scores = super().obtain_scores(env_name)
            spec = registry.lookup(env_name)
            for i in range(n):
                o = po.OracleEnv(spec.task, spec.rand_flags, spec.preproc, spec.max_episode_steps, seed=i)
                o.reset()
                for t, acts in enumerate(recorded):
                    _, _, d, s = o.step(int(acts[i]))
                assert d and s == scores[i], (env_name, i)
            return scores

    frame = Checked("MoveToRegion-Demo-LoRes4E-v0", n, policy, run_id="random").do_eval()
    assert len(frame) == 1 + len(registry.DEMO_ENVS_TO_TEST_ENVS_MAP["MoveToRegion-Demo-LoRes4E-v0"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,tries", [("MatchRegions-TestAll-LoRes4E-v0", 3), ("FindDupe-TestAll-LoRes4E-v0", 3),
                                        ("FixColour-TestAll-LoRes4E-v0", 3), ("ClusterColour-TestAll-LoResStack-v0", 3),
                                        ("MakeLine-TestAll-LoRes4E-v0", 2)])
def test_layout_retry_parity(name, tries, monkeypatch):
    """pm_randomise_all_poses retries (geom.py:295-341) with the try budget of pm_randomise_pose
    lowered from 10000 to `tries` on both sides (MG_DEBUG_MAX_TRIES / OracleEnv.set_max_tries), so most
    seeds need >= 1 failed whole-layout retry (seeds found by tools/scan_retry_seeds.py).  Covers:
    each entity's filter captured per retry (entities left with categories 0 by a failed retry stay
    non-colliding, in placement, physics and goal queries), rollback to the saved absolute poses on
    PlacementError, and the PlacementError flag.  Episodes cross an auto-reset (max_episode_steps 12)."""
    monkeypatch.setenv("MG_DEBUG_MAX_TRIES", str(tries))
    spec = registry.lookup(name)
    n, steps, L = 48, 26, 12
    seeds = list(range(n))
    vec = magical_amd.make_vec(name, n, seeds=seeds, max_episode_steps=L)
    orc = []
    for s in seeds:
        o = po.OracleEnv(spec.task, spec.rand_flags, spec.preproc, L, seed=s)
        o.set_max_tries(tries)
        orc.append(o)
    placement = np.zeros(n, dtype=bool)
    retried = 0
    obs = vec.reset()
    ref = []
    for i, o in enumerate(orc):
        try:
            ref.append(oracle_obs_split(spec, o.reset()))
        except po.PlacementError:
            placement[i] = True
            ref.append(None)
            continue
        retried += o.placement_retries() > 0
    assert retried >= n // 4, f"only {retried} of {n} seeds exercised a layout retry"
    errs = vec.errors().cpu().numpy()
    assert np.array_equal((errs & 2) != 0, placement)
    live = [i for i in range(n) if not placement[i]]
    for k in obs:
        got = obs[k].cpu().numpy()
        for i in live:
            assert np.array_equal(got[i], ref[i][k]), f"reset obs {k} env {i}"
    acts = np.random.RandomState(6).randint(0, 18, (steps, n))
    for t in range(steps):
        obs, rew, done, info = vec.step(torch.as_tensor(acts[t], dtype=torch.uint8))
        got = {k: v.cpu().numpy() for k, v in obs.items()}
        got_done, got_score = done.cpu().numpy(), info["eval_score"].cpu().numpy()
        bodies = vec.bodies()[0].cpu().numpy()
        errs = vec.errors().cpu().numpy()
        for i in live:
            if placement[i]:
                continue
            o, r, d, s = orc[i].step(int(acts[t, i]))
            assert bool(got_done[i]) == d and got_score[i] == s, f"step {t} env {i} score {got_score[i]} vs {s}"
            if d:
                try:
                    o = orc[i].reset()
                except po.PlacementError:
                    placement[i] = True
                    assert errs[i] & 2, f"step {t} env {i}: PlacementError on the oracle only"
                    continue
            else:
                b = orc[i].bodies()
                assert np.abs(bodies[i, :len(b)] - b).max() <= POSE_TOL, f"step {t} env {i} bodies"
            ref_i = oracle_obs_split(spec, o)
            for k in got:
                assert np.array_equal(got[k][i], ref_i[k]), f"step {t} env {i} obs {k}"
    vec.close()


# (name, gather mode, episode length, options): frames mode keeps the stacks as window-ring views (mg_restack_window,
# valid until the next step_async) except LoRes3EA and window=False (materialised by mg_restack, valid for nbuf - 1
# steps); chunks=2 runs the shard as a pipelined env pool under the exchange
GATHER_GPU_CASES = [("MoveToRegion-Demo-LoRes4E-v0", "frames", 40, {}),
                    ("MoveToRegion-Demo-LoRes4E-v0", "frames", 40, {"window": False}),
                    ("MoveToRegion-Demo-LoRes4E-v0", "frames", 40, {"chunks": 2}),
                    ("MoveToRegion-Demo-LoRes4E-v0", "stacked", 40, {}),
                    ("MoveToRegion-Demo-LoResCHW4E-v0", "frames", 40, {}),
                    ("ClusterColour-Demo-LoResStack-v0", "frames", 12, {}),
                    ("ClusterColour-Demo-LoResStack-v0", "frames", 12, {"window": False}),
                    ("ClusterColour-Demo-LoResStack-v0", "stacked", 12, {}),
                    ("MoveToCorner-Demo-LoRes3EA-v0", "frames", 15, {}),
                    ("MoveToCorner-Demo-LoRes4A-v0", "frames", 15, {}),
                    ("MoveToCorner-Demo-LoRes4A-v0", "frames", 15, {"chunks": 2}),
                    ("PickAndPlace-Demo-LoRes4E-v0", "frames", 15, {}),
                    ("PickAndPlace-Demo-LoRes4E-v0", "frames", 15, {"chunks": 2})]


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,L,opts", GATHER_GPU_CASES,
                         ids=[f"{c[0].split('-')[0]}-{c[0].split('-')[2]}-{c[1]}-" + "-".join(f"{k}{v}" for k, v in c[3].items())
                              for c in GATHER_GPU_CASES])
def test_packed_gather_pipeline_single_rank(tmp_path, name, mode, L, opts):
    """The multi-GPU exchange path on one GPU (a 1-rank RCCL group): the simulator writes each step's
    outputs straight into views of a packed buffer (bind_outputs; gather_mode 'frames': the current frames
    only), one all_gather_into_tensor per step on a side stream, then (frames) the receiver-side restack
    (window ring views, or mg_restack's materialised stacks) rebuilds the frame stacks; three buffer sets
    rotate.  Every step's gathered [1, n, ...] results equal a plain VecMagicalEnv run bit for bit (obs incl.
    the rebuilt stacks and the CHW views, reward, done, eval_score, PickAndPlace's target), over 45 steps that
    cross auto-resets (episode length L).  Results are read one step late (after the next step was launched)
    where the contract allows it -- materialised stacks and the stacked mode -- and before the next step for
    window-ring views."""
    import torch.distributed as dist
    from magical_amd import dist as mdist
    n, steps = 70, 45
    dist.init_process_group("nccl", init_method=f"file://{tmp_path}/pg", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        shard = mdist.ShardedVecEnv(name, n, rank=0, device="cuda:0", gather=True, gather_mode=mode,
                                    max_episode_steps=L, **opts)
        window = isinstance(getattr(shard, "restacker", None), mdist.WindowRestacker)
        assert window == (mode == "frames" and opts.get("window", True) and "3EA" not in name)
        lag = 0 if window else 1
        ref = magical_amd.make_vec(name, n, seeds=mdist.shard_seeds(n, 0), max_episode_steps=L)
        acts = np.random.RandomState(4).randint(0, 18, (steps, n))
        got = shard.reset()
        want = ref.reset()
        assert list(got) == list(want)
        for k in want:
            assert torch.equal(got[k][0], want[k]), f"reset {k}"
        handles, resets, prev = [], 0, {}
        for t in range(steps):
            a = torch.as_tensor(acts[t], dtype=torch.uint8)
            handles.append(shard.step_async(a))
            obs, rew, done, info = ref.step(a)
            resets += int(done.sum().item())
            prev[t] = ({k: v.clone() for k, v in obs.items()}, rew.clone(), done.clone(), info["eval_score"].clone(),
                       ref.target.clone() if ref.target is not None else None)
            u = t - lag
            if u >= 0:
                g_obs, g_rew, g_done, g_info = handles[u].results()
                w = prev.pop(u)
                assert list(g_obs) == list(w[0])
                for k in w[0]:
                    assert torch.equal(g_obs[k][0], w[0][k]), f"step {u} {k}"
                assert torch.equal(g_rew[0], w[1]) and torch.equal(g_done[0], w[2])
                assert torch.equal(g_info["eval_score"][0], w[3])
                if "target" in g_info:
                    assert torch.equal(g_info["target"][0], w[4]), f"step {u} target"
        assert resets >= n * (steps // L - 1)
        shard.close()
        ref.close()
    finally:
        dist.destroy_process_group()


TWO_RANK_WORKER = r"""
import os, sys
sys.path[:0] = [{root!r} + "/magical-1_amd"]
import numpy as np, torch, torch.distributed as dist
import magical_amd
from magical_amd import dist as mdist
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", init_method="env://")
name, mode, L, opts, n, steps = {name!r}, {mode!r}, {L}, {opts!r}, {n}, {steps}
shard = mdist.ShardedVecEnv(name, n, rank=rank, device="cuda:0", gather=True, gather_mode=mode,
                            max_episode_steps=L, **opts)
window = isinstance(getattr(shard, "restacker", None), mdist.WindowRestacker)
lag = 0 if window else 1
acts = np.random.RandomState(4).randint(0, 18, (steps, world * n))
lo, hi = mdist.shard_range(n, rank)
# rank 0 checks every gathered step against one process running all world * n envs (env i seeded 1000 + i)
ref = magical_amd.make_vec(name, world * n, seeds=list(range(1000, 1000 + world * n)), max_episode_steps=L) \
    if rank == 0 else None
bad = []
def check(tag, got, want):
    for k in want[0]:
        g = got[0][k].reshape((world * n,) + tuple(want[0][k].shape[1:]))
        if not torch.equal(g, want[0][k]):
            bad.append(f"{{tag}} {{k}}")
    if len(want) > 1:
        for i, key in ((1, "reward"), (2, "done")):
            if not torch.equal(got[i].reshape(-1), want[i]):
                bad.append(f"{{tag}} {{key}}")
        if not torch.equal(got[3]["eval_score"].reshape(-1), want[3]["eval_score"]):
            bad.append(f"{{tag}} eval_score")
got = shard.reset()
if rank == 0:
    check("reset", (got,), (ref.reset(),))
handles, prev, resets = [], {{}}, 0
for t in range(steps):
    handles.append(shard.step_async(torch.as_tensor(acts[t, lo:hi], dtype=torch.uint8)))
    if rank == 0:
        obs, rew, done, info = ref.step(torch.as_tensor(acts[t], dtype=torch.uint8))
        resets += int(done.sum().item())
        prev[t] = ({{k: v.clone() for k, v in obs.items()}}, rew.clone(), done.clone(),
                   {{"eval_score": info["eval_score"].clone()}})
    u = t - lag
    if u >= 0:
        r = handles[u].results()
        if rank == 0:
            check(f"step {{u}}", r, prev.pop(u))
if lag:
    r = handles[-1].results()
    if rank == 0:
        check(f"step {{steps - 1}}", r, prev.pop(steps - 1))
shard.close()
dist.barrier()
dist.destroy_process_group()
if rank == 0:
    print("resets", resets, "mismatches", len(bad), bad[:8], flush=True)
    sys.exit(1 if bad or resets < world * n else 0)
"""

TWO_RANK_CASES = [("MoveToRegion-Demo-LoRes4E-v0", "frames", 12, {"chunks": 2}),   # bench.py's N > 1 path
                  ("MoveToRegion-Demo-LoRes4E-v0", "stacked", 12, {}),
                  ("ClusterColour-Demo-LoResStack-v0", "frames", 10, {}),
                  ("MoveToCorner-Demo-LoRes4A-v0", "frames", 12, {"chunks": 2})]


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,L,opts", TWO_RANK_CASES,
                         ids=[f"{c[0].split('-')[0]}-{c[1]}-" + "-".join(f"{k}{v}" for k, v in c[3].items())
                              for c in TWO_RANK_CASES])
def test_two_rank_gather_on_one_gpu(tmp_path, name, mode, L, opts):
    """The multi-GPU exchange with world_size 2 (W > 1 of the GPU pool / window-ring path was unpinned):
    two processes, each a shard of 16 envs on the simulator, exchange every step's packed outputs with
    all_gather_into_tensor and rebuild the stacks on the receiver (window rings / materialised), the pipelined
    pool under the gather for MoveToRegion as bench.py runs it at N > 1.  RCCL refuses two ranks on one device, so
    the group here is gloo on the same card (the collective copies through the host); on a node each rank has its
    own GPU and the group is RCCL.  Rank 0 checks every gathered [2, 16, ...] step -- observations incl. the rebuilt
    stacks, reward, done, eval_score -- against one process running all 32 envs, bit for bit, across auto-resets."""
    import socket
    import subprocess
    import sys
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "worker.py"
    script.write_text(TWO_RANK_WORKER.format(root=root, name=name, mode=mode, L=L, opts=opts, n=16, steps=30))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-u", str(script)], env=env))
    rcs = []
    try:
        for p in procs:
            rcs.append(p.wait(timeout=150))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("preproc", ["LoRes4E", "LoResStack", "LoRes4A"])
def test_restack_window_matches_oracle_rule(preproc):
    """mg_restack_window on synthetic gathered batches (world 3, 37 envs per rank) with random frames and random
    done flags over 22 steps (the window ring's K = 8 wraps twice; its duplicate slots in use), an all-fresh reset
    first and again in the middle: the strided views equal the oracle's restatement of the reference's
    frame-stack rule and mg_restack's materialised stacks bit for bit."""
    from magical_amd import dist as mdist, registry
    name = {"LoRes4E": "MoveToRegion-Demo-LoRes4E-v0", "LoResStack": "ClusterColour-Demo-LoResStack-v0",
            "LoRes4A": "MoveToRegion-Demo-LoRes4A-v0"}[preproc]
    spec = registry.lookup(name)
    W, n = 3, 37
    lay = mdist.PackedLayout.for_spec(spec, n, frames_only=True)
    win = mdist.WindowRestacker(lay, W, torch.device("cuda", 0))
    nat = mdist.NativeRestacker(lay, W, torch.device("cuda", 0))
    orc = po.OracleRestacker(lay, preproc)
    rs = np.random.RandomState(12)
    keys = mdist.stacked_keys(preproc)
    for t in range(22):
        recv = torch.from_numpy(rs.randint(0, 256, W * lay.nbytes).astype(np.uint8))
        v = lay.unpack(recv)
        v["done"].copy_(torch.from_numpy(rs.rand(W, n) < 0.15))
        fresh = t in (0, 13)
        out_c = {k: torch.zeros((W * n, 96, 96, 12), dtype=torch.uint8) for k in keys}
        out_m = {k: torch.zeros((W * n, 96, 96, 12), dtype=torch.uint8, device="cuda") for k in keys}
        orc(recv, out_c, t, fresh)
        rg = recv.cuda()
        nat(rg, out_m, t, fresh)
        views = win(rg, None, t, fresh)
        torch.cuda.synchronize()
        assert list(views) == list(keys)
        for k in keys:
            assert views[k].shape == (W * n, 96, 96, 12) and views[k].stride() == ((8 + 3) * 27648, 96, 1, 9216)
            assert torch.equal(views[k].cpu(), out_c[k]), (t, k)
            assert torch.equal(views[k], out_m[k]), (t, k)


@pytest.mark.gpu
@pytest.mark.parametrize("preproc", ["LoRes4E", "LoResStack", "LoRes3EA", "LoRes4A"])
def test_restack_kernel_matches_oracle_rule(preproc):
    """mg_restack on synthetic gathered batches (world 3, 37 envs per rank: a ragged last workgroup) with
    random frames and random done flags over 9 steps, an all-fresh reset first and again in the middle:
    the stacks equal the oracle's restatement of the reference's frame-stack rule bit for bit."""
    from magical_amd import dist as mdist, registry
    name = {"LoRes4E": "MoveToRegion-Demo-LoRes4E-v0", "LoResStack": "ClusterColour-Demo-LoResStack-v0",
            "LoRes3EA": "MoveToRegion-Demo-LoRes3EA-v0", "LoRes4A": "MoveToRegion-Demo-LoRes4A-v0"}[preproc]
    spec = registry.lookup(name)
    W, n = 3, 37
    lay = mdist.PackedLayout.for_spec(spec, n, frames_only=True)
    nat = mdist.NativeRestacker(lay, W, torch.device("cuda", 0))
    orc = po.OracleRestacker(lay, preproc)
    rs = np.random.RandomState(11)
    keys = mdist.stacked_keys(preproc)
    for t in range(9):
        recv = torch.from_numpy(rs.randint(0, 256, W * lay.nbytes).astype(np.uint8))
        v = lay.unpack(recv)
        v["done"].copy_(torch.from_numpy(rs.rand(W, n) < 0.2))
        fresh = t in (0, 5)
        out_c = {k: torch.zeros((W * n, 96, 96, 12), dtype=torch.uint8) for k in keys}
        out_g = {k: torch.zeros((W * n, 96, 96, 12), dtype=torch.uint8, device="cuda") for k in keys}
        orc(recv, out_c, t, fresh)
        nat(recv.cuda(), out_g, t, fresh)
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(out_g[k].cpu(), out_c[k]), (t, k)




@pytest.mark.gpu
@pytest.mark.parametrize("name", ["FindDupe-TestAll-LoRes4E-v0", "MoveToCorner-TestAll-LoRes4E-v0"])
def test_single_env_reset_after_placement_error(monkeypatch, name):
    """gym single-env semantics after a PlacementError (geom.py:335-336 raises out of reset()): the next
    reset() draws a new layout from the advancing RNG and succeeds or fails on its own -- the error flag
    of one reset does not stick to later ones, and FindDupe / FixColour-style query blocks are
    placed again.  The try budget is lowered on both sides (MG_DEBUG_MAX_TRIES / set_max_tries) so that
    failures happen; every reset's outcome and observation equal the oracle's."""
    from magical_amd.envs import PlacementError
    monkeypatch.setenv("MG_DEBUG_MAX_TRIES", "1")
    spec = registry.lookup(name)
    found = None
    for seed in range(200):
        o = po.OracleEnv(spec.task, spec.rand_flags, spec.preproc, spec.max_episode_steps, seed=seed)
        o.set_max_tries(1)
        outcomes = []
        for _ in range(6):
            try:
                outcomes.append(o.reset())
            except po.PlacementError:
                outcomes.append(None)
        fails = [k for k, x in enumerate(outcomes) if x is None]
        if fails and any(x is not None for x in outcomes[fails[0] + 1:]):
            found = seed
            break
    assert found is not None, "no seed with a failed reset followed by a successful one"
    env = magical_amd.make(name, seed=found)
    for k, ref in enumerate(outcomes):
        if ref is None:
            with pytest.raises(PlacementError):
                env.reset()
            continue
        obs = env.reset()
        want = oracle_obs_split(spec, ref)
        for key in want:
            assert np.array_equal(obs[key], want[key]), (k, key)
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,chunks,L", [("MoveToRegion-Demo-LoRes4E-v0", 256, 2, 40),
                                             ("MoveToCorner-Demo-LoRes4E-v0", 96, 3, 25),
                                             ("PickAndPlace-Demo-LoResCHW4A-v0", 64, 2, 15),
                                             ("ClusterColour-Demo-LoResStack-v0", 64, 3, 20)])
def test_pipelined_pool_matches_batch(name, n, chunks, L):
    """magical_amd.pipeline: C simulators on C streams (env i of the pool seeded as env i of the batch) give the
    batch's outputs bit for bit, across episode boundaries, with the caller's action tensor overwritten right
    after every step() (the pool double-buffers actions on the device)."""
    from magical_amd import pipeline
    seeds = [1000 + i for i in range(n)]
    ref = mg_envs.VecMagicalEnv(name, n, seeds=seeds, max_episode_steps=L)
    pool = pipeline.PipelinedVecEnv(name, n, chunks=chunks, seeds=seeds, max_episode_steps=L)
    o_ref, o_pool = ref.reset(), pool.reset()
    pool.wait()
    for k in o_ref:
        assert torch.equal(o_ref[k], o_pool[k]), k
    acts = np.random.RandomState(42).randint(0, 18, (2 * L + 5, n)).astype(np.uint8)
    a_dev = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    for t in range(acts.shape[0]):
        a_dev.copy_(torch.from_numpy(acts[t]))
        o_ref, r_ref, d_ref, i_ref = ref.step(a_dev)
        o_pool, r_pool, d_pool, i_pool = pool.step(a_dev)
        a_dev.fill_(255)   # the pool must not read the caller's tensor after step() returns
        pool.wait()
        for k in o_ref:
            assert torch.equal(o_ref[k], o_pool[k]), (k, t)
        assert torch.equal(r_ref, r_pool) and torch.equal(d_ref, d_pool), t
        assert torch.equal(i_ref["eval_score"], i_pool["eval_score"]), t
    assert int((pool.errors() != 0).sum()) == 0
    pool.close()
    ref.close()


@pytest.mark.gpu
def test_pipelined_pool_target_after_every_entry_point():
    """PickAndPlace's target columns (and every other output) of a two-chunk pool against the flat batch after each
    call that rewrites the target: reset(), step_seq() with an auto-reset inside the call, restore(), reset_scenes()
    with a mask over both chunks, and step()."""
    from magical_amd import pipeline
    name, n, L = "PickAndPlace-Demo-LoResCHW4A-v0", 8, 6
    seeds = [1000 + i for i in range(n)]
    ref = mg_envs.VecMagicalEnv(name, n, seeds=seeds, max_episode_steps=L)
    pool = pipeline.PipelinedVecEnv(name, n, chunks=2, seeds=seeds, max_episode_steps=L)
    assert pool.bounds == [0, 4, 8]
    acts = torch.from_numpy(np.random.RandomState(42).randint(0, 18, (12, n)).astype(np.uint8))

    def same(o_ref, o_pool, at):
        pool.wait()
        assert list(o_ref) == list(o_pool) and all(k in o_pool for k in mg_envs.TARGET_KEYS), at
        for k in o_ref:
            assert torch.equal(o_ref[k], o_pool[k]), (at, k)
        for k, v in (("reward", ref.reward), ("done", ref.done), ("eval_score", ref.eval_score)):
            assert torch.equal(v, pool.buffers[k]), (at, k)
        if ref.seq_steps is not None:
            assert torch.equal(ref.seq_steps, pool.seq_steps), (at, "steps")

    same(ref.reset(), pool.reset(), "reset")
    ended = torch.zeros(n, dtype=torch.bool, device="cuda:0")
    for i in range(2):   # 4 + 2 env-steps: every env ends its episode in the second call and is auto-reset there
        a = acts[4 * i:4 * i + 4]
        (o_ref, _, d_ref, i_ref), (o_pool, _, _, i_pool) = ref.step_seq(a), pool.step_seq(a)
        same(o_ref, o_pool, ("step_seq", i))
        assert i_pool["steps"] is pool.seq_steps and i_ref["steps"] is ref.seq_steps
        ended |= d_ref
    assert bool(ended.all())
    snap, at_snap = pool.snapshot(), {k: v.clone() for k, v in o_pool.items()}
    for t in range(8, 11):
        (o_ref, *_), (o_pool, *_) = ref.step(acts[t]), pool.step(acts[t])
        same(o_ref, o_pool, ("step", t))
    o_ref, o_pool = ref.restore(snap), pool.restore(snap)
    same(o_ref, o_pool, "restore")
    for k in at_snap:
        assert torch.equal(at_snap[k], o_pool[k]), ("restore shows the recorded observation", k)
    scenes = pool.get_scenes()
    assert scenes.tobytes() == ref.get_scenes().tobytes()
    mask = torch.tensor([1, 0, 1, 0, 0, 1, 1, 0], dtype=torch.bool)
    (o_ref, s_ref), (o_pool, s_pool) = ref.reset_scenes(scenes, mask=mask), pool.reset_scenes(scenes, mask=mask)
    same(o_ref, o_pool, "reset_scenes")
    assert torch.equal(s_ref, s_pool) and s_pool.tolist() == [0, -1, 0, -1, -1, 0, 0, -1]
    (o_ref, *_), (o_pool, *_) = ref.step(acts[11]), pool.step(acts[11])
    same(o_ref, o_pool, "step after reset_scenes")
    assert int((pool.errors() != 0).sum()) == 0
    pool.close()
    ref.close()
