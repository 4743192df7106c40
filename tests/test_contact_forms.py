"""Placed-contact twin of every compiled step form, with ragged last workgroups.

test_oracle_narrowphase.py::test_gpu_narrowphase_twin compares the arbiter tables of contact-rich scenes with the
oracle in each scene's default step form at env counts that fill every workgroup; test_gpu_parity.py's form table
walks 45 random steps from reset, which on the robot scenes meet no contact.  Here every (form, envs per workgroup)
pair of csrc/mg_stepforms.h (MG_STEP_FORMS) runs placed contacts at env counts that leave the last workgroup ragged,
and the last real env -- the one the quad forms' shadow lanes reload -- carries live arbiters after the first step and
on at least three steps, as does env 0.

Pairs and env counts (B envs per workgroup; n = B + 1 and 2 B - 1; B = 1 and the cooperative form: n = 3; B = 64:
n = 65).  A "shadow" is a slot of the last workgroup that has no env of its own: in the quad forms (5, 6) its lanes run
the whole step on a private LDS copy of env n - 1 and never write HBM; in form 0 its lane leaves the kernel at once.

    scene          pair     n    last workgroup: slots with a real env / slots without
    MoveToRegion   (5, 8)    9   slot 0 = env 8        / slots 1-7 shadows of env 8
                             15  slots 0-6 = env 8-14  / slot 7 a shadow of env 14
                   (5, 16)   17  slot 0 = env 16       / slots 1-15 shadows of env 16
                             31  slots 0-14 = env 16-30 / slot 15 a shadow of env 30
                   (0, 8)    9, 15   as (5, 8), the spare lanes idle
                   (0, 64)   65  slot 0 = env 64       / 63 idle lanes
                   (0, 1)    3   one env per workgroup, none ragged
    MoveToCorner   (6, 8)    9, 15   as (5, 8)
                   (6, 16)   17, 31  as (5, 16)
                   (0, 8)    9, 15;  (0, 64)  65;  (0, 1)  3
    ClusterColour-Demo, MatchRegions-TestAll
                   (4, 1)    3   one env per 64-lane workgroup, none ragged
                   (0, 8)    9, 15;  (0, 64)  65;  (0, 1)  3

Inputs.  Env i of a scene is the same env at every n (the cases of a scene share one oracle run of 65 envs):
seeded ENV_SEED0 + i = 9100 + i, and one numpy RandomState(s_i), s_i = LAYOUT[scene].get(i, i), draws first its
contacts and then its 6 actions, randint(0, 18, 6); MoveToRegion then takes action 1 (forward, fingers open) twice,
which drives the robot along or into the wall it was placed at.
  * Block scenes: reset, then test_oracle_narrowphase._twin_layout(..., robot_first = i even) sets the block poses.
  * MoveToRegion: reset, test_render_poses.PRE_ACTIONS (ten steps, which close the fingers; where (i // 3) is even the
    robot's bodies are then put back to their reset poses, fingers open, keeping their velocities), then the robot is
    moved rigidly (_move_robot) against wall w = i % 4 (0: y = -1, 1: x = +1, 2: y = +1, 3: x = -1) in the manner
    i % 3, so that neighbouring lanes of a workgroup take different branches of the narrowphase.  In draw order:
      0 "wall":   depth; u = uniform(-0.5, 0.5) along the wall; the heading's sense along the wall, randint(2); its
                  tilt uniform(-0.08, 0.08).  The body centre lies 0.8 + depth from the arena centre along the wall's
                  normal (ROBOT_RAD 0.2, wall surfaces at +-1), the fingers point along the wall;
      1 "corner": depth against wall w, a second depth against wall w + 1 (two arbiters), tilt uniform(-0.08, 0.08)
                  of a heading along wall w, away from wall w + 1;
      2 "finger": depth; u; heading towards the wall + uniform(-0.3, 0.3); the finger polygons' farthest vertex lies
                  `depth` inside the wall and the body stays about 0.1 clear of it.
    depth = uniform(-0.005, 0.04), as _twin_layout draws it.
LAYOUT lists the envs whose s_i is not i: the first of i + 100, i + 200, ... with which the oracle alone gives the env
a live arbiter after step 1 that is of its manner (MoveToRegion: two arbiters in a corner, the body touching in the
wall and corner manners, only fingers touching in the finger manner; env 2 also meets a two-contact arbiter) and, for
the first and last env of a case or of a chunk of the pool test (0, 2, 3, 7, 8, 12, 14, 16, 30, 64), live arbiters on
three steps.  The CPU tests below assert on the oracle alone that every case covers what the GPU test requires.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest

from magical_amd import registry, tables
from test_gpu_parity import oracle_env, oracle_obs_split
from test_oracle_narrowphase import (_twin_layout, assert_twin_step, count_arbiter, epa_runs, gpu_tables, new_seen,
                                     oracle_tables)
from test_render_poses import PRE_ACTIONS, _body0, _move_robot, _place_on_gpu

REGION, CORNER = "MoveToRegion-Demo-LoRes4E-v0", "MoveToCorner-Demo-LoRes4E-v0"
CLUSTER, MATCH = "ClusterColour-Demo-LoResStack-v0", "MatchRegions-TestAll-LoRes4E-v0"
NMAX = 65
ENV_SEED0 = 9100
STEPS = 6
# env -> RandomState seed of its contacts where it is not the env's index (see the module docstring)
LAYOUT = {
    REGION: {0: 200, 2: 302, 7: 107, 8: 108, 9: 109, 10: 110, 12: 112, 14: 1014, 16: 116, 19: 119, 21: 121, 34: 134,
             38: 138, 40: 340, 43: 143, 48: 148, 50: 150, 52: 152, 54: 154, 57: 157, 62: 562, 64: 264},
    CORNER: {9: 109, 16: 116, 30: 130, 34: 134, 38: 138, 46: 146, 62: 162},
    CLUSTER: {},
    MATCH: {},
}

_V, _B, _B0 = "MG_STEP_VARIANT", "MG_STEP_BLK", "MG_STEP_BLK0"
_HBM = [((0, 8), {_V: "0", _B0: "8"}), ((0, 64), {_V: "0", _B0: "64"}), ((0, 1), {_V: "0", _B0: "1"})]
# every pair of MG_STEP_FORMS on every scene kind it runs, and the switches that force it
PAIRS = {
    REGION: [((5, 8), {_V: "5", _B: "8"}), ((5, 16), {_V: "5", _B: "16"})] + _HBM,
    CORNER: [((6, 8), {_V: "6", _B: "8"}), ((6, 16), {_V: "6", _B: "16"})] + _HBM,
    CLUSTER: [((4, 1), {_V: "4", _B: "1"})] + _HBM,
    MATCH: [((4, 1), {_V: "4", _B: "1"})] + _HBM,
}


def env_counts(pair):
    blk = pair[1]
    return (3,) if blk == 1 else (65,) if blk == 64 else (blk + 1, 2 * blk - 1)


CASES = [(name, pair, env, n) for name, pairs in PAIRS.items() for pair, env in pairs for n in env_counts(pair)]
IDS = [f"{name.split('-')[0]}-{pair[0]}/{pair[1]}-n{n}" for name, pair, env, n in CASES]


def actions(ref):
    """[steps, n] actions of the envs `ref`"""
    return np.stack([rec.acts for rec in ref], axis=1)


# ---------------------------------------------------------------------------
# MoveToRegion: the robot against the walls
WALL_N = [(0.0, -1.0), (1.0, 0.0), (0.0, 1.0), (-1.0, 0.0)]     # outward normals of walls 0..3
MANNERS = ("wall", "corner", "finger")


def _heading(fx, fy):
    """the body angle whose forward direction (the fingers' side: local +y) is (fx, fy)"""
    return math.atan2(-fx, fy)


def _finger_reach(o, r0, nx, ny):
    """how far the finger polygons' farthest vertex lies from the robot's centre along (nx, ny)"""
    b = o.bodies()
    outer = tables.robot_tables()[0]
    reach = -math.inf
    for k in range(2):
        fx, fy, fa = b[r0 + 4 + k, :3]
        c, s = math.cos(fa), math.sin(fa)
        for poly in outer[k]:
            for vx, vy in poly:
                wx, wy = fx + c * vx - s * vy, fy + s * vx + c * vy
                reach = max(reach, (wx - b[r0, 0]) * nx + (wy - b[r0, 1]) * ny)
    return reach


def region_pose(o, r0, i, rs):
    """move env i's robot into its contact (module docstring); returns the manner"""
    manner = MANNERS[i % 3]
    nx, ny = WALL_N[i % 4]
    tx, ty = -ny, nx
    depth = rs.uniform(-0.005, 0.04)
    if manner == "wall":
        u = rs.uniform(-0.5, 0.5)
        e = 0.8 + depth
        sgn = 1.0 if rs.randint(2) else -1.0
        _move_robot(o, r0, (e * nx + u * tx, e * ny + u * ty, _heading(sgn * tx, sgn * ty) + rs.uniform(-0.08, 0.08)))
    elif manner == "corner":
        mx, my = WALL_N[(i + 1) % 4]
        e, f = 0.8 + depth, 0.8 + rs.uniform(-0.005, 0.04)
        _move_robot(o, r0, (e * nx + f * mx, e * ny + f * my, _heading(-mx, -my) + rs.uniform(-0.08, 0.08)))
    else:
        u = rs.uniform(-0.5, 0.5)
        a = _heading(nx, ny) + rs.uniform(-0.3, 0.3)
        _move_robot(o, r0, (u * tx, u * ty, a))
        e = 1.0 + depth - _finger_reach(o, r0, nx, ny)
        _move_robot(o, r0, (e * nx + u * tx, e * ny + u * ty, a))
    return manner


# ---------------------------------------------------------------------------
# the oracle's side, once per scene
def place(name, i, layout_seed=None):
    """Env i of `name` placed on the oracle.  Returns a record: .orc, .seed, .ops ((body, x, y, angle): what both
    sides are set to), .rob (the robot's bodies), .manner (MoveToRegion)."""
    spec = registry.lookup(name)
    seed = ENV_SEED0 + i
    o = oracle_env(spec, seed)
    o.reset()
    kinds, types, cols, poses = o.entities()
    b0 = _body0(kinds)
    r0 = b0[[k for k, kind in enumerate(kinds) if kind == 2][0]]
    rs = np.random.RandomState(LAYOUT[name].get(i, i) if layout_seed is None else layout_seed)
    rec = SimpleNamespace(orc=o, seed=seed, rob=set(range(r0, r0 + 6)), manner=None)
    if name == REGION:
        rest = o.bodies()
        for a in PRE_ACTIONS:
            o.step(a)
        if (i // 3) % 2 == 0:       # the fingers back at their open reset angles (their velocities stay)
            for b in sorted(rec.rob):
                o.set_body_pose(b, *rest[b, :3])
        rec.manner = region_pose(o, r0, i, rs)
        final = o.bodies()
        rec.ops = [(b, float(final[b, 0]), float(final[b, 1]), float(final[b, 2])) for b in range(len(final))]
    else:
        lay = _twin_layout(kinds, types, poses, rs, robot_first=i % 2 == 0)
        rec.ops = [(b0[b], float(x), float(y), float(a)) for b, (x, y, a) in lay.items()]
    for op in rec.ops:
        o.set_body_pose(*op)
    rec.acts = np.concatenate([rs.randint(0, 18, STEPS), [1, 1] if name == REGION else []]).astype(np.uint8)
    return rec


def roll(name, rec, i):
    """step the placed oracle env through its actions: .steps (oracle_tables per step), .obs (the last
    observation), .epa (EPA runs)"""
    spec = registry.lookup(name)
    e0 = epa_runs()
    rec.steps = []
    for a in rec.acts:
        obs, _, done, _ = rec.orc.step(int(a))
        assert not done
        rec.steps.append(oracle_tables(rec.orc))
    rec.epa = epa_runs() - e0
    rec.obs = oracle_obs_split(spec, obs)
    return rec


@functools.lru_cache(maxsize=None)
def reference(name):
    """the NMAX placed and stepped oracle envs of a scene (shared by its cases; read only)"""
    return [roll(name, place(name, i), i) for i in range(NMAX)]


def live_steps(rec):
    return [len(ra) > 0 for _, ra, _ in rec.steps]


def coverage(name, n):
    ref = reference(name)[:n]
    seen = new_seen()
    for rec in ref:
        for _, ra, _ in rec.steps:
            for w in ra:
                count_arbiter(w, rec.rob, seen)
    return seen, sum(rec.epa for rec in ref)


def required(name):
    need = ["arbiters", "two", "one", "wall", "robot"]
    return need + (["block_block"] if name in (CLUSTER, MATCH) else [])


def assert_covers(name, n, seen, epa, live_first, live_last):
    """what a case must have compared (issue items 3 and 5)"""
    assert min(seen[k] for k in required(name)) > 0 and seen["arbiters"] >= 2 * n, seen
    if name != REGION:
        assert epa > 0, "no configuration took the EPA path"
    for who, live in (("env 0", live_first), (f"env {n - 1}", live_last)):
        assert live[0] and sum(live) >= 3, f"{who}: live arbiters on steps {live}"


# ---------------------------------------------------------------------------
# CPU tests: the oracle alone meets what the GPU test requires
def test_pairs_are_the_compiled_forms():
    """PAIRS holds every X(form, blk) row of csrc/mg_stepforms.h: the quad forms on their own scene, the cooperative
    form on the many-block scenes, the HBM form everywhere"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "magical-1_amd", "csrc",
                            "mg_stepforms.h")).read()
    rows = {}
    for fam in ("COOP", "QUAD", "HBM"):
        body = re.search(r"#define MG_STEP_FORMS_%s\(X\)(.*)" % fam, src).group(1)
        rows[fam] = {(int(f), int(b)) for f, b in re.findall(r"X\((\d+), (\d+)\)", body)}
    assert all(rows.values())
    own = {REGION: {p for p in rows["QUAD"] if p[0] == 5}, CORNER: {p for p in rows["QUAD"] if p[0] == 6},
           CLUSTER: rows["COOP"], MATCH: rows["COOP"]}
    assert own[REGION] | own[CORNER] == rows["QUAD"]
    for name, pairs in PAIRS.items():
        assert {p for p, _ in pairs} == own[name] | rows["HBM"], name


@pytest.mark.parametrize("name", list(PAIRS))
def test_oracle_alone_covers_every_case(name):
    ref = reference(name)
    for i, rec in enumerate(ref):
        assert live_steps(rec)[0], f"env {i}: no arbiter after step 1"
    for n in sorted({n for nm, _, _, n in CASES if nm == name}):
        seen, epa = coverage(name, n)
        assert_covers(name, n, seen, epa, live_steps(ref[0]), live_steps(ref[n - 1]))
    if name == REGION:
        assert {rec.manner for rec in ref[:3]} == set(MANNERS)
        for i, rec in enumerate(ref):
            first = rec.steps[0][1]
            main, fingers = min(rec.rob), {max(rec.rob) - 1, max(rec.rob)}
            assert all(w[3] < 0 or w[4] < 0 for w in first), f"env {i}: a contact that is not with a wall"
            touching = {int(w[3]) for w in first} | {int(w[4]) for w in first}
            if rec.manner == "corner":
                assert len(first) >= 2, f"env {i}: a corner pose with {len(first)} arbiters"
            if rec.manner == "finger":
                assert touching & fingers and main not in touching, f"env {i}: bodies {touching} touch the wall"
            else:
                assert main in touching, f"env {i}: the body does not touch the wall"
        # warm-started impulses cross env-steps: arbiters in their normal state, and some on the two forward steps
        assert sum(int(w[1]) == 1 for rec in ref for _, ra, _ in rec.steps for w in ra) >= NMAX
        assert sum(sum(live_steps(rec)[STEPS:]) for rec in ref) >= NMAX // 4
    if name == CORNER:      # the pool test's chunks end at envs 3, 7 and 12
        for i in (0, 3, 7, 12):
            assert sum(live_steps(ref[i])) >= 3, f"env {i}"


# ---------------------------------------------------------------------------
# GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("name,pair,env,n", CASES, ids=IDS)
def test_placed_contacts_in_every_form(name, pair, env, n, monkeypatch):
    """After every step the GPU's bodies and arbiter tables equal the oracle's (assert_twin_step) in the forced form
    at a ragged env count; envs 0 and n - 1 carry live arbiters; the last observation is the oracle's bit for bit."""
    import torch
    import magical_amd
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ref = reference(name)[:n]
    acts = actions(ref)
    vec = magical_amd.make_vec(name, n, seeds=[rec.seed for rec in ref])
    assert vec.step_form()[:2] == pair
    if name == REGION:
        _place_on_gpu(vec, ref, torch)
    else:
        vec.reset()
        for i, rec in enumerate(ref):
            for op in rec.ops:
                vec.set_body_pose(i, *op)
    seen = new_seen()
    live = np.zeros((len(acts), n), dtype=bool)
    for t in range(len(acts)):
        obs, _, done, _ = vec.step(torch.as_tensor(acts[t], dtype=torch.uint8))
        got = gpu_tables(vec)
        assert_twin_step(t, got, [rec.steps[t] for rec in ref], [rec.rob for rec in ref], seen)
        live[t] = got[1][:, 3] > 0
    assert not done.cpu().numpy().any()
    got_obs = {k: v.cpu().numpy() for k, v in obs.items()}
    for i, rec in enumerate(ref):
        assert set(got_obs) == set(rec.obs)
        for k in got_obs:
            assert np.array_equal(got_obs[k][i], rec.obs[k]), f"last step env {i} obs {k}"
    print(name, pair, n, seen, "EPA runs", sum(rec.epa for rec in ref))
    assert_covers(name, n, seen, sum(rec.epa for rec in ref), list(live[:, 0]), list(live[:, n - 1]))
    assert int(vec.errors().abs().sum().item()) == 0
    vec.close()


@pytest.mark.gpu
def test_pipelined_pool_with_placed_contacts():
    """PipelinedVecEnv over three chunks that are each smaller than a workgroup (bounds 0, 4, 8, 13), the contacts of
    test_placed_contacts_in_every_form placed through the pool: bodies and observations after each of 6 steps equal
    those of the plain VecMagicalEnv with the same seeds and placements bit for bit (which the test above ties to the
    oracle)."""
    import torch
    from magical_amd import envs as mg_envs
    from magical_amd.pipeline import PipelinedVecEnv
    n = 13
    ref = reference(CORNER)[:n]
    seeds = [rec.seed for rec in ref]
    pool = PipelinedVecEnv(CORNER, n, chunks=3, seeds=seeds)
    assert pool.bounds == [0, 4, 8, 13]
    plain = mg_envs.VecMagicalEnv(CORNER, n, seeds=seeds)
    for v in (pool, plain):
        v.reset()
        for i, rec in enumerate(ref):
            for op in rec.ops:
                v.set_body_pose(i, *op)
    acts = torch.as_tensor(actions(ref)).cuda()
    live = np.zeros((STEPS, n), dtype=bool)
    for t in range(STEPS):
        got, _, _, _ = pool.step(acts[t])
        want, _, _, _ = plain.step(acts[t])
        pool.wait()
        assert list(got) == list(want)
        for k in want:
            assert torch.equal(got[k], want[k]), f"step {t} obs {k}"
        bodies, counts = plain.bodies()
        parts = [sim.bodies() for sim in pool.sims]
        assert torch.equal(torch.cat([p[0] for p in parts]), bodies), f"step {t} bodies"
        assert torch.equal(torch.cat([p[1] for p in parts]), counts), f"step {t} counts"
        live[t] = counts[:, 3].cpu().numpy() > 0
    for k in range(3):      # every chunk's last env, and the first of all, carry contacts
        last = pool.bounds[k + 1] - 1
        assert live[0, last] and live[:, last].sum() >= 3, (last, live[:, last])
    assert live[0, 0] and live[:, 0].sum() >= 3
    assert int(pool.errors().abs().sum().item()) == 0 and int(plain.errors().abs().sum().item()) == 0
    pool.close(), plain.close()
