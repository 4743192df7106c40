"""The robot-scene render class resolves 4x4 blocks from row coverage masks (csrc/mg_render.h, kMask): parity with
the oracle where the mask form can go wrong.

A band-list slot covers one x-run of each row, so a block's row is four bits formed from the run's clamped ends; the
slots are walked in reverse draw order, each claiming what it covers of the still unclaimed pixels, the outline layer's
entity bits in between at their ordinals, and the block's colour sum is count x colour per claimant.

Rollouts (GPU).  MoveToRegion-TestAll and MoveToCorner-TestAll LoRes4E, 32 envs, 12 steps, actions from the library's
Philox stream (mg_random_actions, key 42): after every step every observation key -- the allo frame, the ego frame and
the frame stack -- equals the oracle's byte for byte; mg_render_full's 384 x 384 frames equal the oracle's after steps 0
and 11; errors() is 0.

Placed poses (GPU), 16 envs per task, bodies set on both sides to the same doubles (as tests/test_render_poses.py):
  * an x-extreme of the moved body's pixels in the allo frame exactly on a 4-pixel block boundary and one pixel to
    either side of it, for the left and for the right extreme (the robot at heading 0 in MoveToRegion; the block at
    angle 0 in MoveToCorner: a square's vertical edges where the seed gives one);
  * the block cut by the ego frame's first and last column, and the robot against every wall, where the arena's spans
    are clipped to l = 0 or end at 383 (the ego camera follows the robot, which is therefore never itself cut);
  * outline against fill: the robot across each edge of the goal's dashed outline (MoveToRegion); a star and a circle
    block under the robot and against a wall's outline (MoveToCorner).  The robot scenes hold a goal or a block, never
    both (magical_amd/scene.py _order), so no robot scene puts a block on a goal's outline;
  * a fresh episode: the observation of reset() itself, whose allo frame also resolves the static layer (the second
    resolve pass), and the step after it, which copies that layer.
Compared byte for byte: reset()'s observation with the oracle's, mg_render_full at the placed poses with the oracle's
frames, every key of the observation one step later with the oracle's, and that observation's current frames with
the oracle's INTER_AREA restatement of mg_render_full after the step.

Code object (CPU, from the built library's kernel notes): the class's kernels take at most 72 registers and 17 408 B
of LDS, no spilled VGPR, and no more scratch than before the mask form (48 / 32 / 64 / 48 B for modes 0 / 1 / 2 / 3,
with 9 / 0 / 20 / 6 spilled VGPRs, nearly all around the setup's per-geom matrix products; the class now forms those one
thread per matrix row).  Measured with the mask form: 72 / 65 / 72 / 59 registers, 17 360 B, 32 B of scratch and no
spilled VGPR in every mode.
"""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import pyoracle as po
from magical_amd import registry, tables
from test_gpu_parity import oracle_env, oracle_obs_split
from test_render_poses import _CORNER_SEEDS, _body0, _edge_point, _move_robot
from test_step_streamed_rows import LIB, _readelf, kernel_notes

REGION, CORNER = "MoveToRegion-TestAll-LoRes4E-v0", "MoveToCorner-TestAll-LoRes4E-v0"
ROLL_N, ROLL_STEPS, FULL_AT = 32, 12, (0, 11)
PLACED_N = 16
PX = 2.0 / 376      # less than one allo pixel per step of the sweeps below (188 px per unit): every residue occurs


def _seeds(name, n):
    return list(range(2000, 2000 + n)) if name == REGION else _CORNER_SEEDS[:n]


# ---------------------------------------------------------------------------
# placed poses
def _columns(o, move, far, near):
    """(leftmost, rightmost) allo column whose pixels change when `move` takes a body from `far` (left half of the
    arena) to `near` (right half): the body's x-extremes at `near`"""
    move(far)
    a = o.render_full()[0]
    move(near)
    b = o.render_full()[0]
    cols = np.flatnonzero((a != b).any(-1).any(0))
    cols = cols[cols >= 200]
    return int(cols[0]), int(cols[-1])


def _sweep(o, move, y, ang):
    """x positions at which the moved body's leftmost allo column is 0, 3 and 1 mod 4 (on a block boundary, one pixel
    left and right of it) and its rightmost 3, 2 and 0 mod 4, found on the oracle in half-pixel steps"""
    want = [("l", 0), ("l", 3), ("l", 1), ("r", 3), ("r", 2), ("r", 0)]
    found = {}
    for k in range(24):
        x = 0.3 + k * PX
        lo, hi = _columns(o, move, (-0.7, y, ang), (x, y, ang))
        found.setdefault(("l", lo % 4), (x, lo, hi))
        found.setdefault(("r", hi % 4), (x, lo, hi))
    assert all(w in found for w in want), sorted(found)
    return [(w, found[w]) for w in want]


@functools.lru_cache(maxsize=None)
def placed_plan(name):
    """16 placed oracle envs of `name`: per env .seed, .reset_obs (flat), .ops ((body, x, y, angle) of every body), .full
    (the oracle's frames at the placed pose), .action, .step_obs (flat, one step later), .what"""
    spec = registry.lookup(name)
    seeds = _seeds(name, 96)
    recs = []

    def new_env(seed):
        o = oracle_env(spec, seed)
        rec = SimpleNamespace(orc=o, seed=seed, reset_obs=o.reset().copy())
        kinds, types, cols, eposes = o.entities()
        b0 = _body0(kinds)
        rec.r0 = b0[[k for k, kind in enumerate(kinds) if kind == 2][0]]
        blocks = [k for k, kind in enumerate(kinds) if kind == 3]
        goals = [k for k, kind in enumerate(kinds) if kind == 1]
        rec.bb = b0[blocks[0]] if blocks else None
        rec.btype = int(types[blocks[0]]) if blocks else None
        rec.goal = tuple(float(v) for v in eposes[goals[0]]) if goals else None
        return rec

    def seal(rec, what, k):
        o = rec.orc
        final = o.bodies()
        rec.ops = [(b, float(final[b, 0]), float(final[b, 1]), float(final[b, 2])) for b in range(len(final))]
        for op in rec.ops:
            o.set_body_pose(*op)
        rec.full = [f.copy() for f in o.render_full()]
        rec.action = (5 * k + 3) % 18
        rec.step_obs = o.step(rec.action)[0].copy()
        rec.what = what
        recs.append(rec)

    clamp = lambda v: min(max(v, -0.8), 0.8)
    walls = [(0.8, 0.0, 0.3), (0.0, 0.8, 1.9), (-0.8, 0.0, 3.5), (0.0, -0.8, 5.1), (0.8, 0.8, 0.0), (-0.8, -0.8, 2.2)]
    if name == REGION:
        it = iter(seeds)
        probe = new_env(next(it))
        sweep = _sweep(probe.orc, lambda p: _move_robot(probe.orc, probe.r0, p), 0.3, 0.0)
        for (side, res), (x, lo, hi) in sweep:
            rec = new_env(next(it))
            _move_robot(rec.orc, rec.r0, (x, 0.3, 0.0))
            got = _columns(rec.orc, lambda p: _move_robot(rec.orc, rec.r0, p), (-0.7, 0.3, 0.0), (x, 0.3, 0.0))
            assert got == (lo, hi)      # the robot's pixels do not depend on the seed
            seal(rec, f"robot {side} {res}", len(recs))
        for j in range(4):
            rec = new_env(next(it))
            gx, gy, gh, gw = rec.goal
            x, y = [(gx + gw / 2, gy), (gx - gw / 2, gy), (gx, gy + gh / 2), (gx, gy - gh / 2)][j]
            _move_robot(rec.orc, rec.r0, (clamp(x), clamp(y), 0.7 + 1.1 * j))
            seal(rec, f"robot on goal edge {j}", len(recs))
        for pose in walls:
            rec = new_env(next(it))
            _move_robot(rec.orc, rec.r0, pose)
            seal(rec, f"robot at wall {pose}", len(recs))
    else:
        envs = [new_env(s) for s in seeds[:40]]
        by_type = lambda t: [r for r in envs if r.btype == t]
        squares, stars, circles = by_type(tables.SQUARE), by_type(tables.STAR), by_type(tables.CIRCLE)
        assert len(squares) >= 6 and len(stars) >= 2 and len(circles) >= 2, (len(squares), len(stars), len(circles))
        probe = squares[0]
        _move_robot(probe.orc, probe.r0, (-0.6, -0.6, 0.0))
        sweep = _sweep(probe.orc, lambda p: probe.orc.set_body_pose(probe.bb, *p), 0.3, 0.0)
        for rec, ((side, res), (x, lo, hi)) in zip(squares[:6], sweep):
            _move_robot(rec.orc, rec.r0, (-0.6, -0.6, 0.0))
            rec.orc.set_body_pose(rec.bb, x, 0.3, 0.0)
            seal(rec, f"square {side} {res}", len(recs))
        rest = [r for r in envs if r not in squares[:6] and r not in stars[:2] and r not in circles[:2]]
        for edge, rec in zip(("x0", "x383"), rest):
            pose = (0.1, -0.2, 0.9)
            _move_robot(rec.orc, rec.r0, pose)
            pt = _edge_point(pose, edge, [(pose[0], pose[1])])
            assert pt is not None
            col = {"x0": 0, "x383": 383}[edge]
            rec.orc.set_body_pose(rec.bb, -pt[0], -pt[1], 0.45)
            away = rec.orc.render_full()[1][:, col].copy()
            rec.orc.set_body_pose(rec.bb, pt[0], pt[1], 0.45)
            assert not np.array_equal(rec.orc.render_full()[1][:, col], away), f"the block does not reach ego column {col}"
            seal(rec, f"block cut at ego {edge}", len(recs))
        for rec in (stars[0], circles[0]):      # under the robot: its fills and outline over the block's
            _move_robot(rec.orc, rec.r0, (0.2, 0.1, 1.3))
            rec.orc.set_body_pose(rec.bb, 0.25, 0.12, 0.6)
            seal(rec, f"block type {rec.btype} under the robot", len(recs))
        for rec in (stars[1], circles[1]):      # against the right wall: the block over the arena's outline
            _move_robot(rec.orc, rec.r0, (0.5, 0.3, 2.0))
            rec.orc.set_body_pose(rec.bb, 0.85, 0.3, 0.8)
            seal(rec, f"block type {rec.btype} at the wall", len(recs))
        for pose, rec in zip(walls[:4], rest[2:]):
            _move_robot(rec.orc, rec.r0, pose)
            seal(rec, f"robot at wall {pose}", len(recs))
    assert len(recs) == PLACED_N, len(recs)
    return recs


@pytest.mark.parametrize("name", [REGION, CORNER])
def test_placed_plan_has_the_boundary_cases(name):
    recs = placed_plan(name)
    whats = [r.what for r in recs]
    for side, residues in (("l", (0, 3, 1)), ("r", (3, 2, 0))):
        for res in residues:
            assert any(w.endswith(f" {side} {res}") for w in whats), (side, res, whats)
    assert sum("wall" in w for w in whats) >= 4
    for r in recs:      # the placed frames differ from the reset frames: the placement took effect
        assert not np.array_equal(r.full[0], r.full[1])
        assert all(abs(x) <= 0.86 and abs(y) <= 0.86 for _, x, y, _ in r.ops[:1])


def _assert_obs(tag, spec, got, flat, i):
    want = oracle_obs_split(spec, flat)
    assert set(got) == set(want)
    for k in got:
        if not np.array_equal(got[k][i], want[k]):
            d = np.argwhere(got[k][i] != want[k])[0]
            pytest.fail(f"{tag} env {i} obs {k}: first difference at {tuple(int(v) for v in d)}: "
                        f"{got[k][i][tuple(d)]} vs oracle {want[k][tuple(d)]}; {int((got[k][i] != want[k]).sum())} bytes differ")


def _assert_full(tag, full, ref, i):
    for v, view in enumerate(("allo", "ego")):
        if not np.array_equal(full[i, v], ref[v]):
            y, x = np.argwhere((full[i, v] != ref[v]).any(-1))[0]
            pytest.fail(f"{tag} env {i} {view} frame: first differing pixel x={x} y={y}: {full[i, v, y, x]} vs oracle "
                        f"{ref[v][y, x]}; {int((full[i, v] != ref[v]).any(-1).sum())} pixels differ")


@pytest.mark.gpu
@pytest.mark.parametrize("name", [REGION, CORNER])
def test_placed_poses_match_the_oracle(name):
    import torch
    import magical_amd
    recs = placed_plan(name)
    spec = registry.lookup(name)
    n = len(recs)
    vec = magical_amd.make_vec(name, n, seeds=[r.seed for r in recs])
    obs = {k: v.cpu().numpy() for k, v in vec.reset().items()}
    for i, r in enumerate(recs):        # a fresh episode: the static layer's second resolve pass
        _assert_obs("reset", spec, obs, r.reset_obs, i)
    for i, r in enumerate(recs):
        for b, x, y, a in r.ops:
            vec.set_body_pose(i, b, x, y, a)
    full = vec.render_full().cpu().numpy()
    for i, r in enumerate(recs):
        _assert_full(f"placed ({r.what})", full, r.full, i)
    obs, _, done, _ = vec.step(torch.as_tensor([r.action for r in recs], dtype=torch.uint8))
    obs = {k: v.cpu().numpy() for k, v in obs.items()}
    assert not done.cpu().numpy().any()
    full = vec.render_full().cpu().numpy()
    errs = vec.errors().cpu().numpy()
    vec.close()
    for i, r in enumerate(recs):
        _assert_obs(f"step after placement ({r.what})", spec, obs, r.step_obs, i)
        for k, view in (("allo", 0), ("ego", 1)):
            want = po.downsample(full[i, view])
            assert np.array_equal(obs[k][i][:, :, -3:], want), f"env {i} ({r.what}) obs {k} vs its own full frame"
    assert not errs.any(), {i: int(e) for i, e in enumerate(errs) if e}


# ---------------------------------------------------------------------------
# rollouts
@pytest.mark.gpu
@pytest.mark.parametrize("name", [REGION, CORNER])
def test_rollout_frames_match_the_oracle(name):
    import magical_amd
    spec = registry.lookup(name)
    seeds = _seeds(name, ROLL_N)
    vec = magical_amd.make_vec(name, ROLL_N, seeds=seeds)
    orc = [oracle_env(spec, s) for s in seeds]
    obs = {k: v.cpu().numpy() for k, v in vec.reset().items()}
    assert {"allo", "ego", "past_obs"} <= set(obs)
    for i, o in enumerate(orc):
        _assert_obs("reset", spec, obs, o.reset(), i)
    for t in range(ROLL_STEPS):
        acts = vec.random_actions(t)
        obs = {k: v.cpu().numpy() for k, v in vec.step(acts)[0].items()}
        acts = acts.cpu().numpy()
        assert acts.max() < 18
        for i, o in enumerate(orc):
            flat, _, d, _ = o.step(int(acts[i]))
            if d:
                flat = o.reset()
            _assert_obs(f"step {t}", spec, obs, flat, i)
        if t in FULL_AT:
            full = vec.render_full().cpu().numpy()
            for i, o in enumerate(orc):
                _assert_full(f"step {t}", full, o.render_full(), i)
    assert int(vec.errors().abs().sum().item()) == 0
    vec.close()


# ---------------------------------------------------------------------------
# code object
SMALL = "_Z13render_kernelI10RenderSmemILi28E"
SCRATCH_BEFORE = {0: 48, 1: 32, 2: 64, 3: 48}      # bytes per lane, kernel modes 0-3, before the mask form


def test_small_class_kernels_keep_their_budget():
    readelf = _readelf()
    if not os.path.exists(LIB) or readelf is None:
        pytest.skip("the library (or llvm-readelf) is absent")
    notes = kernel_notes(LIB, readelf)
    small = {name: v for name, v in notes.items() if name.startswith(SMALL)}
    assert len(small) == 4, sorted(small)
    bad = []
    for name, k in sorted(small.items()):
        mode = int(name.split("EELi")[1][0])
        print(f"small class mode {mode}: {k['vgpr_count']} registers, LDS {k['group_segment_fixed_size']} B, "
              f"scratch {k['private_segment_fixed_size']} B, spilled VGPRs {k['vgpr_spill_count']}")
        if k["vgpr_count"] > 72:
            bad.append(f"mode {mode}: {k['vgpr_count']} registers")
        if k["group_segment_fixed_size"] > 17408:
            bad.append(f"mode {mode}: LDS {k['group_segment_fixed_size']} B")
        if k["vgpr_spill_count"] != 0:
            bad.append(f"mode {mode}: {k['vgpr_spill_count']} spilled VGPRs")
        if k["private_segment_fixed_size"] > SCRATCH_BEFORE[mode]:
            bad.append(f"mode {mode}: scratch {k['private_segment_fixed_size']} B > {SCRATCH_BEFORE[mode]} B")
    assert not bad, bad
