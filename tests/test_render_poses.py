"""Render parity at placed poses: the robot against walls and in corners, at axis-aligned and generic
headings, with blocks cut by the ego frame's edges.

The rollout tests (test_gpu_parity.py) reach only the poses a random walk from reset() visits.  Here the
robot's six bodies are moved rigidly (oenv_set_body_pose / mg_set_body_pose, the same doubles on both
sides) to the poses where the raster's special cases live -- clipline with a float32 slope, truncation of
negative pixel coordinates, horizontal / vertical line cases, arena edges far outside the ego frame, fill
spans cut at x < 0 and x > 383 -- and the frames of mg_render_full are compared with the oracle's bit for
bit (test A).  Test B ties the fused LoRes paths (kernel modes 0 and 2) to mode 1 through the oracle's
INTER_AREA restatement.  The CPU tests state what the inputs must contain to be able to find a fault;
seeds and poses were chosen so that the oracle alone satisfies them.

Every pose keeps the robot centre in [-0.8, 0.8]^2 (ROBOT_RAD 0.2, arena [-1, 1]^2) and block centres in
[-0.85, 0.85]^2.  One env per pose; env i is seeded seeds[i].
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest

import pyoracle as po
from magical_amd import registry, tables
from test_gpu_parity import oracle_env

# ---------------------------------------------------------------------------
# robot poses
_E = 0.8
CORNERS = [(-_E, -_E), (_E, -_E), (_E, _E), (-_E, _E)]
WALL_MIDS = [(_E, 0.0), (0.0, _E), (-_E, 0.0), (0.0, -_E)]
CENTRE = (0.0, 0.0)
EXACT_HEADINGS = [k * math.pi / 2 for k in range(4)]            # the exact doubles
HEADINGS8 = [(k // 2) * math.pi / 2 if k % 2 == 0 else k * math.pi / 4 for k in range(8)]
# headings of no special value: generic slopes, and slopes a little off an axis (not the 1e-9 offsets below)
GENERIC_HEADINGS = [0.1234, 0.7071, 1.0, 1.5607, 1.5718, 2.2, 2.7, 3.1406, 3.1426, 3.9, 4.5, 4.7114, 4.7134,
                    5.3, 5.9, 6.2822]


def _robot_poses():
    out = [(x, y, a) for (x, y) in CORNERS + WALL_MIDS + [CENTRE] for a in HEADINGS8]
    out += [(x, y, a + d) for (x, y) in WALL_MIDS for a in EXACT_HEADINGS for d in (-1e-9, 1e-9)]
    spots = WALL_MIDS + CORNERS
    out += [(*spots[j % 8], a) for j, a in enumerate(GENERIC_HEADINGS)]
    # interleaved, so that every run of consecutive table entries mixes positions and headings
    return [out[(j * 7) % len(out)] for j in range(len(out))]


ROBOT_POSES = _robot_poses()
assert len(ROBOT_POSES) == 120 and len(set(ROBOT_POSES)) == 120

# base (unwrapped) name -> (seeds, first table entry); the two small-class names together cover the table
# (entries 0..95 and 24..119), the many-block names entries 0..47 and 72..119.  Seeds: the first ones from the
# stated start whose oracle reset places (MoveToCorner-TestAll raises PlacementError for about a third).
_CORNER_SEEDS = [s for s in range(2000, 2140) if s not in (
    2003, 2009, 2012, 2018, 2022, 2026, 2027, 2029, 2030, 2031, 2042, 2047, 2050, 2051, 2060, 2061, 2063, 2064,
    2066, 2069, 2070, 2071, 2074, 2075, 2080, 2083, 2084, 2085, 2088, 2098, 2099, 2100, 2102, 2110, 2113, 2115,
    2117, 2119, 2120, 2124, 2132, 2134, 2136, 2138)][:96]
CASES = {
    "MoveToRegion-TestAll-v0": (list(range(2000, 2096)), 0),
    "MoveToCorner-TestAll-v0": (_CORNER_SEEDS, 24),
    "ClusterColour-Demo-v0": (list(range(2000, 2048)), 72),
    "MatchRegions-TestAll-v0": (list(range(2000, 2048)), 0),
}
BLOCK_TYPES = {tables.SQUARE, tables.PENTAGON, tables.STAR, tables.CIRCLE}

PRE_ACTIONS = [16, 11, 14, 5, 17, 10, 13, 2, 12, 15]   # 10 steps: forward / back, both turns, fingers mostly closing
BLOCK_LIM = 0.85
BLOCK_RAD = 0.16    # bounds every block shape: the star's outer radius is 1.3 * SHAPE_RAD = 0.156
EDGES = ("x0", "x383", "y0", "y383")
KINDS = EDGES + ("goal", "under", "int", "ulp")


def base_name(name):
    """the unwrapped name of the same task and variant: the placement does not depend on the preprocessor"""
    parts = name.split("-")
    return "-".join(parts[:2] + ["v0"])


def poses_of(name):
    seeds, first = CASES[base_name(name)]
    return ROBOT_POSES[first:first + len(seeds)]


def _body0(kinds):
    """first body of every entity (bodies in entity add order: blocks 1, robot 6, others 0)"""
    out, nb = {}, 0
    for k, kind in enumerate(kinds):
        out[k] = nb
        nb += 1 if kind == 3 else 6 if kind == 2 else 0
    return out


def _move_robot(o, r0, pose):
    """Move the robot's six bodies (main, control, two eyes, two fingers) rigidly so that the main body sits
    at `pose`: rotated and translated about the main body.  The eye bodies carry no position (they stay at the
    origin, entities.py:291-304; only their angle is drawn), so only their angle turns."""
    b = o.bodies()
    x0, y0, a0 = b[r0, :3]
    X, Y, A = pose
    d = A - a0
    c, s = math.cos(d), math.sin(d)
    o.set_body_pose(r0, X, Y, A)
    for j in (1, 4, 5):
        rx, ry = b[r0 + j, 0] - x0, b[r0 + j, 1] - y0
        o.set_body_pose(r0 + j, X + (c * rx - s * ry), Y + (s * rx + c * ry), b[r0 + j, 2] + d)
    for j in (2, 3):
        o.set_body_pose(r0 + j, b[r0 + j, 0], b[r0 + j, 1], b[r0 + j, 2] + d)


def ego_pixel(pose, x, y):
    m = tables.ego_view(*pose)
    p = m @ np.array([x, y, 1.0])
    return p[0], p[1]


def _edge_point(pose, edge, others):
    """World point inside the block bounds that projects onto the middle of `edge` of the ego frame (or along
    it), as far from the other bodies' centres as the edge allows; None when the edge sees no such point."""
    inv = np.linalg.inv(tables.ego_view(*pose))
    best, best_d = None, -1.0
    for t in range(12, 372, 8):
        px, py = {"x0": (0.0, t), "x383": (383.0, t), "y0": (t, 0.0), "y383": (t, 383.0)}[edge]
        w = inv @ np.array([px, py, 1.0])
        x, y = float(w[0]), float(w[1])
        if abs(x) > BLOCK_LIM or abs(y) > BLOCK_LIM:
            continue
        d = min(math.hypot(x - ox, y - oy) for ox, oy in others)
        if d > best_d:
            best, best_d = (x, y), d
    return best


def _allo_boundary(o, body, x0, y, a):
    """Adjacent doubles (xa, xb), xa < xb within one allo pixel right of x0, between which the oracle's allo
    frame changes: moving the block from xa to xb takes a vertex's pixel coordinate across an integer, which
    (int) truncation turns into the next pixel.  The coordinate moves by at most one ulp per ulp of x here
    (188 px per unit), so it is the integer exactly at xb and one ulp below it at xa."""
    def frame(x):
        o.set_body_pose(body, x, y, a)
        return o.render_full()[0]
    lo, hi = x0, x0 + 2.04 / 384
    f0 = frame(lo)
    if np.array_equal(frame(hi), f0):
        return None
    while math.nextafter(lo, math.inf) < hi:
        mid = lo + (hi - lo) / 2
        if np.array_equal(frame(mid), f0):
            lo = mid
        else:
            hi = mid
    return lo, hi


def _count(line, colour):
    return int(np.all(line == colour, axis=-1).sum())


def build_plan(name):
    """One placed oracle env per pose of `name`'s table slice.  Returns a list of records: .orc (the oracle
    after placement), .ops ((body, x, y, angle) for every body: what both sides are set to), .pose, .stepped,
    .kind / .edge / .block (the placed block, if any) and the facts the CPU tests assert."""
    name = base_name(name)
    spec = registry.lookup(name)
    seeds, _ = CASES[name]
    pal = po.palette()
    plan = []
    for i, (seed, pose) in enumerate(zip(seeds, poses_of(name))):
        o = oracle_env(spec, seed)
        o.reset()                       # PlacementError here: a seed that must not be in CASES
        rec = SimpleNamespace(orc=o, seed=seed, pose=pose, stepped=i % 2 == 1, kind=None, edge=None, block=None)
        reset_ego = o.render_full()[1]
        kinds, types, cols, eposes = o.entities()
        rec.types = [int(t) for k, t in zip(kinds, types) if k == 3]
        b0 = _body0(kinds)
        r0 = b0[[k for k, kind in enumerate(kinds) if kind == 2][0]]
        rest = o.bodies()
        if rec.stepped:
            for a in PRE_ACTIONS:
                o.step(a)
        moved = o.bodies()
        rec.finger_moved = bool(np.abs((moved[r0 + 4:r0 + 6, 2] - moved[r0, 2])
                                       - (rest[r0 + 4:r0 + 6, 2] - rest[r0, 2])).max() > 1e-3)
        _move_robot(o, r0, pose)
        blocks = [k for k, kind in enumerate(kinds) if kind == 3]
        goals = [k for k, kind in enumerate(kinds) if kind == 1]
        if blocks:
            kind = KINDS[(i // 2) % 8]
            if kind == "goal" and not goals:
                kind = EDGES[(i // 16) % 4]
            ent = blocks[(i // 16) % len(blocks)]
            bb = b0[ent]
            cur = o.bodies()
            others = [(cur[r0, 0], cur[r0, 1])] + [(cur[b0[k], 0], cur[b0[k], 1]) for k in blocks if k != ent]
            ang = 0.3 + 0.37 * i
            before = o.render_full()[1]
            if kind in EDGES:
                for edge in EDGES[EDGES.index(kind):] + EDGES[:EDGES.index(kind)]:
                    pt = _edge_point(pose, edge, others)
                    if pt is not None:
                        o.set_body_pose(bb, pt[0], pt[1], ang)
                        rec.edge = edge
                        break
                if rec.edge is None:    # a wall fills the view: no edge of the frame sees the block bounds
                    kind = "under"
                    o.set_body_pose(bb, pose[0], pose[1], ang)
                else:
                    after = o.render_full()[1]
                    line = {"x0": np.s_[:, 0], "x383": np.s_[:, 383], "y0": np.s_[0], "y383": np.s_[383]}[rec.edge]
                    base = pal[cols[ent]][0]
                    rec.edge_pixels = (_count(before[line], base), _count(after[line], base))
            elif kind == "goal":
                gx, gy, gh, gw = eposes[goals[0]]
                o.set_body_pose(bb, min(max(gx + gw / 2, -BLOCK_LIM), BLOCK_LIM), gy, ang)
            elif kind == "under":
                o.set_body_pose(bb, pose[0], pose[1], ang)
            else:
                x0 = min(max(cur[bb, 0], -BLOCK_LIM), BLOCK_LIM - 0.01)
                y0 = min(max(cur[bb, 1], -BLOCK_LIM), BLOCK_LIM)
                rec.boundary = _allo_boundary(o, bb, x0, y0, 0.0)
                if rec.boundary is not None:
                    o.set_body_pose(bb, rec.boundary[1 if kind == "int" else 0], y0, 0.0)
                else:
                    o.set_body_pose(bb, x0, y0, 0.0)
            rec.kind, rec.block = kind, bb
        final = o.bodies()
        rec.ops = [(b, float(final[b, 0]), float(final[b, 1]), float(final[b, 2])) for b in range(len(final))]
        for op in rec.ops:      # both sides receive every body's pose, whether it moved or not
            o.set_body_pose(*op)
        assert np.array_equal(o.bodies()[:, :3], final[:, :3])
        rec.ego_changed = not np.array_equal(o.render_full()[1], reset_ego)
        rec.robot_body = r0
        # the placed bodies (the robot's main body, the placed block) against each other and every block
        placed = [(final[r0, 0], final[r0, 1], tables.ROBOT_RAD, -1)]
        if rec.block is not None:
            placed.append((final[rec.block, 0], final[rec.block, 1], BLOCK_RAD, rec.block))
        rest_of = placed[:1] + [(final[b0[k], 0], final[b0[k], 1], BLOCK_RAD, b0[k]) for k in blocks]
        rec.clear = all(math.hypot(p[0] - q[0], p[1] - q[1]) >= p[2] + q[2]
                        for p in placed for q in rest_of if p[3] != q[3])
        plan.append(rec)
    return plan


_plans = functools.lru_cache(maxsize=None)(build_plan)


def plan_for(name):
    """the shared plan of `name`'s task and variant; its users only render the oracles"""
    return _plans(base_name(name))


def step_action(i):
    return (5 * i + 3) % 18


# ---------------------------------------------------------------------------
# CPU tests: the inputs can find a fault
def test_pose_table_has_the_special_poses():
    for pos in CORNERS + WALL_MIDS + [CENTRE]:
        for a in HEADINGS8:
            assert (*pos, a) in ROBOT_POSES
    for pos in WALL_MIDS:
        for a in EXACT_HEADINGS:
            assert (*pos, a - 1e-9) in ROBOT_POSES and (*pos, a + 1e-9) in ROBOT_POSES
    assert all(abs(x) <= 0.8 and abs(y) <= 0.8 for x, y, _ in ROBOT_POSES)
    assert EXACT_HEADINGS == [0.0, math.pi / 2, math.pi, 3 * math.pi / 2]
    assert not set(GENERIC_HEADINGS) & set(HEADINGS8) and len(GENERIC_HEADINGS) == 16
    covered = set()
    for name in ("MoveToRegion-TestAll-v0", "MoveToCorner-TestAll-v0"):
        covered |= set(poses_of(name))
    assert covered == set(ROBOT_POSES), "the small class does not see every pose"


@pytest.mark.parametrize("name", list(CASES))
def test_poses_leave_the_frame(name):
    """Every exact-multiple heading occurs; the arena's corners, projected with tables.ego_view, fall at a
    negative pixel coordinate for at least a quarter of the poses and beyond 383 on each axis for at least a
    quarter."""
    poses = poses_of(name)
    n = len(poses)
    assert n == len(CASES[name][0]) and n <= (96 if name.startswith("MoveTo") else 48)
    assert {a for _, _, a in poses} >= set(EXACT_HEADINGS)
    neg = bx = by = 0
    for pose in poses:
        px = [ego_pixel(pose, cx, cy) for cx in (-1.0, 1.0) for cy in (-1.0, 1.0)]
        neg += any(p[0] < 0 or p[1] < 0 for p in px)
        bx += any(p[0] > 383 for p in px)
        by += any(p[1] > 383 for p in px)
    assert 4 * neg >= n and 4 * bx >= n and 4 * by >= n, (neg, bx, by, n)


@pytest.mark.parametrize("name", list(CASES))
def test_placed_scenes_are_what_they_claim(name):
    plan = plan_for(name)           # (a PlacementError of any seed fails here: no env is skipped)
    assert len(plan) == len(CASES[name][0])
    if name.startswith(("MoveToCorner", "MatchRegions")):
        assert {t for r in plan for t in r.types} >= BLOCK_TYPES
    for i, r in enumerate(plan):
        assert r.ego_changed, f"env {i} pose {r.pose}: the ego frame is the reset frame"
        assert abs(r.orc.bodies()[r.robot_body, 0]) <= 0.8 and abs(r.orc.bodies()[r.robot_body, 1]) <= 0.8
        if r.stepped:
            assert r.finger_moved, f"env {i}: fingers at their rest angles after the fixed actions"
    if name.startswith("MoveToRegion"):
        return
    assert {r.kind for r in plan} == set(KINDS) - (set() if name.startswith("MatchRegions") else {"goal"})
    assert {r.edge for r in plan if r.edge} == set(EDGES)
    for i, r in enumerate(plan):
        x, y = r.ops[r.block][1:3]
        assert abs(x) <= BLOCK_LIM and abs(y) <= BLOCK_LIM
        if r.kind in EDGES:
            px, py = ego_pixel(r.pose, x, y)
            want = {"x0": (px, 0), "x383": (px, 383), "y0": (py, 0), "y383": (py, 383)}[r.edge]
            assert abs(want[0] - want[1]) <= 2, (i, r.edge, px, py)
            # the block's own colour reaches the frame's first / last row or column: it is really cut
            assert r.edge_pixels[1] > r.edge_pixels[0], (i, r.pose, r.edge, r.edge_pixels)
        if r.kind in ("int", "ulp"):
            assert r.boundary is not None, f"env {i}: no pixel boundary within one pixel"
            xa, xb = r.boundary
            assert math.nextafter(xa, math.inf) == xb and x == (xb if r.kind == "int" else xa)


B_CASES = [("MoveToRegion-TestAll-LoRes4E-v0", False), ("MoveToCorner-TestAll-LoRes4A-v0", False),
           ("ClusterColour-Demo-LoResStack-v0", False), ("MatchRegions-TestAll-LoRes4E-v0", False),
           ("MoveToRegion-TestAll-LoRes4E-v0", True)]


def clear_subset(plan):
    return [i for i, r in enumerate(plan) if r.clear]


@pytest.mark.parametrize("name", sorted({c[0] for c in B_CASES}))
def test_stepped_subset_is_collision_free(name):
    """Test B's envs: no two of the robot's main body and the blocks closer than the sum of their radii, and
    one oracle step from the placed state returns without table overflow."""
    plan = build_plan(name)         # a private copy: the step moves the oracles
    sub = clear_subset(plan)
    assert 3 * len(sub) >= len(plan), f"only {len(sub)} of {len(plan)} poses are collision free"
    exact = {plan[i].pose[2] for i in sub} & set(EXACT_HEADINGS)
    # (ClusterColour-Demo's fixed layout of 8 blocks leaves no clear spot at some wall poses)
    assert len(exact) == 4 if name.startswith("MoveTo") else len(exact) >= 3
    assert {plan[i].stepped for i in sub} == {False, True}
    even = odd = 0
    for i in sub:
        plan[i].orc.step(step_action(i))    # raises on table overflow
        for fr in plan[i].orc.render_full():
            ss = fr.reshape(96, 4, 96, 4, 3).astype(np.int32).sum(axis=(1, 3))
            half, q = ss % 16 == 8, ss // 16
            lo = po.downsample(fr)
            assert np.array_equal(lo[half], (q + (q & 1))[half])
            even += int((half & (q % 2 == 0)).sum())
            odd += int((half & (q % 2 == 1)).sum())
    # 4x4 blocks whose mean is an exact half, with an even and with an odd floor: rounding half to even differs
    # from rounding half up on the first and from truncation on the second
    assert even > 0 and odd > 0, (even, odd)


# ---------------------------------------------------------------------------
# GPU tests
def _place_on_gpu(vec, plan, torch):
    """reset, the fixed actions (every env steps; the poses of all bodies are overwritten next), then every
    body of every env set to the oracle's doubles"""
    vec.reset()
    n = len(plan)
    for a in PRE_ACTIONS:
        vec.step(torch.full((n,), a, dtype=torch.uint8))
    for i, r in enumerate(plan):
        for b, x, y, a in r.ops:
            vec.set_body_pose(i, b, x, y, a)


@pytest.mark.gpu
@pytest.mark.parametrize("name,retry", [("MoveToRegion-TestAll-v0", 0), ("MoveToCorner-TestAll-v0", 0),
                                        ("ClusterColour-Demo-v0", 0), ("MatchRegions-TestAll-v0", 0),
                                        ("MatchRegions-TestAll-v0", 1), ("MatchRegions-TestAll-v0", 2),
                                        ("MatchRegions-TestAll-v0", 3)])
def test_placed_frames(name, retry, monkeypatch):
    """mg_render_full (kernel mode 1) at the placed poses equals the oracle's frames bit for bit, with no error
    flag; MG_DEBUG_RENDER_RETRY puts every class of the many-block chain through the same poses."""
    import torch
    import magical_amd
    monkeypatch.setenv("MG_DEBUG_RENDER_RETRY", str(retry))
    plan = plan_for(name)
    n = len(plan)
    vec = magical_amd.make_vec(name, n, seeds=[r.seed for r in plan])
    _place_on_gpu(vec, plan, torch)
    full = vec.render_full().cpu().numpy()
    errs = vec.errors().cpu().numpy()
    vec.close()
    for i, r in enumerate(plan):
        for v, (view, ref) in enumerate(zip(("allo", "ego"), r.orc.render_full())):
            if not np.array_equal(full[i, v], ref):
                y, x = np.argwhere((full[i, v] != ref).any(-1))[0]
                pytest.fail(f"env {i} (seed {r.seed}) {view} frame, robot pose {r.pose}, block {r.kind}/{r.edge}: "
                            f"first differing pixel x={x} y={y}: {full[i, v, y, x]} vs oracle {ref[y, x]}; "
                            f"{int((full[i, v] != ref).any(-1).sum())} pixels differ")
    assert not errs.any(), {i: int(e) for i, e in enumerate(errs) if e}


@pytest.mark.gpu
@pytest.mark.parametrize("name,window", B_CASES)
def test_placed_lores_matches_full(name, window):
    """One step from the placed poses: the current LoRes frames of the observation (kernel mode 0; mode 2 with
    window rings; the newest three channels of stacked keys) equal the oracle's INTER_AREA downsample of the
    GPU's own mg_render_full after that step, byte for byte.  No physics parity is involved."""
    import torch
    import magical_amd
    whole = plan_for(name)
    sub = clear_subset(whole)
    plan = [whole[i] for i in sub]
    n = len(plan)
    spec = registry.lookup(name)
    vec = magical_amd.make_vec(name, n, seeds=[r.seed for r in plan], window=window)
    assert (vec.window_k > 0) == window
    _place_on_gpu(vec, plan, torch)
    obs, _, done, _ = vec.step(torch.as_tensor([step_action(i) for i in sub], dtype=torch.uint8))
    got = {k: v.cpu().numpy() for k, v in obs.items()}
    assert not done.cpu().numpy().any()
    full = vec.render_full().cpu().numpy()
    errs = vec.errors().cpu().numpy()
    vec.close()
    past_view = {"LoRes4E": 1, "LoRes4A": 0, "LoRes3EA": 1}.get(spec.preproc)
    checked = 0
    for k, arr in got.items():
        view = {"allo": 0, "ego": 1, "past_obs": past_view}[k]
        assert arr.shape[1:3] == (96, 96) and arr.shape[3] in (3, 12)
        for j, i in enumerate(sub):
            want = po.downsample(full[j, view])
            cur = arr[j, :, :, arr.shape[3] - 3:]
            if not np.array_equal(cur, want):
                y, x = np.argwhere((cur != want).any(-1))[0]
                pytest.fail(f"env {i} (seed {plan[j].seed}) obs {k}, robot pose {plan[j].pose}: first differing "
                            f"LoRes pixel x={x} y={y}: {cur[y, x]} vs downsampled full render {want[y, x]}")
            checked += 1
    assert checked == n * len(got) and {"allo", "ego"} <= set(got)
    assert not errs.any(), {sub[j]: int(e) for j, e in enumerate(errs) if e}
