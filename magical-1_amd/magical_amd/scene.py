"""Explicit scenes: an env's layout as data (include/magical_sim.h: mg_scene, mg_get_scene, mg_reset_scene).

A `Scene` is the host form of one mg_scene record: the entities after the arena in the order the task's reset adds
them, the five physics variables and PickAndPlace's target.  `pack` / `unpack` convert between lists of scenes and the
numpy structured array (`native.SCENE_DTYPE`) that `VecMagicalEnv.reset_scenes` / `get_scenes` move to and from the
device.  `validate` restates the device's rules with the same status codes, so a generator can check a level without
a GPU; `demo_scene` is a task's Demo layout.

    scenes = [demo_scene("MoveToRegion") for _ in range(env.num_envs)]
    scenes[3].ents[1].x = 0.5                         # move env 3's robot
    obs, status = env.reset_scenes(scenes, check=True)
"""
import copy
import math
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from . import native, registry, tables

GOAL, ROBOT, BLOCK = 1, 2, 3   # mg_scene_ent.kind: MG_ENT_* (csrc/mg_common.h; the arena, 0, is implicit)
DISABLED = 1                   # mg_scene_ent.flags bit 0
PV_DEFAULT = (3.0, 1.0, 4.0, 1.5, 0.1)   # csrc/mg_reset.h:484 PV_DEF, PhysVar declaration order
GOAL_MIN, GOAL_MAX, ANGLE_MAX = 0.1, 0.8, 100.0   # csrc/mg_scene.h MG_SCENE_GOAL_MIN / _MAX / MG_SCENE_ANGLE_MAX
MAX_BODIES, MAX_SHAPES, MAX_CONS, MAX_ARB = 16, 64, 32, 48   # csrc/mg_common.h MG_MAX_*
STATUS_TEXT = native.SCENE_STATUS_TEXT

_T = registry.TASK_IDS
_R, _G, _B, _Y = tables.RED, tables.GREEN, tables.BLUE, tables.YELLOW
_SQ, _PE, _ST, _CI = tables.SQUARE, tables.PENTAGON, tables.STAR, tables.CIRCLE
SHAPE_COLOURS = (_R, _G, _B, _Y)   # csrc/mg_reset.h:376 MG_SHAPE_COLOURS
SHAPE_TYPES = (_SQ, _PE, _ST, _CI)   # csrc/mg_reset.h:377 MG_SHAPE_TYPES


@dataclass
class Entity:
    kind: int
    type: int = 0
    colour: int = 0
    flags: int = 0
    x: float = 0.0
    y: float = 0.0
    angle: float = 0.0
    h: float = 0.0
    w: float = 0.0


def goal(cx, cy, h, w, colour):
    """a goal region by its CENTRE"""
    return Entity(GOAL, 0, colour, 0, cx, cy, 0.0, h, w)


def goal_from_corner(x, y, h, w, colour):
    """a goal region by its top-left corner, as the task files give it (csrc/mg_reset.h:403-407 inst_goal)"""
    return goal(x + w / 2, y - h / 2, h, w, colour)


def robot(x, y, angle):
    return Entity(ROBOT, 0, tables.GREY, 0, x, y, angle)


def block(type, colour, x, y, angle):
    return Entity(BLOCK, type, colour, 0, x, y, angle)


@dataclass
class Scene:
    ents: List[Entity] = field(default_factory=list)
    pv: Tuple[float, ...] = PV_DEFAULT
    target_ent: int = -1                     # PickAndPlace: index into ents of the block to place
    target_xy: Tuple[float, float] = (0.0, 0.0)

    def copy(self):
        return copy.deepcopy(self)


def pack(scenes):
    """list of Scene -> structured array [len(scenes)] of native.SCENE_DTYPE (entries past n_ents zero)"""
    arr = np.zeros(len(scenes), dtype=native.SCENE_DTYPE)
    for i, s in enumerate(scenes):
        if len(s.ents) > native.SCENE_MAX_ENTS:
            raise ValueError(f"pack: scene {i} has {len(s.ents)} entities, more than {native.SCENE_MAX_ENTS}")
        if len(s.pv) != 5:
            raise ValueError(f"pack: scene {i} needs 5 physics variables")
        r = arr[i]
        r["n_ents"], r["target_ent"] = len(s.ents), s.target_ent
        r["pv"], r["target_xy"] = s.pv, s.target_xy
        for k, t in enumerate(s.ents):
            r["ent"][k] = (t.kind, t.type, t.colour, t.flags, t.x, t.y, t.angle, t.h, t.w)
    return arr


def unpack(arr):
    """structured array -> list of Scene (n_ents clipped to the record's 13 slots)"""
    arr = np.asarray(arr, dtype=native.SCENE_DTYPE).reshape(-1)
    out = []
    for r in arr:
        n = min(max(int(r["n_ents"]), 0), native.SCENE_MAX_ENTS)
        ents = [Entity(int(t["kind"]), int(t["type"]), int(t["colour"]), int(t["flags"]), float(t["x"]), float(t["y"]),
                       float(t["angle"]), float(t["h"]), float(t["w"])) for t in r["ent"][:n]]
        out.append(Scene(ents, tuple(float(v) for v in r["pv"]), int(r["target_ent"]),
                         (float(r["target_xy"][0]), float(r["target_xy"][1]))))
    return out


# ---- the handle's slot caps (csrc/mg_stepforms.h) -----------------------------------------------------------
_NSHAPES = None


def block_nshapes():
    """shapes per block type (the library's block_nshapes)"""
    global _NSHAPES
    if _NSHAPES is None:
        _NSHAPES = [len(b["polys"]) for _, b in sorted(tables.block_tables().items())]
    return _NSHAPES


def step_caps(task_id, rand_flags):
    """(bodies, shapes, constraints, arbiter slots) of a task's scenes: csrc/mg_stepforms.h:118-134 step_caps"""
    star = block_nshapes()[_ST]
    per = star
    if task_id == _T["MoveToRegion"]:
        nblk = 0
    elif task_id == _T["MoveToCorner"]:
        nblk, per = 1, (star if rand_flags & registry.SHAPE_TYPE else 1)
    elif task_id in (_T["ClusterColour"], _T["ClusterShape"]):
        nblk = 10 if rand_flags & registry.SHAPE_COUNT else 8
    elif task_id == _T["MakeLine"]:
        nblk = 4
    elif task_id == _T["FindDupe"]:
        nblk = 7
    elif task_id in (_T["FixColour"], _T["PickAndPlace"]):
        nblk = 3
    else:
        nblk = 8 if rand_flags & registry.SHAPE_COUNT else 5
    ns = 5 + nblk * per
    pairs = 4 * ns + 5 * (ns - 5) + ((ns - 5) * (ns - 6)) // 2
    return 6 + nblk, ns, 10 + 2 * nblk, ((pairs + 3) // 4 * 4 if pairs < MAX_ARB else MAX_ARB)


def compiled_constraints(caps):
    """does a scene with these caps run step form 5 or 6 (csrc/mg_stepforms.h:41-46, 142-149), whose constraint lists
    are compiled?  Then a scene's counts must equal the caps."""
    return tuple(caps) in ((6, 5, 10, 20), (7, 6, 12, 32))


def _order(task_id, n):
    """(goals, blocks, robot first, count ok): csrc/mg_scene.h scene_order"""
    if n < 1 or n > native.SCENE_MAX_ENTS:
        return 0, 0, False, False
    if task_id == _T["MoveToRegion"]:
        return 1, n - 2, False, n - 2 == 0
    if task_id == _T["MoveToCorner"]:
        return 0, n - 1, True, n - 1 == 1
    if task_id in (_T["ClusterColour"], _T["ClusterShape"]):
        return 0, n - 1, False, n - 1 >= 7
    if task_id == _T["MakeLine"]:
        return 0, n - 1, False, n - 1 >= 3
    if task_id == _T["FindDupe"]:
        return 1, n - 2, False, n - 2 >= 3
    if task_id == _T["FixColour"]:
        nr = (n - 1) // 2
        return nr, nr, False, n % 2 == 1 and nr >= 2
    if task_id == _T["PickAndPlace"]:
        return 0, n - 1, True, n - 1 == 3
    return 1, n - 2, False, n - 2 >= 1


def _within(v, bound):
    return abs(v) <= bound   # False for NaN


def validate(scene, task, rand_flags=0, exact=None):
    """mg_reset_scene's status for `scene` on a handle of `task` (a name or id) and `rand_flags`: 0 would be built, 1
    entity count or kind order is not the task's, 2 a field is out of range, 3 the scene does not fit the handle's
    slot caps, 4 PickAndPlace's target_ent is not a block -- the lowest code that applies (csrc/mg_scene.h
    scene_status).  exact: whether the counts must equal the caps; default: the handle's scenes run step form 5 or 6."""
    task_id = _T[task] if isinstance(task, str) else int(task)
    ents, n = scene.ents, len(scene.ents)
    ngoal, nblk, robot_first, ok = _order(task_id, n)
    if not ok:
        return native.SCENE_BAD_ORDER
    for i, t in enumerate(ents):
        want = (ROBOT if i == 0 else BLOCK) if robot_first else (GOAL if i < ngoal else BLOCK if i < n - 1 else ROBOT)
        if t.kind != want:
            return native.SCENE_BAD_ORDER
    if task_id == _T["MatchRegions"] and not any(t.colour == ents[0].colour for t in ents[1:n - 1]):
        return native.SCENE_BAD_ORDER
    bad = len(scene.pv) != 5 or any(not (v > 0.0 and v <= 1.7976931348623157e308) for v in scene.pv)
    for t in ents:
        bad = bad or (t.flags & ~1) != 0 or not _within(t.x, 1.0) or not _within(t.y, 1.0)
        if t.kind == GOAL:
            bad = bad or t.type != 0 or t.colour not in SHAPE_COLOURS or not t.angle == 0.0 or \
                not GOAL_MIN <= t.h <= GOAL_MAX or not GOAL_MIN <= t.w <= GOAL_MAX
        else:
            bad = bad or not _within(t.angle, ANGLE_MAX) or not t.h == 0.0 or not t.w == 0.0
            if t.kind == BLOCK:
                bad = bad or not 0 <= t.type < tables.NUM_SHAPE_TYPES or t.colour not in SHAPE_COLOURS
            else:
                bad = bad or t.type != 0
    if task_id == _T["PickAndPlace"]:
        bad = bad or not _within(scene.target_xy[0], 1.0) or not _within(scene.target_xy[1], 1.0)
    if bad:
        return native.SCENE_BAD_RANGE
    caps = step_caps(task_id, rand_flags)
    nb, nc = 6 + nblk, 10 + 2 * nblk
    ns = 5 + sum(block_nshapes()[t.type] for t in ents if t.kind == BLOCK)
    if not (nb <= caps[0] and ns <= caps[1] and nc <= caps[2] and nb <= MAX_BODIES and ns <= MAX_SHAPES and nc <= MAX_CONS):
        return native.SCENE_NO_FIT
    if (compiled_constraints(caps) if exact is None else exact) and (nb, ns, nc) != tuple(caps[:3]):
        return native.SCENE_NO_FIT
    if task_id == _T["PickAndPlace"] and not (0 <= scene.target_ent < n and ents[scene.target_ent].kind == BLOCK):
        return native.SCENE_BAD_TARGET
    return native.SCENE_BUILT


# ---- Demo layouts -----------------------------------------------------------------------------------------------
# The Demo constants live in the reset kernel only (csrc/mg_reset.h, which cites the reference's task files); they are
# stated again here with the kernel's lines.
_PI = math.pi
# csrc/mg_reset.h:427-441 CC_COLOURS / CC_TYPES / CC_POSES / CC_ROBOT ([0] ClusterColour, [1] ClusterShape)
_CC_COLOURS = ((_B, _B, _B, _G, _G, _R, _Y, _Y), (_Y, _B, _R, _R, _G, _Y, _B, _G))
_CC_TYPES = ((_CI, _ST, _SQ, _PE, _PE, _SQ, _ST, _PE), (_SQ, _PE, _PE, _PE, _CI, _ST, _ST, _CI))
_CC_POSES = (((-0.5147, 0.14149, -0.38871), (-0.1347, -0.71414, 1.0533), (-0.74247, -0.097592, 1.1571),
              (-0.077363, -0.42964, -0.64379), (0.51978, 0.1853, -1.1762), (-0.5278, -0.21642, 2.9356),
              (-0.54039, 0.48292, 0.072818), (-0.16761, 0.64303, -2.3255)),
             ((-0.414, 0.297, -1.731), (0.068, 0.705, 2.184), (0.821, 0.220, 0.650), (-0.461, -0.749, -2.673),
              (0.867, -0.149, -2.215), (-0.785, -0.140, -0.405), (-0.305, -0.226, 1.341), (0.758, -0.708, -2.140)))
_CC_ROBOT = ((0.71692, -0.34374, 0.83693), (0.286, -0.202, -1.878))
# csrc/mg_reset.h:443-447 (make_line.py:13-27), robot :561
_ML_COLOURS, _ML_TYPES = (_B, _Y, _R, _G), (_ST, _CI, _ST, _PE)
_ML_POSES = ((0.790, -0.820, -0.721), (-0.177, 0.383, -1.733), (-0.051, -0.128, 2.696), (-0.292, -0.745, -0.159))
# csrc/mg_reset.h:449-456 (find_dupe.py:7-37); query, goal and robot :571, :585-594
_FD_OUT_TYPES = (_PE, _CI, _CI, _SQ, _ST, _PE)
_FD_OUT_COLOURS = (_G, _R, _R, _Y, _B, _Y)
_FD_OUT_POSES = ((-0.066751, 0.7552, -2.9266), (-0.05195, 0.31468, 1.5418), (0.57528, -0.46865, -2.2141),
                 (0.40594, -0.74977, 0.24582), (0.45254, 0.3681, -1.0834), (0.76849, -0.10652, 0.10028))
# csrc/mg_reset.h:457-464 (fix_colour.py:12-41), robot :643
_FC_BLOCK_COLOURS, _FC_BLOCK_TYPES = (_G, _G, _B), (_PE, _SQ, _PE)
_FC_BLOCK_POSES = ((0.289, 0.030, 0.307), (0.133, -0.561, 1.699), (-0.336, 0.000, -1.529))
_FC_REGIONS = ((-0.032, 0.348, 0.427, 0.468), (0.019, -0.391, 0.460, 0.458), (-0.681, 0.196, 0.498, 0.418))   # x, y, h, w
_FC_REGION_COLOURS = (_G, _G, _R)


def demo_scene(task, robot_xy=(0.5, 0.5), target_xy=(0.0, 0.0), target_ent=1):
    """The task's Demo layout (a name or id).  Two Demo variants draw from the env's RNG even so: MoveToCorner its robot
    position (rand(2), csrc/mg_reset.h:508) -- robot_xy here -- and PickAndPlace its target position and which of its
    identical blocks to place (csrc/mg_reset.h:683-688) -- target_xy, target_ent."""
    task_id = _T[task] if isinstance(task, str) else int(task)
    if task_id == _T["MoveToRegion"]:   # csrc/mg_reset.h:494-499
        return Scene([goal_from_corner(-0.62, -0.17, 0.76, 0.75, _B), robot(0.058, 0.53, -2.13)])
    if task_id == _T["MoveToCorner"]:   # csrc/mg_reset.h:508-513
        return Scene([robot(robot_xy[0], robot_xy[1], 0.55 * _PI), block(_SQ, _R, 0.1, -0.65, 0.13 * _PI)])
    if task_id in (_T["ClusterColour"], _T["ClusterShape"]):   # csrc/mg_reset.h:519-539
        by = 1 if task_id == _T["ClusterShape"] else 0
        ents = [block(_CC_TYPES[by][i], _CC_COLOURS[by][i], *_CC_POSES[by][i]) for i in range(8)]
        return Scene(ents + [robot(*_CC_ROBOT[by])])
    if task_id == _T["MakeLine"]:   # csrc/mg_reset.h:549-561
        return Scene([block(_ML_TYPES[i], _ML_COLOURS[i], *_ML_POSES[i]) for i in range(4)] + [robot(0.702, -0.255, 0.347)])
    if task_id == _T["FindDupe"]:   # csrc/mg_reset.h:570-594
        ents = [goal_from_corner(-0.72, -0.22, 0.67, 0.72, _Y)]
        ents += [block(_FD_OUT_TYPES[i], _FD_OUT_COLOURS[i], *_FD_OUT_POSES[i]) for i in range(6)]
        return Scene(ents + [block(_PE, _Y, -0.33, -0.49, -0.51), robot(-0.57, 0.25, 3.83)])
    if task_id == _T["FixColour"]:   # csrc/mg_reset.h:612-643
        ents = [goal_from_corner(*_FC_REGIONS[i], _FC_REGION_COLOURS[i]) for i in range(3)]
        ents += [block(_FC_BLOCK_TYPES[i], _FC_BLOCK_COLOURS[i], *_FC_BLOCK_POSES[i]) for i in range(3)]
        return Scene(ents + [robot(0.368, 0.586, 0.718)])
    if task_id == _T["PickAndPlace"]:   # csrc/mg_reset.h:668-688
        ents = [robot(0.0, 0.0, 0.55 * _PI)] + [block(_SQ, _R, 0.1, -0.65, 0.13 * _PI) for _ in range(3)]
        return Scene(ents, target_ent=target_ent, target_xy=(float(target_xy[0]), float(target_xy[1])))
    if task_id == _T["MatchRegions"]:   # csrc/mg_reset.h:700-736
        ents = [goal_from_corner(0.1, 0.7, 0.7, 0.6, _G),
                block(_ST, _G, 0.8, -0.7, 2.37), block(_SQ, _G, -0.68, 0.72, 1.28),
                block(_PE, _B, -0.05, -0.2, -1.09), block(_CI, _Y, -0.75, -0.55, 2.78), block(_PE, _Y, 0.3, -0.82, -1.15)]
        return Scene(ents + [robot(-0.5, 0.1, -_PI * 1.2)])
    raise ValueError(f"demo_scene: unknown task {task!r}")
