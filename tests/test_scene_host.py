"""CPU: the host side of explicit scenes (magical_amd.scene, the mg_scene bindings of magical_amd.native): the record's
layout, pack / unpack, and validate -- the restatement of the device's rules (csrc/mg_scene.h scene_status) with the
same status codes.  The GPU side is tests/test_scene.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from magical_amd import native, registry, scene as sc, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = list(registry.TASK_IDS)
COLOUR_SHAPE_DYN = registry.COLOUR | registry.SHAPE_TYPE | registry.DYNAMICS


def test_record_layout_matches_the_numpy_dtype_and_the_header():
    assert ctypes.sizeof(native.mg_scene_ent) == native.SCENE_ENT_DTYPE.itemsize == 56
    assert ctypes.sizeof(native.mg_scene) == native.SCENE_DTYPE.itemsize == 792
    for struct, dtype in ((native.mg_scene_ent, native.SCENE_ENT_DTYPE), (native.mg_scene, native.SCENE_DTYPE)):
        assert [f[0] for f in struct._fields_] == list(dtype.names)
        for f in struct._fields_:
            assert getattr(struct, f[0]).offset == dtype.fields[f[0]][1], f[0]
            assert getattr(struct, f[0]).size == dtype.fields[f[0]][0].itemsize, f[0]
    assert native.SCENE_DTYPE.fields["ent"][0].shape == (native.SCENE_MAX_ENTS,)
    # the header declares the same fields in the same order (comments stripped)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "magical_sim.h")).read(), flags=re.S)
    for name, dtype in (("mg_scene_ent", native.SCENE_ENT_DTYPE), ("mg_scene", native.SCENE_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [re.sub(r"\[\d+\]", "", v.strip()) for v in decl.split(None, 1)[1].split(",")]
        assert fields == list(dtype.names), name
    assert "mg_get_scene" in native.EXPORTS and "mg_reset_scene" in native.EXPORTS


def test_pack_unpack_round_trip():
    scenes = [sc.demo_scene(t) for t in TASKS]
    scenes[-1] = sc.demo_scene("PickAndPlace", target_xy=(0.25, -0.75), target_ent=2)
    scenes[2].ents[3].flags = sc.DISABLED
    scenes[0].pv = (2.5, 0.9, 3.0, 1.25, 0.08)
    arr = sc.pack(scenes)
    assert arr.dtype == native.SCENE_DTYPE and arr.shape == (len(TASKS),)
    assert sc.unpack(arr) == scenes
    assert sc.pack(sc.unpack(arr)).tobytes() == arr.tobytes()
    for r, s in zip(arr, scenes):   # entries past n_ents are zero
        assert r["n_ents"] == len(s.ents)
        assert r["ent"][len(s.ents):].tobytes() == bytes(56 * (native.SCENE_MAX_ENTS - len(s.ents)))
    fd = arr[TASKS.index("FindDupe")]
    assert list(fd["ent"]["kind"][:9]) == [sc.GOAL] + [sc.BLOCK] * 7 + [sc.ROBOT]
    # a goal is stored by its centre: the corner the task file gives plus half its size
    g = scenes[0].ents[0]
    assert (g.x, g.y, g.h, g.w) == (-0.62 + 0.75 / 2, -0.17 - 0.76 / 2, 0.76, 0.75)
    with pytest.raises(ValueError):
        sc.pack([sc.Scene([sc.robot(0, 0, 0)] * 14)])


@pytest.mark.parametrize("task", TASKS)
def test_demo_scene_is_valid(task):
    s = sc.demo_scene(task)
    assert sc.validate(s, task, 0) == 0
    assert sc.validate(s, registry.TASK_IDS[task], 0) == 0
    assert sc.validate(s, task, COLOUR_SHAPE_DYN) == 0 or task == "MoveToCorner"
    # the Demo scene fills the Demo handle's slot caps exactly where the constraint list is compiled
    caps = sc.step_caps(registry.TASK_IDS[task], 0)
    nblk = sum(t.kind == sc.BLOCK for t in s.ents)
    assert (6 + nblk, 10 + 2 * nblk) == (caps[0], caps[2])


def test_step_caps_match_the_header():
    """csrc/mg_stepforms.h step_caps / step_form_caps, as tests/golden/step_forms_select.json records them"""
    assert sc.step_caps(0, 0) == (6, 5, 10, 20) and sc.step_caps(1, 0) == (7, 6, 12, 32)
    assert sc.compiled_constraints(sc.step_caps(0, 0)) and sc.compiled_constraints(sc.step_caps(1, 0))
    assert not sc.compiled_constraints(sc.step_caps(1, registry.SHAPE_TYPE))
    assert sc.step_caps(2, 0) == (14, 53, 26, 48)   # form 4's caps: 8 blocks, stars included
    assert sc.step_caps(2, registry.SHAPE_COUNT)[0] == 16


def _with(s, i, **kw):
    s = s.copy()
    for k, v in kw.items():
        setattr(s.ents[i], k, v)
    return s


def test_validate_status_1_count_or_kind_order():
    region, cluster = sc.demo_scene("MoveToRegion"), sc.demo_scene("ClusterColour")
    assert sc.validate(sc.Scene(region.ents[::-1]), "MoveToRegion") == 1          # robot before the goal
    assert sc.validate(sc.Scene(region.ents + [sc.block(1, 0, 0, 0, 0)]), "MoveToRegion") == 1
    assert sc.validate(sc.Scene([]), "MoveToRegion") == 1
    assert sc.validate(sc.Scene(cluster.ents[2:]), "ClusterColour") == 1          # 6 blocks: below Cluster's 7
    assert sc.validate(sc.Scene(cluster.ents[1:]), "ClusterColour") == 0          # 7
    assert sc.validate(region, "MoveToCorner") == 1
    corner = sc.demo_scene("MoveToCorner")
    assert sc.validate(sc.Scene(corner.ents + corner.ents[1:]), "MoveToCorner") == 1   # exactly one block
    line = sc.demo_scene("MakeLine")
    assert sc.validate(sc.Scene(line.ents[2:]), "MakeLine") == 1 and sc.validate(sc.Scene(line.ents[1:]), "MakeLine") == 0
    dupe = sc.demo_scene("FindDupe")
    assert sc.validate(sc.Scene(dupe.ents[:1] + dupe.ents[6:]), "FindDupe") == 1   # one outer block and the query
    assert sc.validate(sc.Scene(dupe.ents[:1] + dupe.ents[5:]), "FindDupe") == 0
    fix = sc.demo_scene("FixColour")
    assert sc.validate(sc.Scene(fix.ents[:1] + fix.ents[3:4] + fix.ents[6:]), "FixColour") == 1   # one region
    assert sc.validate(sc.Scene(fix.ents[:2] + fix.ents[3:5] + fix.ents[6:]), "FixColour") == 0   # two
    assert sc.validate(sc.Scene(fix.ents[:3] + fix.ents[3:5] + fix.ents[6:]), "FixColour") == 1   # 3 regions, 2 blocks
    pnp = sc.demo_scene("PickAndPlace")
    assert sc.validate(sc.Scene(pnp.ents[:3], target_ent=1), "PickAndPlace") == 1
    match = sc.demo_scene("MatchRegions")
    assert sc.validate(sc.Scene(match.ents[:1] + match.ents[3:]), "MatchRegions") == 1   # no block of the goal's colour
    assert sc.validate(sc.Scene(match.ents[:2] + match.ents[-1:]), "MatchRegions") == 0  # one block, of that colour
    assert sc.validate(sc.Scene(match.ents * 2), "MatchRegions") == 1                      # 14 entities


def test_validate_status_2_ranges():
    region, corner = sc.demo_scene("MoveToRegion"), sc.demo_scene("MoveToCorner")
    for bad in (_with(region, 0, colour=7), _with(region, 0, colour=tables.GREY), _with(region, 0, type=1),
                _with(region, 0, h=0.09), _with(region, 0, w=0.81), _with(region, 0, h=math.nan), _with(region, 0, angle=0.5),
                _with(region, 1, x=1.0000001), _with(region, 1, y=-math.inf), _with(region, 1, angle=100.5),
                _with(region, 1, angle=math.nan), _with(region, 1, flags=2), _with(region, 1, h=0.5), _with(region, 1, type=1)):
        assert sc.validate(bad, "MoveToRegion") == 2, bad
    for bad in (_with(corner, 1, type=7), _with(corner, 1, type=-1), _with(corner, 1, colour=4), _with(corner, 1, flags=-1)):
        assert sc.validate(bad, "MoveToCorner") == 2, bad
    for ok in (_with(region, 0, h=0.1, w=0.8), _with(region, 1, x=1.0, y=-1.0, angle=-100.0), _with(region, 1, flags=1),
               _with(region, 1, colour=99)):   # the robot's colour is ignored
        assert sc.validate(ok, "MoveToRegion") == 0, ok
    for pv in ((3, 1, 4, 1.5, 0.0), (3, 1, 4, -1.5, 0.1), (math.inf, 1, 4, 1.5, 0.1), (3, math.nan, 4, 1.5, 0.1)):
        s = region.copy()
        s.pv = pv
        assert sc.validate(s, "MoveToRegion") == 2, pv
    assert sc.validate(sc.demo_scene("PickAndPlace", target_xy=(1.5, 0.0)), "PickAndPlace") == 2
    # the lowest code wins: a bad enum in a scene that also does not fit
    cluster = sc.demo_scene("ClusterColour")
    nine = sc.Scene(cluster.ents[:1] + cluster.ents)
    assert sc.validate(_with(nine, 0, colour=9), "ClusterColour") == 2


def test_validate_status_3_fit():
    # a star on a MoveToCorner handle created without the shape-type flag
    corner = sc.demo_scene("MoveToCorner")
    star = _with(corner, 1, type=tables.STAR)
    assert sc.validate(star, "MoveToCorner", 0) == 3
    assert sc.validate(star, "MoveToCorner", registry.SHAPE_TYPE) == 0
    assert sc.validate(_with(corner, 1, type=tables.PENTAGON), "MoveToCorner", 0) == 0   # one shape, as the square
    # a ninth block on a Cluster handle created without the count flag
    cluster = sc.demo_scene("ClusterColour")
    nine = sc.Scene(cluster.ents[:1] + cluster.ents)
    assert sc.validate(nine, "ClusterColour", 0) == 3
    assert sc.validate(nine, "ClusterColour", registry.SHAPE_COUNT) == 0
    eleven = sc.Scene(cluster.ents[:3] + cluster.ents)
    assert sc.validate(eleven, "ClusterColour", registry.SHAPE_COUNT) == 3
    # eight stars are more shapes than 8 blocks' caps
    stars = cluster.copy()
    for t in stars.ents[:8]:
        t.type = tables.STAR
    assert sc.validate(stars, "ClusterColour", 0) == 0   # form 4's caps are sized for 8 stars
    # exact: a compiled constraint list takes nothing but its own counts
    assert sc.validate(sc.Scene(cluster.ents[1:]), "ClusterColour", 0, exact=True) == 3


def test_validate_status_4_target():
    for bad in (0, -1, 4, 99):   # the robot, none, past the end
        assert sc.validate(sc.demo_scene("PickAndPlace", target_ent=bad), "PickAndPlace") == 4, bad
    for ok in (1, 2, 3):
        assert sc.validate(sc.demo_scene("PickAndPlace", target_ent=ok), "PickAndPlace") == 0
    assert sc.validate(sc.demo_scene("MoveToRegion"), "MoveToRegion") == 0   # target_ent -1 elsewhere


def test_status_texts_cover_every_code():
    assert set(sc.STATUS_TEXT) == {-1, 0, 1, 2, 3, 4}
