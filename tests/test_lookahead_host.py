"""CPU: the host side of mg_lookahead -- header, ctypes binding, build units."""
import ctypes
import os
import re

from magical_amd import build, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("score", "double"), ("steps", "int32_t"), ("bodies", "double"), ("counts", "int32_t"), ("errors", "int32_t")]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "magical_sim.h")).read(), flags=re.S)


def test_header_declares_the_call_and_its_outputs():
    src = _header()
    body = {name: b for b, name in re.findall(r"typedef struct \{(.*?)\}\s*(\w+);", src, flags=re.S)}["mg_lookahead_out"]
    decls = [re.match(r"(\w+)\s*\*\s*(\w+)$", d.strip()).groups() for d in body.split(";") if d.strip()]
    assert [(n, t) for t, n in decls] == FIELDS
    proto = re.search(r"int mg_lookahead\((.*?)\);", src, flags=re.S).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["mg_sim *sim", "const uint8_t *actions_dev", "int32_t H", "const mg_lookahead_out *out", "void *stream"]


def test_binding_matches_the_header():
    assert "mg_lookahead" in native.EXPORTS
    assert [f for f, _ in native.mg_lookahead_out._fields_] == [f for f, _ in FIELDS]
    assert all(t is ctypes.c_void_p for _, t in native.mg_lookahead_out._fields_)
    assert ctypes.sizeof(native.mg_lookahead_out) == 5 * ctypes.sizeof(ctypes.c_void_p)
    fn = native.load().mg_lookahead
    vp = ctypes.c_void_p
    assert fn.argtypes[:3] == [vp, vp, ctypes.c_int32] and fn.argtypes[4] is vp
    assert fn.argtypes[3]._type_ is native.mg_lookahead_out and fn.restype is ctypes.c_int32
    # refused on the host, before any GPU call: nothing is launched for a null handle
    assert fn(None, None, 1, None, None) == -22


def test_build_table_matches_the_include_lines():
    """a header missing from a unit's list is a stale-object bug: every list is exactly what the unit includes, directly
    or through its headers"""
    def includes(f, seen):
        for h in re.findall(r'^#include "(mg_\w+\.h)"', open(os.path.join(build.CSRC, f)).read(), re.M):
            if h not in seen:
                seen.add(h)
                includes(h, seen)
        return seen
    for u, hs in build.UNITS.items():
        assert sorted(hs) == sorted(includes(u, set())), u


def test_build_lists_the_lookahead_units():
    units = [u for u in build.UNITS if "look" in u]
    assert sorted(units) == ["mg_look_hbm.hip", "mg_look_quad.hip", "mg_look_v4.hip", "mg_lookahead.hip"]
    on_disk = sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    assert on_disk == sorted(build.UNITS)   # every translation unit under csrc/ is built, and nothing else is listed
    for u in units:
        for h in build.UNITS[u]:
            assert os.path.exists(os.path.join(build.CSRC, h)), (u, h)
        if u != "mg_lookahead.hip":
            assert "mg_lookahead.h" in build.UNITS[u] and "mg_stepk.h" in build.UNITS[u]
