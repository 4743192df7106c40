"""CPU: mg_imagine's host side -- the header's declaration against the ctypes binding, the argument checks of the C call and
of the Python wrappers that run before any library call, and a numpy restatement of the stack rule (stack_rule), which
tests/test_imagine.py uses as a second check on the stacks the device builds.
"""
import collections
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from magical_amd import build, envs, native, pipeline, registry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the stack rule ---------------------------------------------------------------------------------------------------
def stack_rule(hist, frames, lead=None):
    """include/magical_sim.h, mg_imagine, "Stacks".  hist: the three most recent real frames [3, ..., 3], OLDEST first
    (g_-3, g_-2, g_-1); frames: the imagined frames [F, ..., 3]; -> [F, ..., 12] with stack[f] = (g_f-3, g_f-2, g_f-1,
    g_f), channel k = channel k % 3 of the k // 3-th of them.  lead [F, ..., 3] (LoRes3EA: the allo frames) replaces the
    oldest of the four: allo_f | ego_f-2 | ego_f-1 | ego_f."""
    g = np.concatenate([hist, frames], axis=0)   # g_j at index j + 3
    out = np.stack([np.concatenate([g[f + k] for k in range(4)], axis=-1) for f in range(frames.shape[0])])
    if lead is not None:
        out[..., 0:3] = lead
    return out


def _img(v):
    """a 2 x 2 RGB image whose bytes say which frame, pixel and channel they are: v + 16 * pixel + channel"""
    return (v + 16 * np.arange(4).reshape(2, 2, 1) + np.arange(3)).astype(np.uint8)


@pytest.mark.parametrize("kind", ["stack_allo", "stack_ego", "past_obs_4e_4a", "past_obs_3ea"])
def test_stack_rule_on_a_hand_built_case(kind):
    """history 1, 2, 3 (oldest first) and imagined frames 4, 5, 6, 7, 8 of one env.  The plain kinds -- LoResStack's two
    stacks, LoRes4E's and LoRes4A's past_obs -- are the same rule on the view's own frames: stack f holds frames f + 1 ..
    f + 4.  LoRes3EA: the allo frame (100 + f) leads, then ego frames f + 2 .. f + 4."""
    hist = np.stack([_img(64 * 1), _img(64 * 2), _img(64 * 3)])[:, None]           # [3, 1 env, 2, 2, 3]
    frames = np.stack([_img(4 + k) for k in range(5)])[:, None]                     # values 4 .. 8, no 64 multiple
    ids = [64 * 1, 64 * 2, 64 * 3, 4, 5, 6, 7, 8]
    if kind == "past_obs_3ea":
        lead = np.stack([_img(100 + k) for k in range(5)])[:, None]
        got = stack_rule(hist, frames, lead)
    else:
        got = stack_rule(hist, frames)
    assert got.shape == (5, 1, 2, 2, 12) and got.dtype == np.uint8
    for f in range(5):
        want_ids = ids[f:f + 4]
        if kind == "past_obs_3ea":
            want_ids = [100 + f] + want_ids[1:]
        for p in range(4):
            px = got[f, 0, p // 2, p % 2]
            want = [(v + 16 * p + c) & 255 for v in want_ids for c in range(3)]   # written out byte by byte
            assert px.tolist() == want, (kind, f, p)
    # frame 0's stack is history + the first frame; from frame 3 on no history is left in it
    assert got[0, 0, 0, 0, 0] == (100 if kind == "past_obs_3ea" else 64) and got[0, 0, 0, 0, 9] == 4
    assert got[3, 0, 0, 0, 3] == 5 and got[4, 0, 0, 0, 9] == 8


def test_stack_rule_is_the_frame_stack_of_successive_steps():
    """the rule against a deque of the last four frames, as FlattenFrameStack keeps it"""
    rs = np.random.RandomState(0)
    real = rs.randint(0, 256, (3, 2, 4, 4, 3)).astype(np.uint8)
    frames = rs.randint(0, 256, (6, 2, 4, 4, 3)).astype(np.uint8)
    dq = collections.deque(list(real), maxlen=4)
    got = stack_rule(real, frames)
    for f in range(6):
        dq.append(frames[f])
        if f == 0:
            continue   # (the deque holds three frames + 1 only now: frame 0 is checked by hand above)
        assert np.array_equal(got[f], np.concatenate(list(dq), axis=-1)), f


# ---- header, binding, build -------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "magical_sim.h")).read(), flags=re.S)


def test_header_declares_the_call_and_the_struct():
    proto = re.search(r"int mg_imagine\((.*?)\);", _header(), flags=re.S).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["mg_sim *sim", "const uint8_t *actions_dev", "int32_t H", "int32_t every",
                    "const mg_lookahead_out *out", "const mg_imagine_out *frames", "void *stream"]
    body = re.search(r"typedef struct \{([^}]*)\}\s*mg_imagine_out;", _header(), flags=re.S).group(1)
    fields = [re.match(r"uint8_t \*(\w+)$", " ".join(d.split())).group(1) for d in body.split(";") if d.strip()]
    assert fields == ["allo", "ego", "stack_allo", "stack_ego"]
    assert fields == [f for f, _ in native.mg_imagine_out._fields_]
    assert all(t is ctypes.c_void_p for _, t in native.mg_imagine_out._fields_)
    assert ctypes.sizeof(native.mg_imagine_out) == 4 * ctypes.sizeof(ctypes.c_void_p)
    text = open(os.path.join(ROOT, "include", "magical_sim.h")).read()
    doc = text[:text.index("int mg_imagine(")].rsplit("typedef struct", 1)[1]
    for word in ("u8[F][N][96][96][3]", "u8[F][N][96][96][12]", "1 <= every <= H", "oldest first", "LoRes3EA",
                 "no real step", "-22", "untouched"):
        assert word in doc, word


def test_binding_matches_the_header():
    assert "mg_imagine" in native.EXPORTS
    fn = native.load().mg_imagine
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    assert fn.argtypes == [vp, vp, i32, i32, ctypes.POINTER(native.mg_lookahead_out),
                           ctypes.POINTER(native.mg_imagine_out), vp]
    assert fn.restype is i32


def test_build_lists_the_unit():
    assert "mg_imagine.hip" in build.UNITS and "mg_imagine.h" in build.UNITS["mg_imagine.hip"]
    src = open(os.path.join(build.CSRC, "mg_imagine.hip")).read()
    included = set(re.findall(r'#include "(\w+\.h)"', src))
    assert included <= set(build.UNITS["mg_imagine.hip"])
    assert "imagine_stack_kernel" in src and "mg_imagine.hip" in open(os.path.join(build.CSRC, "mg_sim.h")).read()
    # the frame-less render form is instantiated for every capacity class by the launcher's one macro
    raster = open(os.path.join(build.CSRC, "mg_raster.hip")).read()
    assert "render_kernel<RenderSmem<CLS>, 3>" in raster
    for cls in ("RG_SMALL", "RG_MEDIUM0", "RG_MEDIUM1", "RG_MEDIUM2", "RG_LARGE"):
        assert "RG_LAUNCH(%s)" % cls in raster, cls


def test_c_refusals_without_gpu():
    """-22 before any GPU call: null arguments, no frame output, H and every out of range, the unwrapped surface (a
    zeroed stand-in for the handle has preproc 0: the checks read nothing else of it)"""
    lib = native.load()
    fn = lib.mg_imagine
    acts = (ctypes.c_uint8 * 16)()
    ap = ctypes.cast(acts, ctypes.c_void_p)
    buf = ctypes.create_string_buffer(64)
    fr = native.mg_imagine_out(allo=ctypes.addressof(buf) & ~15)
    fake = ctypes.create_string_buffer(1 << 16)
    h = ctypes.cast(fake, ctypes.c_void_p)
    assert fn(None, ap, 1, 1, None, ctypes.byref(fr), None) == -22 and b"null" in lib.mg_last_error()
    assert fn(h, None, 1, 1, None, ctypes.byref(fr), None) == -22 and b"null" in lib.mg_last_error()
    assert fn(h, ap, 1, 1, None, None, None) == -22 and b"null" in lib.mg_last_error()
    assert fn(h, ap, 1, 1, None, ctypes.byref(native.mg_imagine_out()), None) == -22 and b"no frame" in lib.mg_last_error()
    for H in (0, -1, 4097):
        assert fn(h, ap, H, 1, None, ctypes.byref(fr), None) == -22 and b"[1, 4096]" in lib.mg_last_error(), H
    for H, every in ((4, 0), (4, 5), (4, -1), (1, 2)):
        assert fn(h, ap, H, every, None, ctypes.byref(fr), None) == -22 and b"[1, H]" in lib.mg_last_error(), (H, every)
    assert fn(h, ap, 4, 2, None, ctypes.byref(fr), None) == -22 and b"unwrapped" in lib.mg_last_error()


# ---- the Python wrappers ----------------------------------------------------------------------------------------------
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("library call %s before the arguments were checked" % name)


def _shell(name, n=5):
    """a VecMagicalEnv without a simulator: what imagine() reads before it calls the library"""
    e = object.__new__(envs.VecMagicalEnv)
    e.spec, e.num_envs, e.device, e.lib, e.handle = registry.lookup(name), n, torch.device("cpu"), _NoLibrary(), None
    pp = e.spec.preproc
    e._chw = pp is not None and registry.PREPROCESSORS[pp].get("channels_first", False)
    return e


@pytest.mark.parametrize("bad,kw", [
    (np.zeros((3, 4), np.uint8), {}),                 # env axis is not num_envs
    (np.zeros((2, 3, 5), np.uint8), {}),              # three axes
    (np.zeros((0, 5), np.uint8), {}),                 # H = 0
    (np.zeros((4097, 5), np.uint8), {}),              # H > 4096
    (np.zeros((3, 5), np.float32), {}),               # not integers
    (np.zeros((3, 5), bool), {}),
    (np.zeros((3, 5), np.uint8), {"every": 0}),
    (np.zeros((3, 5), np.uint8), {"every": 4}),
    (np.zeros((3, 5), np.uint8), {"every": 1.5}),
    (np.zeros((3, 5), np.uint8), {"every": True}),
    (np.zeros((3, 5), np.uint8), {"out": {"allo": torch.zeros((3, 5, 96, 96, 3), dtype=torch.float32)}}),
    (np.zeros((3, 5), np.uint8), {"out": {"allo": torch.zeros((2, 5, 96, 96, 3), dtype=torch.uint8)}}),
    (np.zeros((3, 5), np.uint8), {"out": {"past_obs": torch.zeros((3, 5, 96, 96, 12), dtype=torch.uint8)}}),   # stacks=False
])
def test_wrapper_refuses_before_any_library_call(bad, kw):
    with pytest.raises(ValueError):
        _shell("MoveToRegion-Demo-LoRes4E-v0").imagine(bad, **kw)


def test_wrapper_refuses_the_unwrapped_surface():
    with pytest.raises(ValueError, match="LoRes"):
        _shell("MoveToRegion-Demo-v0").imagine(np.zeros((3, 5), np.uint8))


def test_imagine_actions_and_layout():
    a, every, F = envs.imagine_actions(np.arange(35).reshape(7, 5) % 18, 5, 3)
    assert a.dtype == torch.uint8 and tuple(a.shape) == (7, 5) and (every, F) == (3, 3)
    assert envs.imagine_actions(np.zeros(5, np.int64), 5, 1)[2] == 1   # [N] is H = 1
    assert envs.imagine_actions(np.zeros((7, 5), np.int64), 5, np.int64(7))[1:] == (7, 1)
    for pp in ("LoRes4E", "LoResStack", "LoRes3EA", "LoRes4A", "LoResCHW4E", "LoResCHW4A"):
        bufs, keys = envs.imagine_layout(pp, False)
        assert bufs == ["allo", "ego"] and list(keys.items()) == [("allo", "allo"), ("ego", "ego")]
    want = {"LoRes4E": [("allo", "allo"), ("ego", "ego"), ("past_obs", "stack_ego")],
            "LoResCHW4E": [("allo", "allo"), ("ego", "ego"), ("past_obs", "stack_ego")],
            "LoResCHW4A": [("allo", "allo"), ("ego", "ego"), ("past_obs", "stack_ego")],
            "LoRes3EA": [("allo", "allo"), ("ego", "ego"), ("past_obs", "stack_ego")],
            "LoRes4A": [("allo", "allo"), ("ego", "ego"), ("past_obs", "stack_allo")],
            "LoResStack": [("allo", "stack_allo"), ("ego", "stack_ego")]}
    for pp, items in want.items():
        bufs, keys = envs.imagine_layout(pp, True)
        assert list(keys.items()) == items, pp
        assert bufs[:2] == ["allo", "ego"] and set(bufs[2:]) == {b for _, b in items if b.startswith("stack_")}, pp
        # the keys are step()'s for the preprocessor
        spec = registry.lookup("MoveToRegion-Demo-%s-v0" % pp)
        assert list(keys) == list(envs._obs_shapes(spec)), pp


def test_python_surface():
    import inspect
    sig = inspect.signature(envs.VecMagicalEnv.imagine)
    assert list(sig.parameters) == ["self", "actions", "every", "stacks", "details", "out"]
    assert [sig.parameters[k].default for k in ("every", "stacks", "details", "out")] == [1, False, False, None]
    assert hasattr(pipeline.PipelinedVecEnv, "imagine") and hasattr(envs.MagicalEnv, "imagine")
    from magical_amd import dist
    assert not hasattr(dist.ShardedVecEnv, "imagine") and "no imagine()" in dist.ShardedVecEnv.__doc__
