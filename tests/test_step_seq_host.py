"""CPU: the host side of mg_step_seq -- header, ctypes binding, refusals, build units -- and the numpy restatement of
its horizon rule and reward sum that tests/test_step_seq.py checks the GPU against."""
import ctypes
import os
import re

import numpy as np

from magical_amd import build, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement (include/magical_sim.h, mg_step_seq) --------------------------------------------------------
def seq_horizon(R, max_steps, episode_steps):
    """i32[N]: env-steps env e runs in a call of R: R when max_steps <= 0, else min(R, max(left, 1))"""
    es = np.asarray(episode_steps, dtype=np.int64)
    if max_steps <= 0:
        return np.full(es.shape, R, dtype=np.int32)
    return np.minimum(R, np.maximum(max_steps - es, 1)).astype(np.int32)


def seq_done(R, max_steps, episode_steps):
    """bool[N]: step n ends the episode (mg_step: max_steps > 0 and episode_steps + n >= max_steps)"""
    es = np.asarray(episode_steps, dtype=np.int64)
    return (es + seq_horizon(R, max_steps, es) >= max_steps) if max_steps > 0 else np.zeros(es.shape, dtype=bool)


def seq_reward(reward_trace, n):
    """f32[N]: (float)(r_1 + ... + r_n) of reward_trace f64[R][N] (row h = r_{h+1}), summed left to right in double, one
    rounded add each, starting from r_1 itself"""
    return seq_reward_sum(reward_trace, n).astype(np.float32)


def seq_reward_sum(reward_trace, n):
    """f64[N]: the double that seq_reward casts"""
    tr = np.asarray(reward_trace, dtype=np.float64)
    out = np.zeros(tr.shape[1], dtype=np.float64)
    for e in range(tr.shape[1]):
        acc = np.float64(tr[0, e])
        for k in range(1, int(n[e])):
            acc = np.float64(acc + tr[k, e])
        out[e] = acc
    return out


def test_restated_horizon_and_reward():
    L = 12
    es = np.array([11, 9, 5, 0, 12, 15, -3])
    assert seq_horizon(7, L, es).tolist() == [1, 3, 7, 7, 1, 1, 7]
    assert seq_done(7, L, es).tolist() == [True, True, True, False, True, True, False]
    assert seq_horizon(1, L, es).tolist() == [1] * 7 and seq_done(1, L, es).tolist() == [True, False, False, False, True, True, False]
    assert seq_horizon(5, 0, es).tolist() == [5] * 7 and not seq_done(5, 0, es).any()
    tr = np.array([[1e16, 0.25], [1.0, 0.5], [1.0, 9.0]])
    got = seq_reward(tr, np.array([3, 2]))
    assert seq_reward_sum(tr, np.array([3, 2]))[0] == 1e16 != 1e16 + (1.0 + 1.0)   # left to right, one rounded add each
    assert got[0] == np.float32(1e16)
    assert got[1] == np.float32(0.75) and got.dtype == np.float32
    assert seq_reward(np.array([[-0.0]]), np.array([1]))[0].tobytes() == np.float32(-0.0).tobytes()   # n = 1: r_1 itself


# ---- header, binding, build -----------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "magical_sim.h")).read(), flags=re.S)


def test_header_declares_the_call():
    proto = re.search(r"int mg_step_seq\((.*?)\);", _header(), flags=re.S).group(1)
    args = [" ".join(a.split()) for a in proto.split(",")]
    assert args == ["mg_sim *sim", "const uint8_t *actions_dev", "int32_t R", "int32_t *steps_dev", "void *stream"]
    text = open(os.path.join(ROOT, "include", "magical_sim.h")).read()
    doc = text[:text.index("int mg_step_seq(")].rsplit("/*", 1)[1]
    for word in ("u8[R][N]", "1 <= R <= 4096", "min(R, max(left, 1))", "left to right", "ONE render", "-22"):
        assert word in doc, word


def test_binding_matches_the_header():
    assert "mg_step_seq" in native.EXPORTS
    fn = native.load().mg_step_seq
    vp = ctypes.c_void_p
    assert fn.argtypes == [vp, vp, ctypes.c_int32, vp, vp] and fn.restype is ctypes.c_int32


def test_refusals_without_gpu():
    """-22 before any GPU call, as test_abi_argument_validation_without_gpu: null sim, null actions, R = 0, R = 4097"""
    lib = native.load()
    fn = lib.mg_step_seq
    acts = (ctypes.c_uint8 * 4)()
    ap = ctypes.cast(acts, ctypes.c_void_p)
    assert fn(None, ap, 1, None, None) == -22 and b"null" in lib.mg_last_error()
    # a handle that is never dereferenced: the argument checks come before anything reads the sim
    fake = ctypes.create_string_buffer(1 << 16)
    h = ctypes.cast(fake, ctypes.c_void_p)
    assert fn(h, None, 1, None, None) == -22 and b"null" in lib.mg_last_error()
    assert fn(h, ap, 0, None, None) == -22 and b"[1, 4096]" in lib.mg_last_error()
    assert fn(h, ap, 4097, None, None) == -22 and b"[1, 4096]" in lib.mg_last_error()
    assert fn(h, ap, -1, None, None) == -22


def test_build_lists_the_seq_units():
    units = sorted(u for u in build.UNITS if "seq" in u)
    assert units == ["mg_seq_hbm.hip", "mg_seq_quad.hip", "mg_seq_v4.hip"]
    for u in units:
        assert os.path.exists(os.path.join(build.CSRC, u))
        assert "mg_seq.h" in build.UNITS[u] and "mg_stepk.h" in build.UNITS[u] and "mg_lookahead.h" not in build.UNITS[u]
    src = open(os.path.join(build.CSRC, "mg_seq.h")).read()
    assert "step_seq_kernel" in src and "launch_env_kernel<step_seq_kernel<VAR, BLK, false>, VAR, BLK>" in src


def test_python_surface():
    from magical_amd import envs, pipeline, sb3
    import inspect
    assert hasattr(envs.VecMagicalEnv, "step_seq") and hasattr(envs.VecMagicalEnv, "step_repeat")
    assert hasattr(envs.MagicalEnv, "step_seq") and hasattr(pipeline.PipelinedVecEnv, "step_seq")
    assert "frame_skip" in inspect.signature(sb3.MagicalVecEnv.__init__).parameters
