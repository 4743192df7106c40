"""CPU: the helpers the env wrappers share (magical_amd.envs: seq_actions, check_out, scene_tensor, assemble_obs;
magical_amd.pipeline: cat_bits, join).  Every wrapper method goes through them, so their argument handling, error
texts, key order and env order are pinned here once; the GPU side is tests/test_gpu_parity.py."""
import collections

import numpy as np
import pytest
import torch

from magical_amd import envs, native, pipeline, scene as sc

CPU = torch.device("cpu")


def test_seq_actions_shapes_dtype_and_inputs():
    N = 13
    ids = np.arange(4 * N).reshape(4, N) % 18
    for given in (torch.as_tensor(ids), ids, ids.tolist(), torch.as_tensor(ids, dtype=torch.uint8)):   # int64, numpy, list
        a = envs.seq_actions(given, N, "step_seq", "R")
        assert a.dtype == torch.uint8 and tuple(a.shape) == (4, N) and np.array_equal(a.numpy(), ids)
    one = envs.seq_actions(ids[0], N, "lookahead", "H")
    assert one.dtype == torch.uint8 and tuple(one.shape) == (1, N) and np.array_equal(one.numpy()[0], ids[0])
    empty = envs.seq_actions(torch.empty((0, N), dtype=torch.uint8), N, "lookahead", "H", CPU)
    assert empty.dtype == torch.uint8 and tuple(empty.shape) == (0, N)


@pytest.mark.parametrize("fn,letter", [("step_seq", "R"), ("lookahead", "H")])
def test_seq_actions_error_texts(fn, letter):
    for bad, got in ((np.zeros((4, 12), np.uint8), "(4, 12)"), (np.zeros((2, 3, 13), np.uint8), "(2, 3, 13)"), (5, "()")):
        with pytest.raises(ValueError) as e:
            envs.seq_actions(bad, 13, fn, letter)
        assert str(e.value) == f"{fn}: actions must be [{letter}, 13], got {got}"


def test_join_puts_every_key_in_env_order():
    sizes, K, H, J = (4, 4, 5), 3, 2, 2
    n = sum(sizes)
    rs = np.random.RandomState(3)
    whole = collections.OrderedDict([
        ("score", rs.rand(n)), ("scores", rs.rand(K, n)), ("score_trace", rs.rand(H, n)),
        ("bodies", rs.rand(n, 16, 6)), ("counts", rs.randint(0, 9, (n, 4)).astype(np.int32)),
        ("plans", rs.randint(0, 18, (H, K, n)).astype(np.uint8)),
        ("weights", rs.randint(0, 1 << 16, (J, 18, n)).astype(np.uint16))])
    parts, lo = [], 0
    for m in sizes:
        parts.append(collections.OrderedDict(
            (k, torch.from_numpy(np.ascontiguousarray(v[lo:lo + m] if k in ("bodies", "counts") else v[..., lo:lo + m])))
            for k, v in whole.items()))
        lo += m
    out = pipeline.join(parts)
    assert list(out) == list(whole)
    for k, v in whole.items():
        assert out[k].dtype == parts[0][k].dtype and tuple(out[k].shape) == v.shape, k
        assert out[k].numpy().tobytes() == v.tobytes(), k
    assert out["weights"].dtype == torch.uint16


def test_cat_bits_keeps_unsigned_dtypes_and_bytes():
    rs = np.random.RandomState(4)
    keys = [rs.randint(0, 1 << 32, (m, 624), dtype=np.uint64).astype(np.uint32) for m in (4, 4, 5)]
    out = pipeline.cat_bits([torch.from_numpy(k) for k in keys])
    assert out.dtype == torch.uint32 and tuple(out.shape) == (13, 624)
    assert out.numpy().tobytes() == np.concatenate(keys).tobytes()
    w = [rs.randint(0, 1 << 16, (2, 18, m)).astype(np.uint16) for m in (4, 4, 5)]
    out = pipeline.cat_bits([torch.from_numpy(x) for x in w], dim=-1)
    assert out.dtype == torch.uint16 and out.numpy().tobytes() == np.concatenate(w, axis=-1).tobytes()
    pos = [torch.arange(m, dtype=torch.int32) for m in (4, 4, 5)]
    assert torch.equal(pipeline.cat_bits(pos), torch.cat(pos))


def _hwc(n, c, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (n, 6, 5, c)).astype(np.uint8))


@pytest.mark.parametrize("with_target", [False, True])
@pytest.mark.parametrize("with_past", [False, True])
@pytest.mark.parametrize("chw", [False, True])
def test_assemble_obs_key_order_and_permute(with_target, with_past, chw):
    n = 3
    allo, ego, past = _hwc(n, 3, 0), _hwc(n, 3, 1), _hwc(n, 12, 2) if with_past else None
    target = torch.arange(4 * n, dtype=torch.float32).reshape(n, 4) if with_target else None
    out = envs.assemble_obs(allo, ego, past, None, 0, chw, target)
    assert isinstance(out, collections.OrderedDict)
    assert list(out) == ["allo", "ego"] + (list(envs.TARGET_KEYS) if with_target else []) + (["past_obs"] if with_past else [])
    for k, raw in (("allo", allo), ("ego", ego), ("past_obs", past)):
        if raw is not None:
            assert torch.equal(out[k], raw.permute(0, 3, 1, 2) if chw else raw), k
            assert out[k].data_ptr() == raw.data_ptr(), k   # a view, not a copy
    if with_target:   # never permuted
        assert torch.equal(out["target_type"], target[:, 0:1]) and torch.equal(out["target_colour"], target[:, 1:2])
        assert torch.equal(out["target_position"], target[:, 2:4])


def test_assemble_obs_window_stacks():
    n, K, s0 = 2, envs.WINDOW_K, 5
    rs = np.random.RandomState(7)
    ring_a, ring_e = (torch.from_numpy(rs.randint(0, 256, (n, K + 3, 3, 96, 96)).astype(np.uint8)) for _ in range(2))
    frame = torch.zeros((n, 96, 96, 3), dtype=torch.uint8)
    # one ring (the LoRes4E / LoRes4A / CHW family): its stack is past_obs, the frames stay
    for rings, ring in (([None, ring_e], ring_e), ([ring_a, None], ring_a)):
        for chw in (False, True):
            out = envs.assemble_obs(frame, frame, None, rings, s0, chw, None)
            want = envs.window_stack(ring, s0, K)
            assert list(out) == ["allo", "ego", "past_obs"]
            assert torch.equal(out["past_obs"], want.permute(0, 3, 1, 2) if chw else want)
            assert tuple(out["allo"].shape) == ((n, 3, 96, 96) if chw else (n, 96, 96, 3))
    # two rings (LoResStack): the stacks are the views themselves
    out = envs.assemble_obs(None, None, None, [ring_a, ring_e], s0, False, None)
    assert list(out) == ["allo", "ego"]
    assert torch.equal(out["allo"], envs.window_stack(ring_a, s0, K)) and torch.equal(out["ego"], envs.window_stack(ring_e, s0, K))
    # channel c of the stack is plane c % 3 of slot s0 + c // 3
    assert torch.equal(out["ego"][..., 7], ring_e[:, s0 + 2, 1])


def test_scene_tensor_takes_lists_arrays_and_tensors():
    scenes = [sc.demo_scene("MoveToRegion"), sc.demo_scene("PickAndPlace", target_xy=(0.25, -0.75), target_ent=2),
              sc.demo_scene("MoveToCorner")]
    arr = sc.pack(scenes)
    raw = torch.from_numpy(arr.view(np.uint8).copy())
    for in_place in (True, False):
        got = [envs.scene_tensor(x, 3, CPU, in_place=in_place) for x in (scenes, arr, raw)]
        for t in got:
            assert t.dtype == torch.uint8 and tuple(t.shape) == (3 * native.SCENE_DTYPE.itemsize,) and t.is_contiguous()
            assert t.numpy().tobytes() == arr.tobytes()
        for bad in (scenes[:2], arr[:2], raw[:-792], raw.view(torch.int8)):
            with pytest.raises(ValueError):
                envs.scene_tensor(bad, 3, CPU, in_place=in_place)
    assert envs.scene_tensor(raw, 3, CPU) is raw   # used in place
    with pytest.raises(ValueError) as e:
        envs.scene_tensor(arr[:2], 3, CPU)
    assert str(e.value) == "reset_scenes: 2 scenes for 3 envs"
    with pytest.raises(ValueError) as e:
        envs.scene_tensor(raw[::2], 6, CPU)
    assert str(e.value) == f"reset_scenes: a scene tensor must be contiguous uint8 of {6 * 792} bytes on cpu"
    with pytest.raises(ValueError) as e:
        envs.scene_tensor(arr[:2], 3, CPU, in_place=False)
    assert str(e.value) == "reset_scenes: 3 scenes of 792 bytes each"


def test_check_out():
    buf = torch.empty(24, dtype=torch.uint8)
    assert envs.check_out(buf, "snapshot", 24, CPU) is buf
    assert envs.check_out(buf.view(2, 3, 4), "get_scenes", 24, CPU).data_ptr() == buf.data_ptr()   # bytes: any shape
    cube = buf.view(2, 3, 4)
    assert envs.check_out(cube, "sample_plans", (2, 3, 4), CPU) is cube
    bytes_text = "{}: out must be a contiguous uint8 tensor of 24 bytes on cpu"
    for fn in ("get_scenes", "snapshot"):
        for bad in (torch.empty(23, dtype=torch.uint8), torch.empty(24, dtype=torch.int8),
                    torch.empty(48, dtype=torch.uint8)[::2]):
            with pytest.raises(ValueError) as e:
                envs.check_out(bad, fn, 24, CPU)
            assert str(e.value) == bytes_text.format(fn)
    for bad in (buf.view(2, 4, 3), buf, cube.to(torch.int8), torch.empty((2, 3, 8), dtype=torch.uint8)[:, :, ::2]):
        with pytest.raises(ValueError) as e:
            envs.check_out(bad, "sample_plans", (2, 3, 4), CPU)
        assert str(e.value) == "sample_plans: out must be a contiguous uint8 [2, 3, 4] tensor on cpu"
