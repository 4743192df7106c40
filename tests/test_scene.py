"""GPU: explicit scenes (mg_get_scene / mg_reset_scene; VecMagicalEnv.get_scenes / reset_scenes, MagicalEnv.get_scene /
reset_scene, PipelinedVecEnv).  The reference of almost every test is the reset kernel itself, an independent path to the
same state: a handle started by reset() against a handle with other seeds started from a scene.  Comparisons are bit for
bit (byte equality) unless a test says otherwise.  N = 70 for the robot scenes (more than one wavefront of envs, a ragged
last step workgroup at 8 envs per workgroup), N = 5 for the many-block tasks.
"""
import numpy as np
import pytest
import torch

from magical_amd import envs as mg_envs, native, registry, scene as sc, tables
from magical_amd.pipeline import PipelinedVecEnv

pytestmark = pytest.mark.gpu

TASKS = list(registry.TASK_IDS)
ROBOT_SCENES = ("MoveToRegion", "MoveToCorner")
CSD = registry.COLOUR | registry.SHAPE_TYPE | registry.DYNAMICS
T = 30
L = 100   # episode length of the handles: no episode ends inside a test's T steps unless the test wants it


def nenvs(task):
    return 70 if task in ROBOT_SCENES else 5


def name_of(task, variant="Demo"):
    return f"{task}-{variant}-{'LoResStack' if task.startswith('Cluster') else 'LoRes4E'}-v0"


def make(task, seed, variant="Demo", n=None, **kw):
    kw.setdefault("max_episode_steps", L)
    return mg_envs.VecMagicalEnv(name_of(task, variant), n or nenvs(task), base_seed=seed, **kw)


def actions(n):
    return torch.as_tensor(np.random.RandomState(42).randint(0, 18, (T, n)), dtype=torch.uint8)


def raw(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


def state(env, obs):
    """everything the issue compares: bodies with counts, arbiters, error flags, every bound observation, H = 0 scores"""
    bodies, counts = env.bodies()
    arb, hs = env.arbiters()
    out = {"bodies": raw(bodies), "counts": raw(counts), "arbiters": raw(arb), "hashes": raw(hs), "errors": raw(env.errors()),
           "score": raw(env.score())}
    for k, v in obs.items():
        out["obs." + k] = raw(v)
    return out


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], f"{what}: {k} differs"


def run_both(A, B, obs_a, obs_b, what):
    """A and B agree now, in reward / done / eval_score of each of the same T steps, and afterwards"""
    assert_same(state(A, obs_a), state(B, obs_b), what + " at reset")
    acts = actions(A.num_envs)
    for t in range(T):
        obs_a, ra, da, ia = A.step(acts[t])
        obs_b, rb, db, ib = B.step(acts[t])
        assert raw(ra) == raw(rb) and raw(da) == raw(db) and raw(ia["eval_score"]) == raw(ib["eval_score"]), (what, t)
    assert_same(state(A, obs_a), state(B, obs_b), what + f" after {T} steps")


def demo_scenes(task, A):
    """the Demo scene for every env of A; what the Demo variant itself draws from the RNG (MoveToCorner's robot
    position, PickAndPlace's target) is taken from A"""
    arr = sc.pack([sc.demo_scene(task)] * A.num_envs)
    got = A.get_scenes()
    if task == "MoveToCorner":
        arr["ent"]["x"][:, 0], arr["ent"]["y"][:, 0] = got["ent"]["x"][:, 0], got["ent"]["y"][:, 0]
    if task == "PickAndPlace":
        arr["target_ent"], arr["target_xy"] = got["target_ent"], got["target_xy"]
    return arr, got


@pytest.mark.parametrize("task", TASKS)
def test_demo_scene_equals_the_reset_kernel(task):
    """The registered PickAndPlace-Demo draws colours, shape types and a full layout (registry.py: it has no variant
    without): its handles here take rand_flags = 0, the task's constants, which is what demo_scene states."""
    kw = {"rand_flags": 0} if task == "PickAndPlace" else {}
    A, B = make(task, 1000, **kw), make(task, 5000, **kw)
    obs_a = A.reset()
    arr, got = demo_scenes(task, A)
    assert arr.tobytes() == got.tobytes(), "demo_scene is not what the Demo reset builds"
    obs_b, status = B.reset_scenes(arr)
    assert status.tolist() == [0] * A.num_envs
    assert B.get_scenes().tobytes() == arr.tobytes()
    run_both(A, B, obs_a, obs_b, task)
    A.close(), B.close()


@pytest.mark.parametrize("task", ["MoveToCorner", "ClusterColour", "MatchRegions", "FindDupe", "FixColour", "PickAndPlace"])
def test_round_trip_on_layout_fixed_randomised_variants(task):
    """colour | shape type | dynamics, Demo layout: the derived roles and PickAndPlace's target show in the scores"""
    A, B = make(task, 1000, rand_flags=CSD), make(task, 5000, rand_flags=CSD)
    obs_a = A.reset()
    arr = A.get_scenes()
    assert len({r.tobytes() for r in arr}) > 1, "the variant draws nothing"
    for s in sc.unpack(arr):
        assert sc.validate(s, task, CSD) == 0
    obs_b, status = B.reset_scenes(arr)
    assert status.tolist() == [0] * A.num_envs
    assert B.get_scenes().tobytes() == arr.tobytes()
    run_both(A, B, obs_a, obs_b, task)
    A.close(), B.close()


@pytest.mark.parametrize("task,variant", [("MatchRegions", "TestAll"), ("ClusterColour", "TestLayout")])
def test_round_trip_on_layout_randomised_variants(task, variant):
    """The sampler's chain of rigid shifts cannot be rebuilt from one pose: block bodies and the robot's root body are
    bit-equal, the robot's other bodies within 1e-9 (the project's body-state tolerance; the true difference is a few
    roundings of numbers below 2).  Entity tables, counts and error flags are equal.  Nothing is claimed after stepping."""
    A, B = make(task, 1000, variant), make(task, 5000, variant)
    A.reset()
    arr = A.get_scenes()
    _, status = B.reset_scenes(arr)
    assert status.tolist() == [0] * A.num_envs
    assert B.get_scenes().tobytes() == arr.tobytes()   # kinds, types, colours, enabled flags, root poses, goals, pv
    (ba, ca), (bb, cb) = A.bodies(), B.bodies()
    assert raw(ca) == raw(cb) and raw(A.errors()) == raw(B.errors())
    ba, bb = ba.cpu().numpy(), bb.cpu().numpy()
    for e in range(A.num_envs):
        rb = int(ca[e, 0]) - 6   # the robot is added last: its 6 bodies end the table
        assert ba[e, :rb + 1].tobytes() == bb[e, :rb + 1].tobytes(), e   # blocks and the robot's root body
        diff = np.abs(ba[e, rb + 1:rb + 6] - bb[e, rb + 1:rb + 6]).max()
        print(f"{task} env {e}: other robot bodies differ by at most {diff:.3e}")
        assert diff <= 1e-9, e
    A.close(), B.close()


def test_mid_episode_capture():
    A = make("MoveToRegion", 1000)
    A.reset()
    acts = actions(A.num_envs)
    for t in range(20):
        A.step(acts[t])
    arr = A.get_scenes()
    moved = sc.pack([sc.demo_scene("MoveToRegion")] * A.num_envs)
    assert arr.tobytes() != moved.tobytes()
    rng = [raw(x) for x in A.rng_state()]
    obs, status = A.reset_scenes(arr)
    assert status.tolist() == [0] * A.num_envs
    assert [raw(x) for x in A.rng_state()] == rng
    bodies, counts = A.bodies()
    bodies = bodies.cpu().numpy()
    assert np.array_equal(bodies[:, 0, 0], arr["ent"]["x"][:, 1]) and np.array_equal(bodies[:, 0, 1], arr["ent"]["y"][:, 1])
    assert np.array_equal(bodies[:, 0, 2], arr["ent"]["angle"][:, 1])
    assert not bodies[:, :, 3:6].any()                       # velocities
    assert not counts[:, 3].any() and not A.arbiters()[0].any()   # the arbiter table
    assert A.lookahead(torch.zeros((L + 5, A.num_envs), dtype=torch.uint8))["steps"].tolist() == [L] * A.num_envs   # episode_steps 0
    # finger and drive targets cleared: the handle goes on exactly as one that never stepped before the same scene
    B = make("MoveToRegion", 5000)
    obs_b, _ = B.reset_scenes(arr)
    run_both(A, B, obs, obs_b, "mid-episode capture")
    A.close(), B.close()


def records(env):
    """every env's one-record snapshot blob (the state section of a blob of several is row-major; into a zeroed blob: a
    record's padding bytes are not written)"""
    out = []
    for e in range(env.num_envs):
        blob = torch.zeros(env.snapshot_bytes(1), dtype=torch.uint8, device=env.device)
        out.append(env.snapshot(envs=[e], out=blob).tobytes())
    return out


def test_masks_and_refusals():
    n = 70
    A = make("ClusterColour", 1000, n=n)
    obs = A.reset()
    acts = actions(n)
    for t in range(3):
        obs, *_ = A.step(acts[t])
    scenes = [sc.demo_scene("ClusterColour") for _ in range(n)]
    for s in scenes:
        s.ents[-1].x = 0.6   # not the layout the envs are in
    scenes[3].ents[2].colour = 9                                  # a bad enum
    scenes[64].ents = scenes[64].ents[:1] + scenes[64].ents       # a ninth block: one too many for the handle
    assert sc.validate(scenes[3], "ClusterColour") == 2 and sc.validate(scenes[64], "ClusterColour") == 3
    mask = torch.zeros(n, dtype=torch.bool)
    mask[[0, 3, 64, 69]] = True
    before, obs_before = records(A), {k: v.clone() for k, v in obs.items()}
    obs2, status = A.reset_scenes(scenes, mask=mask)
    want = np.full(n, -1)
    want[[0, 3, 64, 69]] = [0, 2, 3, 0]
    assert status.tolist() == want.tolist()
    after = records(A)
    for e in range(n):
        same = before[e] == after[e]
        same_obs = all(raw(obs2[k][e]) == raw(obs_before[k][e]) for k in obs2)
        assert same == same_obs == (e not in (0, 69)), e
    got = A.get_scenes()
    want_arr = sc.pack(scenes)
    assert got[0].tobytes() == want_arr[0].tobytes() and got[69].tobytes() == want_arr[69].tobytes()
    # the envs built are the ones a second handle builds from the same scene
    B = make("ClusterColour", 5000, n=n)
    obs_b, _ = B.reset_scenes([scenes[0]] * n)
    for k in obs2:
        assert raw(obs2[k][0]) == raw(obs_b[k][0]) and raw(obs2[k][69]) == raw(obs_b[k][69]), k
    # refusals launch nothing: the state and the status buffer keep their bytes
    lib, st = A.lib, A._stream()
    t = A._scene_tensor(want_arr)
    status = torch.full((n,), 77, dtype=torch.int32, device=A.device)
    p = lambda x: None if x is None else __import__("ctypes").c_void_p(x.data_ptr())   # noqa: E731
    assert lib.mg_reset_scene(None, p(t), None, 0, p(status), st) == -22
    assert lib.mg_reset_scene(A.handle, None, None, 0, p(status), st) == -22
    assert lib.mg_reset_scene(A.handle, p(t), None, 0, None, st) == -22
    assert lib.mg_reset_scene(A.handle, p(t), None, 2, p(status), st) == -22
    assert lib.mg_reset_scene(A.handle, p(t), None, -1, p(status), st) == -22
    assert lib.mg_get_scene(A.handle, None, st) == -22 and lib.mg_get_scene(None, p(t), st) == -22
    assert status.tolist() == [77] * n and records(A) == after
    A.close(), B.close()


def test_unbound_outputs_are_refused():
    import ctypes
    A = make("MoveToRegion", 1000, n=2)
    cfg, h = A._cfg, ctypes.c_void_p()
    native.check(A.lib.mg_create(ctypes.byref(cfg), ctypes.byref(h)))   # a second sim, never bound
    t = A._scene_tensor(sc.pack([sc.demo_scene("MoveToRegion")] * 2))
    status = torch.full((2,), 77, dtype=torch.int32, device=A.device)
    assert A.lib.mg_reset(h, None, A._stream()) == -22
    assert A.lib.mg_reset_scene(h, ctypes.c_void_p(t.data_ptr()), None, 0, ctypes.c_void_p(status.data_ptr()), A._stream()) == -22
    assert status.tolist() == [77, 77]
    A.lib.mg_destroy(h)
    A.close()


def test_check_flags_overlaps():
    n = 5
    A = make("ClusterColour", 1000)
    scenes = [sc.demo_scene("ClusterColour") for _ in range(n)]
    # env 1: every entity at least 0.05 clear of the others and of the walls.  A block reaches 0.156 from its centre (a
    # star's outer radius), the robot's fingers less than 0.42 (0.02 + upper arm 0.22 + forearm 0.14, half a thickness):
    # two rows of four blocks, 0.45 and 0.5 apart, and the robot alone 0.65 above them, 0.5 below the wall
    grid = [(-0.68 + 0.45 * i, -0.65 + 0.5 * j) for j in range(2) for i in range(4)]
    for t, (x, y) in zip(scenes[1].ents[:8], grid):
        t.x, t.y = x, y
    scenes[1].ents[8].x, scenes[1].ents[8].y = 0.0, 0.5
    # env 3: two blocks 0.05 apart
    scenes[3] = scenes[1].copy()
    scenes[3].ents[1].x, scenes[3].ents[1].y = scenes[3].ents[0].x + 0.05, scenes[3].ents[0].y
    scenes[0] = scenes[2] = scenes[4] = scenes[1]
    _, status = A.reset_scenes(scenes, check=True)
    assert status.tolist() == [0] * n
    assert A.errors().tolist() == [0, 0, 0, 2 | 64, 0]
    B = make("ClusterColour", 5000)
    _, status = B.reset_scenes(scenes, check=False)
    assert status.tolist() == [0] * n and B.errors().tolist() == [0] * n
    assert raw(A.bodies()[0]) == raw(B.bodies()[0])   # check builds the same envs
    # a wall is an overlap too, and the single env raises
    E = mg_envs.MagicalEnv(name_of("MoveToRegion"))
    s = sc.demo_scene("MoveToRegion")
    E.reset_scene(s, check=True)
    assert E.get_scene() == s
    s.ents[1].x = 0.95
    with pytest.raises(mg_envs.PlacementError):
        E.reset_scene(s, check=True)
    E.reset_scene(s)
    s.ents[1].x = 1.5
    with pytest.raises(ValueError, match="status 2"):
        E.reset_scene(s)
    assert E.get_scene().ents[1].x == 0.95   # a refused scene leaves the env as it was
    E.close()
    A.close(), B.close()


def test_scores_see_the_scene():
    n = 70
    A = make("MoveToRegion", 1000)
    scenes = [sc.demo_scene("MoveToRegion") for _ in range(n)]
    for e in range(0, n, 2):
        scenes[e].ents[1].x, scenes[e].ents[1].y = scenes[e].ents[0].x, scenes[e].ents[0].y   # at the goal's centre
    for e in range(1, n, 2):
        scenes[e].ents[1].x, scenes[e].ents[1].y = 0.9, -0.9
    _, status = A.reset_scenes(scenes)
    assert status.tolist() == [0] * n
    assert A.score().tolist() == [1.0, 0.0] * (n // 2)
    A.close()


def test_shadow_and_auto_reset_untouched():
    """ClusterColour with layout randomisation and auto_reset runs on the next-layout shadow.  Replacing env 2's layout
    at step 10 consumes none of its RNG: the layouts of every env's later auto-resets are the undisturbed run's."""
    n, steps, ep = 5, 40, 12
    runs = []
    for replace in (False, True):
        A = make("ClusterColour", 1000, "TestLayout", max_episode_steps=ep)
        A.reset()
        acts = torch.as_tensor(np.random.RandomState(7).randint(0, 18, (steps, n)), dtype=torch.uint8)
        layouts = [[] for _ in range(n)]
        for t in range(steps):
            if replace and t == 10:
                mask = torch.zeros(n, dtype=torch.bool)
                mask[2] = True
                _, status = A.reset_scenes([sc.demo_scene("ClusterColour")] * n, mask=mask)
                assert status.tolist() == [-1, -1, 0, -1, -1]
            _, _, done, _ = A.step(acts[t])
            got = A.get_scenes()
            for e in np.nonzero(done.cpu().numpy())[0]:
                layouts[e].append((t, got[e].tobytes()))
        runs.append(layouts)
        A.close()
    plain, replaced = runs
    for e in range(n):
        if e != 2:
            assert plain[e] == replaced[e] and len(plain[e]) == 3, e
    assert [t for t, _ in plain[2]] == [11, 23, 35] and [t for t, _ in replaced[2]] == [21, 33]
    assert [s for _, s in replaced[2]] == [s for _, s in plain[2]][:2]
    assert len({s for _, s in plain[2]}) == 3   # and they are different layouts


@pytest.mark.parametrize("mode", ["window", "frames_only", "pipelined", "unwrapped"])
def test_modes(mode):
    n = 70
    A, arr = make("MoveToRegion", 1000), None
    obs_a = A.reset()
    arr = sc.pack([sc.demo_scene("MoveToRegion")] * n)
    acts = actions(n)
    if mode == "window":
        B = make("MoveToRegion", 5000, window=True)
    elif mode == "pipelined":
        B = PipelinedVecEnv(name_of("MoveToRegion"), n, chunks=3, base_seed=5000, max_episode_steps=L)
    elif mode == "unwrapped":
        A.close()
        A = mg_envs.VecMagicalEnv("MoveToRegion-Demo-v0", 3, base_seed=1000, max_episode_steps=L)
        B = mg_envs.VecMagicalEnv("MoveToRegion-Demo-v0", 3, base_seed=5000, max_episode_steps=L)
        obs_a, arr, acts = A.reset(), arr[:3], acts[:, :3]
    else:
        B = make("MoveToRegion", 5000)
        views = {k: torch.zeros_like(v) for k, v in B.output_buffers().items() if k != "past_obs"}
        B.bind_outputs(views, frames_only=True)
    obs_b, status = B.reset_scenes(arr)
    assert status.tolist() == [0] * A.num_envs
    if mode == "pipelined":
        assert B.get_scenes().tobytes() == arr.tobytes()
    keys = ("allo", "ego") if mode == "frames_only" else tuple(obs_a)
    for t in range(T + 1):
        if mode == "pipelined":
            B.wait()
        for k in keys:
            assert raw(obs_a[k]) == raw(obs_b[k]), (mode, t, k)
        if t < T:
            obs_a, ra, da, _ = A.step(acts[t])
            obs_b, rb, db, _ = B.step(acts[t])
            if mode == "pipelined":
                B.wait()
            assert raw(ra) == raw(rb) and raw(da) == raw(db)
    if mode == "pipelined":
        for s in B.sims:
            s.close()
    else:
        B.close()
    A.close()
