"""Gym-style surfaces over the GPU simulator.

* VecMagicalEnv -- N instances of one registered name on one GPU (batched
  counterpart of gym.make(name) under SB3's DummyVecEnv, train_rl.py:87-92):
  reset() -> dict of uint8 device tensors, step(actions) -> (obs, reward f32,
  done bool, {'eval_score': f64}); finished episodes auto-reset in place.
* MagicalEnv -- one instance with the single-env gym API of
  BaseEnv + preprocessors (base_env.py:190-351, benchmarks/__init__.py:51-190):
  numpy observations, done at max_episode_steps, explicit reset().

Every tensor VecMagicalEnv.reset()/step() returns (observations, reward, done,
info values) is one of the simulator's bound output buffers: it is valid until
the next reset()/step() rewrites it (clone it to keep it).  The frame stacks
(LoRes4E / LoRes4A / CHW past_obs, LoResStack allo / ego) are contiguous [N, 96, 96,
12] tensors; window=True makes them strided views of per-view window rings on the
device instead (mg_bind_window: each frame written once, channel-planar; the stack =
4 consecutive slots; the same values, shape and dtype, channel stride 96 * 96) --
measured 4-7% slower in the render kernel than the materialised stacks, whose
writes hide under the kernel's latency.
"""
import collections
import ctypes

import numpy as np
import torch

from . import native, registry, spaces, tables
from .planning import as_objective

_LIBRARY = None


def library():
    global _LIBRARY
    if _LIBRARY is None:
        _LIBRARY = tables.build_library()
    return _LIBRARY


def _obs_shapes(spec):
    pp = spec.preproc
    if pp is None:
        return collections.OrderedDict([("allo", (384, 384, 3)), ("ego", (384, 384, 3))])
    if pp == "LoResStack":
        return collections.OrderedDict([("allo", (96, 96, 12)), ("ego", (96, 96, 12))])
    cf = registry.PREPROCESSORS[pp]["channels_first"]
    shapes = collections.OrderedDict([("allo", (96, 96, 3)), ("ego", (96, 96, 3)), ("past_obs", (96, 96, 12))])
    if cf:
        shapes = collections.OrderedDict((k, (s[2], s[0], s[1])) for k, s in shapes.items())
    return shapes


# PickAndPlace observation extras (pick_and_place.py:23-28), inserted after allo/ego by the base env
# and therefore before the frame stack's past_obs (benchmarks/__init__.py:124-147)
TARGET_KEYS = ("target_type", "target_colour", "target_position")


WINDOW_K = 8   # window ring period: K + 3 slots per env and stacked view (magical_amd.dist uses the same)


def window_views(spec):
    """(allo, ego): which views of a preprocessor are frame stacks a window ring can hold (LoRes3EA's stack is
    allo + 3 ego frames: not one ring's window)."""
    pp = spec.preproc
    return (pp in ("LoResStack", "LoRes4A"), pp in ("LoResStack", "LoRes4E", "LoResCHW4E", "LoResCHW4A"))


def window_stack(ring, s0, K=WINDOW_K):
    """[n, 96, 96, 12] stack view of a window ring u8[n, K + 3, 3, 96, 96] at first slot s0 (include/magical_sim.h
    mg_bind_window): channel c = plane c % 3 of slot s0 + c // 3."""
    fr = 96 * 96 * 3
    return ring.as_strided((ring.shape[0], 96, 96, 12), ((K + 3) * fr, 96, 1, 96 * 96), ring.storage_offset() + s0 * fr)


def observation_space(spec):
    items = [(k, spaces.Box(low=0, high=255, shape=s, dtype=np.uint8)) for k, s in _obs_shapes(spec).items()]
    if spec.task == "PickAndPlace":
        extra = [("target_type", spaces.Box(low=0, high=4, shape=(1,), dtype=np.float32)),
                 ("target_colour", spaces.Box(low=0, high=4, shape=(1,), dtype=np.float32)),
                 ("target_position", spaces.Box(low=-1, high=1, shape=(2,), dtype=np.float32))]
        items = items[:2] + extra + items[2:]
    return spaces.Dict(collections.OrderedDict(items))


def plan_actions(actions, num_envs):
    """plan()'s candidate actions as a uint8 [H, K, num_envs] tensor ([K, num_envs] is H = 1), on the device they came
    on; ValueError for any other shape, no candidate at all, or more rollouts than one mg_plan call takes."""
    a = torch.as_tensor(actions)
    if a.dim() == 2:
        a = a[None]
    if a.dim() != 3 or a.shape[2] != num_envs:
        raise ValueError(f"plan: actions must be [H, K, {num_envs}], got {tuple(a.shape)}")
    if a.shape[1] < 1:
        raise ValueError("plan: at least one candidate per env (K >= 1)")
    if a.shape[1] * num_envs > native.PLAN_MAX_ROLLOUTS:
        raise ValueError(f"plan: K * num_envs = {a.shape[1] * num_envs} rollouts, more than {native.PLAN_MAX_ROLLOUTS}")
    return a.to(torch.uint8)


def _plan_fields(n, K, details, score="score"):
    """(name, shape, dtype) of the results plan / plan_cem / plan_beam share: the three-entry head and, with details,
    the [K, n] triple; the planners call the per-candidate number a score, the beam a value"""
    head = [("best", (n,), torch.int32), ("best_" + score, (n,), torch.float64), ("first_action", (n,), torch.uint8)]
    return head + ([(score + "s", (K, n), torch.float64), ("steps", (K, n), torch.int32),
                    ("errors", (K, n), torch.int32)] if details else [])


def seq_actions(actions, num_envs, fn, letter, device=None):
    """step_seq()'s and lookahead()'s actions as a uint8 [X, num_envs] tensor ([num_envs] is X = 1) on `device` (None:
    where they came from); ValueError, naming `fn` and the axis `letter`, for any other shape."""
    a = torch.as_tensor(actions)
    if a.dim() == 1:
        a = a[None]
    if a.dim() != 2 or a.shape[1] != num_envs:
        raise ValueError(f"{fn}: actions must be [{letter}, {num_envs}], got {tuple(a.shape)}")
    return a.to(device=device, dtype=torch.uint8)


def imagine_actions(actions, num_envs, every, device=None):
    """imagine()'s arguments checked on the host: (actions as a uint8 [H, num_envs] tensor on `device`, every, F =
    ceil(H / every)); ValueError for actions that are not integers, any other shape, H outside [1, 4096] or `every`
    outside [1, H]."""
    a = torch.as_tensor(actions)
    if a.dtype.is_floating_point or a.dtype.is_complex or a.dtype == torch.bool:
        raise ValueError(f"imagine: actions must be integer action ids, got {a.dtype}")
    a = seq_actions(a, num_envs, "imagine", "H", device)
    H = int(a.shape[0])
    if not 1 <= H <= 4096:
        raise ValueError(f"imagine: H must be in [1, 4096], got {H}")
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or not 1 <= int(every) <= H:
        raise ValueError(f"imagine: every must be an integer in [1, {H}], got {every!r}")
    return a, int(every), -(-H // int(every))


def imagine_layout(preproc, stacks):
    """Which of mg_imagine_out's buffers imagine() fills for a preprocessor, and where the observation keys come from:
    (buffer names, OrderedDict key -> buffer name).  stacks=False: the 3-channel current frames of both views.
    stacks=True: the keys step() returns -- LoResStack's allo and ego are the stacks (built from the plain frames, which
    are filled too), the others' past_obs is the stack of their stacked view (LoRes3EA: allo_f | three ego frames)."""
    if preproc is None:
        raise ValueError("imagine: the unwrapped 384^2 surface has no LoRes frame")
    keys = collections.OrderedDict([("allo", "allo"), ("ego", "ego")])
    if stacks:
        if preproc == "LoResStack":
            keys = collections.OrderedDict([("allo", "stack_allo"), ("ego", "stack_ego")])
        else:
            keys["past_obs"] = "stack_allo" if preproc == "LoRes4A" else "stack_ego"
    return ["allo", "ego"] + [b for b in keys.values() if b.startswith("stack_")], keys


def check_out(out, fn, shape, device):
    """An out= argument: `out` if it is a contiguous uint8 tensor on `device` of `shape` (an int: so many bytes in any
    shape), else ValueError."""
    flat = isinstance(shape, int)
    if ((out.numel() != shape) if flat else (tuple(out.shape) != tuple(shape))) or out.dtype != torch.uint8 \
            or out.device != device or not out.is_contiguous():
        what = f"tensor of {shape} bytes" if flat else f"{list(shape)} tensor"
        raise ValueError(f"{fn}: out must be a contiguous uint8 {what} on {device}")
    return out


def scene_tensor(scenes, num_envs, device, in_place=True):
    """reset_scenes()'s `scenes` -- a list of scene.Scene, a structured array of native.SCENE_DTYPE or a uint8 tensor --
    as a flat uint8 tensor of num_envs * 792 bytes on `device`.  in_place: a tensor must already be that and is
    returned as it is (VecMagicalEnv); otherwise it is flattened and moved there (the pool, which slices it per chunk)."""
    size = native.SCENE_DTYPE.itemsize
    if isinstance(scenes, torch.Tensor):
        ok = scenes.numel() == num_envs * size and scenes.dtype == torch.uint8
        if not in_place:
            if not ok:
                raise ValueError(f"reset_scenes: {num_envs} scenes of {size} bytes each")
            return scenes.reshape(-1).to(device).contiguous()
        if not ok or scenes.device != device or not scenes.is_contiguous():
            raise ValueError(f"reset_scenes: a scene tensor must be contiguous uint8 of {num_envs * size} bytes on {device}")
        return scenes
    if not isinstance(scenes, np.ndarray):
        from .scene import pack
        scenes = pack(list(scenes))
    arr = np.ascontiguousarray(scenes, dtype=native.SCENE_DTYPE).reshape(-1)
    if arr.shape[0] != num_envs:
        raise ValueError(f"reset_scenes: {arr.shape[0]} scenes for {num_envs} envs" if in_place
                         else f"reset_scenes: {num_envs} scenes of {size} bytes each")
    return torch.from_numpy(arr.view(np.uint8)).to(device)


def assemble_obs(allo, ego, past, rings, s0, chw, target):
    """The observation dict both env classes return, from the raw HWC buffers.  rings: None, or the (allo, ego) window
    rings whose stacks at first slot s0 stand in for buffers -- two rings (LoResStack) are the allo and ego stacks
    themselves, one is past_obs.  chw: the image keys become CHW views.  target: PickAndPlace's [n, 4] float32 target
    (SB3's DummyVecEnv buffers it as float32, per the spaces) or None.  Key order: allo, ego, target keys, past_obs."""
    if rings is not None:
        stacks = [None if r is None else window_stack(r, s0, r.shape[1] - 3) for r in rings]
        if stacks[0] is not None and stacks[1] is not None:
            allo, ego = stacks
        else:
            past = stacks[0] if stacks[0] is not None else stacks[1]
    out = collections.OrderedDict([("allo", allo), ("ego", ego)])
    if target is not None:
        out["target_type"], out["target_colour"], out["target_position"] = target[:, 0:1], target[:, 1:2], target[:, 2:4]
    if past is not None:
        out["past_obs"] = past
    if chw:
        for k in ("allo", "ego", "past_obs"):
            if k in out:
                out[k] = out[k].permute(0, 3, 1, 2)
    return out


class VecMagicalEnv:
    """Batched MAGICAL env on one MI355X (C ABI: include/magical_sim.h)."""

    def __init__(self, env_name, num_envs, device="cuda:0", seeds=None, base_seed=0, auto_reset=True,
                 max_episode_steps=None, debug_reward=None, window=False, rand_flags=None):
        self.spec = registry.lookup(env_name)
        if not self.spec.gpu_supported:
            raise NotImplementedError(f"{env_name}: task not on the GPU hot path yet")
        pp = self.spec.preproc
        if self.spec.task == "PickAndPlace" and pp == "LoResStack":
            # EagerDictFrameStack concatenates every observation value along the last axis; the
            # scalar target_type / target_colour make that raise in the reference as well
            raise ValueError(f"{env_name}: the reference cannot frame-stack PickAndPlace's scalar observations")
        # rand_flags: a variant the registry has no name for (registry.LAYOUT_MINOR .. DYNAMICS bits) in place of the
        # name's own, e.g. colour | shape type | dynamics with the Demo layout
        flags = self.spec.rand_flags if rand_flags is None else int(rand_flags)
        if debug_reward is not None:  # gym.make(name, debug_reward=...)
            flags = (flags | registry.DEBUG_REWARD) if debug_reward else (flags & ~registry.DEBUG_REWARD)
        self.debug_reward = bool(flags & registry.DEBUG_REWARD)
        self.rand_flags = flags
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        self.lib = native.load()
        self._chw = pp is not None and registry.PREPROCESSORS[pp].get("channels_first", False)
        gpu_pp = {None: 0, "LoRes4E": 1, "LoResStack": 2, "LoRes3EA": 3, "LoRes4A": 4, "LoResCHW4E": 1, "LoResCHW4A": 1}[pp]
        cfg = native.mg_config()
        cfg.task = self.spec.task_id
        cfg.rand_flags = flags
        cfg.preproc = gpu_pp
        cfg.num_envs = self.num_envs
        cfg.device = self.device.index or 0
        self.max_episode_steps = int(max_episode_steps or self.spec.max_episode_steps)
        cfg.max_episode_steps = self.max_episode_steps
        cfg.base_seed = base_seed
        cfg.auto_reset = 1 if auto_reset else 0
        if seeds is not None:
            self._seeds = (ctypes.c_uint32 * self.num_envs)(*[int(s) & 0xffffffff for s in seeds])
            cfg.seeds = self._seeds
        lib_struct = library()
        cfg.library = ctypes.cast(ctypes.pointer(lib_struct), ctypes.c_void_p)
        cfg.library_size = ctypes.sizeof(tables.mg_library)
        torch.cuda.init()
        handle = ctypes.c_void_p()
        native.check(self.lib.mg_create(ctypes.byref(cfg), ctypes.byref(handle)))
        self.handle = handle
        self._cfg = cfg   # (mg_snapshot_bytes sizes a blob from it)
        n, dev = self.num_envs, self.device
        u8 = dict(dtype=torch.uint8, device=dev)
        wa, we = window_views(self.spec) if window and pp is not None else (False, False)
        self.window_k = WINDOW_K if (wa or we) else 0
        self.wring = [None, None]
        if self.window_k:
            shape = (n, self.window_k + 3, 3, 96, 96)
            self.wring = [torch.zeros(shape, **u8) if wa else None, torch.zeros(shape, **u8) if we else None]
        if pp is None:
            self.full = torch.empty((n, 2, 384, 384, 3), **u8)
            self.obs_allo = self.obs_ego = self.obs_past = None
        elif pp == "LoResStack":
            self.obs_allo = None if wa else torch.empty((n, 96, 96, 12), **u8)
            self.obs_ego = None if we else torch.empty((n, 96, 96, 12), **u8)
            self.obs_past = None
        else:
            self.obs_allo = torch.empty((n, 96, 96, 3), **u8)
            self.obs_ego = torch.empty((n, 96, 96, 3), **u8)
            self.obs_past = None if self.window_k else torch.empty((n, 96, 96, 12), **u8)
        self.reward = torch.zeros(n, dtype=torch.float32, device=dev)
        self.done = torch.zeros(n, dtype=torch.bool, device=dev)  # the C ABI writes u8 0/1: same bytes
        self.eval_score = torch.zeros(n, dtype=torch.float64, device=dev)
        self.seq_steps = None   # step_seq's info['steps'] i32[n] (not a bound output): allocated by the first step_seq
        self.target = torch.zeros((n, 4), dtype=torch.float64, device=dev) if self.spec.task == "PickAndPlace" else None
        self.frames_only = False
        self.reset_count = 0   # explicit reset() calls (magical_amd.dist checks its frame rings against it)
        if self.window_k:
            self._bind_window()
        self._bind()
        self.action_space = spaces.Discrete(18)
        self.observation_space = observation_space(self.spec)

    # -- helpers -----------------------------------------------------------
    def _bind(self):
        buf = native.mg_buffers()
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        buf.obs_allo, buf.obs_ego, buf.obs_past = ptr(self.obs_allo), ptr(self.obs_ego), ptr(self.obs_past)
        buf.reward, buf.done, buf.eval_score = ptr(self.reward), ptr(self.done), ptr(self.eval_score)
        buf.target = ptr(self.target)
        buf.frames_only = 1 if self.frames_only else 0
        native.check(self.lib.mg_bind_outputs(self.handle, ctypes.byref(buf)))

    def _bind_window(self):
        ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        native.check(self.lib.mg_bind_window(self.handle, ptr(self.wring[0]), ptr(self.wring[1]), self.window_k))

    def bind_window(self, ring_allo, ring_ego):
        """Use caller-owned window rings u8[n, K + 3, 3, 96, 96] (e.g. slices of a pool's rings: every env of a
        magical_amd.pipeline pool in one ring) instead of this env's own; before the next reset()."""
        if not self.window_k:
            raise ValueError("bind_window: this env materialises its stacks (window=False or no stacked view)")
        self.wring = [ring_allo if self.wring[0] is not None else None, ring_ego if self.wring[1] is not None else None]
        self._bind_window()

    def window_start(self):
        """First slot of the current outputs' window (mg_window_start)."""
        s0 = ctypes.c_int32()
        native.check(self.lib.mg_window_start(self.handle, ctypes.byref(s0)))
        return s0.value

    def bind_outputs(self, views, frames_only=False, target=None):
        """Write the following steps' outputs into caller-owned device tensors (e.g. views into one packed
        buffer per step, magical_amd.dist.PackedLayout): keys as output_buffers().  frames_only: 'allo' /
        'ego' receive only the current [n, 96, 96, 3] frames for every LoRes preprocessor (no stacks;
        magical_amd.dist's compact gather restacks on the receivers) -- changing the mode needs a reset.
        PickAndPlace's target (written only at reset) stays in the env's own persistent buffer (views["target"]
        is ignored: a per-step packed buffer would hold a stale one), unless `target` names a persistent [n, 4]
        f64 tensor to use instead -- bind it before the reset that fills it (magical_amd.pipeline)."""
        if self.spec.preproc is None:
            raise ValueError("bind_outputs: the unwrapped 384^2 view is rendered on demand, not bound")
        self.obs_allo, self.obs_ego = views.get("allo"), views.get("ego")   # (window-ring stacks: not bound)
        self.obs_past = None if frames_only else views.get("past_obs")
        self.reward, self.done, self.eval_score = views["reward"], views["done"], views["eval_score"]
        if self.target is not None and target is not None:
            self.target = target
        self.frames_only = bool(frames_only)
        self._bind()

    def output_buffers(self):
        """The currently bound output tensors: raw (HWC) observation buffers, reward, done, eval_score[, target]."""
        out = collections.OrderedDict((k, v) for k, v in (("allo", self.obs_allo), ("ego", self.obs_ego)) if v is not None)
        if self.obs_past is not None:
            out["past_obs"] = self.obs_past
        out["reward"], out["done"], out["eval_score"] = self.reward, self.done, self.eval_score
        if self.target is not None:
            out["target"] = self.target
        return out

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _obs(self):
        if self.spec.preproc is None:
            allo, ego, past = self.full[:, 0], self.full[:, 1], None
        else:
            allo, ego, past = self.obs_allo, self.obs_ego, self.obs_past
        windowed = self.window_k and not self.frames_only
        return assemble_obs(allo, ego, past, self.wring if windowed else None, self.window_start() if windowed else 0,
                            self._chw, None if self.target is None else self.target.to(torch.float32))

    def _finish(self):
        """the tail of every call that changes what the envs show: the observation, the unwrapped view rendered first"""
        if self.spec.preproc is None:
            self.render_full(out=self.full)
        return self._obs()

    def _alloc(self, fields, zeros=()):
        """fresh result tensors on the device from (name, shape, dtype) triples, uninitialised but for `zeros`"""
        return collections.OrderedDict(
            (name, (torch.zeros if name in zeros else torch.empty)(shape, dtype=dtype, device=self.device))
            for name, shape, dtype in fields)

    # -- API -----------------------------------------------------------------
    def seed(self, seeds):
        arr = (ctypes.c_uint32 * self.num_envs)(*[int(s) & 0xffffffff for s in seeds])
        native.check(self.lib.mg_seed(self.handle, arr))
        return list(seeds)

    def reset(self, mask=None):
        m = None if mask is None else ctypes.c_void_p(mask.to(self.device, torch.uint8).contiguous().data_ptr())
        native.check(self.lib.mg_reset(self.handle, m, self._stream()))
        self.reset_count += 1
        return self._finish()

    def step(self, actions):
        a = actions
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.uint8 and a.device == self.device and a.is_contiguous()):
            a = torch.as_tensor(actions).to(self.device, torch.uint8).contiguous()
        self._last_actions = a
        native.check(self.lib.mg_step(self.handle, ctypes.c_void_p(a.data_ptr()), self._stream()))
        return self._finish(), self.reward, self.done, {"eval_score": self.eval_score}

    def step_seq(self, actions):
        """Several env-steps per call with one render (frame skip; mg_step_seq).  actions: [R, N] uint8 (tensor or
        array-like; [N] is R = 1), step h of env e at actions[h, e], 1 <= R <= 4096.  Env e runs n = min(R, steps left
        in its episode, at least 1) env-steps, bit-identical to as many step() calls, stops at its terminal step and is
        auto-reset as step() would; then every env is rendered ONCE, so the frame stacks hold the frames seen at call
        boundaries.  Returns (obs, reward, done, info): reward is the float32 of the n rewards summed in double, done
        says whether step n ended the episode, info holds 'eval_score' (the score at that step, else 0) and 'steps'
        i32[N] (n).  step_seq(a[None]) is step(a)."""
        a = seq_actions(actions, self.num_envs, "step_seq", "R", self.device).contiguous()
        self._last_actions = a   # (alive until the next call: the kernel reads it on the stream)
        if self.seq_steps is None:   # (no fill: the kernel writes every env's element)
            self.seq_steps = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        native.check(self.lib.mg_step_seq(self.handle, ctypes.c_void_p(a.data_ptr()), int(a.shape[0]),
                                          ctypes.c_void_p(self.seq_steps.data_ptr()), self._stream()))
        return self._finish(), self.reward, self.done, {"eval_score": self.eval_score, "steps": self.seq_steps}

    def step_repeat(self, actions, repeat):
        """step_seq with every env's action held for `repeat` env-steps (action repeat).  actions: [N] uint8."""
        a = torch.as_tensor(actions)
        if a.dim() != 1 or a.shape[0] != self.num_envs:
            raise ValueError(f"step_repeat: actions must be [{self.num_envs}], got {tuple(a.shape)}")
        a = a.to(self.device, torch.uint8)
        return self.step_seq(a[None].expand(int(repeat), -1).contiguous())

    def random_actions(self, step, key=42, out=None):
        out = out if out is not None else torch.empty(self.num_envs, dtype=torch.uint8, device=self.device)
        native.check(self.lib.mg_random_actions(self.handle, ctypes.c_void_p(out.data_ptr()), key, step, self._stream()))
        return out

    def set_episode_steps(self, steps):
        """Overwrite every env's episode step counter (throughput runs stagger episode phases)."""
        s = torch.as_tensor(steps).to(self.device, torch.int32).contiguous()
        native.check(self.lib.mg_set_episode_steps(self.handle, ctypes.c_void_p(s.data_ptr()), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()

    def render_full(self, out=None):
        out = out if out is not None else torch.empty((self.num_envs, 2, 384, 384, 3), dtype=torch.uint8,
                                                      device=self.device)
        native.check(self.lib.mg_render_full(self.handle, ctypes.c_void_p(out.data_ptr()), self._stream()))
        return out

    def bodies(self):
        out = torch.empty((self.num_envs, 16, 6), dtype=torch.float64, device=self.device)
        counts = torch.empty((self.num_envs, 4), dtype=torch.int32, device=self.device)
        native.check(self.lib.mg_get_bodies(self.handle, ctypes.c_void_p(out.data_ptr()),
                                            ctypes.c_void_p(counts.data_ptr()), self._stream()))
        return out, counts

    def rng_state(self):
        """every env's MT19937 state as numpy's RandomState.get_state()[1:3]: (key uint32 [N, 624], pos int32 [N])
        device tensors (mg_get_rng; pyoracle.OracleEnv.rng_state() per env)"""
        key = torch.empty((self.num_envs, 624), dtype=torch.uint32, device=self.device)
        pos = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        native.check(self.lib.mg_get_rng(self.handle, ctypes.c_void_p(key.data_ptr()), ctypes.c_void_p(pos.data_ptr()),
                                         self._stream()))
        return key, pos

    def step_form(self):
        """(form, envs per workgroup, (bodies, shapes, constraints, arbiter slots) caps) of the step kernel
        (mg_step_form)"""
        out = (ctypes.c_int32 * 6)()
        native.check(self.lib.mg_step_form(self.handle, out))
        return int(out[0]), int(out[1]), tuple(int(x) for x in out[2:6])

    def arbiters(self):
        """solved arbiters per env in active order: f64 [N, 48, 28] and contact hashes u64 [N, 48, 2]
        (mg_get_arbiters; the active count is bodies()[1][:, 3])"""
        out = torch.empty((self.num_envs, 48, 28), dtype=torch.float64, device=self.device)
        hs = torch.empty((self.num_envs, 48, 2), dtype=torch.uint64, device=self.device)
        native.check(self.lib.mg_get_arbiters(self.handle, ctypes.c_void_p(out.data_ptr()),
                                              ctypes.c_void_p(hs.data_ptr()), self._stream()))
        return out, hs

    def set_body_pose(self, env, body, x, y, angle):
        """Place body `body` of env `env` (Body.position / Body.angle setters; parity tests)."""
        native.check(self.lib.mg_set_body_pose(self.handle, int(env), int(body), float(x), float(y), float(angle),
                                               self._stream()))

    def errors(self):
        out = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        native.check(self.lib.mg_get_errors(self.handle, ctypes.c_void_p(out.data_ptr()), self._stream()))
        return out

    # -- explicit scenes ---------------------------------------------------------
    def get_scenes(self, out=None):
        """Every env's CURRENT layout as a structured array [N] of native.SCENE_DTYPE (mg_get_scene; scene.unpack turns
        it into Scene objects): entity table, each entity's pose as it stands, goal geometry, physics variables,
        PickAndPlace's target.  Read-only.  out: a contiguous uint8 device tensor of N * 792 bytes to fill instead, in
        which case that tensor is returned and nothing is copied to the host."""
        nbytes = self.num_envs * native.SCENE_DTYPE.itemsize
        buf = (torch.empty(nbytes, dtype=torch.uint8, device=self.device) if out is None
               else check_out(out, "get_scenes", nbytes, self.device))
        native.check(self.lib.mg_get_scene(self.handle, ctypes.c_void_p(buf.data_ptr()), self._stream()))
        if out is not None:
            return out
        return buf.cpu().numpy().view(native.SCENE_DTYPE).copy()

    def _scene_tensor(self, scenes):
        return scene_tensor(scenes, self.num_envs, self.device)

    def reset_scenes(self, scenes, mask=None, check=False):
        """Start envs from given layouts (mg_reset_scene): a masked reset() whose layouts are `scenes` -- a structured
        array [N] of native.SCENE_DTYPE, a list of N scene.Scene, or a uint8 device tensor of N * 792 bytes used in
        place -- instead of the variant's draws.  Returns (obs, status): status i32[N] on the device, 0 built, -1 not
        selected by `mask` (bool / uint8 [N]; None: every env), > 0 refused and left untouched (scene.STATUS_TEXT;
        scene.validate gives the same code on the host).  check=True runs the reset's overlap test on the built envs:
        one with overlapping entities gets error flags 2 | 64 (errors()), and is built all the same.  The envs' RNG
        streams are not consumed: their next auto-reset draws what it would have drawn."""
        t = self._scene_tensor(scenes)
        m = None if mask is None else torch.as_tensor(mask).to(self.device, torch.uint8).contiguous()
        status = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
        self._last_scenes = (t, m)   # (alive until the next call: the kernel reads them on the stream)
        native.check(self.lib.mg_reset_scene(self.handle, ctypes.c_void_p(t.data_ptr()),
                                             None if m is None else ctypes.c_void_p(m.data_ptr()), 1 if check else 0,
                                             ctypes.c_void_p(status.data_ptr()), self._stream()))
        self.reset_count += 1
        return self._finish(), status

    # -- snapshots ---------------------------------------------------------------
    def snapshot_bytes(self, n=None):
        """Bytes of a snapshot blob of n (default: all) envs of this env (mg_snapshot_bytes; no GPU work)."""
        nbytes = self.lib.mg_snapshot_bytes(ctypes.byref(self._cfg), self.num_envs if n is None else int(n))
        if nbytes < 0:
            native.check(int(nbytes))
        return int(nbytes)

    def snapshot(self, envs=None, out=None):
        """Record the state of the envs in `envs` (a sequence of indices; default: every env in order) into a
        `magical_amd.snapshot.Snapshot` on this device: record k holds env envs[k] -- physics, RNG stream, episode
        phase, frame stacks, everything that makes `restore` + the same actions bit-identical to not having
        stopped.  Enqueued on the current stream.  The outputs must still hold the latest observation (they are
        the env's own buffers unless bind_outputs replaced them).  Not with window=True or frames_only outputs
        (NativeError).  Host-side state of wrappers is not part of it: magical_amd.sb3.MagicalVecEnv's Monitor
        statistics and dist.ShardedVecEnv's rings / ranks are out of scope.  out: a uint8 device tensor of
        snapshot_bytes(n) bytes to fill instead of a new one."""
        from .snapshot import Snapshot
        n = self.num_envs if envs is None else len(envs)
        nbytes = self.snapshot_bytes(n)
        blob = (torch.empty(nbytes, dtype=torch.uint8, device=self.device) if out is None
                else check_out(out, "snapshot", nbytes, self.device))
        arr = None if envs is None else (ctypes.c_int32 * n)(*[int(e) for e in envs])
        native.check(self.lib.mg_snapshot(self.handle, arr, n, ctypes.c_void_p(blob.data_ptr()), self._stream()))
        return Snapshot(blob, count=n)

    def restore(self, snap, envs=None, recs=None):
        """Put recorded envs back: env envs[k] <- record recs[k] of `snap` (recs default 0, 1, ..; it may repeat a
        record to broadcast it; envs default 0 .. n-1, else distinct), and return the observation, in which the
        restored envs show what they showed when recorded (reward / done / eval_score describe a step and keep
        their values).  A `PoolSnapshot` of a PipelinedVecEnv with the same env order restores every env (envs and
        recs must be None).  The blob's header is checked on the host and again by the library against this env's
        task, variant flags and preprocessor: a mismatch, a truncated blob or a bad index raises NativeError and
        leaves the env untouched.  Synchronises the current stream once (the header check)."""
        from .snapshot import PoolSnapshot
        if isinstance(snap, PoolSnapshot):
            if envs is not None or recs is not None or len(snap) != self.num_envs:
                raise ValueError("restore: a PoolSnapshot restores every env of a batch of the same size, in order")
            for k, chunk in enumerate(snap.chunks):
                self._restore(chunk, range(snap.bounds[k], snap.bounds[k + 1]), None)
        else:
            self._restore(snap, envs, recs)
        return self._finish()

    def _restore(self, snap, envs, recs):
        if snap.device != self.device:
            snap = snap.to(self.device)
        snap.header   # host-side check: magic, version, truncation
        if envs is not None and recs is not None and len(envs) != len(recs):
            raise ValueError("restore: envs and recs must have the same length")
        n = len(envs) if envs is not None else len(recs) if recs is not None else len(snap)
        ea = None if envs is None else (ctypes.c_int32 * n)(*[int(e) for e in envs])
        ra = None if recs is None else (ctypes.c_int32 * n)(*[int(r) for r in recs])
        native.check(self.lib.mg_restore(self.handle, ctypes.c_void_p(snap.blob.data_ptr()), ea, ra, n, self._stream()))

    # -- lookahead ---------------------------------------------------------------
    def _objective_struct(self, objective, fn):
        """the mg_objective of an `objective=` argument that is not None"""
        o = as_objective(objective, fn)
        return native.mg_objective(kind=o.kind_id, reserved=0, gamma=o.gamma, tail=o.tail)

    def lookahead(self, actions, bodies=False, objective=None, trace=False):
        """What happens if these envs run these actions -- without touching them (mg_lookahead).  actions: [H, N]
        uint8 (tensor or array-like; [N] is H = 1; H = 0, an empty [0, N], scores the current states), step h of env e
        at actions[h, e].  Every env runs min(H, steps left in its episode) env-steps of physics only (no render, no
        auto-reset) on a scratch copy of its state, bit-identical to as many step() calls, and is then scored.
        Returns fresh device tensors: 'score' f64[N] (the task's score of the final state; eval_score where the
        episode ends inside the horizon), 'steps' i32[N] (env-steps simulated), 'errors' i32[N] (errors() as it
        would stand); with bodies=True also 'bodies' f64[N, 16, 6] and 'counts' i32[N, 4] of the final state, as
        bodies().  The env itself -- state, RNG, episode phase, frames, outputs -- is unchanged.  Enqueued on the
        current stream; works with window=True and frames_only outputs.
        objective (a magical_amd.Objective; mg_lookahead_obj) adds 'value' f64[N] (the objective's value of the
        rollout), 'peak' f64[N] (the best discounted score at any step, the entry state included) and 'peak_step'
        i32[N] (the first step that reached it; 0: the entry state).  trace=True adds 'score_trace' f64[H, N] (the
        score after step h + 1, held at the final score past the env's last step) and 'reward_trace' f64[H, N] (the
        reward step() would pay at step h + 1 before its cast to float32, 0 past the env's last step); without an
        objective the traces are those of Objective('final').  With neither, nothing changes."""
        a = seq_actions(actions, self.num_envs, "lookahead", "H", self.device).contiguous()
        n, f64, i32 = self.num_envs, torch.float64, torch.int32
        res = self._alloc([("score", (n,), f64), ("steps", (n,), i32), ("errors", (n,), i32)]
                          + ([("bodies", (n, 16, 6), f64), ("counts", (n, 4), i32)] if bodies else []))
        out = native.mg_lookahead_out(**{k: v.data_ptr() for k, v in res.items()})
        ap, H = ctypes.c_void_p(a.data_ptr()) if a.shape[0] else None, int(a.shape[0])
        if objective is None and not trace:
            native.check(self.lib.mg_lookahead(self.handle, ap, H, ctypes.byref(out), self._stream()))
        else:
            obj = self._objective_struct("final" if objective is None else objective, "lookahead")
            extra = self._alloc(
                ([("value", (n,), f64), ("peak", (n,), f64), ("peak_step", (n,), i32)] if objective is not None else [])
                + ([("score_trace", (H, n), f64), ("reward_trace", (H, n), f64)] if trace else []))
            oo = native.mg_objective_out(**{k: v.data_ptr() for k, v in extra.items() if v.numel()})
            native.check(self.lib.mg_lookahead_obj(self.handle, ap, H, ctypes.byref(obj), ctypes.byref(out),
                                                   ctypes.byref(oo), self._stream()))
            res.update(extra)
        self._last_lookahead = a   # (alive until the next call: the kernel reads it on the stream)
        return res

    def score(self):
        """f64[N]: the task's score (score_on_end_of_traj) of every env's current state, mid-episode or not -- a
        zero-step lookahead."""
        return self.lookahead(torch.empty((0, self.num_envs), dtype=torch.uint8))["score"]

    def imagine(self, actions, every=1, stacks=False, details=False, out=None):
        """What the agent would SEE if these envs ran these actions -- without touching them (mg_imagine): lookahead()'s
        rollout, rendered after every `every` env-steps.  actions: [H, N] integer action ids (tensor or array-like; [N]
        is H = 1), 1 <= H <= 4096, 1 <= every <= H; F = ceil(H / every) frames per env.  Frame f of env e is the LoRes
        current frame of its state after min((f + 1) * every, n) env-steps, n = min(H, steps left in its episode): the
        bytes the f+1-th of F successive step_seq(actions[f * every:(f + 1) * every]) calls would show within the
        episode.  An env whose episode ends inside the horizon stops there (no auto-reset) and repeats its terminal
        frame.  Returns an OrderedDict of fresh uint8 device tensors with a leading F axis: stacks=False gives 'allo' and
        'ego', the 3-channel current frames [F, N, 96, 96, 3]; stacks=True gives the keys step() returns for the
        preprocessor -- LoResStack 'allo' and 'ego' [F, N, 96, 96, 12], the others 'allo', 'ego' and 'past_obs' [F, N,
        96, 96, 12] -- where a stack holds the four newest frames up to frame f, oldest first, the env's real history
        before frame 0 (after a terminal step the repeated frame keeps entering the stack: such stacks correspond to no
        real step).  Channels-first preprocessors return permuted views, as step() does.  details=True adds 'score',
        'steps' and 'errors' -- and 'bodies' and 'counts' of the final state -- bit for bit lookahead(actions,
        bodies=True)'s (errors also carries a render capacity flag raised while drawing).
        out: a dict of contiguous HWC uint8 tensors to fill instead, keyed like the result.  stacks=True needs the
        env's own frame history: NativeError with window=True or frames_only outputs; plain frames work in every mode.
        Enqueued on the current stream."""
        a, every, F = imagine_actions(actions, self.num_envs, every, self.device)
        bufs, keys = imagine_layout(self.spec.preproc, stacks)
        n = self.num_envs
        shape = {b: (F, n, 96, 96, 12 if b.startswith("stack_") else 3) for b in bufs}
        if out is not None and not set(out) <= set(keys):
            raise ValueError(f"imagine: out has keys {sorted(set(out) - set(keys))}, the result has {list(keys)}")
        given = {} if out is None else {keys[k]: check_out(v, "imagine", shape[keys[k]], self.device) for k, v in out.items()}
        mem = {b: given[b] if b in given else torch.empty(shape[b], dtype=torch.uint8, device=self.device) for b in bufs}
        fr = native.mg_imagine_out(**{b: t.data_ptr() for b, t in mem.items()})
        a = a.contiguous()
        res = self._alloc([("score", (n,), torch.float64), ("steps", (n,), torch.int32), ("errors", (n,), torch.int32),
                           ("bodies", (n, 16, 6), torch.float64), ("counts", (n, 4), torch.int32)] if details else [])
        lo = native.mg_lookahead_out(**{k: v.data_ptr() for k, v in res.items()}) if details else None
        native.check(self.lib.mg_imagine(self.handle, ctypes.c_void_p(a.data_ptr()), int(a.shape[0]), every,
                                         None if lo is None else ctypes.byref(lo), ctypes.byref(fr), self._stream()))
        self._last_imagine = a   # (alive until the next call: the kernels read it on the stream)
        obs = collections.OrderedDict((k, mem[b].permute(0, 1, 4, 2, 3) if self._chw else mem[b]) for k, b in keys.items())
        obs.update(res)
        return obs

    # -- planning ----------------------------------------------------------------
    def plan(self, actions, details=False, objective=None):
        """Which of K candidate action sequences is best for each env -- without touching the envs (mg_plan).
        actions: [H, K, N] uint8 (tensor or array-like; [K, N] is H = 1; an empty [0, K, N] scores the current states K
        times), step h of candidate k of env e at actions[h, k, e].  Candidate k of env e is exactly
        lookahead(actions[:, k])[e]; all K * N rollouts run as one grid on a fan pool the sim owns.  Returns fresh
        device tensors: 'best' i32[N] (the candidate with the highest score, the lowest k on ties), 'best_score'
        f64[N], 'first_action' u8[N] (actions[0, best[e], e]; zeros when H = 0); with details=True also 'scores'
        f64[K, N], 'steps' i32[K, N] and 'errors' i32[K, N] as lookahead's.  Error flags do not exclude a candidate.
        Enqueued on the current stream, except that a call needing a larger fan pool than the last allocates it and
        synchronises the device.
        objective (a magical_amd.Objective; mg_plan_obj): 'scores' and 'best_score' hold the objective's value --
        lookahead(actions[:, k], objective=objective)['value'] -- and 'best' is chosen on it."""
        a = plan_actions(actions, self.num_envs).to(self.device).contiguous()
        H, K = int(a.shape[0]), int(a.shape[1])
        res = self._alloc(_plan_fields(self.num_envs, K, details), zeros=("first_action",))   # (zeros: H = 0 writes none)
        out = native.mg_plan_out(**{k: v.data_ptr() for k, v in res.items()})
        ap = ctypes.c_void_p(a.data_ptr()) if H else None
        if objective is None:
            native.check(self.lib.mg_plan(self.handle, ap, H, K, ctypes.byref(out), self._stream()))
        else:
            obj = self._objective_struct(objective, "plan")
            native.check(self.lib.mg_plan_obj(self.handle, ap, H, K, ctypes.byref(obj), ctypes.byref(out), self._stream()))
        self._last_plan = a   # (alive until the next call: the kernels read it on the stream)
        return res

    def sample_plans(self, H, K, repeat=1, key=42, step=0, out=None):
        """u8[H, K, N] random-shooting candidates for plan() (mg_plan_sample): every action is held for `repeat`
        env-steps, and with J = ceil(H / repeat) the row [h, k] equals random_actions(step + k * J + h // repeat, key)."""
        H, K = int(H), int(K)
        if out is None:
            out = torch.empty((max(H, 0), max(K, 0), self.num_envs), dtype=torch.uint8, device=self.device)
        check_out(out, "sample_plans", (H, K, self.num_envs), self.device)   # (a negative H or K fails here, too)
        # (H = 0: the call checks K and repeat and writes nothing, but refuses a null pointer)
        buf = out if out.numel() else torch.empty(1, dtype=torch.uint8, device=self.device)
        native.check(self.lib.mg_plan_sample(self.handle, ctypes.c_void_p(buf.data_ptr()), H, K, int(repeat), int(key),
                                             int(step), self._stream()))
        return out

    def plan_cem(self, H, K, iters, elites, alpha=1, repeat=1, key=42, step=0, weights=None, details=False,
                 objective=None):
        """Cross-entropy planning on the device (mg_plan_cem): `iters` rounds of K candidate sequences of H env-steps
        per env (each action held for `repeat` steps, J = ceil(H / repeat) slots), every round rolled out as plan()
        does, the per-env, per-slot action weights refitted to its `elites` best candidates (alpha + elite counts)
        and, from the second round on, candidate 0 the best sequence so far.  Round i draws at counters step +
        (i * K + k) * J + slot: a call consumes iters * K * J of them.  weights=None starts uniform; a contiguous
        uint16 [J, 18, N] tensor on the env's device is the warm start and is updated in place.  Returns fresh device
        tensors: 'best' i32[N] (index into the last round's candidates), 'best_score' f64[N], 'first_action' u8[N],
        'plan' u8[H, N] (the best sequence), 'weights' u16[J, 18, N] (the given tensor when one was given),
        'iter_best' f64[iters, N]; with details=True also 'actions' u8[H, K, N] (the last round's candidates) and
        their 'scores' f64[K, N], 'steps' i32[K, N], 'errors' i32[K, N].  The envs are untouched, as by plan().
        objective (a magical_amd.Objective; mg_plan_cem_obj): every round is plan(objective=objective), so the scores,
        'best_score' and 'iter_best' are the objective's values and the elites and the incumbent are chosen on them."""
        obj = None if objective is None else self._objective_struct(objective, "plan_cem")
        H, K, iters, repeat, n, dev = int(H), int(K), int(iters), int(repeat), self.num_envs, self.device
        if H < 1 or K < 1 or iters < 1 or repeat < 1:
            raise ValueError("plan_cem: H, K, iters and repeat must be at least 1")
        if K * n > native.PLAN_MAX_ROLLOUTS:
            raise ValueError(f"plan_cem: K * num_envs = {K * n} rollouts, more than {native.PLAN_MAX_ROLLOUTS}")
        J = -(-H // repeat)
        warm = weights is not None
        if not warm:
            weights = torch.empty((J, 18, n), dtype=torch.uint16, device=dev)
        elif (not torch.is_tensor(weights) or tuple(weights.shape) != (J, 18, n) or weights.dtype != torch.uint16
                or weights.device != dev or not weights.is_contiguous()):
            raise ValueError(f"plan_cem: weights must be a contiguous uint16 [{J}, 18, {n}] tensor on {dev}")
        acts = torch.empty((H, K, n), dtype=torch.uint8, device=dev)
        res = self._alloc(_plan_fields(n, K, details) + [("iter_best", (iters, n), torch.float64)])
        out = native.mg_plan_cem_out(**{k: v.data_ptr() for k, v in res.items()})
        args = (self.handle, ctypes.c_void_p(acts.data_ptr()), ctypes.c_void_p(weights.data_ptr()), int(warm), H, K, iters,
                int(elites), int(alpha), repeat, int(key), int(step))
        if obj is None:
            native.check(self.lib.mg_plan_cem(*args, ctypes.byref(out), self._stream()))
        else:
            native.check(self.lib.mg_plan_cem_obj(*args, ctypes.byref(obj), ctypes.byref(out), self._stream()))
        plan = acts.gather(1, res["best"].long()[None, None, :].expand(H, 1, n))[:, 0]
        ordered = collections.OrderedDict([(k, res[k]) for k in ("best", "best_score", "first_action")])
        ordered["plan"], ordered["weights"], ordered["iter_best"] = plan, weights, res["iter_best"]
        if details:
            ordered["actions"] = acts
            for k in ("scores", "steps", "errors"):
                ordered[k] = res[k]
        return ordered

    def plan_beam(self, actions, seg, survivors, details=False, objective=None):
        """Beam search over action segments on the device (mg_plan_beam): plan() that prunes while it rolls out.
        actions: [H, K, N] uint8 as plan()'s, H >= 1.  After every `seg` env-steps but the last segment's, each env
        keeps its `survivors` slots with the highest value (the lower k first among equal values) where they are and
        overwrites loser j, in ascending k, with a copy of survivor j mod survivors; slot k then goes on with its own
        actions[h, k].  Returns fresh device tensors: 'best' i32[N] (the slot of the best lineage after the last
        segment, the lowest k on ties), 'best_value' f64[N], 'first_action' u8[N], 'plan' u8[H, N] (that lineage's
        actions); with details=True also 'plans' u8[H, K, N] (column (k, e): the actions of the lineage that ends in
        slot k -- plan(plans) reproduces 'values', 'steps' and 'errors'), 'values' f64[K, N], 'steps' i32[K, N],
        'errors' i32[K, N], 'depth_values' f64[D, K, N] (D = ceil(H / seg): the values after every segment, before its
        resample) and 'parents' i32[D - 1, K, N] (the slot each slot was copied from; k itself for a survivor).
        survivors == K or seg >= H is plan(actions).  The envs are untouched, as by plan().  objective (a
        magical_amd.Objective): the values are the objective's, continued from segment to segment."""
        obj = None if objective is None else self._objective_struct(objective, "plan_beam")
        a = plan_actions(actions, self.num_envs)
        H, K, n, dev = int(a.shape[0]), int(a.shape[1]), self.num_envs, self.device
        seg, survivors = int(seg), int(survivors)
        if H < 1:
            raise ValueError("plan_beam: at least one step (H >= 1)")
        if not 1 <= seg <= H:
            raise ValueError(f"plan_beam: seg must be in [1, {H}], got {seg}")
        if not 1 <= survivors <= K:
            raise ValueError(f"plan_beam: survivors must be in [1, {K}], got {survivors}")
        a = a.to(dev).contiguous()
        D = -(-H // seg)
        plans = torch.empty((H, K, n), dtype=torch.uint8, device=dev)
        res = self._alloc(_plan_fields(n, K, details, "value") + [("best_plan", (H, n), torch.uint8)]
                          + ([("depth_values", (D, K, n), torch.float64), ("parents", (D - 1, K, n), torch.int32)]
                             if details else []))
        out = native.mg_plan_beam_out(**{k: v.data_ptr() for k, v in res.items() if v.numel()})
        native.check(self.lib.mg_plan_beam(self.handle, ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(plans.data_ptr()),
                                           H, K, seg, survivors, None if obj is None else ctypes.byref(obj),
                                           ctypes.byref(out), self._stream()))
        self._last_plan = a   # (alive until the next call: the kernels read it on the stream)
        ordered = collections.OrderedDict([(k, res[k]) for k in ("best", "best_value", "first_action")])
        ordered["plan"] = res["best_plan"]
        if details:
            ordered["plans"] = plans
            for k in ("values", "steps", "errors", "depth_values", "parents"):
                ordered[k] = res[k]
        return ordered

    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.lib.mg_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PlacementError(Exception):
    """geom.py:111: raised by reset() when the layout randomiser gives up (after 10 retries)."""


class MagicalEnv:
    """Single instance with the reference's gym.Env surface (numpy observations)."""

    metadata = {"render.modes": ["rgb_array"]}

    def __init__(self, env_name, device="cuda:0", seed=None, debug_reward=None):
        self.spec = registry.lookup(env_name)
        self._vec = VecMagicalEnv(env_name, 1, device=device, auto_reset=False, debug_reward=debug_reward)
        self.max_episode_steps = self.spec.max_episode_steps
        self.action_space = spaces.Discrete(18)
        self.observation_space = observation_space(self.spec)
        self._episode_steps = None
        self.seed(seed)

    def seed(self, seed=None):
        """base_env.py:134-141: RandomState(seed); None draws from the global numpy RNG."""
        if seed is None:
            seed = np.random.randint(0, (1 << 31) - 1)
        self._vec.seed([seed])
        return [seed]

    def action_to_flags(self, int_action):
        return ACTION_ID_TO_FLAGS[int(int_action)]

    def flags_to_action(self, flags):
        return FLAGS_TO_ACTION_ID[tuple(flags)]

    def _require_reset(self, fn):
        if self._episode_steps is None:
            raise RuntimeError(f"call reset() before {fn}()")

    @staticmethod
    def _candidates(actions, fn):
        """[H, K] action ids as the one-env vec env's uint8 [H, K, 1]"""
        a = torch.as_tensor(np.asarray(actions), dtype=torch.uint8)
        if a.dim() != 2:
            raise ValueError(f"{fn}: actions must be [H, K], got {tuple(a.shape)}")
        return a[:, :, None]

    def _np_obs(self, obs):
        out = collections.OrderedDict()
        for k, v in obs.items():
            if k in TARGET_KEYS:  # pick_and_place.py:103-107: python ints and a float64 array
                t = self._vec.target[0].cpu().numpy()
                out[k] = int(t[0]) if k == "target_type" else int(t[1]) if k == "target_colour" else t[2:4].copy()
            else:
                out[k] = v[0].cpu().numpy()
        return out

    def reset(self):
        self._episode_steps = 0
        obs = self._np_obs(self._vec.reset())
        if int(self._vec.errors()[0].item()) & 2:  # pm_randomise_all_poses raised (geom.py:335-336)
            raise PlacementError("could not place entities after 10 layout retries (geom.py:295-341)")
        return obs

    def get_scene(self):
        """The current layout as a scene.Scene (VecMagicalEnv.get_scenes for this one env)."""
        from .scene import unpack
        return unpack(self._vec.get_scenes())[0]

    def reset_scene(self, scene, check=False):
        """reset() from a given layout (a scene.Scene): ValueError naming the status for a refused scene, which leaves
        the env as it was; with check=True, PlacementError when entities overlap (the env is built all the same)."""
        from .scene import STATUS_TEXT
        obs, status = self._vec.reset_scenes([scene], check=check)
        st = int(status[0].item())
        if st != 0:
            raise ValueError(f"reset_scene: status {st}: {STATUS_TEXT.get(st, 'unknown')}")
        self._episode_steps = 0
        obs = self._np_obs(obs)
        if check and int(self._vec.errors()[0].item()) & 2:
            raise PlacementError("reset_scene: entities of the scene overlap (status 0, error flags 2 | 64)")
        return obs

    def step(self, action):
        self._require_reset("step")
        obs, rew, done, info = self._vec.step(torch.tensor([int(action)], dtype=torch.uint8))
        self._episode_steps += 1
        d = bool(done[0].item())
        score = float(info["eval_score"][0].item())
        return self._np_obs(obs), float(rew[0].item()), d, {"eval_score": score}

    def step_seq(self, actions):
        """Run `actions` (a sequence of 1 .. 4096 action ids) as env-steps, stopping at the episode's end, and render
        once: (obs, summed reward, done, {'eval_score', 'steps': env-steps run}) -- VecMagicalEnv.step_seq for this
        one env."""
        self._require_reset("step_seq")
        a = torch.as_tensor(list(actions), dtype=torch.uint8).reshape(-1, 1)
        obs, rew, done, info = self._vec.step_seq(a)
        n = int(info["steps"][0].item())
        self._episode_steps += n
        return self._np_obs(obs), float(rew[0].item()), bool(done[0].item()), \
            {"eval_score": float(info["eval_score"][0].item()), "steps": n}

    def score(self):
        """The task's score (score_on_end_of_traj) of the current state, at any point of the episode; step() reports
        it as info['eval_score'] only on the step that ends one."""
        self._require_reset("score")
        return float(self._vec.score()[0].item())

    def lookahead(self, actions, objective=None, trace=False):
        """Score of the state after running `actions` (a sequence of action ids, cut at the episode's end) from the
        current state, which stays as it is: (score, env-steps simulated).  With an objective (a
        magical_amd.Objective) or trace=True the result is a dict instead: 'score' and 'steps' as above, with an
        objective 'value', 'peak' (floats) and 'peak_step' (int), with trace=True 'score_trace' and 'reward_trace'
        as float64 arrays [H] (VecMagicalEnv.lookahead for this one env)."""
        self._require_reset("lookahead")
        a = torch.as_tensor(list(actions), dtype=torch.uint8).reshape(-1, 1)
        res = self._vec.lookahead(a, objective=objective, trace=trace)
        out = {"score": float(res["score"][0].item()), "steps": int(res["steps"][0].item())}
        if objective is None and not trace:
            return out["score"], out["steps"]
        if objective is not None:
            out.update(value=float(res["value"][0].item()), peak=float(res["peak"][0].item()),
                       peak_step=int(res["peak_step"][0].item()))
        if trace:
            out.update(score_trace=res["score_trace"][:, 0].cpu().numpy(), reward_trace=res["reward_trace"][:, 0].cpu().numpy())
        return out

    def imagine(self, actions, every=1, stacks=False):
        """The LoRes observations the agent would see along `actions` (a sequence of 1 .. 4096 action ids, cut at the
        episode's end, after which the terminal frame repeats) from the current state, which stays as it is: an
        OrderedDict of uint8 arrays with a leading F = ceil(len(actions) / every) axis, keys and meaning as
        VecMagicalEnv.imagine's for this one env."""
        self._require_reset("imagine")
        a = torch.as_tensor(np.asarray(actions)).reshape(-1, 1)
        return collections.OrderedDict((k, v[:, 0].cpu().numpy())
                                       for k, v in self._vec.imagine(a, every=every, stacks=stacks).items())

    def plan(self, actions, objective=None):
        """The best of K candidate action sequences from the current state, which stays as it is.  actions: [H, K]
        action ids (candidate k is the column actions[:, k]).  Returns (best, best_score, scores): the index of the
        highest-scoring candidate (the lowest on ties), its score, and every candidate's score as a float64 array [K].
        With an objective (a magical_amd.Objective) the scores are its values and the best is chosen on them."""
        self._require_reset("plan")
        a = self._candidates(actions, "plan")
        res = self._vec.plan(a, details=True, objective=objective)
        return int(res["best"][0].item()), float(res["best_score"][0].item()), res["scores"][:, 0].cpu().numpy()

    def plan_cem(self, H, K, iters, elites, alpha=1, repeat=1, key=42, step=0, objective=None):
        """Cross-entropy planning from the current state, which stays as it is (VecMagicalEnv.plan_cem for this one
        env, from uniform weights).  Returns (plan, best_score, iter_best): the best action sequence found as a
        uint8 array [H], its score, and the best score of every iteration as a float64 array [iters].  With an
        objective (a magical_amd.Objective) the scores are its values."""
        self._require_reset("plan_cem")
        res = self._vec.plan_cem(H, K, iters, elites, alpha=alpha, repeat=repeat, key=key, step=step,
                                 objective=objective)
        return res["plan"][:, 0].cpu().numpy(), float(res["best_score"][0].item()), res["iter_best"][:, 0].cpu().numpy()

    def plan_beam(self, actions, seg, survivors, objective=None):
        """Beam search over action segments from the current state, which stays as it is (VecMagicalEnv.plan_beam for
        this one env).  actions: [H, K] action ids.  Returns (plan, best_value, values): the best lineage's actions as a
        uint8 array [H], its value, and every slot's value after the last segment as a float64 array [K]."""
        self._require_reset("plan_beam")
        a = self._candidates(actions, "plan_beam")
        res = self._vec.plan_beam(a, seg, survivors, details=True, objective=objective)
        return res["plan"][:, 0].cpu().numpy(), float(res["best_value"][0].item()), res["values"][:, 0].cpu().numpy()

    def get_state(self):
        """The env's whole state as bytes (a one-record snapshot blob, magical_amd.snapshot): physics, RNG, episode
        phase and frame stacks.  Host-side wrapper statistics (e.g. an SB3 Monitor around this env) are not in it."""
        self._require_reset("get_state")
        return self._vec.snapshot().tobytes()

    def set_state(self, state):
        """Back to a state from get_state() (this env name; NativeError otherwise); returns its observation."""
        from .snapshot import Snapshot
        obs = self._vec.restore(Snapshot.frombytes(state))
        if self._episode_steps is None:
            self._episode_steps = 0
        return self._np_obs(obs)

    def render(self, mode="rgb_array"):
        if mode != "rgb_array":
            raise NotImplementedError("headless: only rgb_array")
        full = self._vec.render_full()[0].cpu().numpy()
        return collections.OrderedDict([("allo", full[0]), ("ego", full[1])])

    def close(self):
        self._vec.close()


# entities.py:148-190
_UD = [0, 1, 2]            # NONE, UP, DOWN
_LR = [0, 4, 8]            # NONE, LEFT, RIGHT
ACTION_NUMS_FLAGS_NAMES = []
for _aid in range(18):
    _grip = 16 if _aid < 9 else 32
    _ud, _lr = _UD[_aid % 3], _LR[(_aid // 3) % 3]
    _names = {0: "", 1: "Up", 2: "Down"}[_ud] + {0: "", 4: "Left", 8: "Right"}[_lr] + ("Open" if _grip == 16 else "Close")
    ACTION_NUMS_FLAGS_NAMES.append((_aid, (_ud, _lr, _grip), _names))
ACTION_ID_TO_FLAGS = {a: f for a, f, _ in ACTION_NUMS_FLAGS_NAMES}
FLAGS_TO_ACTION_ID = {f: a for a, f, _ in ACTION_NUMS_FLAGS_NAMES}
