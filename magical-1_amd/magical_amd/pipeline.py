"""Pipelined env pool: one batch of envs as C simulators on C HIP streams.

Why: the robot scenes' step kernel holds a whole CU's LDS per workgroup (16 envs x ~9.8 KB) and runs one
wavefront per CU for ~0.54 ms whatever the env count, and the render kernel fills the CUs with 16 KB
workgroups after it; in one stream the two alternate and neither fills the chip.  Split into C chunks, each
with its own stream, chunk k's render runs beside chunk k+1's step kernel and the next step of chunk 0
starts as soon as chunk 0's own render is done (round 4, `tools/overlap_ab.py`: MoveToRegion 4096 envs
2.54 M -> 2.79 M env-steps/s at C = 2, MoveToCorner 1.94 -> 2.08 M; the cooperative many-block scenes are
slower chunked, ClusterColour 1.48 -> 1.23 M, and keep C = 1).

Semantics: every env is exactly the env of the unchunked `VecMagicalEnv` with the same seed (env i of the
pool is env i mod m of chunk i // m, seeded as global env i), stepped with its own action in the same order,
so observations are bit-identical (`tests/test_gpu_parity.py::test_pipelined_pool_matches_batch`).  Chunks
are equal shares of the envs rounded to the step kernel's 16-env workgroups; at most 3, since a process has
4 hardware queues (GPU_MAX_HW_QUEUES) and the caller's stream takes one.  What
changes is completion: `step()` only enqueues; a chunk's outputs (views into the pool's full-batch tensors)
are complete once `wait(k)` / `wait()` has ordered the caller's stream after it -- the asynchronous env-pool
contract (as EnvPool's async mode), not gym's synchronous one.  Actions are double-buffered on the device,
so the caller may overwrite its action tensor right after `step()` returns.
"""
import collections
import ctypes

import torch

from . import native
from .envs import VecMagicalEnv, assemble_obs, imagine_actions, plan_actions, scene_tensor, seq_actions


_SIGNED = {torch.uint16: torch.int16, torch.uint32: torch.int32}


def cat_bits(tensors, dim=0):
    """torch.cat that also takes uint16 and uint32, for which it has no kernel: they are joined as their signed twins,
    the same bytes"""
    signed = _SIGNED.get(tensors[0].dtype)
    if signed is None:
        return torch.cat(tensors, dim=dim)
    return torch.cat([t.view(signed) for t in tensors], dim=dim).view(tensors[0].dtype)


def join(parts, stream=None):
    """The chunks' result dicts as one, every key concatenated in env order: envs are the first axis of 'bodies' and
    'counts' and the last axis of every other result ([n], [K, n], [H, n], [H, K, n], [J, 18, n]).  stream: the stream
    that reads the parts here, where they were allocated on the chunks' own."""
    out = collections.OrderedDict()
    for key in parts[0]:
        tensors = [p[key] for p in parts]
        out[key] = cat_bits(tensors, dim=0 if key in ("bodies", "counts") else -1)
        if stream is not None:
            for t in tensors:
                t.record_stream(stream)
    return out


# tasks measured faster pipelined (round 4): their scenes run the compile-time robot forms of the step
# kernel (16 envs per workgroup: one workgroup per CU at 4096 envs, the CU's whole LDS)
PIPELINED_TASKS = ("MoveToRegion", "MoveToCorner")


def default_chunks(spec, num_envs):
    """bench.py --chunks auto: 3 for MoveToRegion at >= 4096 envs, 2 for the robot scenes at >= 2048, else 1.
    (Round 6, with the 16-row-band render: a third chunk measured MoveToRegion 3.37 -> 3.42 M env-steps/s at 4096
    envs, two repetitions (profiles/r06_b16/chunks_b16), its render-bound pipeline gaining from the smaller step
    launches; MoveToCorner, whose pipeline is step-bound, 2.59 -> 2.61 M, within noise, and its 0.74 ms step kernel
    then serves 1365 envs instead of 2048 -- kept at 2.  Before the 16-row render, MoveToRegion's third chunk was
    3.16 -> 3.19 M (profiles/r06_d).  A 1365-env chunk's render fills 1.2 rounds of the CUs' workgroup slots, so its
    isolated HBM fraction reads lower than a 2048-env chunk's.)"""
    if spec.task not in PIPELINED_TASKS:
        return 1
    if spec.task == "MoveToRegion" and num_envs >= 4096:
        return 3
    return 2 if num_envs >= 2048 and num_envs % 2 == 0 else 1


class PipelinedVecEnv:
    def __init__(self, env_name, num_envs, chunks=2, device="cuda:0", seeds=None, base_seed=0, **kw):
        num_envs, chunks = int(num_envs), int(chunks)
        if chunks < 1 or chunks > min(num_envs, 3):
            raise ValueError(f"PipelinedVecEnv: {num_envs} envs do not split into {chunks} chunks")
        self.num_envs, self.chunks = num_envs, chunks
        # chunk bounds: equal shares rounded to the step kernel's 16-env workgroups where the count allows
        q = 16 if num_envs >= 16 * chunks else 1
        units = num_envs // q
        self.bounds = [q * (units * k // chunks) for k in range(chunks)] + [num_envs]
        self.device = torch.device(device)
        seeds = list(seeds) if seeds is not None else [base_seed + i for i in range(num_envs)]
        if len(seeds) != num_envs:
            raise ValueError("PipelinedVecEnv: one seed per env")
        b = self.bounds
        self.sims = [VecMagicalEnv(env_name, b[k + 1] - b[k], device=device, seeds=seeds[b[k]:b[k + 1]], **kw)
                     for k in range(chunks)]
        s0 = self.sims[0]
        self.spec, self.lib, self.max_episode_steps = s0.spec, s0.lib, s0.max_episode_steps
        self.action_space, self.observation_space = s0.action_space, s0.observation_space
        if self.spec.preproc is None:
            raise ValueError("PipelinedVecEnv: LoRes preprocessors only (the 384^2 view is rendered on demand)")
        # the pool's full-batch outputs; chunk k writes rows [bounds[k], bounds[k + 1]) on its own stream
        # (PickAndPlace's target included: the auto-reset rewrites it inside the chunk's step, so it is complete
        # only after wait(), like the observations -- ADVICE r4)
        self.buffers = collections.OrderedDict(
            (k, torch.zeros((num_envs,) + tuple(v.shape[1:]), dtype=v.dtype, device=self.device))
            for k, v in s0.output_buffers().items())
        # window rings of the stacked views (VecMagicalEnv window mode): one ring per view for the whole pool,
        # chunk k's envs a contiguous slice of it (env-major), so the pool's stacks are one strided view
        self.window_k = s0.window_k
        self.wring = [None if r is None else torch.zeros((num_envs,) + tuple(r.shape[1:]), dtype=r.dtype, device=self.device)
                      for r in s0.wring]
        for k, sim in enumerate(self.sims):
            views = {key: buf[b[k]:b[k + 1]] for key, buf in self.buffers.items()}
            if self.window_k:
                sim.bind_window(*[None if r is None else r[b[k]:b[k + 1]] for r in self.wring])
            sim.bind_outputs(views, target=views.get("target"))
        # (a high-priority stream for chunk 0 measured no different, round 4: profiles/r04_resetwaves/)
        self.streams = [torch.cuda.Stream(self.device) for _ in range(chunks)]
        self.abuf = torch.zeros((2, num_envs), dtype=torch.uint8, device=self.device)
        # done[k][slot]: chunk k finished the step that read action slot `slot`
        self.done_ev = [[None, None] for _ in range(chunks)]
        self.t = 0
        self.seq_steps = None     # step_seq's info['steps'] for the whole pool (allocated by the first call)
        self.reset_count = 0     # explicit reset() calls (magical_amd.dist checks its frame rings against it)
        self.target = self.buffers.get("target")
        # the observation's float32 target columns, converted on each chunk's stream right after its step (a
        # conversion on the caller's stream inside step() would read the target before the chunk wrote it)
        self.target_f = None if self.target is None else torch.zeros(self.target.shape, dtype=torch.float32,
                                                                     device=self.device)
        self._target_out = None   # bind_outputs' "target" view (magical_amd.dist's packed buffer)
        self._last = []           # the chunk streams' events of the last step() (magical_amd.dist waits on them)

    # -- ordering ------------------------------------------------------------------
    def _caller(self):
        return torch.cuda.current_stream(self.device)

    def _fork(self):
        """The chunk streams wait for the caller's work so far."""
        ev = torch.cuda.Event()
        ev.record(self._caller())
        for st in self.streams:
            st.wait_event(ev)

    def wait(self, chunk=None):
        """Order the caller's stream after chunk `chunk` (all chunks when None): its outputs are then complete."""
        cs = self._caller()
        for k in (range(self.chunks) if chunk is None else [chunk]):
            ev = torch.cuda.Event()
            ev.record(self.streams[k])
            cs.wait_event(ev)

    def _per_chunk(self, fn, pre_wait=True, post_wait=True):
        """[fn(k, sim, lo, hi) for every chunk k], each called under the chunk's stream, whose envs are [lo, hi).
        pre_wait: every chunk's earlier work is done before any chunk starts; post_wait: the caller's stream is
        ordered after what fn enqueued."""
        if pre_wait:
            self.wait()
        self._fork()
        out = []
        for k, (sim, st) in enumerate(zip(self.sims, self.streams)):
            with torch.cuda.stream(st):
                out.append(fn(k, sim, self.bounds[k], self.bounds[k + 1]))
        if post_wait:
            self.wait()
        return out

    def _publish_target(self, k=None):
        """PickAndPlace: copy the persistent float64 target into the observation's float32 columns and into
        bind_outputs' "target" view, on the current stream -- chunk k's rows right after a call that may have reset its
        envs (a conversion on the caller's stream would read the target before the chunk wrote it), every row when
        k is None."""
        if self.target_f is None:
            return
        rows = slice(None) if k is None else slice(self.bounds[k], self.bounds[k + 1])
        self.target_f[rows].copy_(self.target[rows])
        if self._target_out is not None:
            self._target_out[rows].copy_(self.target[rows])

    def _after_reset(self):
        """the tail of reset() and reset_scenes(), whose per-chunk resets ran on the caller's stream"""
        self._publish_target()
        self.reset_count += 1
        self._last = []
        self._fork()
        return self._obs()

    def step_events(self):
        """Events recorded on every chunk's stream after its last step() (a consumer on another stream, e.g.
        magical_amd.dist's collective, waits on them instead of ordering the caller's stream after the chunks,
        which would make the next step's chunks wait for each other)."""
        return list(self._last)

    def bind_outputs(self, views, frames_only=False):
        """Bind full-batch [num_envs, ...] output views (VecMagicalEnv.bind_outputs keys): chunk k writes rows
        [bounds[k], bounds[k + 1]) of each.  Called between steps (magical_amd.dist binds a packed buffer set per
        step); the chunks' streams are ordered after the caller's stream by the next step()'s fork."""
        b = self.bounds
        for k, sim in enumerate(self.sims):
            sim.bind_outputs({key: v[b[k]:b[k + 1]] for key, v in views.items() if key != "target"},
                             frames_only=frames_only)
        # PickAndPlace: the pool's persistent target is copied into views["target"] on each chunk's stream right
        # after the chunk's step (reset: on the caller's stream), so the view is complete when the chunk is
        self._target_out = views.get("target") if self.target is not None else None

    # -- API -----------------------------------------------------------------------
    def reset(self, mask=None):
        self.wait()
        for k, sim in enumerate(self.sims):
            sim.reset(None if mask is None else mask[self.bounds[k]:self.bounds[k + 1]])
        return self._after_reset()

    def get_scenes(self):
        """VecMagicalEnv.get_scenes for the whole pool: a structured array [num_envs] in env order."""
        import numpy as np
        self.wait()
        return np.concatenate([sim.get_scenes() for sim in self.sims])

    def reset_scenes(self, scenes, mask=None, check=False):
        """VecMagicalEnv.reset_scenes for the whole pool, split per chunk as reset() is (on the caller's stream, once
        every chunk's last step is done): `scenes` is a structured array [num_envs], a list of num_envs scene.Scene or a
        uint8 device tensor of num_envs * 792 bytes; returns (obs, status i32[num_envs])."""
        size, b = native.SCENE_DTYPE.itemsize, self.bounds
        scenes = scene_tensor(scenes, self.num_envs, self.device, in_place=False)
        m = None if mask is None else torch.as_tensor(mask).to(self.device, torch.uint8)
        self.wait()
        status = [sim.reset_scenes(scenes[b[k] * size:b[k + 1] * size], None if m is None else m[b[k]:b[k + 1]],
                                   check=check)[1] for k, sim in enumerate(self.sims)]
        return self._after_reset(), torch.cat(status)

    def step(self, actions):
        # (the benchmarked path: its own loop, not _per_chunk, whose closure and result list it does not need)
        a = actions
        if not (isinstance(a, torch.Tensor) and a.dtype == torch.uint8 and a.device == self.device):
            a = torch.as_tensor(actions).to(self.device, torch.uint8)
        slot = self.t & 1
        cs = self._caller()
        for k in range(self.chunks):   # the step two calls ago has read this slot
            if self.done_ev[k][slot] is not None:
                cs.wait_event(self.done_ev[k][slot])
        self.abuf[slot].copy_(a)
        self._fork()
        b = self.bounds
        for k, (sim, st) in enumerate(zip(self.sims, self.streams)):
            with torch.cuda.stream(st):
                sim.step(self.abuf[slot, b[k]:b[k + 1]])
                self._publish_target(k)
            ev = torch.cuda.Event()
            ev.record(st)
            self.done_ev[k][slot] = ev
        self._last = [self.done_ev[k][slot] for k in range(self.chunks)]
        self.t += 1
        return self._obs(), self.buffers["reward"], self.buffers["done"], {"eval_score": self.buffers["eval_score"]}

    def step_seq(self, actions):
        """VecMagicalEnv.step_seq for the whole pool: actions [R, num_envs] ([num_envs]: R = 1); chunk k runs its
        columns [bounds[k], bounds[k + 1]) as one mg_step_seq call on its own stream, as step() does, and like step()
        the call only enqueues: a chunk's outputs are complete after wait(k) / wait().  info holds 'eval_score' and
        'steps' i32[num_envs]."""
        a = seq_actions(actions, self.num_envs, "step_seq", "R", self.device)
        b = self.bounds
        if self.seq_steps is None:   # the chunks' info['steps'] as slices of one pool tensor
            self.seq_steps = torch.empty(self.num_envs, dtype=torch.int32, device=self.device)
            for k, sim in enumerate(self.sims):
                sim.seq_steps = self.seq_steps[b[k]:b[k + 1]]
        # a column slice is strided: every chunk gets its own contiguous [R, m] copy.  As step() copies the actions
        # into abuf, they are made on the caller's stream before the fork, so they run beside the chunks' unfinished
        # work (this call does not wait() for it); the planning calls, which do, make theirs on the chunks' streams
        parts = [a[:, b[k]:b[k + 1]].contiguous() for k in range(self.chunks)]

        def run(k, sim, lo, hi):
            parts[k].record_stream(self.streams[k])
            sim.step_seq(parts[k])
            self._publish_target(k)
            return self.streams[k].record_event()
        self._last = self._per_chunk(run, pre_wait=False, post_wait=False)
        return self._obs(), self.buffers["reward"], self.buffers["done"], \
            {"eval_score": self.buffers["eval_score"], "steps": self.seq_steps}

    def snapshot(self):
        """The pool's state as a `magical_amd.snapshot.PoolSnapshot`: one blob per chunk, taken on the chunk's own
        stream once every chunk's last step is done (wait()); the caller's stream is ordered after the blobs.  It
        restores into a pool with the same chunking, or into a plain VecMagicalEnv of the same envs in the same
        order (VecMagicalEnv.restore).  Materialised stacks only (not window=True)."""
        from .snapshot import PoolSnapshot
        blobs = [torch.empty(sim.snapshot_bytes(), dtype=torch.uint8, device=self.device) for sim in self.sims]
        return PoolSnapshot(self._per_chunk(lambda k, sim, lo, hi: sim.snapshot(out=blobs[k])), self.bounds)

    def restore(self, snap):
        """Put every env of the pool back to a PoolSnapshot of the same chunking, each chunk on its own stream, and
        return the observation (complete: the caller's stream is ordered after the chunks)."""
        from .snapshot import PoolSnapshot
        if not isinstance(snap, PoolSnapshot) or snap.bounds != self.bounds:
            raise ValueError(f"PipelinedVecEnv.restore: a PoolSnapshot with chunk bounds {self.bounds}")
        snap = snap.to(self.device)

        def run(k, sim, lo, hi):
            sim.restore(snap.chunks[k])
            self._publish_target(k)
        self._per_chunk(run)
        self._last = []
        return self._obs()

    # The planning calls: chunk k works on its envs [bounds[k], bounds[k + 1]) on its own stream once every chunk's last
    # step is done, and the results are concatenated in env order (complete: the caller's stream is ordered after the
    # chunks).  An env slice of the arguments is strided, so every chunk gets its own contiguous copy, made on its stream.
    def lookahead(self, actions, bodies=False, objective=None, trace=False):
        """VecMagicalEnv.lookahead for the whole pool: actions [H, num_envs] ([num_envs]: H = 1); objective and trace
        as VecMagicalEnv.lookahead's, per chunk."""
        a = seq_actions(actions, self.num_envs, "lookahead", "H", self.device)
        return join(self._per_chunk(lambda k, sim, lo, hi: sim.lookahead(
            a[:, lo:hi].contiguous(), bodies=bodies, objective=objective, trace=trace)), self._caller())

    def imagine(self, actions, every=1, stacks=False, details=False):
        """VecMagicalEnv.imagine for the whole pool: actions [H, num_envs] ([num_envs]: H = 1); chunk k imagines its
        columns on its own stream and the results are joined in env order -- the frames and stacks [F, num_envs, ...]
        along their env axis, the details as lookahead()'s.  (No out=: every chunk fills tensors of its own.)"""
        a, every, _ = imagine_actions(actions, self.num_envs, every, self.device)
        parts = self._per_chunk(lambda k, sim, lo, hi: sim.imagine(a[:, lo:hi].contiguous(), every=every, stacks=stacks,
                                                                   details=details))
        frames = [collections.OrderedDict((key, p.pop(key)) for key in ("allo", "ego", "past_obs") if key in p) for p in parts]
        out = collections.OrderedDict((key, torch.cat([f[key] for f in frames], dim=1)) for key in frames[0])
        for f in frames:   # (allocated on the chunks' streams, read here on the caller's: as join's parts)
            for t in f.values():
                t.record_stream(self._caller())
        out.update(join(parts, self._caller()) if details else {})
        return out

    def plan(self, actions, details=False, objective=None):
        """VecMagicalEnv.plan for the whole pool: actions [H, K, num_envs] ([K, num_envs]: H = 1); objective as
        VecMagicalEnv.plan's."""
        a = plan_actions(actions, self.num_envs).to(self.device)
        return join(self._per_chunk(lambda k, sim, lo, hi: sim.plan(
            a[:, :, lo:hi].contiguous(), details=details, objective=objective)), self._caller())

    def plan_beam(self, actions, seg, survivors, details=False, objective=None):
        """VecMagicalEnv.plan_beam for the whole pool, per chunk as plan()."""
        a = plan_actions(actions, self.num_envs).to(self.device)
        return join(self._per_chunk(lambda k, sim, lo, hi: sim.plan_beam(
            a[:, :, lo:hi].contiguous(), seg, survivors, details=details, objective=objective)), self._caller())

    def sample_plans(self, H, K, repeat=1, key=42, step=0, out=None):
        """u8[H, K, num_envs] random-shooting candidates (VecMagicalEnv.sample_plans per chunk).  Chunk k draws with
        key + k and numbers its envs from 0, as random_actions does: with J = ceil(H / repeat), the row [h, k] equals
        this pool's random_actions(step + k * J + h // repeat, key)."""
        H, K = int(H), int(K)
        if out is None:
            out = torch.empty((max(H, 0), max(K, 0), self.num_envs), dtype=torch.uint8, device=self.device)
        if tuple(out.shape) != (H, K, self.num_envs) or out.dtype != torch.uint8 or out.device != self.device:
            raise ValueError(f"sample_plans: out must be a uint8 [{H}, {K}, {self.num_envs}] tensor on {self.device}")
        b = self.bounds
        for k, sim in enumerate(self.sims):   # (on the caller's stream, as random_actions)
            out[:, :, b[k]:b[k + 1]] = sim.sample_plans(H, K, repeat=repeat, key=key + k, step=step)
        return out

    def plan_cem(self, H, K, iters, elites, alpha=1, repeat=1, key=42, step=0, weights=None, details=False,
                 objective=None):
        """VecMagicalEnv.plan_cem for the whole pool, per chunk as plan(): chunk k draws with key + k (envs numbered
        from 0, as sample_plans).  weights: None, or a uint16 [J, 18, num_envs] tensor on the pool's device, the warm
        start, updated in place (each chunk works on its own contiguous copy of its columns, which is copied back).
        objective as VecMagicalEnv.plan_cem's."""
        J = -(-int(H) // max(int(repeat), 1))
        if weights is not None and (not torch.is_tensor(weights) or tuple(weights.shape) != (J, 18, self.num_envs)
                                    or weights.dtype != torch.uint16 or weights.device != self.device):
            raise ValueError(f"plan_cem: weights must be a uint16 [{J}, 18, {self.num_envs}] tensor on {self.device}")

        def run(k, sim, lo, hi):   # (uint16 is sliced and copied as int16: the same bytes, a type every torch op takes)
            w = None if weights is None else weights.view(torch.int16)[:, :, lo:hi].contiguous().view(torch.uint16)
            return sim.plan_cem(H, K, iters, elites, alpha=alpha, repeat=repeat, key=key + k, step=step, weights=w,
                                details=details, objective=objective)
        out = join(self._per_chunk(run), self._caller())
        if weights is not None:
            weights.view(torch.int16).copy_(out["weights"].view(torch.int16))
            out["weights"] = weights
        return out

    def _obs(self):
        # (every chunk has stepped as often: one window start for the whole pool)
        return assemble_obs(self.buffers.get("allo"), self.buffers.get("ego"), self.buffers.get("past_obs"),
                            self.wring if self.window_k else None, self.sims[0].window_start() if self.window_k else 0,
                            self.sims[0]._chw, self.target_f)

    def random_actions(self, step, key=42, out=None):
        """Device Philox actions for a random policy (chunk k draws with key + k)."""
        out = out if out is not None else torch.empty(self.num_envs, dtype=torch.uint8, device=self.device)
        b = self.bounds
        for k, sim in enumerate(self.sims):
            sim.random_actions(step, key=key + k, out=out[b[k]:b[k + 1]])
        return out

    def set_episode_steps(self, steps):
        self.wait()
        s = torch.as_tensor(steps)
        for k, sim in enumerate(self.sims):
            sim.set_episode_steps(s[self.bounds[k]:self.bounds[k + 1]])
        self._fork()

    def set_body_pose(self, env, body, x, y, angle):
        """VecMagicalEnv.set_body_pose for env `env` of the pool: forwarded to its chunk (parity tests)."""
        env = int(env)
        if env < 0 or env >= self.num_envs:
            raise ValueError(f"set_body_pose: env {env} of {self.num_envs}")
        k = max(c for c in range(self.chunks) if self.bounds[c] <= env)
        self.wait()
        self.sims[k].set_body_pose(env - self.bounds[k], body, x, y, angle)
        self._fork()

    def errors(self):
        self.wait()
        return torch.cat([sim.errors() for sim in self.sims])

    def rng_state(self):
        """VecMagicalEnv.rng_state of the whole pool: (key uint32 [num_envs, 624], pos int32 [num_envs])"""
        self.wait()
        parts = [sim.rng_state() for sim in self.sims]
        return cat_bits([k for k, _ in parts]), torch.cat([p for _, p in parts])

    def enable_timing(self, steps):
        """Per-chunk HIP-event timing of the kernels (mg_enable_timing on every chunk's simulator)."""
        self.wait()
        for sim in self.sims:
            native.check(self.lib.mg_enable_timing(sim.handle, int(steps)))

    def read_timing(self):
        """[chunks][4] totals over the timed launches (mg_read_timing: step ms, render ms, launches, reset ms)."""
        out = []
        for sim in self.sims:
            tm = (ctypes.c_double * 4)()
            native.check(self.lib.mg_read_timing(sim.handle, tm))
            out.append(list(tm))
        return out

    def close(self):
        for st in self.streams:   # the chunks' queued kernels read the simulators' memory
            st.synchronize()
        for sim in self.sims:
            sim.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
