"""Time mg_lookahead against the step kernel it loops and against what it replaces.

    python tools/lookahead_bench.py --name MoveToRegion-Demo-LoRes4E-v0 --envs 4096
    python tools/lookahead_bench.py --name ClusterColour-Demo-LoResStack-v0 --envs 8192

One simulator with an episode length no run reaches (nothing ends early, nothing auto-resets), warmed up with random
actions so contacts are live.  For every horizon H (default 1, 4, 16) each repetition times in turn, with HIP events
on the stream, the operations alternating so that they share the machine's noise:

  * lookahead   -- mg_lookahead of H actions into preallocated outputs (scratch copy + the H-step kernel + score);
  * step_kernel -- H mg_step calls under mg_enable_timing; mg_read_timing's out[0] is the step kernel alone (no
                   auto-reset pass, no render): the baseline H x step kernel;
  * step_path   -- the same H mg_step calls end to end (step kernel, render, frame stacks) plus the mg_restore that
                   puts the envs back: what a planner pays without mg_lookahead.  The restore also returns the sim to
                   the state every repetition starts from.

Prints one JSON line: median / min / max milliseconds per horizon and the ratios lookahead / (H x step kernel) and
step_path / lookahead of the medians.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "magical-1_amd"))

from magical_amd import envs as mg_envs, native  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="MoveToRegion-Demo-LoRes4E-v0")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--horizons", default="1,4,16")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20, help="env steps before the first measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lookahead_bench: no GPU (times are measured on the device or not at all)")
    n, hs = args.envs, [int(h) for h in args.horizons.split(",")]
    env = mg_envs.VecMagicalEnv(args.name, n, max_episode_steps=10 ** 6)
    lib, dev = env.lib, env.device
    env.reset()
    for t in range(args.steps):
        env.step(env.random_actions(t))
    snap = env.snapshot()
    acts = torch.stack([env.random_actions(1000 + t).clone() for t in range(max(hs))])
    score = torch.empty(n, dtype=torch.float64, device=dev)
    steps = torch.empty(n, dtype=torch.int32, device=dev)
    out = native.mg_lookahead_out(score=score.data_ptr(), steps=steps.data_ptr())
    ap_, st = ctypes.c_void_p(acts.data_ptr()), env._stream()
    tm = (ctypes.c_double * 4)()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    res = {"name": args.name, "envs": n, "step_form": list(env.step_form()[:2]), "reps": args.reps, "horizons": {}}
    for H in hs:
        def look():
            native.check(lib.mg_lookahead(env.handle, ap_, H, ctypes.byref(out), st))

        def path():
            for h in range(H):
                env.step(acts[h])
            env.restore(snap)

        t_look, t_kern, t_path = [], [], []
        for rep in range(args.warmup + args.reps):
            a = timed(look)
            native.check(lib.mg_enable_timing(env.handle, H))
            b = timed(path)
            native.check(lib.mg_read_timing(env.handle, tm))
            native.check(lib.mg_enable_timing(env.handle, 0))
            assert int(tm[2]) == H
            if rep >= args.warmup:
                t_look.append(a), t_path.append(b), t_kern.append(tm[0])
        assert int(steps.min()) == H and int(steps.max()) == H
        lk, kn, pt = statistics.median(t_look), statistics.median(t_kern), statistics.median(t_path)
        res["horizons"][str(H)] = {"lookahead": stats(t_look), "step_kernel_x_H": stats(t_kern), "step_path": stats(t_path),
                                   "lookahead_over_step_kernels": round(lk / kn, 3),
                                   "step_path_over_lookahead": round(pt / lk, 2)}
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
