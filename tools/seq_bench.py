"""Time mg_step_seq against the R mg_step calls it replaces.

    python tools/seq_bench.py --name MoveToRegion-Demo-LoRes4E-v0 --envs 4096
    python tools/seq_bench.py --name ClusterColour-Demo-LoResStack-v0 --envs 8192

One simulator with an episode length no run reaches (nothing ends early, nothing auto-resets), warmed up with random
actions so contacts are live.  For every R (default 1, 2, 4, 8, 16) each repetition times in turn, with HIP events on
the stream, the two operations alternating so that they share the machine's noise, each from the same state (an
untimed mg_restore in between):

  * seq   -- one mg_step_seq call of R actions, whole call (physics kernel, reset phase, one render), and under
             mg_enable_timing its physics kernel alone (mg_read_timing's out[0]);
  * steps -- R mg_step calls, whole (R step kernels, R renders), and out[0]: R x the step kernel.

Prints one JSON line: median / min / max milliseconds per R, and the ratios seq / steps of the medians for the physics
kernels and for the whole calls.
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
    ap.add_argument("--repeats", default="1,2,4,8,16", help="the R values")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20, help="env steps before the first measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("seq_bench: no GPU (times are measured on the device or not at all)")
    n, rs = args.envs, [int(r) for r in args.repeats.split(",")]
    env = mg_envs.VecMagicalEnv(args.name, n, max_episode_steps=10 ** 6)
    lib = env.lib
    env.reset()
    for t in range(args.steps):
        env.step(env.random_actions(t))
    snap = env.snapshot()
    acts = torch.stack([env.random_actions(1000 + t).clone() for t in range(max(rs))])
    tm = (ctypes.c_double * 4)()

    def timed(fn, calls):
        """(whole ms by HIP events around fn, physics-kernel ms by the sim's own events)"""
        native.check(lib.mg_enable_timing(env.handle, calls))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        native.check(lib.mg_read_timing(env.handle, tm))
        native.check(lib.mg_enable_timing(env.handle, 0))
        assert int(tm[2]) == calls
        return e0.elapsed_time(e1), tm[0]

    def stats(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    res = {"name": args.name, "envs": n, "step_form": list(env.step_form()[:2]), "reps": args.reps, "repeats": {}}
    for R in rs:
        def seq():
            env.step_seq(acts[:R])

        def steps():
            for h in range(R):
                env.step(acts[h])

        sw, sk, tw, tk = [], [], [], []
        for rep in range(args.warmup + args.reps):
            env.restore(snap)
            a = timed(seq, 1)
            assert int(env.seq_steps.min()) == R and int(env.seq_steps.max()) == R
            env.restore(snap)
            b = timed(steps, R)
            if rep >= args.warmup:
                sw.append(a[0]), sk.append(a[1]), tw.append(b[0]), tk.append(b[1])
        med = statistics.median
        res["repeats"][str(R)] = {"seq_call": stats(sw), "seq_kernel": stats(sk), "steps_calls": stats(tw),
                                  "step_kernel_x_R": stats(tk), "kernel_ratio": round(med(sk) / med(tk), 3),
                                  "call_ratio": round(med(sw) / med(tw), 3),
                                  "seq_call_per_env_step_ms": round(med(sw) / R, 4)}
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
