"""Time a reset from explicit scenes against the same handle's own reset.

    python tools/scene_bench.py --name MoveToRegion-Demo-LoRes4E-v0 --envs 4096
    python tools/scene_bench.py --name ClusterColour-Demo-LoResStack-v0 --envs 8192

One simulator; the scenes are the handle's own layouts after a reset (get_scenes), kept on the device.  After a warm-up,
every one of `runs` repetitions times in turn, with HIP events on the stream around each call (the operations alternate
so that they share the machine's noise), `reps` calls of each:

  * reset         -- mg_reset(NULL): the task's reset kernel, the next-layout shadow's hand-over where the task has one,
                     the render;
  * scene         -- mg_reset_scene of every env, check off: validation, build, the same render;
  * scene_check   -- the same with check on (one more kernel: the overlap queries);
  * get           -- mg_get_scene of every env.

Prints one JSON line: per operation the median milliseconds of every run, their median over the runs and the run-to-run
spread (max - min of the run medians), and scene / scene_check over reset.
"""
import argparse
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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scene_bench: no GPU (times are measured on the device or not at all)")
    n = args.envs
    env = mg_envs.VecMagicalEnv(args.name, n)
    env.reset()
    scenes = torch.empty(n * native.SCENE_DTYPE.itemsize, dtype=torch.uint8, device=env.device)
    env.get_scenes(out=scenes)
    _, status = env.reset_scenes(scenes)
    assert not status.any().item(), "the handle's own layouts must be built"
    ops = {
        "reset": lambda: env.reset(),
        "scene": lambda: env.reset_scenes(scenes),
        "scene_check": lambda: env.reset_scenes(scenes, check=True),
        "get": lambda: env.get_scenes(out=scenes),
    }
    runs = {k: [] for k in ops}
    for run in range(args.runs):
        times = {k: [] for k in ops}
        for rep in range(args.warmup + args.reps):
            for k, op in ops.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                op()
                e1.record()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    times[k].append(e0.elapsed_time(e1))
            env.step(env.random_actions(1000 * run + rep))   # the state moves on between repetitions
        for k in ops:
            runs[k].append(statistics.median(times[k]))
    out = {"name": args.name, "envs": n, "runs": args.runs, "reps": args.reps, "step_form": env.step_form()[0]}
    for k, v in runs.items():
        out[k] = {"run_median_ms": [round(x, 4) for x in v], "median_ms": round(statistics.median(v), 4),
                  "spread_ms": round(max(v) - min(v), 4)}
    out["scene_over_reset"] = round(out["scene"]["median_ms"] / out["reset"]["median_ms"], 3)
    out["scene_check_over_reset"] = round(out["scene_check"]["median_ms"] / out["reset"]["median_ms"], 3)
    print(json.dumps(out))
    env.close()


if __name__ == "__main__":
    main()
