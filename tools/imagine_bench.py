"""Time mg_imagine against the only other way to see a hypothetical rollout: snapshot() + F x step_seq() + restore().

    python tools/imagine_bench.py --name MoveToRegion-Demo-LoRes4E-v0 --envs 1024
    python tools/imagine_bench.py --name ClusterColour-Demo-LoResStack-v0 --envs 1024

One simulator with an episode length no run reaches, warmed up with random actions so contacts are live and the frame
ring holds distinct frames.  For every `every` (default 1 and 4, H = 16) and stacks off / on, each repetition times in
turn, with HIP events on the stream, the two operations alternating so that they share the machine's noise, each from the
same state:

  * imagine -- one imagine(actions, every, stacks) call into preallocated tensors: F rollout launches, F frame-less
               renders, the stack pass;
  * route   -- snapshot() into a preallocated blob, F step_seq() calls of `every` actions, each followed by the copies
               that keep what imagine returns (the current frames, or the stacked observation), and restore().

Prints one JSON line: median / min / max milliseconds per setting, imagined frames (env x frame) per second, the bytes
imagine writes to its outputs per call, and the ratio imagine / route of the medians (below 1: imagine is faster).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "magical-1_amd"))

from magical_amd import envs as mg_envs  # noqa: E402

FR = 96 * 96 * 3


def imagine_bytes(preproc, n, F, stacks):
    """bytes one imagine() call writes to its output tensors: both views' plain frames, and with stacks the 12-channel
    stack of every stacked view (imagine_layout)"""
    bufs, _ = mg_envs.imagine_layout(preproc, stacks)
    return sum(F * n * FR * (4 if b.startswith("stack_") else 1) for b in bufs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="MoveToRegion-Demo-LoRes4E-v0")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--every", default="1,4")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20, help="env steps before the first measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("imagine_bench: no GPU (times are measured on the device or not at all)")
    n, H = args.envs, args.horizon
    env = mg_envs.VecMagicalEnv(args.name, n, max_episode_steps=10 ** 6)
    env.reset()
    for t in range(args.steps):
        env.step(env.random_actions(t))
    acts = torch.stack([env.random_actions(1000 + t).clone() for t in range(H)])
    blob = torch.empty(env.snapshot_bytes(), dtype=torch.uint8, device=env.device)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    res = {"name": args.name, "envs": n, "H": H, "step_form": list(env.step_form()[:2]), "reps": args.reps, "settings": []}
    for every in [int(x) for x in args.every.split(",")]:
        F = -(-H // every)
        for stacks in (False, True):
            _, keys = mg_envs.imagine_layout(env.spec.preproc, stacks)
            shape = {k: (F, n, 96, 96, 12 if b.startswith("stack_") else 3) for k, b in keys.items()}
            out = {k: torch.empty(s, dtype=torch.uint8, device=env.device) for k, s in shape.items()}
            keep = {k: torch.empty(s, dtype=torch.uint8, device=env.device) for k, s in shape.items()}

            def imagine():
                env.imagine(acts, every, stacks=stacks, out=out)

            def route():
                snap = env.snapshot(out=blob)
                for f in range(F):
                    obs = env.step_seq(acts[f * every:(f + 1) * every])[0]
                    for k, dst in keep.items():
                        v = obs[k].permute(0, 2, 3, 1) if env._chw else obs[k]
                        dst[f].copy_(v if v.shape[-1] == dst.shape[-1] else v[..., 9:12])
                env.restore(snap)

            ti, tr = [], []
            for rep in range(args.warmup + args.reps):
                a, b = timed(imagine), timed(route)
                if rep >= args.warmup:
                    ti.append(a), tr.append(b)
            for k in out:   # the two routes show the same bytes (the state is restored after each route)
                assert torch.equal(out[k], keep[k]), (every, stacks, k)
            med = statistics.median
            res["settings"].append({
                "every": every, "F": F, "stacks": stacks, "imagine": stats(ti), "route": stats(tr),
                "imagine_frames_per_s": round(n * F / (med(ti) * 1e-3)), "route_frames_per_s": round(n * F / (med(tr) * 1e-3)),
                "imagine_bytes_written": imagine_bytes(env.spec.preproc, n, F, stacks),
                "ratio_imagine_over_route": round(med(ti) / med(tr), 3)})
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
