"""Time env snapshots against a flat device copy of the same bytes.

    python tools/snapshot_bench.py --name MoveToRegion-Demo-LoRes4E-v0 --envs 4096
    python tools/snapshot_bench.py --name ClusterColour-Demo-LoResStack-v0 --envs 8192

One simulator; after a warm-up, every repetition times in turn (HIP events on the stream, the operations
alternating so that they share the machine's noise):

  * copy          -- hipMemcpyAsync device-to-device of the all-envs blob's byte count (torch copy_ of two uint8
                     tensors): the yardstick, independent of the code under test;
  * snapshot      -- mg_snapshot of every env into a preallocated blob;
  * restore       -- mg_restore of every env (header check with its stream synchronise, state and frame scatter,
                     output rebuild, the next-layout shadow's hand-over where the task has one);
  * snapshot64 / restore64 -- the same for 64 envs scattered over the batch.

Prints one JSON line: bytes, median / min / max milliseconds of each, GB/s (bytes read + bytes written over the
median) and the ratio of each all-envs median to the copy's.  A restore's events also cover the host's launch
gaps after its synchronise; restore_host_ms is the host clock around restore + synchronise for comparison.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "magical-1_amd"))

from magical_amd import envs as mg_envs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="MoveToRegion-Demo-LoRes4E-v0")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--subset", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20, help="env steps before the first snapshot")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("snapshot_bench: no GPU (times are measured on the device or not at all)")
    n = args.envs
    env = mg_envs.VecMagicalEnv(args.name, n)
    env.reset()
    env.set_episode_steps(torch.arange(n) % env.max_episode_steps)
    for t in range(args.steps):
        env.step(env.random_actions(t))
    m = min(args.subset, n)
    sub = [(k * n) // m + (7 * k) % max(1, n // m) for k in range(m)]   # scattered, distinct, not a run
    assert len(set(sub)) == m and max(sub) < n
    blob = torch.empty(env.snapshot_bytes(), dtype=torch.uint8, device=env.device)
    blob_sub = torch.empty(env.snapshot_bytes(m), dtype=torch.uint8, device=env.device)
    flat = torch.empty_like(blob)
    snap = env.snapshot(out=blob)
    snap_sub = env.snapshot(envs=sub, out=blob_sub)
    ops = {
        "copy": lambda: flat.copy_(blob),
        "snapshot": lambda: env.snapshot(out=blob),
        "restore": lambda: env.restore(snap),
        "snapshot64": lambda: env.snapshot(envs=sub, out=blob_sub),
        "restore64": lambda: env.restore(snap_sub, envs=sub),
    }
    times = {k: [] for k in ops}
    host = []
    for rep in range(args.warmup + args.reps):
        for k, op in ops.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            op()
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if rep >= args.warmup:
                times[k].append(e0.elapsed_time(e1))
                if k == "restore":
                    host.append((t1 - t0) * 1e3)
        env.step(env.random_actions(1000 + rep))   # the state moves on between repetitions
    out = {"name": args.name, "envs": n, "reps": args.reps, "blob_bytes": blob.numel(), "record_bytes": snap.header.record_bytes,
           "state_bytes": snap.header.state_bytes, "frames": snap.header.nframes, "subset": m, "subset_bytes": blob_sub.numel()}
    for k, v in times.items():
        nbytes = blob_sub.numel() if k.endswith("64") else blob.numel()
        med = statistics.median(v)
        out[k] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "GBps": round(2 * nbytes / med / 1e6, 1)}
    out["restore_host_ms"] = round(statistics.median(host), 4)
    out["snapshot_over_copy"] = round(out["snapshot"]["median_ms"] / out["copy"]["median_ms"], 3)
    out["restore_over_copy"] = round(out["restore"]["median_ms"] / out["copy"]["median_ms"], 3)
    print(json.dumps(out))
    env.close()


if __name__ == "__main__":
    main()
