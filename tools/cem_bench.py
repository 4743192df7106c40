"""Time mg_plan_cem against its floor and against what it replaces.

    python tools/cem_bench.py --name MoveToRegion-Demo-LoRes4E-v0 --envs 1024
    python tools/cem_bench.py --name ClusterColour-Demo-LoResStack-v0 --envs 1024

One simulator with an episode length no run reaches (nothing ends early), warmed up with random actions so contacts
are live.  For every K (default 16, 64) at horizon H (default 16), `iters` iterations (default 4) and K / 4 elites,
each repetition times in turn, with HIP events on the stream, the operations alternating so that they share the
machine's noise:

  * cem        -- one mg_plan_cem into preallocated outputs and caller-owned candidates and weights;
  * plans      -- `iters` plain mg_plan calls on candidates made beforehand, into preallocated outputs: the rollouts,
                  fan-outs and reductions of a cem call and nothing else, the floor;
  * torch_loop -- the same method from Python: sample_plans for iteration 0, then between plan() calls a topk over
                  the scores, a gather of the elites' actions, one-hot counts plus alpha, a multinomial draw of the
                  next candidates, the transposition to [H][K][N] and the incumbent's column.

A cem call is the plans' launches plus its own kernels (one draw, then an elite threshold and a refit / draw per
iteration), so the time spent in those is reported as cem - plans, and as a share of cem.  Prints one JSON line:
median / min / max milliseconds per operation, the ratios of the medians, and whether torch_loop / cem exceeds the
run-to-run spread (torch_loop's minimum above cem's maximum).
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
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--candidates", default="16,64")
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--alpha", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20, help="env steps before the first measurement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cem_bench: no GPU (times are measured on the device or not at all)")
    n, H, iters, alpha = args.envs, args.horizon, args.iters, args.alpha
    ks = [int(k) for k in args.candidates.split(",")]
    env = mg_envs.VecMagicalEnv(args.name, n, max_episode_steps=10 ** 6)
    lib, dev, st = env.lib, env.device, env._stream()
    env.reset()
    for t in range(args.steps):
        env.step(env.random_actions(t))
    env.plan(env.sample_plans(1, max(ks)))   # the fan pool for the largest K: later calls allocate nothing
    torch.cuda.synchronize()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def stats(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    res = {"name": args.name, "envs": n, "step_form": list(env.step_form()[:2]), "H": H, "iters": iters,
           "alpha": alpha, "reps": args.reps, "K": {}}
    idx = torch.arange(n, device=dev)
    for K in ks:
        E = max(1, K // 4)
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        c_acts = torch.empty((H, K, n), dtype=torch.uint8, device=dev)
        c_w = torch.empty((H, 18, n), dtype=torch.uint16, device=dev)
        c_best, c_score, c_iter = torch.empty(n, **i32), torch.empty(n, **f64), torch.empty((iters, n), **f64)
        c_first = torch.empty(n, dtype=torch.uint8, device=dev)
        cout = native.mg_plan_cem_out(best=c_best.data_ptr(), best_score=c_score.data_ptr(),
                                      first_action=c_first.data_ptr(), iter_best=c_iter.data_ptr())
        pre = [env.sample_plans(H, K, key=77, step=1000 + i * K * H) for i in range(iters)]
        p_best, p_score = torch.empty(n, **i32), torch.empty(n, **f64)
        p_first = torch.empty(n, dtype=torch.uint8, device=dev)
        pout = native.mg_plan_out(best=p_best.data_ptr(), best_score=p_score.data_ptr(), first_action=p_first.data_ptr())
        last = {}

        def cem():
            native.check(lib.mg_plan_cem(env.handle, ctypes.c_void_p(c_acts.data_ptr()), ctypes.c_void_p(c_w.data_ptr()),
                                         0, H, K, iters, E, alpha, 1, 77, 1000, ctypes.byref(cout), st))

        def plans():
            for i in range(iters):
                native.check(lib.mg_plan(env.handle, ctypes.c_void_p(pre[i].data_ptr()), H, K, ctypes.byref(pout), st))

        def torch_loop():
            acts = env.sample_plans(H, K, key=77, step=1000)
            for i in range(iters):
                r = env.plan(acts, details=True)
                top = r["scores"].topk(E, dim=0).indices                               # [E, N]
                elite = acts.gather(1, top[None].expand(H, E, n)).long()               # [H, E, N]
                counts = torch.nn.functional.one_hot(elite, 18).sum(dim=1) + alpha     # [H, N, 18]
                last["weights"], last["best_score"] = counts, r["best_score"]
                if i == iters - 1:
                    break
                drawn = torch.multinomial(counts.reshape(H * n, 18).float(), K, replacement=True)   # [H * N, K]
                nxt = drawn.reshape(H, n, K).permute(0, 2, 1).to(torch.uint8).contiguous()
                nxt[:, 0] = acts[:, r["best"].long(), idx]                             # the incumbent
                acts = nxt

        cem(), plans(), torch_loop()
        torch.cuda.synchronize()
        # iteration 0 of the three routes is the same plan of the same candidates
        first = env.plan(pre[0])["best_score"]
        assert torch.equal(c_iter[0], first)
        assert bool((c_iter[1:] >= c_iter[:-1]).all()) and torch.equal(c_iter[-1], c_score)
        t = {"cem": [], "plans": [], "torch_loop": []}
        for rep in range(args.warmup + args.reps):
            row = {"cem": timed(cem), "plans": timed(plans), "torch_loop": timed(torch_loop)}
            if rep >= args.warmup:
                for key, v in row.items():
                    t[key].append(v)
        med = {key: statistics.median(v) for key, v in t.items()}
        res["K"][str(K)] = dict({key: stats(v) for key, v in t.items()}, elites=E,
                                cem_minus_plans_ms=round(med["cem"] - med["plans"], 4),
                                cem_kernels_share_of_cem=round((med["cem"] - med["plans"]) / med["cem"], 4),
                                torch_loop_over_cem=round(med["torch_loop"] / med["cem"], 3),
                                faster_beyond_spread=bool(min(t["torch_loop"]) > max(t["cem"])))
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
