"""Time mg_plan against what it replaces: K consecutive mg_lookahead calls plus the torch reduction.

    python tools/plan_bench.py --name MoveToRegion-Demo-LoRes4E-v0 --envs 1024
    python tools/plan_bench.py --name ClusterColour-Demo-LoResStack-v0 --envs 1024
    python tools/plan_bench.py --beam --name ClusterColour-Demo-LoResStack-v0 --envs 1024   (mg_plan_beam: beam_bench)

One simulator with an episode length no run reaches (nothing ends early), warmed up with random actions so contacts
are live.  For every K (default 16, 64) at horizon H (default 16) each repetition times in turn, with HIP events on
the stream, the operations alternating so that they share the machine's noise:

  * plan      -- one mg_plan of u8[H][K][N] candidates into preallocated outputs (fan-out copy, one grid of K * N
                 rollouts, the best-of-K reduction);
  * k_calls   -- K mg_lookahead calls on the same sim, candidate k's action column each (its own contiguous [H][N]
                 block, prepared outside the timed region), the K score vectors written into one [K][N] tensor, then
                 torch's argmax over k and the two gathers (best score, first action): what a planner does without
                 mg_plan;
  * plan_h0 / k_calls_h0 -- the same two with H = 0: copy, launch and scoring cost without any env-step.  The fan-out
                 copy's share of a plan is reported as plan_h0 / plan.

The results of the two routes are checked equal before timing.  Prints one JSON line: median / min / max
milliseconds, the ratio k_calls / plan of the medians, and the fan pool's size (device memory taken by the first plan
of the largest K, per rollout, and scaled to MG_PLAN_MAX_ROLLOUTS).
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


def objective_bench(args, env, ks, timed, stats, res):
    """--objective: for every K, each repetition times in turn mg_plan, mg_plan_obj with FINAL (the same kernels),
    RETURN (tail 1) and PEAK (the traced rollout kernel: a write-back and a score per env-step), and H mg_step calls of
    a second sim of K * N envs under mg_enable_timing, whose out[0] is the step kernel alone: the yardstick for a
    rollout that writes back and scores every step, as mg_step does.  Adds to res["K"][K] the medians with min / max
    and each route's ratio to mg_plan and to the step kernels."""
    lib, dev, st, n, H = env.lib, env.device, env._stream(), env.num_envs, args.horizon
    routes = {"plan": None, "final": native.mg_objective(kind=native.OBJ_FINAL, gamma=1.0, tail=0.0),
              "return": native.mg_objective(kind=native.OBJ_RETURN, gamma=args.gamma, tail=1.0),
              "peak": native.mg_objective(kind=native.OBJ_PEAK, gamma=args.gamma, tail=0.0)}
    for K in ks:
        acts = env.sample_plans(H, K, key=77, step=1000)
        best = torch.empty(n, dtype=torch.int32, device=dev)
        score = torch.empty(n, dtype=torch.float64, device=dev)
        scores = torch.empty((K, n), dtype=torch.float64, device=dev)
        out = native.mg_plan_out(best=best.data_ptr(), best_score=score.data_ptr(), scores=scores.data_ptr())
        ap_ = ctypes.c_void_p(acts.data_ptr())

        def run(obj):
            if obj is None:
                native.check(lib.mg_plan(env.handle, ap_, H, K, ctypes.byref(out), st))
            else:
                native.check(lib.mg_plan_obj(env.handle, ap_, H, K, ctypes.byref(obj), ctypes.byref(out), st))

        run(None)
        ref = scores.clone()
        run(routes["final"])
        torch.cuda.synchronize()
        assert torch.equal(scores, ref)
        big = mg_envs.VecMagicalEnv(args.name, K * n, max_episode_steps=10 ** 6)
        big.reset()
        big_acts = [big.random_actions(t) for t in range(H)]
        tm = (ctypes.c_double * 4)()
        t = {key: [] for key in list(routes) + ["step_kernel_x_H"]}
        for rep in range(args.warmup + args.reps):
            row = {key: timed(lambda o=obj: run(o)) for key, obj in routes.items()}
            native.check(lib.mg_enable_timing(big.handle, H))
            for h in range(H):
                big.step(big_acts[h])
            torch.cuda.synchronize()
            native.check(lib.mg_read_timing(big.handle, tm))
            native.check(lib.mg_enable_timing(big.handle, 0))
            row["step_kernel_x_H"] = tm[0]
            if rep >= args.warmup:
                for key, v in row.items():
                    t[key].append(v)
        big.close()
        med = {key: statistics.median(v) for key, v in t.items()}
        res["K"][str(K)] = dict({key: stats(v) for key, v in t.items()},
                                over_plan={key: round(med[key] / med["plan"], 3) for key in ("final", "return", "peak")},
                                over_step_kernels={key: round(med[key] / med["step_kernel_x_H"], 3)
                                                   for key in ("plan", "return", "peak")})


def beam_bench(args, env, ks, timed, stats, res):
    """--beam: for every K, each repetition times in turn mg_plan and mg_plan_beam on the same candidates with segments
    of --seg steps and K / 4 survivors (beam), with every slot surviving (beam_all: the same launches, nothing to
    copy) and with one segment (beam_one: mg_plan's launches).  beam's plans are first checked to reproduce its values
    under mg_plan.  copy_ms = beam - beam_all is what the resamples' copies cost, tails_ms = beam_all - beam_one the
    extra launches; clone_store_gbs = the bytes the D - 1 resamples write -- (K - survivors) * N columns of a rollout's
    share of the fan pool each -- over copy_ms."""
    lib, dev, st, n, H, seg = env.lib, env.device, env._stream(), env.num_envs, args.horizon, args.seg
    D = -(-H // seg)
    free0 = torch.cuda.mem_get_info(dev)[0]
    env.plan(env.sample_plans(1, max(ks)))   # the fan pool for the largest K: later calls allocate nothing
    torch.cuda.synchronize()
    per = (free0 - torch.cuda.mem_get_info(dev)[0]) / (max(ks) * n)
    res.update(seg=seg, bytes_per_rollout=round(per, 1))
    for K in ks:
        B = max(1, K // 4)
        acts = env.sample_plans(H, K, key=77, step=1000)
        got = env.plan_beam(acts, seg, B, details=True)
        ref = env.plan(got["plans"], details=True)
        assert torch.equal(got["values"], ref["scores"]) and torch.equal(got["steps"], ref["steps"])
        assert torch.equal(got["best"], ref["best"]) and bool((got["plans"] != acts).any())
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        best, value, first = torch.empty(n, **i32), torch.empty(n, **f64), torch.empty(n, dtype=torch.uint8, device=dev)
        values, plans = torch.empty((K, n), **f64), torch.empty_like(acts)
        pout = native.mg_plan_out(best=best.data_ptr(), best_score=value.data_ptr(), first_action=first.data_ptr(),
                                  scores=values.data_ptr())
        bout = native.mg_plan_beam_out(best=best.data_ptr(), best_value=value.data_ptr(), first_action=first.data_ptr(),
                                       values=values.data_ptr())
        ap_, pp = ctypes.c_void_p(acts.data_ptr()), ctypes.c_void_p(plans.data_ptr())

        def plan():
            native.check(lib.mg_plan(env.handle, ap_, H, K, ctypes.byref(pout), st))

        def beam(sg, b):
            native.check(lib.mg_plan_beam(env.handle, ap_, pp, H, K, sg, b, None, ctypes.byref(bout), st))

        routes = {"plan": plan, "beam": lambda: beam(seg, B), "beam_all": lambda: beam(seg, K),
                  "beam_one": lambda: beam(H, B)}
        t = {key: [] for key in routes}
        for r in range(args.warmup + args.reps):
            row = {key: timed(fn) for key, fn in routes.items()}
            if r >= args.warmup:
                for key, v in row.items():
                    t[key].append(v)
        med = {key: statistics.median(v) for key, v in t.items()}
        copy_ms, written = med["beam"] - med["beam_all"], (D - 1) * (K - B) * n * per
        res["K"][str(K)] = dict({key: stats(v) for key, v in t.items()}, survivors=B,
                                beam_over_plan=round(med["beam"] / med["plan"], 3),
                                copy_ms=round(copy_ms, 4), tails_ms=round(med["beam_all"] - med["beam_one"], 4),
                                copy_share_of_beam=round(copy_ms / med["beam"], 3),
                                clone_store_gbs=round(written / (copy_ms * 1e-3) / 1e9, 1) if copy_ms > 0 else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--name", default="MoveToRegion-Demo-LoRes4E-v0")
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--candidates", default="16,64")
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20, help="env steps before the first measurement")
    ap.add_argument("--objective", action="store_true",
                    help="time mg_plan against mg_plan_obj with FINAL, RETURN and PEAK instead (see objective_bench)")
    ap.add_argument("--gamma", type=float, default=0.99, help="--objective: the discount of RETURN and PEAK")
    ap.add_argument("--beam", action="store_true", help="time mg_plan against mg_plan_beam instead (see beam_bench)")
    ap.add_argument("--seg", type=int, default=4, help="--beam: env-steps per segment")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("plan_bench: no GPU (times are measured on the device or not at all)")
    n, H, ks = args.envs, args.horizon, [int(k) for k in args.candidates.split(",")]
    env = mg_envs.VecMagicalEnv(args.name, n, max_episode_steps=10 ** 6)
    lib, dev, st = env.lib, env.device, env._stream()
    env.reset()
    for t in range(args.steps):
        env.step(env.random_actions(t))
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

    res = {"name": args.name, "envs": n, "step_form": list(env.step_form()[:2]), "H": H, "reps": args.reps, "K": {}}
    if args.objective:
        objective_bench(args, env, ks, timed, stats, res)
        print(json.dumps(res))
        env.close()
        return
    if args.beam:
        beam_bench(args, env, ks, timed, stats, res)
        print(json.dumps(res))
        env.close()
        return
    free0 = torch.cuda.mem_get_info(dev)[0]
    env.plan(env.sample_plans(1, max(ks)))   # the fan pool for the largest K: later calls allocate nothing
    torch.cuda.synchronize()
    pool = free0 - torch.cuda.mem_get_info(dev)[0]
    per = pool / (max(ks) * n)
    res["fan_pool"] = {"rollouts": max(ks) * n, "bytes": pool, "bytes_per_rollout": round(per, 1),
                       "gib_at_max_rollouts": round(per * native.PLAN_MAX_ROLLOUTS / 2 ** 30, 2)}
    for K in ks:
        acts = env.sample_plans(H, K, key=77, step=1000)                 # [H, K, N]
        cols = acts.permute(1, 0, 2).contiguous()                         # [K, H, N]: candidate k's [H][N] block
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        p_best, p_score, p_first = torch.empty(n, **i32), torch.empty(n, **f64), torch.empty(n, dtype=torch.uint8, device=dev)
        p_scores, p_steps = torch.empty((K, n), **f64), torch.empty((K, n), **i32)
        pout = native.mg_plan_out(best=p_best.data_ptr(), best_score=p_score.data_ptr(), first_action=p_first.data_ptr(),
                                  scores=p_scores.data_ptr(), steps=p_steps.data_ptr())
        l_scores, l_steps = torch.empty((K, n), **f64), torch.empty((K, n), **i32)
        louts = [native.mg_lookahead_out(score=l_scores[k].data_ptr(), steps=l_steps[k].data_ptr()) for k in range(K)]
        ap_ = ctypes.c_void_p(acts.data_ptr())
        cps = [ctypes.c_void_p(cols[k].data_ptr()) for k in range(K)]
        idx = torch.arange(n, device=dev)
        last = {}

        def plan(h=H):
            native.check(lib.mg_plan(env.handle, ap_ if h else None, h, K, ctypes.byref(pout), st))

        def k_calls(h=H):
            for k in range(K):
                native.check(lib.mg_lookahead(env.handle, cps[k] if h else None, h, ctypes.byref(louts[k]), st))
            best = l_scores.argmax(dim=0)
            last["best"], last["score"], last["first"] = best, l_scores[best, idx], acts[0, best, idx]

        plan(), k_calls()
        torch.cuda.synchronize()
        assert torch.equal(p_scores, l_scores) and torch.equal(p_steps, l_steps) and int(p_steps.min()) == H
        assert torch.equal(p_best.long(), last["best"]) and torch.equal(p_score, last["score"])
        assert torch.equal(p_first, last["first"])
        t = {"plan": [], "k_calls": [], "plan_h0": [], "k_calls_h0": []}
        for rep in range(args.warmup + args.reps):
            row = {"plan": timed(plan), "k_calls": timed(k_calls), "plan_h0": timed(lambda: plan(0)),
                   "k_calls_h0": timed(lambda: k_calls(0))}
            if rep >= args.warmup:
                for key, v in row.items():
                    t[key].append(v)
        med = {key: statistics.median(v) for key, v in t.items()}
        res["K"][str(K)] = dict({key: stats(v) for key, v in t.items()},
                                k_calls_over_plan=round(med["k_calls"] / med["plan"], 3),
                                k_calls_h0_over_plan_h0=round(med["k_calls_h0"] / med["plan_h0"], 3),
                                copy_share_of_plan=round(med["plan_h0"] / med["plan"], 3),
                                rollout_steps_per_s=round(K * n * H / (med["plan"] * 1e-3)))
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
