// mg_lookahead.h -- the lookahead kernel template (mg_lookahead: H env-steps of physics on a scratch copy of the
// state, then the task's score) and its launcher.  One instantiation per (form, envs per workgroup) pair of the
// step kernel's table (mg_stepforms.h), in translation units of their own (mg_look_quad.hip: 5 / 6, mg_look_v4.hip:
// 4, mg_look_hbm.hip: 0); mg_lookahead.hip dispatches.
//
// The kernel is step_kernel's lane map (mg_lanes.h), the env-step loop (mg_rollout.h: the scene check, the loop and its
// barrier protocol, one text shared with step_seq_kernel, and why an env's state after h iterations has the bits that h
// calls of mg_step give it) and then its own tail.  S is the sim's scratch pool (never its own state), and there is no
// episode counter, reward, done flag or reset -- only the outputs of LookOut.
//
// TRACE (mg_lookahead_obj, mg_plan_obj, mg_plan_cem_obj; a second instantiation of every pair; the loop's EVERY): the
// env's view goes back to its scratch column after EVERY env-step, as mg_step's does, and the env's scoring lane
// evaluates the task's score s_k and mg_step's reward r_k there with score_env / debug_reward as they are -- the bits of
// mg_step's scoring by construction -- and accumulates the objective (LookObj, mg_launch.h; the definitions:
// include/magical_sim.h and DESIGN.md).  mg_plan_beam continues an objective over several launches on one pool through
// LookObj.carry: the accumulators are stored per rollout on exit and, when the carry says so, loaded on entry in place
// of obj_begin.
#pragma once
#include "mg_stepk.h"

// the outputs (LookOut: mg_launch.h) of env e from the scratch state S after its n simulated env-steps (one lane per
// env).  SCORE = false (TRACE): the caller has s_n already and stores it itself
template <bool SCORE = true>
MG_DEV void look_emit(const MGState &S, const mg_library *L, int e, int task, int n, const LookOut &o) {
    if constexpr (SCORE) o.score[e] = score_env(S, L, e, task);
    if (o.steps) o.steps[e] = n;
    if (o.errors) o.errors[e] = S.overflow[e];
    env_bodies_record(S, e, o.bodies, o.counts);
}

// ---- TRACE: the objective's accumulators, in registers of the env's scoring lane --------------------------------
// Every operation is one rounded double operation (no contraction: -ffp-contract=off), in the order of the
// definitions: g_0 = 1, g_k = g_{k-1} * gamma; G += g_{k-1} * r_k; v = g_k * s_k, P = v and kp = k when v > P.
struct ObjAcc {
    double G, P, g, s;   // the return so far, the peak so far, g_k, s_k (k: env-steps done)
    int kp;
    int k0;              // env-steps done in earlier launches (LookCarry; 0 without one): kp counts from the first launch
    bool ended;          // one of those steps ended the episode
};

// x_0: the scratch column as the fan-out copy left it (called before the env's first write-back)
MG_DEV void obj_begin(ObjAcc &a, const MGState &S, const mg_library *L, int e, int task) {
    a.s = score_env(S, L, e, task);
    a.G = 0.0; a.P = a.s; a.g = 1.0; a.kp = 0;
    a.k0 = 0; a.ended = false;
}

// the same with a carry (o.carry.G not null, e < n_envs) that says load: the accumulators as the earlier launches left
// them; s_k is scored from the scratch column, which holds x_k -- the bits the earlier launch's last obj_step got
MG_DEV void obj_resume(ObjAcc &a, const MGState &S, const mg_library *L, int e, int task, const LookCarry &c) {
    a.s = score_env(S, L, e, task);
    a.G = c.G[e]; a.P = c.P[e]; a.g = c.g[e]; a.kp = c.kp[e];
    a.k0 = c.k[e]; a.ended = c.ended[e] != 0;
}

// after env-step k = h + 1, with x_k in the scratch column (h < n <= H and e < n_envs: the trace index h * n_envs + e
// lies inside f64[H][n_envs]); done: the step ends the episode, as mg_step decides it
MG_DEV void obj_step(ObjAcc &a, const MGState &S, const mg_library *L, int e, int task, int h, bool done, const LookObj &o) {
    const double s = score_env(S, L, e, task);
    const double r = o.debug ? debug_reward(S, L, e, task) : done ? s : 0.0;   // the double mg_step casts to float
    a.G = a.G + a.g * r;
    a.g = a.g * o.gamma;
    const double v = a.g * s;
    if (v > a.P) { a.P = v; a.kp = a.k0 + h + 1; }
    a.s = s;
    const size_t i = (size_t)h * (size_t)S.n_envs + (size_t)e;
    if (o.score_trace) o.score_trace[i] = s;
    if (o.reward_trace) o.reward_trace[i] = r;
}

// the env's outputs after its n env-steps: LookOut as look_emit's (score = s_n), the objective's, and the trace rows
// h in [n, H) (score clamped to s_n, reward 0)
MG_DEV void obj_emit(const ObjAcc &a, const MGState &S, const mg_library *L, int e, int task, int n, int H, bool done_n,
                     const LookOut &out, const LookObj &o) {
    if (out.score) out.score[e] = a.s;
    look_emit<false>(S, L, e, task, n, out);
    double G = a.G;
    const bool ends = n >= 1 && done_n;
    if (o.carry.G) {   // (before the tail term: the next launch adds to the sum itself)
        const LookCarry &c = o.carry;
        c.G[e] = a.G; c.P[e] = a.P; c.g[e] = a.g; c.kp[e] = a.kp;
        c.k[e] = a.k0 + n; c.ended[e] = (a.ended || ends) ? 1 : 0;
    }
    if (!ends && !a.ended) G = G + (a.g * o.tail) * a.s;   // the episode goes on past the horizon: its tail value
    if (o.value) o.value[e] = o.kind == LOOK_OBJ_RETURN ? G : o.kind == LOOK_OBJ_PEAK ? a.P : a.s;
    if (o.peak) o.peak[e] = a.P;
    if (o.peak_step) o.peak_step[e] = a.kp;
    for (int h = n; h < H; h++) {
        const size_t i = (size_t)h * (size_t)S.n_envs + (size_t)e;
        if (o.score_trace) o.score_trace[i] = a.s;
        if (o.reward_trace) o.reward_trace[i] = 0.0;
    }
}

// S: the scratch pool, holding a copy of every env's state.  actions: u8[H][n_envs], step-major.  Env e runs
// n = min(H, max_steps - episode_steps) env-steps (H when max_steps <= 0).  obj: read by TRACE only.
template <int VAR, int BLK, bool TRACE = false>
__global__ void __launch_bounds__(64) lookahead_kernel(MGState S, const mg_library *__restrict__ L, int task, int max_steps,
                                                       const uint8_t *__restrict__ actions, int H, LookOut out, LookObj obj) {
    extern __shared__ __align__(16) unsigned char smem[];
    using F = StepForm<VAR, BLK>;
#include "mg_lanes.h"
    const uint8_t *act = actions + e;   // step h: act[h * n_envs], h < H and e < n_envs
    const size_t astride = (size_t)S.n_envs;
    int n = H;
    if (max_steps > 0) {
        const int left = max_steps - S.episode_steps[e];
        n = left < 0 ? 0 : left < H ? left : H;
    }
    // TRACE: env-step n ends the episode (mg_step: max_steps > 0 && episode_steps + n >= max_steps; n <= left, so
    // no earlier step does).  The scoring lane -- the one lane of the env that reaches the outputs at the end -- holds
    // the accumulators; it scores x_0 here, before anything is written to the env's scratch column (the first
    // write-back lies behind the first env-step's barriers, which that lane takes part in)
    [[maybe_unused]] bool done_n = false;
    [[maybe_unused]] ObjAcc acc;
    if constexpr (TRACE) {
        done_n = max_steps > 0 && n >= 1 && S.episode_steps[e] + n >= max_steps;
        if (!shadow && (F::COOP ? lane == 0 : sub == 0)) {
            if (obj.carry.G && obj.carry.load) obj_resume(acc, S, L, e, task, obj.carry);
            else obj_begin(acc, S, L, e, task);
        }
    }
    // a refused env has its error flag in the scratch's `overflow` and emits its outputs with n = 0
#define LOOK_EMIT(steps, ends) \
    do { \
        if constexpr (TRACE) obj_emit(acc, S, L, e, task, (steps), H, (ends), out, obj); \
        else look_emit(S, L, e, task, (steps), out); \
    } while (0)
#define MG_ROLLOUT_EVERY TRACE
#define MG_ROLLOUT_IF_BOTH(a, b) if ((a) && (b))
#define MG_ROLLOUT_REFUSE() do { } while (0)
#define MG_ROLLOUT_REFUSED_COOP() do { if (lane == 0) LOOK_EMIT(0, false); } while (0)
#define MG_ROLLOUT_REFUSED_TAIL true
#define MG_ROLLOUT_AFTER_STEP(h) obj_step(acc, S, L, e, task, (h), done_n && (h) + 1 == n, obj)
#include "mg_rollout.h"
    LOOK_EMIT(n, done_n);
#undef LOOK_EMIT
}

template <int VAR, int BLK, bool TRACE>
hipError_t launch_look(const MGState &S, const mg_library *L, int task, int max_steps, const uint8_t *actions, int H,
                       const LookOut &out, const LookObj &obj, hipStream_t st) {
    return launch_env_kernel<lookahead_kernel<VAR, BLK, TRACE>, VAR, BLK>("lookahead", S, st, L, task, max_steps, actions, H,
                                                                         out, obj);
}

// a translation unit instantiates its row of the form table, plain and TRACE: MG_STEP_FORMS_QUAD(MG_LOOK_INSTANTIATE)
#define MG_LOOK_INSTANTIATE_ONE(F, B, TRACE) \
    template hipError_t launch_look<F, B, TRACE>(const MGState &, const mg_library *, int, int, const uint8_t *, int, \
                                                 const LookOut &, const LookObj &, hipStream_t);
#define MG_LOOK_INSTANTIATE(F, B) MG_LOOK_INSTANTIATE_ONE(F, B, false) MG_LOOK_INSTANTIATE_ONE(F, B, true)
