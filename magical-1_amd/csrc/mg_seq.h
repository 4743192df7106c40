// mg_seq.h -- the step-sequence kernel template (mg_step_seq: up to R env-steps of physics on the LIVE envs in one
// launch, then mg_step's episode bookkeeping and auto-reset once) and its launcher.  One instantiation per (form, envs
// per workgroup) pair of the step kernel's table (mg_stepforms.h), in translation units of their own (mg_seq_quad.hip:
// 5 / 6, mg_seq_v4.hip: 4, mg_seq_hbm.hip: 0); mg_physics.hip dispatches.
//
// The kernel is step_kernel's lane map (mg_lanes.h), the env-step loop (mg_rollout.h: the scene check, the loop and its
// barrier protocol, one text shared with lookahead_kernel) and then step_kernel's tail per env on its scoring lane, from
// the HBM column: episode_steps (+n), score_env if terminal, reward / done / eval_score / steps, the fused reset_env,
// reset_mask.  So the state after the call has the bits that n calls of mg_step leave.  Running every env's tail after
// the loop keeps barrier participation simple: the envs of one workgroup end at different h.
//
// Env e runs n = min(R, max(max_steps - episode_steps, 1)) env-steps (R when max_steps <= 0): only step n can end the
// episode, and an env already past its end takes one step, as mg_step does.
//
// Debug-reward sims (cfg.flags & MG_DEBUG_REWARD) pay r_k after every env-step, so there the env's column goes back to
// HBM after EVERY env-step of its n and the scoring lane evaluates debug_reward there, summing left to right in double.
// That is the EACH instantiation of every pair (the loop's EVERY), chosen by the launch from the sim's flag: as a
// kernel argument, uniform over the launch, it cost the plain path scratch in the quad forms ("Step
// sequences", has the figures of both).
#pragma once
#include "mg_stepk.h"

// actions: u8[R][n_envs], step-major; steps_out: i32[n_envs] or null; the rest as step_kernel's
template <int VAR, int BLK, bool EACH>
__global__ void __launch_bounds__(64) step_seq_kernel(MGState S, const mg_library *__restrict__ L, TaskCfg cfg, int max_steps,
                                                      int auto_reset, const uint8_t *__restrict__ actions, int R, float *reward,
                                                      uint8_t *done, double *eval_score, int32_t *steps_out,
                                                      uint8_t *reset_mask) {
    extern __shared__ __align__(16) unsigned char smem[];
    using F = StepForm<VAR, BLK>;
#include "mg_lanes.h"
    const uint8_t *act = actions + e;   // step h: act[h * n_envs], h < n <= R and e < n_envs
    const size_t astride = (size_t)S.n_envs;
    int n = R;
    if (max_steps > 0) {
        const int left = max_steps - S.episode_steps[e];
        const int l1 = left < 1 ? 1 : left;
        n = l1 < R ? l1 : R;
    }
    [[maybe_unused]] double racc = 0.0;   // EACH: r_1 + ... + r_k so far, on the env's scoring lane
    // a refused env writes what step_kernel's does and ends
#define MG_ROLLOUT_EVERY EACH
#define MG_ROLLOUT_IF_BOTH(a, b) if (a) if (b)
#define MG_ROLLOUT_REFUSE() do { if (reset_mask) reset_mask[e] = 0; if (steps_out) steps_out[e] = 0; } while (0)
#define MG_ROLLOUT_REFUSED_COOP() do { } while (0)
#define MG_ROLLOUT_REFUSED_TAIL false
#define MG_ROLLOUT_AFTER_STEP(h) \
    do { const double r = debug_reward(S, L, e, cfg.task); racc = (h) == 0 ? r : racc + r; } while (0)
#include "mg_rollout.h"
    // step_kernel's tail, once, after the env's n env-steps
    int steps = S.episode_steps[e] + n;
    S.episode_steps[e] = steps;
    bool d = max_steps > 0 && steps >= max_steps;
    double sc = d ? score_env(S, L, e, cfg.task) : 0.0;
    // r_1 + ... + r_n, left to right: without the debug reward r_k = 0.0 for k < n and r_n = sc
    const double rsum = EACH ? racc : n == 1 ? sc : 0.0 + sc;
    if (reward) reward[e] = (float)rsum;
    if (done) done[e] = d ? 1 : 0;
    if (eval_score) eval_score[e] = sc;
    if (steps_out) steps_out[e] = n;
    if constexpr (F::QUAD) {
        if (cfg.fused_reset && d && auto_reset) {
            TaskCfg rc = cfg;
            rc.coop = 0;
            reset_env<VAR == 5 ? MG_TASK_MOVE_TO_REGION : MG_TASK_MOVE_TO_CORNER, 0>(S, L, e, rc);
        }
    }
    if (reset_mask) reset_mask[e] = (d && auto_reset && !cfg.fused_reset) ? 1 : 0;
}

// EACH: the sim pays the debug reward (cfg.flags & MG_DEBUG_REWARD)
template <int VAR, int BLK>
hipError_t launch_step_seq_var(const MGState &S, const mg_library *L, TaskCfg cfg, int max_steps, int auto_reset,
                               const uint8_t *actions, int R, float *reward, uint8_t *done, double *eval_score,
                               int32_t *steps, uint8_t *reset_mask, hipStream_t st) {
    if (cfg.flags & MG_DEBUG_REWARD)
        return launch_env_kernel<step_seq_kernel<VAR, BLK, true>, VAR, BLK>("step_seq", S, st, L, cfg, max_steps, auto_reset,
                                                                            actions, R, reward, done, eval_score, steps,
                                                                            reset_mask);
    return launch_env_kernel<step_seq_kernel<VAR, BLK, false>, VAR, BLK>("step_seq", S, st, L, cfg, max_steps, auto_reset,
                                                                         actions, R, reward, done, eval_score, steps,
                                                                         reset_mask);
}

// a translation unit instantiates its row of the form table: MG_STEP_FORMS_QUAD(MG_SEQ_INSTANTIATE)
#define MG_SEQ_INSTANTIATE(F, B) \
    template hipError_t launch_step_seq_var<F, B>(const MGState &, const mg_library *, TaskCfg, int, int, const uint8_t *, \
                                                  int, float *, uint8_t *, double *, int32_t *, uint8_t *, hipStream_t);
