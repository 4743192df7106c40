// mg_seq.h -- the step-sequence kernel template (mg_step_seq: up to R env-steps of physics on the LIVE envs in one
// launch, then mg_step's episode bookkeeping and auto-reset once) and its launcher.  One instantiation per (form, envs
// per workgroup) pair of the step kernel's table (mg_stepforms.h), in translation units of their own (mg_seq_quad.hip:
// 5 / 6, mg_seq_v4.hip: 4, mg_seq_hbm.hip: 0); mg_physics.hip dispatches.
//
// The kernel is step_kernel (mg_stepk.h) with lookahead_kernel's env-step loop (mg_lookahead.h) inside: step_kernel's
// lane map, scene checks and error paths, ONE load of the LDS view, the env_substeps_* calls in step_kernel's order for
// h < n, the env's column written back at its own last step, and then step_kernel's tail per env on its scoring lane,
// from the HBM column: episode_steps (+n), score_env if terminal, reward / done / eval_score / steps, the fused
// reset_env, reset_mask.  So the state after the call has the bits that n calls of mg_step leave (everything is compiled
// with -ffp-contract=off; what the view does not carry from one env-step to the next is recomputed before use in every
// env-step, as the lookahead's header says).  Running every env's tail after the loop keeps barrier participation simple:
// the envs of one workgroup end at different h.
//
// Env e runs n = min(R, max(max_steps - episode_steps, 1)) env-steps (R when max_steps <= 0): only step n can end the
// episode, and an env already past its end takes one step, as mg_step does.
//
// Debug-reward sims (cfg.flags & MG_DEBUG_REWARD) pay r_k after every env-step, so there the env's column goes back to
// HBM after EVERY env-step of its n and the scoring lane evaluates debug_reward there, as the lookahead's traced form
// does, summing left to right in double.  That is the EACH instantiation of every pair, chosen by the launch from the
// sim's flag: as a kernel argument, uniform over the launch, it cost the plain path scratch in the quad forms (DESIGN.md,
// "Step sequences", has the figures of both).  Everything EACH adds is under `if constexpr (EACH)`.
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
    constexpr StepCaps C = F::C;
    const int lane = F::COOP ? (int)threadIdx.x : F::QUAD ? (int)threadIdx.x / F::QL : BLK == 1 ? 0 : (int)threadIdx.x;
    const int sub = F::QUAD ? (int)threadIdx.x % F::QL : 0;
    int e = xcd_block(blockIdx.x, gridDim.x) * BLK + (F::COOP ? 0 : lane);
    // QUAD: lanes without an env of their own (past n_envs, or a scene the form cannot hold) take part in the
    // workgroup barriers as shadows of a valid env and never write HBM: step_kernel's convention
    bool shadow = false;
    if (e >= S.n_envs) {
        if (!F::QUAD) return;
        shadow = true;
        e = S.n_envs - 1;
    }
    const uint8_t *act = actions + e;   // step h: act[h * n_envs], h < n <= R and e < n_envs
    const size_t astride = (size_t)S.n_envs;
    int n = R;
    if (max_steps > 0) {
        const int left = max_steps - S.episode_steps[e];
        const int l1 = left < 1 ? 1 : left;
        n = l1 < R ? l1 : R;
    }
    [[maybe_unused]] double racc = 0.0;   // EACH: r_1 + ... + r_k so far, on the env's scoring lane
    MGProf P;
    MG_PP_INIT(P);
    if constexpr (F::LDS) {
        bool fits = true;
        if (S.nbodies[e] > C.nb || S.nshapes[e] > C.ns || S.ncons[e] > C.nc) {
            if (!shadow && sub == 0) {
                S.overflow[e] |= 16; // scene larger than the variant's LDS caps (never expected)
                if (reset_mask) reset_mask[e] = 0;
                if (steps_out) steps_out[e] = 0;
            }
            if (!F::QUAD) return;
            fits = false;
        }
        bool ok = F::NCS == 0 || (S.ncons[e] == C.nc && S.robot_body0[e] == 0 && S.robot_cons0[e] == 0);
        for (int c = 0; c < F::NCS; c++) {
            const ConsDesc d = static_cons(c);
            ok = ok && AT(S.ctype, c) == d.type && AT(S.ca, c) == d.a && AT(S.cb, c) == d.b;
        }
        for (int k = 0; k < S.nshapes[e] && k < C.ns && F::NCS > 0; k++) ok = ok && shape_body_slot(AT(S.sbody, k)); // arb_body
        if (!ok && fits) { // the compiled constraint list does not describe this scene (never expected)
            if (!shadow && sub == 0) {
                S.overflow[e] |= 32;
                if (reset_mask) reset_mask[e] = 0;
                if (steps_out) steps_out[e] = 0;
            }
            if (!F::QUAD) return;
        }
        MGState V = S;
        carve_view(V, smem, C, BLK);
        if constexpr (F::QUAD) {
            const bool own = !shadow && fits && ok;
            if (!own) n = 0;
            xfer_state_quad<C.nb, C.ns, C.nc, C.na, F::QL>(S, V, lane, e, sub);
            if (!fits && sub == 0) { // an empty scene in the env's column: nothing indexes past the caps
                V.nbodies[lane] = 0; V.nshapes[lane] = 0; V.ncons[lane] = 0; V.nactive[lane] = 0;
            }
            // every lane meets the workgroup barriers until the workgroup's longest env is done (all 64 lanes are
            // here: nothing has returned in a quad form)
            int hw = n;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const int o = __shfl_xor(hw, off, 64);
                hw = o > hw ? o : hw;
            }
            for (int h = 0; h < hw; h++) {
                env_substeps_quad<F::NCS, F::QL>(V, L, lane, sub, act[h * astride], P);   // (h < hw <= R) ends with a workgroup barrier
                if constexpr (EACH) {
                    // every env-step of the env's own n: its column goes back from its own lanes between that closing
                    // barrier and the one below (no lane writes the view there); the fence and barrier publish the rows
                    // to the env's sub-lane 0, which evaluates the reward from HBM while the others run on into the next
                    // env-step's opening barrier.  hw is uniform over the workgroup and nothing returns or
                    // breaks inside the loop, so all 64 lanes reach this barrier exactly hw times
                    if (own && h < n) xfer_state(S, V, C, lane, e, false, false, sub, F::QL);
                    __threadfence_block();
                    __syncthreads();
                    if (own && sub == 0 && h < n) {
                        const double r = debug_reward(S, L, e, cfg.task);
                        racc = h == 0 ? r : racc + r;
                    }
                } else {
                    // the env's last step: its column goes back from its own lanes, between that barrier and the next
                    // env-step's opening one (no lane writes the view there); afterwards the env goes on in LDS as a
                    // shadow does and does not write HBM again before its tail
                    if (own && h + 1 == n) xfer_state(S, V, C, lane, e, false, false, sub, F::QL);
                }
            }
            // the env's lane 0 scores from HBM rows its sibling lanes wrote back: ordered by the memory model (as
            // step_kernel)
            __threadfence_block();
            __syncthreads();
            if (!own || sub != 0) return;
        } else {   // COOP: n >= 1, uniform over the workgroup (one env)
            xfer_state(S, V, C, 0, e, true, true, lane, 64);
            __syncthreads();
            for (int h = 0; h < n; h++) {
                env_substeps_coop(V, L, lane, act[h * astride], P);   // ends with a workgroup barrier
                if constexpr (EACH) {
                    // all 64 lanes write the view back, fence and barrier, then lane 0 evaluates the reward from HBM; the
                    // view is next written behind the next env-step's first barrier, which waits for lane 0
                    xfer_state(S, V, C, 0, e, false, true, lane, 64);
                    __threadfence_block();
                    __syncthreads();
                    if (lane == 0) {
                        const double r = debug_reward(S, L, e, cfg.task);
                        racc = h == 0 ? r : racc + r;
                    }
                }
            }
            if constexpr (!EACH) xfer_state(S, V, C, 0, e, false, true, lane, 64);
            __threadfence_block();
            __syncthreads();
            if (lane != 0) return;
        }
    } else {
        for (int h = 0; h < n; h++) {
            env_substeps(S, L, e, act[h * astride], P);
            if constexpr (EACH) {
                const double r = debug_reward(S, L, e, cfg.task);
                racc = h == 0 ? r : racc + r;
            }
        }
    }
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
