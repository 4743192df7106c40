// mg_plan.h -- rollout pools and mg_plan's own kernels (mg_plan.hip, with mg_plan / mg_plan_sample and the pools'
// allocation): the fan-out copy of the sim's state into a rollout pool, the best-of-K reduction and the candidate
// sampler of mg_plan_sample.  The rollouts themselves are the lookahead kernel (mg_lookahead.h), launched unchanged on
// the pool.
//
// A rollout pool is a StatePool of M = K * num_envs envs (every [slot][Mpad] row, no frame rings); mg_lookahead's is
// the case K = 1.  Rollout r = k * num_envs + e -- candidate k of env e -- is its env r, so one candidate's envs are
// contiguous in every row and everything that runs along e is coalesced: the copy's stores, the action bytes
// (u8[H][K][num_envs] is u8[H][M]), the [K][num_envs] outputs and the reduction's reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mg_pool.h"

// one state row of the fan-out: env e's element at src_pool + src + e * esize, rollout r's at dst_pool + dst + r * esize
struct PlanRow { uint64_t src, dst; uint32_t esize, pad; };

// One allocation (P.mem) holds the state rows, the rollouts' scores (f64[P.S.N]: the reduction's input also when the
// caller wants no scores), the device table of the fan-out's rows (the rollout rows of the sim's pool zipped with this
// pool's), mg_plan_cem's per-env scratch, the elite threshold (cem_thr f64[num_envs], cem_kthr i32[num_envs]), and
// mg_plan_beam's per-rollout scratch (mg_beam.h), every array [P.S.N]: the objective's carry (LookCarry's arrays), a
// segment's env-steps, the survivor list and the parent slots, and the table of the rows a resample clones -- this
// pool's rollout rows on both sides, then the carry's six
struct RolloutPool {
    StatePool P;
    PlanRow *rows = nullptr;
    int nrows = 0;
    int cap = 0;   // rollouts
    double *scores = nullptr;
    double *cem_thr = nullptr;
    int32_t *cem_kthr = nullptr;
    double *beam_G = nullptr, *beam_P = nullptr, *beam_g = nullptr;
    int32_t *beam_kp = nullptr, *beam_k = nullptr, *beam_ended = nullptr;
    int32_t *beam_steps = nullptr, *beam_surv = nullptr, *beam_parent = nullptr;
    PlanRow *beam_rows = nullptr;
    int beam_nrows = 0;   // with the carry's rows, which come last (a FINAL resample clones beam_nrows - 6)
};

// dst column k * n_envs + e <- src column e, for every row, k < K and e < n_envs
hipError_t mg_launch_plan_fan(const char *src_pool, char *dst_pool, const PlanRow *rows_dev, int nrows, int n_envs, int K,
                              hipStream_t st);
// best[e] = argmax_k scores[k * n_envs + e] (strict >: the lowest k wins a tie); best_score / first_action may be null;
// actions (u8[H][K][n_envs]) may be null when H = 0, and first_action is then left unwritten
hipError_t mg_launch_plan_reduce(const double *scores, const uint8_t *actions, int H, int n_envs, int K, int32_t *best,
                                 double *best_score, uint8_t *first_action, hipStream_t st);
// out u8[H][K][n_envs]: row [h][k] = the actions mg_random_actions draws at step + k * ceil(H / repeat) + h / repeat
hipError_t mg_launch_plan_sample(uint8_t *out, int n_envs, int H, int K, int repeat, uint64_t key, uint64_t step,
                                 hipStream_t st);
