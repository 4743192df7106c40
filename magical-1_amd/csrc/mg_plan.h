// mg_plan.h -- mg_plan's own kernels (mg_plan.hip): the fan-out copy of the sim's state into the fan pool, the
// best-of-K reduction and the candidate sampler of mg_plan_sample.  The rollouts themselves are the lookahead kernel
// (mg_lookahead.h), launched unchanged on the fan pool; the C ABI, the pool and its allocation live in mg_sim.hip.
//
// The fan pool is an MGState of M = K * num_envs envs, laid out as the lookahead scratch is (every [slot][Mpad] row,
// no frame rings).  Rollout r = k * num_envs + e -- candidate k of env e -- is its env r, so one candidate's envs are
// contiguous in every row and everything that runs along e is coalesced: the copy's stores, the action bytes
// (u8[H][K][num_envs] is u8[H][M]), the [K][num_envs] outputs and the reduction's reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// one state row of the fan-out: env e's element at src_pool + src + e * esize, rollout r's at dst_pool + dst + r * esize
struct PlanRow { uint64_t src, dst; uint32_t esize, pad; };

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
