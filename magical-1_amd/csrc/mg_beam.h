// mg_beam.h -- mg_plan_beam's own kernels (mg_beam.hip): the per-env choice of survivors and parent slots after a
// segment, the in-pool resample that clones the parents' columns onto the losers' (state rows and the plans' history),
// and the outputs of the last segment.  The fan-out, the rollouts, the best-of-K reduction and the fan pool are
// mg_plan's, the survivor threshold is mg_plan_cem's, all launched unchanged (mg_plan.h, mg_cem.h, mg_lookahead.h);
// mg_plan_beam and its segment loop are in mg_beam.hip as well.
//
// Layouts (n = num_envs): values f64[K][n], parents i32[K][n], plans u8[H][K][n] as mg_plan's candidates; slot k of env
// e is rollout k * n + e of the fan pool, column k * n + e of each of its rows -- everything that runs along e is
// coalesced.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mg_plan.h"

// After a segment: slot k survives iff s > thr || (s == thr && k <= k_thr) (mg_launch_cem_threshold with E = B, which
// leaves exactly B survivors per env).  parent[k][e] = k for a survivor; the j-th loser in ascending k gets the
// (j mod B)-th survivor in ascending k.  surv: scratch i32[B][n] (the survivor list).  Also episode_steps[k * n + e] +=
// seg_steps[k * n + e] for every slot: the pool's episode counter, which the lookahead kernel does not keep
hipError_t mg_launch_beam_select(const double *values, const double *thr, const int32_t *k_thr, const int32_t *seg_steps,
                                 int32_t *episode_steps, int n_envs, int K, int B, int32_t *surv, int32_t *parent,
                                 hipStream_t st);
// column k * n_envs + e <- column parent[k][e] * n_envs + e of every row, where parent[k][e] != k; both sides in `pool`
// (PlanRow.src and .dst are the pool's own offsets).  Parents are survivors (parent[parent[k][e]][e] == parent[k][e]):
// no column is both read and written
hipError_t mg_launch_beam_clone(char *pool, const PlanRow *rows_dev, int nrows, const int32_t *parent, int n_envs, int K,
                                hipStream_t st);
// plans[h][k][e] <- plans[h][parent[k][e]][e] for h < hend, where parent[k][e] != k
hipError_t mg_launch_beam_history(uint8_t *plans, const int32_t *parent, int hend, int n_envs, int K, hipStream_t st);
// after the last segment: steps[k][e] = the lineage's env-steps = pool episode_steps + seg_steps - the env's own counter
hipError_t mg_launch_beam_steps(const int32_t *pool_episode_steps, const int32_t *seg_steps, const int32_t *env_episode_steps,
                                int n_envs, int K, int32_t *steps, hipStream_t st);
// best_plan[h][e] = plans[h][best[e]][e]
hipError_t mg_launch_beam_gather(const uint8_t *plans, const int32_t *best, int H, int n_envs, int K, uint8_t *best_plan,
                                 hipStream_t st);
