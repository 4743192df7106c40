// mg_cem.h -- mg_plan_cem's own kernels (mg_cem.hip): the elite threshold of an iteration's scores and the per-slot
// update (refit of the sampling weights to the elites, draw of the next iteration's candidates).  The rollouts, the
// fan-out and the best-of-K reduction are mg_plan's, launched unchanged (mg_plan.h, mg_lookahead.h); mg_plan_cem and its
// iteration loop are in mg_cem.hip as well.
//
// Layouts (n = num_envs, J = ceil(H / repeat) held-action slots): candidates u8[H][K][n] as mg_plan takes them,
// scores f64[K][n], weights u16[J][18][n] -- slot j, action a, env e at (j * 18 + a) * n + e -- so everything that
// runs along e is coalesced.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define MG_CEM_ACTIONS 18

// per env the E-th ranked candidate (score descending, the lower k first among equal scores): its score to thr[e], its
// index to k_thr[e].  Candidate k is an elite iff s > thr || (s == thr && k <= k_thr).  1 <= E <= K; no NaN scores
hipError_t mg_launch_cem_threshold(const double *scores, int n_envs, int K, int E, double *thr, int32_t *k_thr,
                                   hipStream_t st);

struct CemUpdate {
    uint8_t *actions;        // u8[H][K][n]: read (refit) at the slots' first rows, written (draw) at every row
    uint16_t *weights;       // u16[J][18][n]
    const double *scores;    // refit: f64[K][n] of the candidates in `actions`
    const double *thr;       // refit: mg_launch_cem_threshold's outputs
    const int32_t *k_thr;
    const int32_t *best;     // refit: i32[n], the candidates' best (mg_launch_plan_reduce)
    int n_envs, H, K, J, repeat, alpha;
    int refit;               // weights <- alpha + elite counts of `actions`, written out
    int uniform;             // without refit: 1 = draw from all-ones weights, 0 = from `weights` as they are
    int draw;                // fill `actions` with K draws per slot from the weights, counters from `counter` on
    int incumbent;           // draw after a refit: candidate 0 <- the refitted candidates' column best[e]
    uint64_t key, counter;   // candidate k's slot j draws at counter + k * J + j
};
// one thread per (slot, env): refit, then draw, as the flags say
hipError_t mg_launch_cem_update(const CemUpdate &u, hipStream_t st);
