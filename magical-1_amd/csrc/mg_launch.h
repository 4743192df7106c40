// mg_launch.h -- host-side launchers of the device kernels (one translation unit per kernel family: mg_reset.hip,
// mg_step_*.hip with their dispatch in mg_physics.hip, mg_raster.hip).  The C ABI calls them from the unit that holds the
// feature (mg_sim.h lists which).  The step kernel's forms, slot caps and LDS view: mg_stepforms.h.
#pragma once
#include <hip/hip_runtime.h>
#include "mg_state.h"
#include "mg_stepforms.h"

// coop: one env per 64-lane wave (reset_kernel_coop); fused_reset: the step kernel runs the auto-reset of its
// done envs itself (robot scenes without layout randomisation, mg_step)
struct TaskCfg { int task, flags, coop, fused_reset; };

struct RenderOut {
    uint8_t *full;        // [N][2][384][384][3] (full-resolution mode) or null
    uint8_t *obs_allo;    // LoRes outputs (layout per preproc), or null
    uint8_t *obs_ego;
    uint8_t *obs_past;
    const uint8_t *mask;  // reset mask: envs with mask[e] == 0 are left untouched (null: all)
    int preproc;
    int frames_only;      // 1: obs_allo / obs_ego get the current [N][96][96][3] frames only (no stacks, no ring)
    int debug_skip;      // profiling builds only: 1 skip outlines, 2 skip fill, 4 skip HBM stores, 8 skip spans
    int small;            // 1: robot + arena + goal + one block at most (MoveToRegion, MoveToCorner) -> small LDS class
    int retry_in;         // set by mg_launch_render: class chain, render only the pairs at this class's level
                          // (S.rg_retry: the level that holds each (env, view) this episode)
    int retry_out;        // ... a pair this class cannot hold moves to the next level (else an env error)
    int cls_level;        // ... position of this class in the chain
    int first_level;      // ... the chain's first class for this task (0: medium-0, 1: medium-1)
    int force_retry;      // tests: classes below this level hand every pair on (1: skip the first, 2: the first two)
    int scache_mode;      // tests / A-B (MG_DEBUG_SCACHE): 1 = no allocentric static layer, 2 = its copied blocks
                          // poisoned (0x55) -- shows where the layer is used
    // window rings (mg_bind_window): a stacked view writes its current frame channel-planar into
    // wring[view] u8[N][wK + 3][3][96][96] (slot wpos = step % wK, and wK + wpos when wpos < 3; a fresh env the
    // slots of frames step-3 .. step) instead of its [96][96][12] stack and frame ring; null: the stack as before
    uint8_t *wring[2];
    int wK, wpos;
    int wnsl[2];              // window slots of this step's frame: [0] a running env (wpos, and wK + wpos when
    int8_t wsl[2][8];         // wpos < 3), [1] a fresh env (the slots of frames step-3 .. step, with duplicates)
};

hipError_t mg_launch_seed(const MGState &S, const uint32_t *seeds_dev, hipStream_t st);
// mg_selftest_mt: one wavefront per seed draws ndraws words through mt_next32's twist path `mode` (0 HBM, 1 LDS with
// 64 lanes, 2 LDS with lanes 0-36).  key / pos: scratch u32[624][n] / i32[n]; out: u32[n][ndraws], mode 2 twice that
hipError_t mg_launch_selftest_mt(const uint32_t *seeds_dev, int n, int ndraws, int mode, uint32_t *key, int32_t *pos,
                                 uint32_t *out, hipStream_t st);
// max_waves > 0 (masked launches only): at most that many wavefronts, each resetting the masked envs of its
// grid-stride range in turn; 0: one wavefront per env
hipError_t mg_launch_reset(const MGState &S, const mg_library *L, TaskCfg cfg, const uint8_t *mask, hipStream_t st,
                           int max_waves = 0);
// one compiled step-kernel form: a (form, envs per workgroup) pair of mg_stepforms.h (defined in mg_stepk.h,
// instantiated in mg_step_*.hip)
template <int VAR, int BLK>
hipError_t launch_step_var(const MGState &S, const mg_library *L, TaskCfg cfg, int max_steps, int auto_reset,
                           const uint8_t *actions, float *reward, uint8_t *done, double *eval_score,
                           uint8_t *reset_mask, hipStream_t st);
hipError_t mg_launch_step(const MGState &S, const mg_library *L, TaskCfg cfg, int form, int blk, int max_steps,
                          int auto_reset, const uint8_t *actions, float *reward, uint8_t *done, double *eval_score,
                          uint8_t *reset_mask, hipStream_t st);
// mg_step_seq: up to R env-steps per env on S itself, then mg_step's tail once (defined in mg_seq.h, instantiated in
// mg_seq_*.hip, dispatched in mg_physics.hip).  actions: u8[R][n_envs]; steps: i32[n_envs] or null
template <int VAR, int BLK>
hipError_t launch_step_seq_var(const MGState &S, const mg_library *L, TaskCfg cfg, int max_steps, int auto_reset,
                               const uint8_t *actions, int R, float *reward, uint8_t *done, double *eval_score,
                               int32_t *steps, uint8_t *reset_mask, hipStream_t st);
hipError_t mg_launch_step_seq(const MGState &S, const mg_library *L, TaskCfg cfg, int form, int blk, int max_steps,
                              int auto_reset, const uint8_t *actions, int R, float *reward, uint8_t *done,
                              double *eval_score, int32_t *steps, uint8_t *reset_mask, hipStream_t st);
// mg_lookahead: H env-steps of physics on S, the sim's scratch copy of the state, then the outputs of LookOut (the
// device pointers of mg_lookahead_out; score is never null).  actions: u8[H][n_envs].  One compiled pair per pair of
// the step kernel (defined in mg_lookahead.h, instantiated in mg_look_*.hip, dispatched in mg_lookahead.hip)
struct LookOut { double *score; int32_t *steps; double *bodies; int32_t *counts; int32_t *errors; };
// mg_lookahead_obj / mg_plan_obj / mg_plan_cem_obj: the same rollout with the task's score s_k and mg_step's reward r_k
// evaluated after every env-step k (the TRACE instantiation of the lookahead kernel, one per pair as above), and the
// objective built on them (include/magical_sim.h: MG_OBJ_*).  The objective travels by value; the outputs are the
// device pointers of mg_objective_out, all of which may be null -- and here LookOut.score may be null too (a plan's
// [K][N] buffer receives `value` instead).  debug: the sim pays the dense debug reward (MG_DEBUG_REWARD).
enum { LOOK_OBJ_FINAL = 0, LOOK_OBJ_RETURN = 1, LOOK_OBJ_PEAK = 2 };   // = MG_OBJ_* (checked in mg_lookahead.hip)
// mg_plan_beam: an objective continued over several launches on one pool.  Per-rollout arrays [n_envs] that hold,
// between two launches, G before the tail term, P, g_k and kp of the env-steps done so far, their number k, and whether
// one of them ended the episode.  G null: no carry (every other call).  load 0: the launch starts the objective as
// always and only stores the carry; 1: it takes it up from the carry.  It stores the carry in either case
struct LookCarry {
    double *G, *P, *g;
    int32_t *kp, *k, *ended;
    int load;
};
struct LookObj {
    int kind, debug;
    double gamma, tail;
    double *value, *peak;
    int32_t *peak_step;
    double *score_trace, *reward_trace;   // f64[H][n_envs], step-major as the actions
    LookCarry carry;
};
// one compiled lookahead kernel: a pair as above, plain (obj is not read) or TRACE
template <int VAR, int BLK, bool TRACE>
hipError_t launch_look(const MGState &S, const mg_library *L, int task, int max_steps, const uint8_t *actions, int H,
                       const LookOut &out, const LookObj &obj, hipStream_t st);
// obj null: the plain kernel; else the TRACE one
hipError_t mg_launch_lookahead(const MGState &S, const mg_library *L, int task, int form, int blk, int max_steps,
                               const uint8_t *actions, int H, const LookOut &out, const LookObj *obj, hipStream_t st);
// mode 0: LoRes outputs (window rings where ro has them), 1: full resolution, 3: mg_imagine's form -- S is a pool without
// frame rings, ro.obs_allo / ro.obs_ego (either may be null: that view is not drawn) receive the plain current frames,
// and only ro's preproc, small, first_level and force_retry are read besides
hipError_t mg_launch_render(const MGState &S, const mg_library *L, const RenderOut &ro, int mode, hipStream_t st);
hipError_t mg_launch_compose3ea(const MGState &S, const uint8_t *obs_allo, const uint8_t *mask, uint8_t *obs_past,
                                hipStream_t st);
// profiling builds (-DMG_PROFILE): copy and clear each translation unit's phase timers
hipError_t mg_prof_read_physics(unsigned long long *out64);
hipError_t mg_prof_read_reset(unsigned long long *out64);
hipError_t mg_prof_read_step_v4(unsigned long long *out64);
hipError_t mg_prof_read_step_quad(unsigned long long *out64);
hipError_t mg_prof_read_step_hbm(unsigned long long *out64);
hipError_t mg_prof_read_raster(unsigned long long *out64);
