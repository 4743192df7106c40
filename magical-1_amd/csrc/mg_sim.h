// mg_sim.h -- the simulator object behind the C ABI (include/magical_sim.h) and what the ABI's translation units share.
// Each feature's entry points sit next to its kernels: create / seed / bind / reset / step / step_seq / getters / destroy in
// mg_sim.hip, snapshots in mg_snapshot.hip, mg_lookahead in mg_lookahead.hip, mg_plan in mg_plan.hip, mg_plan_cem in
// mg_cem.hip (each with its _obj form beside it), mg_plan_beam in mg_beam.hip, replay and restack in mg_replay.hip,
// explicit scenes (mg_get_scene, mg_reset_scene) in mg_scene.hip, imagined observations (mg_imagine) in mg_imagine.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>

#include "../../include/magical_sim.h"
#include "mg_launch.h"
#include "mg_plan.h"
#include "mg_pool.h"
#include "mg_snapshot.h"

// the thread's mg_last_error text; returns code
int set_err(int code, const std::string &msg);
#define HIPC(x)                                                                                        \
    do {                                                                                               \
        hipError_t _e = (x);                                                                           \
        if (_e != hipSuccess) return set_err(-5, std::string(#x) + ": " + hipGetErrorString(_e));      \
    } while (0)

static inline hipStream_t as_stream(void *s) { return (hipStream_t)s; }

struct mg_sim {
    StatePool main;        // main.S is the state every kernel of mg_step runs on (frame rings included)
    // Next-layout shadow (reset prefetch).  BaseEnv.reset draws the whole layout from the env's RNG and
    // nothing else (mg_reset.h reset_env), so the layout of an env's NEXT episode is known as soon as its
    // current one starts.  shadow is a second copy of the per-env state (same layout, no frame rings): right
    // after an env resets, reset_kernel runs on it for that env on a side stream, overlapping the step and render
    // kernels; when the episode ends the auto-reset is a copy shadow -> main of that env (reset_copy_kernel).
    StatePool shadow;
    StateRow *rows = nullptr;   // device copy of main.rows (the same rows in both pools)
    uint8_t *pend = nullptr;    // device u8[N]: envs whose shadow the side stream is preparing
    hipStream_t side = nullptr;
    hipEvent_t ev_copied = nullptr, ev_prepared = nullptr;
    int shadow_ok = 0;          // every env's shadow holds its next layout (set by a full mg_reset)
    int shadow_pending = 0;     // a reset_kernel on the shadow is in flight on the side stream
    int reset_waves = 0;          // auto-reset launches: wavefronts cap (0: one per env; MG_RESET_WAVES, A/B)
    int no_fused_reset = 0;       // MG_FUSED_RESET=0: the robot scenes' auto-reset as its own launch (A/B, tests)
    int reset_waves_shadow = 0;   // the shadow's next-layout launches: the same (MG_RESET_WAVES_SHADOW)
    int copy_wg = 0;              // reset_copy_kernel's workgroups cap (MG_COPY_WG: tests, A/B)
    int force_render_retry = 0;   // tests: the first k render classes of the chain hand every (env, view) on
    int scache_mode = 0;          // tests: RenderOut::scache_mode
    mg_library *dlib = nullptr;
    int task = 0, flags = 0, preproc = 0, max_steps = 0, device = 0, auto_reset = 0;
    mg_buffers out = {};
    int bound = 0;
    // window rings of the stacked views (mg_bind_window; null: materialised stacks), their period, and the step
    // counter that picks the slot (advanced by every mg_step before its render; resets do not advance it)
    uint8_t *wring[2] = {nullptr, nullptr};
    int wK = 0;
    long long wstep = 0;
    StepCaps caps = {};    // the task's per-env slot caps
    int step_form = 0;     // step kernel form and envs per workgroup: a compiled pair of mg_stepforms.h
    int step_blk = 0;
    uint8_t *reset_mask = nullptr;   // device u8[N]: envs to auto-reset after the step
    uint8_t *scene_built = nullptr;  // device u8[N]: envs the latest mg_reset_scene built (its render's mask)
    // snapshots (mg_snapshot.hip; layout: mg_snapshot.h)
    SnapRow *srows = nullptr;        // device table of a record's rows: the state rows and the per-env items layout() keeps out of them
    int nsrows = 0;
    int64_t snap_state_bytes = 0;    // a record's state section bytes (rounded up to 16)
    // index arrays of a call (env list, record list, restore mask): pinned host staging and its device copy, allocated
    // by the first call that passes a list; ev_snap marks the end of the last call that used them
    char *snap_stage = nullptr, *snap_dev = nullptr;
    hipEvent_t ev_snap = nullptr;
    int snap_inflight = 0;
    // rollout pools (mg_plan.h), two allocations so that a lookahead on one stream and a plan on another share no
    // memory: look holds num_envs rollouts (mg_lookahead and mg_imagine, allocated by the first call), fan K * num_envs (mg_plan and
    // mg_plan_cem: allocated by the first call, re-allocated by a call that needs more rollouts)
    RolloutPool look, fan;
    // optional per-kernel timing (hipEvents on the launch stream)
    int timing = 0;
    std::vector<hipEvent_t> ev;   // quadruples: before step_kernel, after it, after the auto-reset, after render_kernel
    size_t ev_used = 0;
};

// mg_sim.hip
// hand the state of the envs in mask (null: all) from one pool to the other on st, then prepare their
// next layouts on the side stream (reset_kernel on the shadow)
int shadow_handover(mg_sim *s, hipStream_t st, const uint8_t *mask, int to_main);
int render_lores(mg_sim *s, hipStream_t st, const uint8_t *mask);
// mg_snapshot.hip: a snapshot record's row table (mg_create)
int snap_init(mg_sim *s);
// mg_plan.hip: what mg_plan and mg_plan_cem check alike; make R hold at least M rollouts (no-op when it does)
int plan_check_sizes(const mg_sim *s, const char *fn, int32_t H, int32_t K);
int rollout_reserve(mg_sim *s, RolloutPool &R, int M, const char *fn);
// mg_lookahead.hip: what every *_obj call refuses in its objective (-22, nothing launched); the objective as the
// traced kernel takes it, without outputs
int objective_check(const mg_objective *o, const char *fn);
LookObj objective_args(const mg_sim *s, const mg_objective *o);
// mg_plan.hip: the rollouts of mg_plan and mg_plan_cem, plain (obj null or FINAL: scores = s_n) or traced (scores =
// the objective's value) on the fan pool's first M envs; carry (mg_plan_beam, traced only): the objective continues
// from launch to launch (LookCarry, mg_launch.h)
int plan_rollouts(mg_sim *s, const MGState &F, const uint8_t *actions, int H, const mg_objective *obj, double *scores,
                  int32_t *steps, int32_t *errors, hipStream_t st, const LookCarry *carry = nullptr);
