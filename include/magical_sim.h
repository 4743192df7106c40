/*
 * magical_sim.h -- C ABI of the MI355X batched MAGICAL simulator.
 *
 * Drop-in boundary for the reference hot path:
 * one mg_sim holds N environment instances of one registered MAGICAL env name
 * (benchmarks/__init__.py:427-1102) on one GPU.  mg_step replaces, for all N
 * instances at once, the reference's per-env call chain
 *     TimeLimit.step -> ResizeDictObservation / FlattenFrameStack /
 *     EagerDictFrameStack (benchmarks/__init__.py:51-190)
 *       -> BaseEnv.step (base_env.py:267-307)
 *            -> Robot.set_action / Robot.update (entities.py:435-476)
 *            -> pymunk Space.step x 10 (base_env.py:248-255)
 *            -> score_on_end_of_traj (task files)
 *            -> BaseEnv.render (base_env.py:324-343, render.py:385-395)
 * and mg_reset replaces BaseEnv.reset (base_env.py:190-246) + on_reset.
 *
 * Conventions: functions return 0 on success or a negative errno-style code;
 * mg_last_error() returns a thread-local message.  No C++ exception crosses the
 * ABI.  Output buffers are caller-owned device pointers; the library owns its
 * internal state and frees it in mg_destroy.  All work is enqueued on the given
 * HIP stream (hipStream_t passed as void*; NULL = default stream).  One handle
 * per GPU, used from one host thread.
 */
#ifndef MAGICAL_SIM_H
#define MAGICAL_SIM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mg_sim mg_sim;

typedef struct {
    int32_t task;              /* 0 MoveToRegion 1 MoveToCorner 2 ClusterColour 3 ClusterShape 4 MatchRegions 5 MakeLine 6 FindDupe 7 FixColour 8 PickAndPlace */
    int32_t rand_flags;        /* bit 0 layout minor, 1 layout full, 2 colour, 3 shape type, 4 count, 5 dynamics,
                                  6 debug_reward (dense shaped reward: move_to_corner.py:85-100, pick_and_place.py:108-124) */
    int32_t preproc;           /* 0 none, 1 LoRes4E (also LoResCHW4E / LoResCHW4A: same bytes), 2 LoResStack,
                                  3 LoRes3EA, 4 LoRes4A (benchmarks/__init__.py:269-307) */
    int32_t num_envs;
    int32_t device;            /* HIP device ordinal */
    int32_t max_episode_steps; /* TimeLimit / BaseEnv.max_episode_steps */
    uint32_t base_seed;        /* env i seeded base_seed + i when seeds == NULL */
    int32_t auto_reset;        /* 1: finished episodes reset inside mg_step (VecEnv); 0: gym single-env semantics */
    const uint32_t *seeds;     /* host array [num_envs] or NULL */
    const void *library;       /* host pointer to an mg_library (layout: magical-1_amd/csrc/mg_common.h,
                                  built by magical_amd.tables from the reference formulas) */
    int64_t library_size;      /* sizeof(mg_library), checked */
} mg_config;

typedef struct {
    uint8_t *obs_allo;   /* LoRes4E/4A: u8[N,96,96,3]; LoResStack: u8[N,96,96,12] */
    uint8_t *obs_ego;    /* same shapes as obs_allo */
    uint8_t *obs_past;   /* LoRes4E/4A: u8[N,96,96,12]; NULL otherwise */
    float *reward;       /* f32[N] (eval_score at done, else 0) */
    uint8_t *done;       /* u8[N] */
    double *eval_score;  /* f64[N] (info['eval_score']) */
    double *target;      /* PickAndPlace: f64[N,4] = (target_type, target_colour, target_position x, y)
                            (pick_and_place.py:87-107 observation extras), written at reset; NULL otherwise */
    int32_t frames_only; /* 0: the preprocessor's outputs above.  1 (multi-GPU compact gather, magical_amd.dist):
                            obs_allo / obs_ego receive only the current LoRes frame of each view, u8[N,96,96,3],
                            for every LoRes preprocessor; obs_past is ignored and no frame stack or ring is kept
                            (the receivers rebuild the stacks with mg_restack).  Switching modes needs a reset. */
} mg_buffers;

/* replaces gym.make(name) for N instances (benchmarks/__init__.py:232-266) */
int mg_create(const mg_config *cfg, mg_sim **out);
/* caller-owned output buffers (device pointers) */
int mg_bind_outputs(mg_sim *sim, const mg_buffers *buf);
/* BaseEnv.reset for every env (mask == NULL) or envs with mask[i] != 0 (device u8[N]);
 * writes the LoRes observation of the reset envs */
int mg_reset(mg_sim *sim, const uint8_t *mask_dev, void *stream);
/* BaseEnv.step for all envs; actions: device u8[N] in [0, 18); envs that reach
 * max_episode_steps report done/reward/eval_score and are reset in place
 * (their observation is the first frame of the next episode) */
int mg_step(mg_sim *sim, const uint8_t *actions_dev, void *stream);
/* Several env-steps per call with one render (frame skip / action repeat; the committing twin of mg_lookahead below).
 * actions_dev: device u8[R][N], step-major as mg_lookahead's (step h of env e at h*N + e), each in [0, 18);
 * 1 <= R <= 4096.  steps_dev: device i32[N] or NULL.
 * Per-env horizon: with left = max_episode_steps - episode_steps, env e runs n = R env-steps when
 * max_episode_steps <= 0, else n = min(R, max(left, 1)) -- an env already past its end takes one step, as mg_step does.
 * It runs n env-steps of BaseEnv.step physics with actions[0..n)[e], the operations of mg_step in the same order:
 * afterwards the state, episode_steps (+n), error flags and RNG have the bits that n mg_step calls would leave.  Only
 * step n can end the episode, so an env stops at its terminal step and its remaining R - n actions are ignored.
 * Outputs (the bound buffers): done[e] = 1 iff step n ended the episode; eval_score[e] = the score at that step, else
 * 0.0; reward[e] = (float)(r_1 + ... + r_n), summed left to right in double, one rounded add each, r_k being the
 * double mg_step casts to float at step k (mg_objective's r_k; without the debug reward the sum is eval_score);
 * steps_dev[e] = n.
 * Auto-reset is mg_step's, unchanged, after the physics and for exactly the envs with done: in the kernel for the
 * robot scenes without layout randomisation, from the next-layout shadow, or as a reset launch.  Then ONE render, as
 * mg_step enqueues it: one frame is pushed per call and the window position advances by one, so frame stacks and
 * window rings hold the frames seen at call boundaries, and a reset env's stack is filled with its first frame.  It
 * works with materialised stacks, window rings, frames_only outputs and the unwrapped surface.  R = 1 is mg_step in
 * every bound output and every state byte.  mg_enable_timing records a call like one mg_step call.
 * Returns -22 and launches nothing for a null sim or actions_dev, R outside [1, 4096], or outputs not bound where
 * mg_step would refuse. */
int mg_step_seq(mg_sim *sim, const uint8_t *actions_dev, int32_t R, int32_t *steps_dev, void *stream);
/* BaseEnv.render('rgb_array') of every env: device u8[N,2,384,384,3] (allo, ego) */
int mg_render_full(mg_sim *sim, uint8_t *out_dev, void *stream);
/* parity dumps: per env per body slot (px, py, angle, vx, vy, w): device f64[N,16,6];
 * counts: device i32[N,4] = (bodies, shapes, constraints, active arbiters) */
int mg_get_bodies(mg_sim *sim, double *out_dev, int32_t *counts_dev, void *stream);
/* parity dumps of the contact solver's state (cpArbiter / cpContact): the solved
 * arbiters of every env in active order, out_dev f64[N,48,28] = (slot, state, count, body a, body b, n.x, n.y,
 * friction u, then per contact r1.x, r1.y, r2.x, r2.y, jnAcc, jtAcc, nMass, tMass, bias, jBias), hash_dev
 * u64[N,48,2] = the contacts' feature hashes; rows past the env's active count are zero.  Test hook of the
 * parity suite (the reference has no such call: pymunk exposes the same data as Arbiter.contact_point_set) */
int mg_get_arbiters(mg_sim *sim, double *out_dev, uint64_t *hash_dev, void *stream);
/* parity dump of every env's RNG, the numpy-legacy MT19937 that resets draw layouts from: key_dev u32[N,624] and
 * pos_dev i32[N] are numpy's RandomState.get_state()[1:3] (pos == 624: the next draw regenerates the key).  Read-only
 * and stream-ordered (one small copy kernel); it reads the main state, the rows mg_snapshot records -- what the env's
 * next in-place reset would draw from, not the next-layout shadow's copy running ahead of it.  Test hook
 * (tests/test_rng_stream.py follows the stream across its regenerations in every reset path) */
int mg_get_rng(mg_sim *sim, uint32_t *key_dev, int32_t *pos_dev, void *stream);
/* set body `body` of env `env` to (x, y, angle) like pymunk's Body.position / Body.angle setters
 * (geom.py:362-384 pm_shift_bodies applies them); for parity tests that place blocks before a step */
int mg_set_body_pose(mg_sim *sim, int env, int body, double x, double y, double angle, void *stream);
/* per-env error flags, device i32[N]: 1 arbiter table full, 2 PlacementError in the env's latest reset
 * (geom.py:335-336; cleared by the next reset, which draws a new layout), 64 PlacementError in any reset so
 * far (sticky), 4 / 8 allo / ego raster assumption or capacity, 16 / 32 scene outside the step kernel's
 * compiled caps / constraint list */
int mg_get_errors(mg_sim *sim, int32_t *out_dev, void *stream);
/* re-seed env RNGs (env.seed): host u32[num_envs].  The many-block tasks' next-layout shadow (layouts drawn
 * ahead on an internal stream) is invalidated: auto-resets run in place on the caller's stream until the next
 * full (mask == NULL) mg_reset re-primes it -- same results, slower resets. */
int mg_seed(mg_sim *sim, const uint32_t *seeds_host);
/* device-side uniform random actions for throughput runs (Philox 4x32-10, key, counter = (step, env)) */
int mg_random_actions(mg_sim *sim, uint8_t *actions_dev, uint64_t key, uint64_t step, void *stream);
int mg_num_envs(const mg_sim *sim);
/* the step kernel this handle launches (diagnostics for bench.py's byte model): out i32[6] = (form: 0 HBM state,
 * 4 cooperative, 5 / 6 robot-scene quad forms; envs per workgroup; the per-env slot caps its HBM <-> LDS transfer
 * moves: bodies, shapes, constraints, arbiter slots) */
int mg_step_form(const mg_sim *sim, int32_t *out);
/* self-test of the device's correctly rounded sin/cos (the physics and render transforms use it):
 * device f64 x[n] -> sin, cos */
int mg_selftest_sincos(const double *x_dev, double *sin_dev, double *cos_dev, int n, void *stream);
/* self-test of the device MT19937's three regeneration ("twist") paths.  One wavefront per seed seeds a scratch
 * generator as mg_seed does (seeds_dev: device u32[n]) and writes the tempered 32-bit words of its next ndraws draws
 * to out_dev, device u32[n][ndraws] -- RandomState(seed).bytes(4 * ndraws) read as little-endian u32.  mode 0: one
 * lane draws over the state in HBM (the auto-reset fused into the robot scenes' step kernels); 1: the state sits in
 * LDS and the wavefront's 64 lanes draw together (the reset kernel); 2: the same with only lanes 0-36 active (the LDS
 * twist's serial branch) -- lane 0 writes out_dev[0 .. n*ndraws), lane 36 a second copy to out_dev[n*ndraws ..
 * 2*n*ndraws), so in mode 2 out_dev holds u32[2][n][ndraws].  The scratch state is allocated and freed by the call,
 * which waits for the kernel on `stream`; no sim is involved.
 * Returns -22 and launches nothing for a null seeds_dev or out_dev, n outside [1, 4096], ndraws outside [1, 8192] or
 * a mode other than 0, 1, 2 */
int mg_selftest_mt(const uint32_t *seeds_dev, int n, int ndraws, int mode, uint32_t *out_dev, void *stream);
/* per-kernel timing of the next max_steps mg_step calls (hipEvents on the launch stream); 0 disables */
int mg_enable_timing(mg_sim *sim, int max_steps);
/* out[0] = total ms in the physics/step kernel, out[1] = total ms in the render kernel,
 * out[2] = number of mg_step calls timed, out[3] = total ms in the auto-reset kernel; resets the counters */
int mg_read_timing(mg_sim *sim, double *out);
/* overwrite every env's episode step counter (BaseEnv.episode_steps, base_env.py:279-283) from device
 * i32[N]: throughput runs stagger episode phases so resets are spread over the timed steps */
int mg_set_episode_steps(mg_sim *sim, const int32_t *steps_dev, void *stream);
/* Demo replay through the LoRes observation stages (replaces saved_trajectories.py:63-149,
 * _MockDemoEnv + preprocess_demos_with_wrapper, for the LoRes preprocessors of
 * benchmarks/__init__.py:232-307).  frames: device u8[nframes,2,384,384,3] (allo, ego) of one or more
 * trajectories concatenated, 16-byte aligned; episode_start: device i32[nframes], the index of the
 * first frame of each frame's trajectory (its reset observation fills the frame stacks);
 * preproc: 1 LoRes4E (CHW4E/CHW4A: same bytes, channels-first views on the host), 2 LoResStack,
 * 3 LoRes3EA, 4 LoRes4A; scratch: device u8[nframes,2,96,96,3] workspace; outputs as mg_buffers for
 * nframes "envs" (out_past NULL for LoResStack).  No mg_sim needed. */
int mg_replay_lores(const uint8_t *frames, int32_t nframes, const int32_t *episode_start, int32_t preproc,
                    uint8_t *scratch, uint8_t *out_allo, uint8_t *out_ego, uint8_t *out_past, void *stream);
/* Receiver side of the compact multi-GPU gather (magical_amd.dist.ShardedVecEnv): rebuilds the LoRes frame
 * stacks (FlattenFrameStack / EagerDictFrameStack, benchmarks/__init__.py:51-147, reset frame filling every
 * slot) of world * n envs from their all-gathered current frames.
 * recv: device u8, `world` rank blocks of rank_stride bytes; block r holds env r*n+i's current allo frame
 * u8[96,96,3] at off_allo + i*27648, its ego frame at off_ego + i*27648 and its done flag u8 at off_done + i
 * (all offsets 16-byte aligned, as the frames-only outputs of mg_bind_outputs write them).
 * ring: device u8[stacks][4][world*n][27648], stacks = 2 for LoResStack (allo, ego), else 1 (the view the
 * stacked output is built from), caller-owned and persistent across calls (step t writes slot t % 4).
 * all_fresh = 1 after a reset of every env; otherwise an env whose done flag is set restarts its stacks
 * (auto-reset: its frame is the next episode's first).  Outputs for world*n envs, as mg_buffers' stacked
 * outputs: preproc 1 (LoRes4E / CHW4E / CHW4A), 3 (LoRes3EA), 4 (LoRes4A): out_past u8[world*n,96,96,12]
 * (allo / ego are the gathered frames themselves); 2 (LoResStack): out_allo, out_ego u8[world*n,96,96,12]. */
int mg_restack(const uint8_t *recv, int32_t world, int32_t n, int64_t rank_stride, int64_t off_allo, int64_t off_ego,
               int64_t off_done, int32_t preproc, int64_t step, int32_t all_fresh, uint8_t *ring, uint8_t *out_allo,
               uint8_t *out_ego, uint8_t *out_past, void *stream);
/* The same stacks as a window ring (round 5): every received frame is written once, channel-planar
 * (u8[3][96][96]), into ring u8[stacks][world*n][K + 3][3][96][96] (stacks as for mg_restack; caller-owned,
 * persistent; K >= 4): frame t of env g goes to slot t % K, and also to slot K + t % K when t % K < 3, so for
 * every env the frames t-3 .. t (oldest first) occupy the consecutive slots s0 .. s0 + 3, s0 = (t + K - 3) % K.
 * The stacked output of step t is then the strided view [world*n, 96, 96, 12] of the ring at byte offset
 * s0 * 27648 with strides (env (K + 3) * 27648, y 96, x 1, channel 9216) -- channel k of a stack = plane k % 3
 * of its frame k / 3 -- identical to mg_restack's outputs value for value, with no stack written.  A fresh env
 * (all_fresh, or its done flag) writes its frame into the slots of frames t-3 .. t.  preproc 1 (LoRes4E /
 * CHW4E / CHW4A), 2 (LoResStack), 4 (LoRes4A); LoRes3EA (allo frame in front of 3 ego frames) is not a window
 * of one ring: use mg_restack.  Step t's views stay valid until the call for step t + 1 is ordered after
 * their readers (the ring's slot t + 1 - K ... is rewritten then; for a fresh env the slots of t-3 .. t). */
int mg_restack_window(const uint8_t *recv, int32_t world, int32_t n, int64_t rank_stride, int64_t off_allo,
                      int64_t off_ego, int64_t off_done, int32_t preproc, int64_t step, int32_t all_fresh, int32_t K,
                      uint8_t *ring, void *stream);
/* Stacked outputs as window rings on the simulator itself (round 5).  ring_allo / ring_ego: device
 * u8[num_envs][K + 3][3][96][96], caller-owned, 16-byte aligned, one for each stacked view of the preprocessor
 * (LoResStack: allo and ego; LoRes4E / CHW4E / CHW4A: ego; LoRes4A: allo), NULL for the others; both NULL
 * turns it off.  Each step's frame of a stacked view is written once, channel-planar, into slot w % K (and
 * K + w % K when w % K < 3; w = the number of mg_step calls so far), a freshly reset env into the slots of
 * frames w-3 .. w, instead of the [96][96][12] stack and its frame ring: the stack is the strided view of the
 * ring at slot mg_window_start() with strides (env (K + 3) * 27648, y 96, x 1, channel 9216), value for value
 * the stack mg_bind_outputs would receive (FlattenFrameStack / EagerDictFrameStack, benchmarks/__init__.py:
 * 51-147).  The stacked outputs of mg_bind_outputs may then be NULL.  Bind before mg_reset; not with
 * frames_only outputs.  A step's views stay valid until the next mg_step / mg_reset on the stream. */
int mg_bind_window(mg_sim *sim, uint8_t *ring_allo, uint8_t *ring_ego, int32_t K);
/* *slot = the window's first slot for the current outputs ((w + K - 3) % K), -1 when no ring is bound */
int mg_window_start(const mg_sim *sim, int32_t *slot);
/* Env state snapshots.  A blob holds `count` env records behind a 256-byte header; a record is everything that makes
 * an env's continuation bit-identical: every per-env state row (bodies, shapes, constraints, arbiter tables with
 * their warm-start accumulators, stamp, curr_dt, entities, episode_steps, PickAndPlace's target, the MT19937 key and
 * position), the error flags, the render's per-episode scratch (class chain level, static layer and its valid flag)
 * and the LoRes frame history with its ring heads.  The blob is opaque and relocatable (copy it, save it, load it
 * on another process); its layout is magical-1_amd/csrc/mg_snapshot.h.  Header, little-endian: u32 magic "MGSN",
 * u32 layout version, i32 task, rand_flags, preproc, the MG_MAX_* caps (bodies, shapes, constraints, arbiters,
 * entities), i32 rows, i32 frames per record, i64 state bytes per record, i64 record bytes, i64 record count, i64
 * blob bytes, zero padding.
 * Supported: materialised stacks and the unwrapped surface.  A sim with window rings (mg_bind_window) or
 * frames_only outputs returns -22 from both calls: its frame stacks live with the caller / the receivers.
 *
 * mg_snapshot_bytes: bytes of a blob of n records for cfg's task and preprocessor = 256 + n * record bytes (the
 * record size depends on the preprocessor only, through the frames it carries); host-only, touches no GPU. */
int64_t mg_snapshot_bytes(const mg_config *cfg, int32_t n);
/* gather: record k of the blob <- env envs[k] (host i32[n], each in [0, num_envs), 1 <= n <= num_envs; NULL = all
 * envs in order, n = num_envs).  blob_dev: device, 16-byte aligned, mg_snapshot_bytes(cfg, n) bytes.  The current
 * frame of a view that keeps no ring (LoRes4E / LoRes3EA allo, LoRes4A ego) is read from the bound output, which
 * must still hold the latest observation.  Enqueued on the stream; the index array is consumed before returning. */
int mg_snapshot(mg_sim *sim, const int32_t *envs, int32_t n, uint8_t *blob_dev, void *stream);
/* scatter: env envs[k] <- record recs[k] of the blob, k < n (host arrays; recs NULL = k, and may repeat: one record
 * broadcast to many envs; envs NULL = 0..n-1, else distinct and in range).  The header is validated first, through one
 * small device-to-host copy that synchronises the stream, before any kernel is launched: a blob of another task,
 * rand_flags, preprocessor, slot caps or layout version, a bad magic value or a bad index returns -22 and leaves the
 * sim untouched.  The blob's contents behind a valid header are trusted.  Then the bound observation outputs of the
 * restored envs (obs_allo, obs_ego, obs_past, PickAndPlace's target) hold the observation the env had when
 * recorded, rebuilt from the restored frame history (nothing is rendered: a render would push a frame); reward, done
 * and eval_score describe a step, not a state, and stay as they are.  The many-block tasks' next-layout shadow of
 * the restored envs is prepared again from the restored RNG state, as after a masked mg_reset. */
int mg_restore(mg_sim *sim, const uint8_t *blob_dev, const int32_t *envs, const int32_t *recs, int32_t n, void *stream);
/* Explicit scenes: an env's layout as data (SURVEY.md section 8(b) planned it as mg_set_layouts).  One fixed-size
 * plain-data record per env, little-endian, no pointers: a [N] array of it is one flat device buffer (sizeof(mg_scene)
 * = 792 bytes, 8-byte aligned rows) and one numpy structured array (magical_amd.native.SCENE_DTYPE).  The arena is
 * implicit; ent[] holds the entities after it in the order the task's reset instantiates them:
 *   MoveToRegion: goal, robot.  MoveToCorner: robot, block.  ClusterColour / ClusterShape, MakeLine: blocks, robot.
 *   FindDupe: goal, outer blocks, query block, robot.  FixColour: nr goals, nr blocks, robot.  PickAndPlace: robot,
 *   3 blocks.  MatchRegions: goal, blocks, robot.
 * Roles are not part of the record; mg_reset_scene derives them as the task's reset does (FindDupe: 1 iff type and colour
 * equal the query block's, else 2; FixColour: 1 iff block i's colour equals region i's, else 2; MatchRegions: 1 iff the
 * colour equals the goal's, else 2; other tasks 0), and PickAndPlace's target ids from the target entity's type and
 * colour.  (The structs carry a tag so that they may hold arrays; the layout is the declaration's, no padding.) */
typedef struct mg_scene_ent {
    int32_t kind;      /* 1 goal region, 2 robot, 3 block: the MG_ENT_* values of magical-1_amd/csrc/mg_common.h */
    int32_t type;      /* blocks: MG_SHAPE_* (square 1, pentagon 2, circle 5, star 6 are the types resets draw); else 0 */
    int32_t colour;    /* blocks and goals: MG_COL_RED 0, GREEN 1, BLUE 2, YELLOW 3; robot: ignored on input, MG_COL_GREY
                          (4) on output */
    int32_t flags;     /* bit 0: disabled -- collides with nothing for the episode (what a failed placement retry leaves
                          behind: MG_GROUP_OFF / goal enabled = 0); other bits 0 */
    double  x, y;      /* robot, block: root body position; goal: the sensor's CENTRE */
    double  angle;     /* robot, block: root body angle; goal: 0 */
    double  h, w;      /* goal only; else 0 */
} mg_scene_ent;
typedef struct mg_scene {
    int32_t n_ents;        /* entities after the arena, 1 .. 13 */
    int32_t target_ent;    /* PickAndPlace: index into ent[] of the block to place; else -1 on output, ignored on input */
    double  pv[5];         /* physics variables in PhysVar declaration order: robot pos / rot joint max force, robot
                              finger max force, shape trans / rot joint max force (defaults 3, 1, 4, 1.5, 0.1) */
    double  target_xy[2];  /* PickAndPlace target position; else 0 on output, ignored on input */
    mg_scene_ent ent[13];  /* MG_MAX_ENTS - 1; entries past n_ents are zero on output, ignored on input */
} mg_scene;
/* Every env's CURRENT layout -> scenes_dev, device mg_scene[num_envs], 8-byte aligned: the entity table (kind, type,
 * colour, enabled state), each entity's pose from its root body as it stands (mid-episode poses, not the reset's), goal
 * centre, h and w, pv, PickAndPlace's target.  One small read-only kernel, stream-ordered, like mg_get_rng; it touches
 * nothing in the sim. */
int mg_get_scene(mg_sim *sim, mg_scene *scenes_dev, void *stream);
/* A masked reset, as mg_reset(mask) is, whose layout comes from scenes_dev[e] (device mg_scene[num_envs], 8-byte
 * aligned, read only) instead of the task's constants and the RNG.  The state env e is left in is what the task's reset
 * leaves for a variant without layout randomisation: episode state, arbiter table, stamp, curr_dt, robot targets and
 * error bit 2 cleared, pv from the record, every entity instantiated once, in record order, directly at its pose
 * (velocities zero; the robot's eye bodies, which the reset instantiates at the origin and the layout sampler drags along
 * with the robot, sit where a rigid move of the task's Demo robot pose to the given pose puts them -- at the origin for
 * the Demo pose itself; nothing reads their position), a goal's centre stored as given, disabled entities folded into
 * MG_GROUP_OFF, PickAndPlace's bound target output written.  The env's MT19937 rows are neither read nor written, and
 * the next-layout shadow and its pending work are left alone: the env's next auto-reset draws what it would have drawn.
 *
 * Validation runs on the device, per env, and is complete before any write to that env.  status_dev (required, device
 * i32[num_envs]) receives, the lowest code that applies:
 *    0 built;  -1 not selected by the mask;
 *    1 entity count or kind order is not the task's (orders above; block counts: Cluster >= 7, MakeLine >= 3, FindDupe
 *      >= 2 outer blocks plus the query, FixColour >= 2 regions with as many blocks, MatchRegions >= 1 block and at
 *      least one of the goal's colour, PickAndPlace exactly 3, MoveToCorner exactly 1);
 *    2 a field is out of range: an enum outside its set, a type / h / w / goal angle that must be 0 and is not, unknown
 *      flag bits, a non-finite number, |x| or |y| > 1, |angle| > 100, a goal's h or w outside [0.1, 0.8] (0.8 is
 *      RAND_GOAL_MAX_SIZE, the largest goal any variant draws: the render classes are sized for it), pv[i] not finite
 *      or <= 0, PickAndPlace's target_xy not finite or beyond +-1;
 *    3 the scene does not fit the handle: bodies, shapes and constraints counted from the record must be <= the slot
 *      caps of the handle's task and rand_flags (what mg_step_form reports for form 0), and EQUAL to them when the
 *      handle runs step form 5 or 6, whose constraint lists are compiled (a star on a MoveToCorner handle created
 *      without the shape-type flag is refused, as is a ninth block on a Cluster handle created without the count flag);
 *    4 PickAndPlace's target_ent is not one of the blocks.
 * An env with status > 0 is left completely untouched (state, flags, frames).
 * check = 1: afterwards every built env runs the reset's own overlap test on every enabled entity (the shape queries of
 * the layout sampler, with the task's ignore rules: FindDupe's query block and goal ignore each other, FixColour's
 * blocks ignore their own region), one wavefront per env; an env with any hit gets error flags 2 | 64 (PlacementError,
 * as a failed layout draw does).  It is still built and its status stays 0.  check = 0 launches no such work.
 * Then one LoRes render of the built envs, exactly as mg_reset(mask) renders: their frame stacks / window-ring slots are
 * filled with the first frame, the render's per-episode scratch starts over, other envs' outputs keep their bytes; the
 * window position does not advance.  Works with materialised stacks, window rings, frames_only outputs and the
 * unwrapped surface.  Everything is enqueued on `stream`; no host sync.
 * Returns -22 and launches nothing for a null sim, scenes_dev or status_dev, a scenes_dev that is not 8-byte aligned,
 * check outside {0, 1}, or outputs not bound where mg_reset would refuse.  mask_dev NULL = all envs. */
int mg_reset_scene(mg_sim *sim, const mg_scene *scenes_dev, const uint8_t *mask_dev, int32_t check,
                   int32_t *status_dev, void *stream);
/* Lookahead: "what happens if these envs run these H actions", without touching the envs.  Caller-owned device
 * outputs: */
typedef struct {
    double  *score;    /* f64[N]: the task's score_on_end_of_traj of the env's state after its last simulated step
                          (whether or not that step ends the episode); required */
    int32_t *steps;    /* i32[N]: env-steps simulated = min(H, max_episode_steps - episode_steps); NULL ok */
    double  *bodies;   /* f64[N,16,6] as mg_get_bodies, of the final state; NULL ok */
    int32_t *counts;   /* i32[N,4] as mg_get_bodies; NULL ok */
    int32_t *errors;   /* i32[N]: error flags as mg_get_errors as they stand at the end of the rollout (the env's
                          flags on entry plus any raised during it); the sim's own flags are not touched; NULL ok */
} mg_lookahead_out;
/* actions_dev: device u8[H][N] (step-major: step h of env e at h*N + e, N = num_envs), each in [0, 18);
 * 0 <= H <= 4096.
 * Every env is simulated from its current state for min(H, remaining) env-steps of physics only -- action decode
 * plus 10 substeps each, exactly BaseEnv.step up to and including _phys_steps_on_frame (base_env.py:248-276) --
 * with the operations of mg_step in the same order, so the final state has the bits that as many mg_step calls
 * would give it.  No render, no frame push, no reward / done / eval_score outputs, no auto-reset and no fused
 * reset.  An env whose episode would end inside the horizon stops at its terminal step, and its score is what
 * mg_step would have reported as eval_score there; with max_episode_steps <= 0 nothing ends early.  An env with
 * 0 remaining steps simulates nothing and is scored as it stands.  H = 0 is "score only": every env's current
 * state is scored, steps = 0, and actions_dev may be NULL.
 * The sim is observationally untouched: state rows, RNG, episode_steps, error flags, frame rings, window rings,
 * bound outputs, the next-layout shadow and its pending work are unchanged, and a following mg_step gives the
 * same bytes as if the call had not happened.  It works in every mode (window rings, frames_only outputs,
 * auto_reset 0 or 1, the unwrapped surface) and touches no frames.
 * The rollout runs on a scratch copy of the state that the sim owns: allocated by the first call (that call
 * alone allocates and therefore synchronises the device), reused by later ones, freed in mg_destroy.  Everything
 * else is enqueued on `stream` with no host sync.  Calls on one stream reuse the scratch in order; two lookaheads
 * in flight on different streams of one handle are not supported (one handle, one host thread, as everywhere).
 * Returns -22 and launches nothing for a null sim / out / out->score, a null actions_dev with H > 0, or H
 * outside [0, 4096]. */
int mg_lookahead(mg_sim *sim, const uint8_t *actions_dev, int32_t H, const mg_lookahead_out *out, void *stream);
/* Plan: "which of these K action sequences is best for each env", without touching the envs.  One call fans every
 * env's state out to K rollouts, runs all K * N of them as one grid and reduces to the best candidate per env on the
 * device.  Caller-owned device outputs (N = num_envs): */
#define MG_PLAN_MAX_ROLLOUTS 262144   /* K * num_envs of one call */
typedef struct {
    int32_t *best;         /* i32[N]: index k of the env's best candidate: highest score, lowest k on ties; required */
    double  *best_score;   /* f64[N]: that candidate's score; NULL ok */
    uint8_t *first_action; /* u8[N]: actions[0][best[e]][e] (H = 0: left unwritten); NULL ok */
    double  *scores;       /* f64[K][N]: every candidate's score, as mg_lookahead_out.score; NULL ok */
    int32_t *steps;        /* i32[K][N]: as mg_lookahead_out.steps; NULL ok */
    int32_t *errors;       /* i32[K][N]: as mg_lookahead_out.errors; NULL ok */
} mg_plan_out;
/* actions_dev: device u8[H][K][N], candidate-major within a step: step h of candidate k of env e at (h*K + k)*N + e,
 * each in [0, 18).  0 <= H <= 4096, 1 <= K <= 4096, K * N <= MG_PLAN_MAX_ROLLOUTS.
 * Rollout k*N + e starts from env e's current state and is exactly what mg_lookahead computes for env e with the
 * action column actions[:, k, e]: the same per-env horizon min(H, remaining), the same stop at the terminal step, the
 * same score, steps and error flags, bit for bit (it is the same kernel, for the (form, envs per workgroup) pair of
 * mg_step, on a grid of K * N envs).  H = 0 scores the current state K times: best = 0, steps = 0, and actions_dev
 * may be NULL.
 * best is the argmax over all K candidates, the lowest k among equal scores (scores are never NaN).  Error flags do
 * not exclude a candidate: they are reported through `errors` for the caller to act on.
 * The sim is observationally untouched: state rows, RNG, episode_steps, error flags, frame rings, window rings,
 * bound outputs, the next-layout shadow and its pending work are unchanged, and a following mg_step gives the
 * same bytes as if the call had not happened.  It works in every mode (window rings, frames_only outputs,
 * auto_reset 0 or 1, the unwrapped surface) and touches no frames.
 * The rollouts run on a fan pool that the sim owns, separate from mg_lookahead's scratch: allocated by the first call
 * for its K * N rollouts, re-allocated by a later call that needs more (those calls alone synchronise the device),
 * freed in mg_destroy.  An allocation failure returns -12 and leaves the sim usable, without a fan pool.  Everything
 * else is enqueued on `stream` with no host sync; two plans in flight on different streams of one handle are not
 * supported.
 * Returns -22 and launches nothing for a null sim / out / out->best, a null actions_dev with H > 0, or H, K or
 * K * N out of range. */
int mg_plan(mg_sim *sim, const uint8_t *actions_dev, int32_t H, int32_t K, const mg_plan_out *out, void *stream);
/* Random-shooting candidates for mg_plan: fills actions_dev u8[H][K][N], each action held for repeat >= 1 env-steps.
 * With J = ceil(H / repeat), row [h][k][:] holds the bytes mg_random_actions(sim, ., key, step + k*J + h/repeat, .)
 * writes (integer division): candidate k uses the J counter values from step + k*J on, so a decision consumes K*J
 * of them.  Returns -22 for null arguments, repeat < 1, or H, K or K * N out of mg_plan's range; H = 0 is a no-op
 * that returns 0. */
int mg_plan_sample(mg_sim *sim, uint8_t *actions_dev, int32_t H, int32_t K, int32_t repeat, uint64_t key, uint64_t step,
                   void *stream);
/* Cross-entropy planning: `iters` rounds of "draw K candidates, roll them out, refit the sampler to the E best",
 * iterated on the device.  Everything but the rollouts is integer arithmetic.  With J = ceil(H / repeat) held-action
 * slots, the sampler is weights_dev, u16[J][18][N]: slot j, action a, env e at (j*18 + a)*N + e, a per-env, per-slot
 * categorical over the 18 actions held as counts.
 * Draw D(w_j, c, e): word = the first Philox4x32-10 output word for `key` and counter (c lo, c hi, e, 0) -- the word
 * mg_random_actions reduces mod 18 --, T = the sum of w_j[0..17][e], r = word % T, the action is the smallest a whose
 * cumulative weight w_j[0] + .. + w_j[a] exceeds r.  T = 0 (possible only in caller-supplied weights) draws as if all
 * weights were 1.  (The bias of the modulo is below T / 2^32 < 6e-6 per action.)
 * Iteration i's candidates: row [h][k][:] = D(w_{h/repeat}, step + (i*K + k)*J + h/repeat, e); with all weights 1,
 * iteration 0 is byte for byte mg_plan_sample(H, K, repeat, key, step).  A call consumes iters*K*J counter values.  In
 * iterations i >= 1 candidate 0 is the incumbent instead: column best[e] of the previous iteration's candidates,
 * copied unchanged, so the best score never decreases and the overall best is among the last candidates.
 * Every iteration is exactly mg_plan on its candidates (fan-out, the rollout grid, the best-of-K reduction).  Its
 * elites are the `elites` candidates of an env with the highest scores, the lower k first among equal scores, and
 * the refit is w[j][a][e] = alpha + the number of elites whose slot-j action (row j*repeat) is a.  It runs after
 * every iteration, the last included: the weights left behind describe the last elites and can warm-start the next
 * decision.  Caller-owned device outputs (N = num_envs): */
typedef struct {
    int32_t *best;         /* i32[N]: index into the LAST iteration's candidates; required */
    double  *best_score;   /* f64[N]; NULL ok */
    uint8_t *first_action; /* u8[N]; NULL ok */
    double  *scores;       /* f64[K][N] of the last iteration; NULL ok */
    int32_t *steps;        /* i32[K][N] of the last iteration; NULL ok */
    int32_t *errors;       /* i32[K][N] of the last iteration; NULL ok */
    double  *iter_best;    /* f64[iters][N]: best score of every iteration; NULL ok */
} mg_plan_cem_out;
/* actions_dev: device u8[H][K][N], a workspace laid out as mg_plan's candidates; on return the last iteration's
 * candidates.  weights_dev: device u16[J][18][N], in/out; warm = 0 starts from all-ones weights (the buffer's
 * contents are not read), warm = 1 from weights_dev as it is.  Both are the caller's: the library allocates neither.
 * 1 <= H <= 4096, K and K * N as for mg_plan, 1 <= iters <= 64, 1 <= elites <= K, 0 <= alpha <= 1024, repeat >= 1.
 * The sim is observationally untouched: state rows, RNG, episode_steps, error flags, frame rings, window rings,
 * bound outputs, the next-layout shadow and its pending work are unchanged, and a following mg_step gives the
 * same bytes as if the call had not happened.  It works in every mode mg_plan does and touches no frames.
 * The rollouts run on mg_plan's fan pool, which also holds the per-env elite threshold the kernels pass between
 * them; the pool is (re)allocated as in mg_plan (those calls alone synchronise the device).  Everything else,
 * every iteration included, is enqueued on `stream` with no host sync.
 * Returns -22 and launches nothing for a null sim / actions_dev / weights_dev / out / out->best, or any argument
 * outside the ranges above (warm other than 0 or 1 included). */
int mg_plan_cem(mg_sim *sim, uint8_t *actions_dev, uint16_t *weights_dev, int32_t warm,
                int32_t H, int32_t K, int32_t iters, int32_t elites, int32_t alpha, int32_t repeat,
                uint64_t key, uint64_t step, const mg_plan_cem_out *out, void *stream);
/* Rollout objectives: what a rollout is worth, from the score and the reward after EVERY simulated env-step instead
 * of the final state's score alone.  For env (or rollout) e with n = min(H, remaining) as mg_lookahead computes it,
 * x_0 the state on entry and x_k the state after k env-steps:
 *   s_k = score_on_end_of_traj(x_k), 0 <= k <= n;
 *   done_k = max_episode_steps > 0 && episode_steps + k >= max_episode_steps, k >= 1 (it can hold at k = n only);
 *   r_k, k >= 1 = the double mg_step casts to float for `reward` at that step: debug_reward(x_k) on a sim with the
 *                 debug-reward flag, else done_k ? s_k : 0.0;
 *   g_0 = 1.0, g_k = g_{k-1} * gamma (sequential products).
 * Every operation below is one rounded IEEE double operation, none fused:
 *   FINAL   value = s_n (mg_lookahead's score).
 *   RETURN  G = 0.0; for k = 1..n: G = G + g_{k-1} * r_k; then, unless the episode ended inside the horizon (n >= 1 and
 *           done_n): G = G + (g_n * tail) * s_n.  value = G.  tail = 0 is the plain truncated return; tail = 1 and
 *           gamma = 1 without the debug reward is s_n exactly.
 *   PEAK    P = s_0, kp = 0; for k = 1..n: v = g_k * s_k, and P = v, kp = k when v > P.  value = P: with gamma = 1 the
 *           best score at any time in the horizon and kp when it was first reached; with gamma < 1 sooner is better. */
enum { MG_OBJ_FINAL = 0, MG_OBJ_RETURN = 1, MG_OBJ_PEAK = 2 };
typedef struct {
    int32_t kind;      /* MG_OBJ_* */
    int32_t reserved;  /* 0 */
    double  gamma;     /* in (0, 1] */
    double  tail;      /* finite, >= 0 */
} mg_objective;
/* Caller-owned device outputs, all NULL ok: */
typedef struct {
    double  *value;        /* f64[N]: the objective's value */
    double  *peak;         /* f64[N]: P as defined above, with the objective's gamma, whatever the kind */
    int32_t *peak_step;    /* i32[N]: kp */
    double  *score_trace;  /* f64[H][N]: row h = s_{min(h+1, n)}; every element is written, none is NaN */
    double  *reward_trace; /* f64[H][N]: row h = r_{h+1} for h < n, else 0.0; cast to float it is mg_step's reward */
} mg_objective_out;
/* mg_lookahead with an objective: `out` keeps its meaning for every kind (score is s_n) and the call is mg_lookahead in
 * everything else -- the untouched sim, the scratch pool, the stream ordering, the H = 0 rules.  obj_out may be NULL
 * (no objective outputs).  With kind FINAL and no objective output requested the call enqueues exactly what
 * mg_lookahead does; otherwise the rollout kernel's traced form runs, which writes the env's state back to scratch
 * and scores it after every env-step.
 * Returns -22 and launches nothing for a null objective, a kind outside 0..2, reserved != 0, gamma outside (0, 1]
 * (NaN included), a negative or non-finite tail, or anything mg_lookahead refuses.  gamma and tail are validated for
 * FINAL too and otherwise ignored by it. */
int mg_lookahead_obj(mg_sim *sim, const uint8_t *actions_dev, int32_t H, const mg_objective *objective,
                     const mg_lookahead_out *out, const mg_objective_out *obj_out, void *stream);
/* mg_plan / mg_plan_cem on an objective: scores, best_score and iter_best hold the objective's VALUE, and best, the
 * elites and the incumbent are chosen on it; candidate k of env e is exactly mg_lookahead_obj of its action column
 * (the same kernel on the fan pool).  Everything else, refusals included, is as in mg_plan / mg_plan_cem and as above
 * for the objective; kind FINAL enqueues exactly what mg_plan / mg_plan_cem do.  No traces: mg_lookahead_obj on a
 * column gives them. */
int mg_plan_obj(mg_sim *sim, const uint8_t *actions_dev, int32_t H, int32_t K, const mg_objective *objective,
                const mg_plan_out *out, void *stream);
int mg_plan_cem_obj(mg_sim *sim, uint8_t *actions_dev, uint16_t *weights_dev, int32_t warm,
                    int32_t H, int32_t K, int32_t iters, int32_t elites, int32_t alpha, int32_t repeat,
                    uint64_t key, uint64_t step, const mg_objective *objective, const mg_plan_cem_out *out, void *stream);
/* Beam search over action segments: mg_plan that prunes while it rolls out.  The horizon is cut into D = ceil(H / seg)
 * segments, segment d the steps [d*seg, min(H, (d+1)*seg)).  Every slot k of env e starts from the env's current state
 * (mg_plan's fan-out).  In segment d slot k applies actions[h][k][e], for the segment's h, to whatever lineage occupies
 * the slot, and plans[h][k][e] = actions[h][k][e].  After every segment but the last the env's slots are resampled:
 * the `survivors` slots with the highest value survive, the lower k first among equal values (mg_plan_cem's elite
 * rule), and stay where they are; with the survivors in increasing k s_0 < s_1 < .. and the losers l_0 < l_1 < ..,
 * loser l_j becomes a copy of s_(j mod survivors): its whole state with the error flags, the objective's accumulators
 * and plans[0 .. segment end).  The copy is made in place in the fan pool, on the device.
 * After each segment the value of slot k is bit for bit what mg_lookahead_obj (mg_lookahead for FINAL) returns for the
 * action prefix of the slot's lineage -- plans[0 .. segment end)[k][e] -- from the env's current state: the same
 * per-env horizon, stop at the terminal step, steps and error flags.  On return column (k, e) of plans_dev is the full
 * action sequence of the lineage that ends in slot k, and mg_plan / mg_plan_obj on plans_dev reproduces values, steps
 * and errors.  survivors == K or seg >= H gives mg_plan / mg_plan_obj on actions_dev in every output, plans == actions
 * and parents[d][k] = k.  Caller-owned device outputs (N = num_envs): */
typedef struct {
    int32_t *best;         /* i32[N]: slot k of the env's best lineage after the last segment (highest value, lowest k
                              on ties); required */
    double  *best_value;   /* f64[N]; NULL ok */
    uint8_t *first_action; /* u8[N] = plans[0][best[e]][e]; NULL ok */
    uint8_t *best_plan;    /* u8[H][N] = plans[:, best[e], e]; NULL ok */
    double  *values;       /* f64[K][N] after the last segment; NULL ok */
    int32_t *steps;        /* i32[K][N] total env-steps of the lineage; NULL ok */
    int32_t *errors;       /* i32[K][N] as mg_plan_out.errors, of the lineage; NULL ok */
    double  *depth_values; /* f64[D][K][N]: slot k's value after segment d, BEFORE the resample; NULL ok */
    int32_t *parents;      /* i32[D-1][K][N]: parent slot chosen at boundary d (k itself for a survivor); NULL ok;
                              unread when D == 1 */
} mg_plan_beam_out;
/* actions_dev: device u8[H][K][N], mg_plan's layout, read only.  plans_dev: device u8[H][K][N], caller-owned output.
 * 1 <= H <= 4096, K and K * N as for mg_plan, 1 <= seg <= H, 1 <= survivors <= K.  objective NULL = FINAL.
 * The sim is observationally untouched, exactly as stated for mg_plan.  The rollouts run on mg_plan's fan pool, which
 * also holds what the segments pass between them; the pool is (re)allocated as in mg_plan (those calls alone
 * synchronise the device).  Everything else, every segment and resample included, is enqueued on `stream` with no host
 * sync.
 * Returns -22 and launches nothing for a null sim / actions_dev / plans_dev / out / out->best, any argument outside the
 * ranges above, or an objective that mg_plan_obj refuses. */
int mg_plan_beam(mg_sim *sim, const uint8_t *actions_dev, uint8_t *plans_dev, int32_t H, int32_t K, int32_t seg,
                 int32_t survivors, const mg_objective *objective, const mg_plan_beam_out *out, void *stream);

/* ---- imagined observations: the LoRes frames of a lookahead rollout ----
 * What the agent would SEE if these actions were played: mg_lookahead's rollout, rendered every `every` env-steps.
 * F = ceil(H / every) frames per env; segment f is the steps [f*every, min(H, (f+1)*every)).  All four buffers are
 * device memory, 16-byte aligned, HWC as a frames_only binding's (mg_buffers). */
typedef struct {
    uint8_t *allo;        /* u8[F][N][96][96][3]: the current allo frame after segment f; NULL ok */
    uint8_t *ego;         /* u8[F][N][96][96][3]; NULL ok */
    uint8_t *stack_allo;  /* u8[F][N][96][96][12]; NULL ok; see the stack rules */
    uint8_t *stack_ego;   /* u8[F][N][96][96][12]; NULL ok */
} mg_imagine_out;
/* actions_dev: device u8[H][N] as mg_lookahead's.  1 <= H <= 4096, 1 <= every <= H.  The per-env horizon is
 * mg_lookahead's: n = min(H, remaining); an env whose episode ends inside the horizon stops at its terminal step.
 *
 * Frames.  Frame f of env e is the LoRes current frame -- the bytes a frames_only binding receives for that view, for
 * every LoRes preprocessor -- of the state after m_f = min((f+1)*every, n) env-steps.  Frames of an env that has
 * stopped repeat its terminal state's frame; there is no auto-reset, as in mg_lookahead.  Within an episode frame f is
 * the current frame the f+1-th of F successive mg_step_seq(actions + f*every*N, every) calls would show.
 *
 * Lookahead outputs.  `out` may be NULL, and if given its score may be NULL too.  score, steps, bodies and counts
 * receive bit for bit what mg_lookahead(sim, actions_dev, H, out) writes; errors the same OR-ed with any raster
 * capacity flag (4 / 8) raised while the imagined frames were drawn.
 *
 * Stacks: what the preprocessor's frame stacking would hold after those calls.  With g_f = frame f and g_-1, g_-2,
 * g_-3 the env's three most recent real frames (the sim's frame ring, newest = -1), stack[f] = (g_f-3, g_f-2, g_f-1,
 * g_f), oldest first: channel k = channel k%3 of frame k/3.  Legal: LoResStack stack_allo and stack_ego; LoRes4E
 * stack_ego; LoRes4A stack_allo; LoRes3EA stack_ego = allo_f | ego_f-2 | ego_f-1 | ego_f (its past_obs layout), which
 * needs both allo and ego.  A stack needs the plain frame buffer(s) it is built from.  After an env's terminal step the
 * repeated frame keeps entering the stack: those stacks correspond to no real step.  Stacks read the sim's own frame
 * history, which a handle with window rings or frames_only outputs does not keep: -22 there (mg_snapshot's rule);
 * plain frames work in every LoRes mode.
 *
 * The sim is observationally untouched, exactly as stated for mg_lookahead (frame rings, static layer, window rings
 * and position, bound outputs and the next-layout shadow included).  The call runs on mg_lookahead's scratch pool
 * (allocated by the first call of either, which alone synchronises) and allocates nothing else; every segment's
 * rollout launch and render and the final stack pass are enqueued on `stream` with no host sync; every == H is one
 * rollout launch.
 * Returns -22 and launches nothing for a null sim / actions_dev / frames, all four frame buffers null, H or every out
 * of range, a misaligned buffer, the unwrapped surface (preproc 0), a stack not legal for the preprocessor, or a stack
 * without its plain frames. */
int mg_imagine(mg_sim *sim, const uint8_t *actions_dev, int32_t H, int32_t every, const mg_lookahead_out *out,
               const mg_imagine_out *frames, void *stream);
void mg_destroy(mg_sim *sim);
const char *mg_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
