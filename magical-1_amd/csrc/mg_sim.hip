// mg_sim.hip -- the simulator object's life and its per-step path in the C ABI (include/magical_sim.h): create, seed,
// bind, reset, step, full-resolution render, the getters and setters, timing and destroy; struct mg_sim: mg_sim.h.
//
// Per env-step (mg_step): step_kernel (mg_physics.hip: one env per lane: action
// decode, 10 x [Robot.update + cpSpaceStep], episode counter, score, in-place
// reset of finished episodes) then render_kernel (mg_raster.hip: one workgroup
// per (env, view): 384^2 raster in LDS bands -> 96^2 area downsample -> LoRes
// frame stack).
#include <cstdio>
#include <cstring>
#include <cstdlib>

#include "mg_sim.h"
#include "mg_phys.h"
#include "mg_philox.h"

static thread_local std::string g_err;
int set_err(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

// ---------------------------------------------------------------------------
// kernels
__global__ void __launch_bounds__(64) bodies_kernel(MGState S, double *out, int32_t *counts) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= S.n_envs) return;
    env_bodies_record(S, e, out, counts);
}

// the solved arbiters of every env in active order (oracle/env.c oenv_get_arbiters has the same layout)
#define MG_ARB_DUMP 28
__global__ void __launch_bounds__(64) arbiters_kernel(MGState S, double *out, uint64_t *hash) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= S.n_envs) return;
    const int na = S.nactive[e];
    for (int i = 0; i < MG_MAX_ARB; i++) {
        double *o = out + ((size_t)e * MG_MAX_ARB + i) * MG_ARB_DUMP;
        uint64_t *h = hash + ((size_t)e * MG_MAX_ARB + i) * 2;
        for (int k = 0; k < MG_ARB_DUMP; k++) o[k] = 0.0;
        h[0] = h[1] = 0;
        if (i >= na) continue;
        const int slot = AT(S.active, i), cnt = AT(S.acount, slot);
        o[0] = slot; o[1] = AT(S.astate, slot); o[2] = cnt; o[3] = AT(S.asa, slot); o[4] = AT(S.asb, slot);
        o[5] = AT(S.anx, slot); o[6] = AT(S.any, slot); o[7] = AT(S.au, slot);
        for (int k = 0; k < cnt && k < 2; k++) {
            double *q = o + 8 + 10 * k;
            q[0] = ACON(k, AC_R1X, slot); q[1] = ACON(k, AC_R1Y, slot); q[2] = ACON(k, AC_R2X, slot);
            q[3] = ACON(k, AC_R2Y, slot); q[4] = ACON(k, AC_JN, slot); q[5] = ACON(k, AC_JT, slot);
            q[6] = ACON(k, AC_NMASS, slot); q[7] = ACON(k, AC_TMASS, slot); q[8] = ACON(k, AC_BIAS, slot);
            q[9] = ACON(k, AC_JB, slot);
            h[k] = AHASH(k, slot);
        }
    }
}

// every env's MT19937 state as numpy's get_state()[1:3]: key[e][624] (the state keeps it word-major), pos[e]
__global__ void __launch_bounds__(256) rng_kernel(MGState S, uint32_t *__restrict__ key, int32_t *__restrict__ pos) {
    const size_t n = (size_t)S.n_envs, t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= 624 * n) return;
    const size_t i = t / n, e = t % n;
    key[e * 624 + i] = S.mt_key[i * (size_t)S.N + e];
    if (i == 0) pos[e] = S.mt_pos[e];
}

__global__ void __launch_bounds__(64) errors_kernel(MGState S, int32_t *out) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= S.n_envs) return;
    out[e] = S.overflow[e];
}

// self-test of the device correctly rounded sincos (tests/test_gpu_parity.py compares with the oracle)
__global__ void __launch_bounds__(256) sincos_kernel(const double *x, double *s, double *c, int n) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mg_sincos(x[i], s[i], c[i]);
}

// uniform random actions (Philox4x32-10: mg_philox.h)
__global__ void __launch_bounds__(256) actions_kernel(uint8_t *out, int n, uint64_t key, uint64_t step) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    out[e] = philox_action(key, step, e);
}

// env e's per-env state rows src -> dst for the envs in mask (pend[e] = mask[e] for every env): the
// auto-reset from the next-layout shadow (src = shadow, to_main), or an explicit reset's state handed to
// the shadow (src = main).  Error flags: bit 2 (PlacementError of this reset) and the sticky bit 64 come
// from the reset that produced the layout.  A grid of at most copy_wg workgroups (mg_sim; 2048, MG_COPY_WG for
// tests): pend is written for every env with coalesced stores, then each workgroup walks its envs (grid-stride)
// and copies the rows of the masked ones -- an auto-reset step masks a few dozen of 8192 envs, and one workgroup
// per env (8192 mostly idle ones on the step's critical path) measured 0.095 -> 0.080 ms per step for the copy and
// reset phase (ClusterColour; MatchRegions 0.107 -> 0.090, profiles/r06_cw).
__global__ void __launch_bounds__(256) reset_copy_kernel(const char *__restrict__ src, char *__restrict__ dst,
                                                         const StateRow *__restrict__ rows, int nrows,
                                                         const uint8_t *__restrict__ mask, uint8_t *__restrict__ pend,
                                                         MGState S, MGState SH, int to_main) {
    const int tid = threadIdx.x;
    for (int e = blockIdx.x * 256 + tid; e < S.n_envs; e += gridDim.x * 256)
        pend[e] = (!mask || mask[e] != 0) ? 1 : 0;
    for (int e = blockIdx.x; e < S.n_envs; e += gridDim.x) {
        if (mask && mask[e] == 0) continue;   // uniform over the workgroup
        for (int r = tid; r < nrows; r += 256) {
            const StateRow w = rows[r];
            const size_t o = w.off + (size_t)e * w.esize;
            copy_elem(dst + o, src + o, w.esize);
        }
        if (tid == 0) {
            if (to_main) {
                S.overflow[e] = (S.overflow[e] & ~2) | (SH.overflow[e] & (2 | 64));
                if (S.target_out) {   // PickAndPlace: reset_env writes the bound target output at reset
                    double *t = S.target_out + 4 * (size_t)e;
                    t[0] = SH.tgt_ids[e]; t[1] = SH.tgt_ids[S.N + e]; t[2] = SH.tgt_x[e]; t[3] = SH.tgt_y[e];
                }
            } else {
                SH.overflow[e] = S.overflow[e];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// launches shared with the other units of the ABI
static int grid64(const mg_sim *s) { return (s->main.S.n_envs + 63) / 64; }

int render_lores(mg_sim *s, hipStream_t st, const uint8_t *mask) {
    RenderOut ro = {};
    ro.full = nullptr;
    ro.mask = mask;
    ro.debug_skip = 0;
    ro.small = s->task == MG_TASK_MOVE_TO_REGION || s->task == MG_TASK_MOVE_TO_CORNER;
    ro.first_level = s->task == MG_TASK_CLUSTER_COLOUR ? 0 : 1;   // render class chain start (mg_raster.hip)
    ro.force_retry = s->force_render_retry;
    ro.scache_mode = s->scache_mode;
#ifdef MG_PROFILE
    if (getenv("MG_DEBUG_SKIP")) ro.debug_skip = atoi(getenv("MG_DEBUG_SKIP"));
#endif
    ro.obs_allo = s->out.obs_allo; ro.obs_ego = s->out.obs_ego; ro.obs_past = s->out.obs_past;
    ro.preproc = s->preproc;
    ro.frames_only = s->out.frames_only;
    ro.wring[0] = s->wring[0]; ro.wring[1] = s->wring[1]; ro.wK = s->wK;
    ro.wpos = s->wK > 0 ? (int)(s->wstep % s->wK) : 0;
    for (int fr = 0; fr < 2 && s->wK > 0; fr++) {   // slot lists of a running / a fresh env (mg_bind_window)
        int n = 0;
        for (int d = 0; d < (fr ? 4 : 1); d++) {
            const int f = (ro.wpos + s->wK - d) % s->wK;
            ro.wsl[fr][n++] = (int8_t)f;
            if (f < 3) ro.wsl[fr][n++] = (int8_t)(s->wK + f);
        }
        ro.wnsl[fr] = n;
    }
    HIPC(mg_launch_render(s->main.S, s->dlib, ro, 0, st));
    if (s->preproc == MG_PREPROC_LORES3EA && !s->out.frames_only)
        HIPC(mg_launch_compose3ea(s->main.S, (const uint8_t *)s->out.obs_allo, mask, (uint8_t *)s->out.obs_past, st));
    return 0;
}

int shadow_handover(mg_sim *s, hipStream_t st, const uint8_t *mask, int to_main) {
    if (s->shadow_pending) HIPC(hipStreamWaitEvent(st, s->ev_prepared, 0));   // pend and the shadow are free
    const char *src = (const char *)(to_main ? s->shadow.mem : s->main.mem);
    char *dst = (char *)(to_main ? s->main.mem : s->shadow.mem);
    const int cgrid = (s->copy_wg > 0 && s->main.S.n_envs > s->copy_wg) ? s->copy_wg : s->main.S.n_envs;
    hipLaunchKernelGGL(reset_copy_kernel, dim3(cgrid), dim3(256), 0, st, src, dst, s->rows, (int)s->main.rows.size(), mask,
                       s->pend, s->main.S, s->shadow.S, to_main);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(s->ev_copied, st));
    HIPC(hipStreamWaitEvent(s->side, s->ev_copied, 0));
    TaskCfg cfg = {s->task, s->flags};
    HIPC(mg_launch_reset(s->shadow.S, s->dlib, cfg, s->pend, s->side, s->reset_waves_shadow));
    HIPC(hipEventRecord(s->ev_prepared, s->side));
    s->shadow_pending = 1;
    return 0;
}

// ---------------------------------------------------------------------------
// C ABI
extern "C" {

const char *mg_last_error(void) { return g_err.c_str(); }

#ifdef MG_PROFILE
// profiling builds only (tools/gpu_phase.py): phase timer totals, then cleared
int mg_debug_read_profile(unsigned long long *out) {
    HIPC(hipDeviceSynchronize());
    for (int i = 0; i < 64; i++) out[i] = 0;
    HIPC(mg_prof_read_physics(out));
    HIPC(mg_prof_read_raster(out));
    return 0;
}
#endif

// everything of mg_create after the sim object exists: a failure returns its code and mg_create destroys what was built
static int sim_init(mg_sim *s, const mg_config *cfg) {
    s->task = cfg->task; s->flags = cfg->rand_flags; s->preproc = cfg->preproc;
    s->max_steps = cfg->max_episode_steps; s->auto_reset = cfg->auto_reset;
    auto env_int = [](const char *name, int unset) { const char *v = getenv(name); return v ? atoi(v) : unset; };
    MGState proto = {};
    proto.n_envs = cfg->num_envs;
    proto.cons_cap = MG_MAX_CONS;
    proto.arb_cap = MG_MAX_ARB;
    proto.max_tries = 10000; // geom.py:198
    if (env_int("MG_DEBUG_MAX_TRIES", 0) > 0) proto.max_tries = env_int("MG_DEBUG_MAX_TRIES", 0); // tests only
    s->reset_waves = env_int("MG_RESET_WAVES", 0);
    s->no_fused_reset = env_int("MG_FUSED_RESET", 1) == 0;
    // the shadow's next layouts run beside the step stream's kernels: 256 wavefronts scanning the pending mask
    // instead of one 352-VGPR wavefront per env, most of which only exit (512: ClusterColour 1.458 -> 1.468 M,
    // MatchRegions 1.329 -> 1.358 M env-steps/s, same box; the in-place robot-scene resets gained nothing).
    // Round 5: 256 -- fewer 352-VGPR wavefronts holding SIMDs beside the render -- MatchRegions 1.375 -> 1.393 M,
    // ClusterColour unchanged; 64 makes a wavefront's serial run of layouts outlast the step (MatchRegions 1.11 M)
    s->reset_waves_shadow = env_int("MG_RESET_WAVES_SHADOW", 256);
    s->copy_wg = env_int("MG_COPY_WG", 2048);
    s->force_render_retry = env_int("MG_DEBUG_RENDER_RETRY", 0);   // tests only
    s->scache_mode = env_int("MG_DEBUG_SCACHE", 0);                // tests only
    const int N = (cfg->num_envs + 63) / 64 * 64;
    hipError_t err = pool_create(s->main, proto, N, true);
    if (err != hipSuccess) return set_err(-12, std::string("mg_create: state pool: ") + hipGetErrorString(err));
    if (hipMalloc((void **)&s->dlib, sizeof(mg_library)) != hipSuccess) return set_err(-12, "mg_create: hipMalloc library");
    HIPC(hipMemcpy(s->dlib, cfg->library, sizeof(mg_library), hipMemcpyHostToDevice));
    // the step kernel's form and envs per workgroup (mg_stepforms.h); MG_STEP_VARIANT, MG_STEP_BLK (LDS forms) and
    // MG_STEP_BLK0 (form 0) override them for experiments and tests
    s->caps = step_caps(cfg->task, cfg->rand_flags, ((const mg_library *)cfg->library)->block_nshapes[MG_SHAPE_STAR]);
    s->step_form = step_pick_form(s->caps, env_int("MG_STEP_VARIANT", -1));
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device);
    s->step_blk = step_pick_blk(s->step_form, cfg->num_envs, cus, env_int("MG_STEP_BLK", 0), env_int("MG_STEP_BLK0", 0));
    if (hipMalloc((void **)&s->reset_mask, (size_t)N) != hipSuccess) return set_err(-12, "mg_create: hipMalloc mask");
    HIPC(hipMemset(s->reset_mask, 0, (size_t)N));
    // (no fill: mg_reset_scene's build kernel writes every env's byte before its render reads it, and one more launch
    // here moves the first step's workgroups to other CUs -- DESIGN.md section 4, step sequences, last paragraph)
    if (hipMalloc((void **)&s->scene_built, (size_t)N) != hipSuccess) return set_err(-12, "mg_create: hipMalloc mask");
    // next-layout shadow: the many-block tasks, whose rejection-sampled layouts make a reset long (the
    // robot scenes reset in ~0.03 ms); MG_RESET_PREFETCH=0/1 overrides
    bool prefetch = s->auto_reset && s->task != MG_TASK_MOVE_TO_REGION && s->task != MG_TASK_MOVE_TO_CORNER;
    if (const char *pf = getenv("MG_RESET_PREFETCH")) prefetch = s->auto_reset && atoi(pf) != 0;
    if (prefetch) {
        HIPC(pool_create(s->shadow, proto, N, false));
        const std::vector<StateRow> &rows = s->main.rows;
        HIPC(hipMalloc((void **)&s->rows, rows.size() * sizeof(StateRow)));
        HIPC(hipMemcpy(s->rows, rows.data(), rows.size() * sizeof(StateRow), hipMemcpyHostToDevice));
        HIPC(hipMalloc((void **)&s->pend, (size_t)N));
        HIPC(hipMemset(s->pend, 0, (size_t)N));
        HIPC(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));
        HIPC(hipEventCreateWithFlags(&s->ev_copied, hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&s->ev_prepared, hipEventDisableTiming));
    }
    if (int rc = snap_init(s)) return rc;
    std::vector<uint32_t> seeds(cfg->num_envs);
    for (int i = 0; i < cfg->num_envs; i++) seeds[i] = cfg->seeds ? cfg->seeds[i] : cfg->base_seed + (uint32_t)i;
    return mg_seed(s, seeds.data());
}

int mg_create(const mg_config *cfg, mg_sim **out) {
    if (!cfg || !out) return set_err(-22, "mg_create: null argument");
    if (cfg->library_size != (int64_t)sizeof(mg_library))
        return set_err(-22, "mg_create: library_size mismatch (expected " + std::to_string(sizeof(mg_library)) + ")");
    if (cfg->num_envs <= 0) return set_err(-22, "mg_create: num_envs must be positive");
    if (cfg->task < 0 || cfg->task > MG_TASK_PICK_AND_PLACE) return set_err(-22, "mg_create: unknown task");
    if (cfg->preproc != MG_PREPROC_LORES4E && cfg->preproc != MG_PREPROC_LORESSTACK &&
        cfg->preproc != MG_PREPROC_LORES4A && cfg->preproc != MG_PREPROC_LORES3EA && cfg->preproc != MG_PREPROC_NONE)
        return set_err(-95, "mg_create: preprocessor not supported by the GPU path");
    HIPC(hipSetDevice(cfg->device));
    mg_sim *s = new mg_sim();
    s->device = cfg->device;
    if (const int rc = sim_init(s, cfg)) {
        mg_destroy(s);   // takes a partly built sim; *out stays unset
        return rc;
    }
    *out = s;
    return 0;
}

int mg_seed(mg_sim *s, const uint32_t *seeds_host) {
    if (!s || !seeds_host) return set_err(-22, "mg_seed: null argument");
    HIPC(hipSetDevice(s->device));
    if (s->shadow_pending) HIPC(hipEventSynchronize(s->ev_prepared));
    s->shadow_pending = 0;
    s->shadow_ok = 0;   // the shadow's layouts came from the old seeds: valid again after a full mg_reset
    uint32_t *d = nullptr;
    HIPC(hipMalloc(&d, sizeof(uint32_t) * s->main.S.n_envs));
    HIPC(hipMemcpy(d, seeds_host, sizeof(uint32_t) * s->main.S.n_envs, hipMemcpyHostToDevice));
    HIPC(mg_launch_seed(s->main.S, d, 0));
    HIPC(hipDeviceSynchronize());
    HIPC(hipFree(d));
    return 0;
}

int mg_bind_outputs(mg_sim *s, const mg_buffers *b) {
    if (!s || !b) return set_err(-22, "mg_bind_outputs: null argument");
    // with window rings bound (mg_bind_window) the stacked outputs are views of the rings: LoResStack's
    // obs_allo / obs_ego and LoRes4E / LoRes4A's obs_past may be null
    const bool win = !b->frames_only && (s->wring[0] || s->wring[1]);
    const bool stack_ae = s->preproc == MG_PREPROC_LORESSTACK;
    if (s->preproc != MG_PREPROC_NONE && (!b->obs_allo || !b->obs_ego) && !(win && stack_ae))
        return set_err(-22, "mg_bind_outputs: obs_allo / obs_ego required");
    if (b->frames_only != 0 && b->frames_only != 1) return set_err(-22, "mg_bind_outputs: frames_only must be 0 or 1");
    if (b->frames_only && s->preproc == MG_PREPROC_NONE)
        return set_err(-22, "mg_bind_outputs: frames_only needs a LoRes preprocessor");
    if ((s->preproc == MG_PREPROC_LORES4E || s->preproc == MG_PREPROC_LORES4A || s->preproc == MG_PREPROC_LORES3EA) &&
        !b->frames_only && !b->obs_past && !(win && s->preproc != MG_PREPROC_LORES3EA))
        return set_err(-22, "mg_bind_outputs: obs_past required for this preprocessor");
    const void *ptrs[3] = {b->obs_allo, b->obs_ego, b->frames_only ? nullptr : b->obs_past};
    for (const void *p : ptrs)
        if (((uintptr_t)p & 15) != 0) return set_err(-22, "mg_bind_outputs: observation buffers must be 16-byte aligned");
    if (s->task == MG_TASK_PICK_AND_PLACE && !b->target)
        return set_err(-22, "mg_bind_outputs: target required for PickAndPlace");
    s->out = *b;
    s->main.S.target_out = b->target;
    s->bound = 1;
    return 0;
}

int mg_reset(mg_sim *s, const uint8_t *mask, void *stream) {
    if (!s) return set_err(-22, "mg_reset: null sim");
    if (!s->bound && s->preproc != MG_PREPROC_NONE) return set_err(-22, "mg_reset: outputs not bound");
    HIPC(hipSetDevice(s->device));
    hipStream_t st = as_stream(stream);
    TaskCfg cfg = {s->task, s->flags};
    HIPC(mg_launch_reset(s->main.S, s->dlib, cfg, mask, st));
    if (s->shadow.mem) {
        const int rc = shadow_handover(s, st, mask, 0);
        if (rc) return rc;
        if (!mask) s->shadow_ok = 1;
    }
    if (s->preproc != MG_PREPROC_NONE) return render_lores(s, st, mask);
    return 0;
}

// The host part of mg_step and mg_step_seq: the fused_reset decision, the timing events, the physics launch (R = 0:
// step_kernel on actions u8[N]; R >= 1: step_seq_kernel on actions u8[R][N], steps as mg_step_seq's), the reset phase on
// the kernel's reset_mask, wstep and the one render
static int step_call(mg_sim *s, const uint8_t *actions, int R, int32_t *steps, hipStream_t st) {
    TaskCfg cfg = {s->task, s->flags};
    // robot scenes without layout randomisation: the step kernel runs the auto-reset itself (mg_stepk.h)
    const bool layout = (s->flags & (MG_RAND_LAYOUT_MINOR | MG_RAND_LAYOUT_FULL)) != 0;
    cfg.fused_reset = s->auto_reset && !s->shadow_ok && !layout && !s->no_fused_reset &&
                      ((s->task == MG_TASK_MOVE_TO_REGION && s->step_form == 5) ||
                       (s->task == MG_TASK_MOVE_TO_CORNER && s->step_form == 6));
    hipEvent_t *ev = nullptr;
    if (s->timing && s->ev_used + 4 <= s->ev.size()) { ev = &s->ev[s->ev_used]; s->ev_used += 4; }
    if (ev) HIPC(hipEventRecord(ev[0], st));
    if (R == 0)
        HIPC(mg_launch_step(s->main.S, s->dlib, cfg, s->step_form, s->step_blk, s->max_steps, s->auto_reset, actions,
                            s->out.reward, s->out.done, s->out.eval_score, s->reset_mask, st));
    else
        HIPC(mg_launch_step_seq(s->main.S, s->dlib, cfg, s->step_form, s->step_blk, s->max_steps, s->auto_reset, actions, R,
                                s->out.reward, s->out.done, s->out.eval_score, steps, s->reset_mask, st));
    if (ev) HIPC(hipEventRecord(ev[1], st));
    if (s->auto_reset) {
        if (s->shadow_ok) {
            const int rc = shadow_handover(s, st, s->reset_mask, 1);
            if (rc) return rc;
        } else if (!cfg.fused_reset) {
            HIPC(mg_launch_reset(s->main.S, s->dlib, cfg, s->reset_mask, st, s->reset_waves));
        }
    }
    if (ev) HIPC(hipEventRecord(ev[2], st));
    int rc = 0;
    s->wstep++;   // this step's frame goes to the window rings' next slot
    if (s->preproc != MG_PREPROC_NONE) rc = render_lores(s, st, nullptr);
    if (ev) HIPC(hipEventRecord(ev[3], st));
    return rc;
}

int mg_step(mg_sim *s, const uint8_t *actions, void *stream) {
    if (!s || !actions) return set_err(-22, "mg_step: null argument");
    if (!s->bound && s->preproc != MG_PREPROC_NONE) return set_err(-22, "mg_step: outputs not bound");
    HIPC(hipSetDevice(s->device));
    return step_call(s, actions, 0, nullptr, as_stream(stream));
}

int mg_step_seq(mg_sim *s, const uint8_t *actions, int32_t R, int32_t *steps, void *stream) {
    if (!s || !actions) return set_err(-22, "mg_step_seq: null argument");
    if (R < 1 || R > 4096) return set_err(-22, "mg_step_seq: R must be in [1, 4096]");
    if (!s->bound && s->preproc != MG_PREPROC_NONE) return set_err(-22, "mg_step_seq: outputs not bound");
    HIPC(hipSetDevice(s->device));
    return step_call(s, actions, R, steps, as_stream(stream));
}

int mg_bind_window(mg_sim *s, uint8_t *ring_allo, uint8_t *ring_ego, int32_t K) {
    if (!s) return set_err(-22, "mg_bind_window: null sim");
    // outputs bound while rings were on may leave the stacked outputs null (mg_bind_outputs): turning the rings
    // off, or changing which views have one, would then make the next render write its stacks through null
    // pointers -- refuse until outputs with the stacks are bound
    if (s->bound && !s->out.frames_only) {
        const int pp = s->preproc;
        const bool lost = pp == MG_PREPROC_LORESSTACK ? ((!ring_allo && !s->out.obs_allo) || (!ring_ego && !s->out.obs_ego))
                        : pp == MG_PREPROC_LORES4E    ? (!ring_ego && !s->out.obs_past)
                        : pp == MG_PREPROC_LORES4A    ? (!ring_allo && !s->out.obs_past) : false;
        if (lost)
            return set_err(-22, "mg_bind_window: a stacked view would have neither a ring nor an output buffer (the "
                                "bound outputs' stacks are null); bind outputs with the stacks (mg_bind_outputs) first");
    }
    if (!ring_allo && !ring_ego) { s->wring[0] = s->wring[1] = nullptr; s->wK = 0; return 0; }
    if (K < 4 || K > 64) return set_err(-22, "mg_bind_window: K must be in [4, 64]");
    const int pp = s->preproc;
    const bool want_a = pp == MG_PREPROC_LORESSTACK || pp == MG_PREPROC_LORES4A;
    const bool want_e = pp == MG_PREPROC_LORESSTACK || pp == MG_PREPROC_LORES4E;
    if (!want_a && !want_e)
        return set_err(-22, "mg_bind_window: preproc must be 1 (LoRes4E), 2 (LoResStack) or 4 (LoRes4A)");
    if ((ring_allo != nullptr) != want_a || (ring_ego != nullptr) != want_e)
        return set_err(-22, "mg_bind_window: a ring for each stacked view (LoResStack: allo and ego; LoRes4E: ego; "
                            "LoRes4A: allo) and none for the others");
    if (((uintptr_t)ring_allo | (uintptr_t)ring_ego) & 15) return set_err(-22, "mg_bind_window: rings must be 16-byte aligned");
    s->wring[0] = ring_allo; s->wring[1] = ring_ego; s->wK = K;
    return 0;
}

int mg_window_start(const mg_sim *s, int32_t *slot) {
    if (!s || !slot) return set_err(-22, "mg_window_start: null argument");
    *slot = s->wK > 0 ? (int32_t)((s->wstep + s->wK - 3) % s->wK) : -1;
    return 0;
}

int mg_render_full(mg_sim *s, uint8_t *out, void *stream) {
    if (!s || !out) return set_err(-22, "mg_render_full: null argument");
    HIPC(hipSetDevice(s->device));
    RenderOut ro;
    memset(&ro, 0, sizeof(ro));
    ro.full = out;
    ro.preproc = s->preproc;
    ro.small = s->task == MG_TASK_MOVE_TO_REGION || s->task == MG_TASK_MOVE_TO_CORNER;
    ro.first_level = s->task == MG_TASK_CLUSTER_COLOUR ? 0 : 1;   // render class chain start (mg_raster.hip)
    ro.force_retry = s->force_render_retry;
    HIPC(mg_launch_render(s->main.S, s->dlib, ro, 1, as_stream(stream)));
    return 0;
}

int mg_get_bodies(mg_sim *s, double *out, int32_t *counts, void *stream) {
    if (!s || !out) return set_err(-22, "mg_get_bodies: null argument");
    HIPC(hipSetDevice(s->device));
    hipLaunchKernelGGL(bodies_kernel, dim3(grid64(s)), dim3(64), 0, as_stream(stream), s->main.S, out, counts);
    HIPC(hipGetLastError());
    return 0;
}

int mg_get_arbiters(mg_sim *s, double *out, uint64_t *hash, void *stream) {
    if (!s || !out || !hash) return set_err(-22, "mg_get_arbiters: null argument");
    HIPC(hipSetDevice(s->device));
    hipLaunchKernelGGL(arbiters_kernel, dim3(grid64(s)), dim3(64), 0, as_stream(stream), s->main.S, out, hash);
    HIPC(hipGetLastError());
    return 0;
}

int mg_get_rng(mg_sim *s, uint32_t *key, int32_t *pos, void *stream) {
    if (!s || !key || !pos) return set_err(-22, "mg_get_rng: null argument");
    HIPC(hipSetDevice(s->device));
    const size_t total = (size_t)624 * (size_t)s->main.S.n_envs;
    hipLaunchKernelGGL(rng_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), s->main.S, key, pos);
    HIPC(hipGetLastError());
    return 0;
}

int mg_selftest_mt(const uint32_t *seeds, int n, int ndraws, int mode, uint32_t *out, void *stream) {
    if (!seeds || !out) return set_err(-22, "mg_selftest_mt: null argument");
    if (n < 1 || n > 4096 || ndraws < 1 || ndraws > 8192)
        return set_err(-22, "mg_selftest_mt: n must be in [1, 4096] and ndraws in [1, 8192]");
    if (mode < 0 || mode > 2) return set_err(-22, "mg_selftest_mt: mode must be 0, 1 or 2");
    // a scratch MT19937 state of its own (never a sim's), freed once the kernel has finished
    uint32_t *key = nullptr;
    int32_t *pos = nullptr;
    if (hipMalloc((void **)&key, sizeof(uint32_t) * 624 * (size_t)n) != hipSuccess)
        return set_err(-12, "mg_selftest_mt: hipMalloc");
    if (hipMalloc((void **)&pos, sizeof(int32_t) * (size_t)n) != hipSuccess) {
        (void)hipFree(key);
        return set_err(-12, "mg_selftest_mt: hipMalloc");
    }
    hipError_t err = mg_launch_selftest_mt(seeds, n, ndraws, mode, key, pos, out, as_stream(stream));
    if (err == hipSuccess) err = hipStreamSynchronize(as_stream(stream));
    (void)hipFree(key);
    (void)hipFree(pos);
    HIPC(err);
    return 0;
}

int mg_selftest_sincos(const double *x, double *s_out, double *c_out, int n, void *stream) {
    if (!x || !s_out || !c_out || n < 0) return set_err(-22, "mg_selftest_sincos: bad argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(sincos_kernel, dim3((n + 255) / 256), dim3(256), 0, as_stream(stream), x, s_out, c_out, n);
    HIPC(hipGetLastError());
    return 0;
}

// pymunk Body.angle / Body.position setters (as geom.pm_shift_bodies applies them): parity tests
__global__ void set_body_pose_kernel(MGState S, int e, int b, double x, double y, double a) {
    body_set_angle(S, e, b, a);
    const double c = AT(S.brc, b), sn = AT(S.brs, b);
    AT(S.bpx, b) = (c * 0.0 + (-sn) * 0.0) + x; // cpBodySetPosition: p = T(cog = 0) + position
    AT(S.bpy, b) = (sn * 0.0 + c * 0.0) + y;
}

int mg_set_body_pose(mg_sim *s, int env, int body, double x, double y, double angle, void *stream) {
    if (!s || env < 0 || env >= s->main.S.n_envs || body < 0 || body >= MG_MAX_BODIES)
        return set_err(-22, "mg_set_body_pose: bad argument");
    HIPC(hipSetDevice(s->device));
    hipLaunchKernelGGL(set_body_pose_kernel, dim3(1), dim3(1), 0, as_stream(stream), s->main.S, env, body, x, y, angle);
    HIPC(hipGetLastError());
    return 0;
}

int mg_get_errors(mg_sim *s, int32_t *out, void *stream) {
    if (!s || !out) return set_err(-22, "mg_get_errors: null argument");
    HIPC(hipSetDevice(s->device));
    hipLaunchKernelGGL(errors_kernel, dim3(grid64(s)), dim3(64), 0, as_stream(stream), s->main.S, out);
    HIPC(hipGetLastError());
    return 0;
}

int mg_random_actions(mg_sim *s, uint8_t *actions, uint64_t key, uint64_t step, void *stream) {
    if (!s || !actions) return set_err(-22, "mg_random_actions: null argument");
    HIPC(hipSetDevice(s->device));
    hipLaunchKernelGGL(actions_kernel, dim3((s->main.S.n_envs + 255) / 256), dim3(256), 0, as_stream(stream), actions,
                       s->main.S.n_envs, key, step);
    HIPC(hipGetLastError());
    return 0;
}

int mg_num_envs(const mg_sim *s) { return s ? s->main.S.n_envs : -22; }

int mg_step_form(const mg_sim *s, int32_t *out) {
    if (!s || !out) return set_err(-22, "mg_step_form: null argument");
    const StepCaps c = step_reported_caps(s->step_form, s->caps);
    out[0] = s->step_form; out[1] = s->step_blk;
    out[2] = c.nb; out[3] = c.ns; out[4] = c.nc; out[5] = c.na;
    return 0;
}

__global__ void __launch_bounds__(64) set_episode_steps_kernel(MGState S, const int32_t *steps) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < S.n_envs) S.episode_steps[e] = steps[e];
}

int mg_set_episode_steps(mg_sim *s, const int32_t *steps, void *stream) {
    if (!s || !steps) return set_err(-22, "mg_set_episode_steps: null argument");
    HIPC(hipSetDevice(s->device));
    hipLaunchKernelGGL(set_episode_steps_kernel, dim3(grid64(s)), dim3(64), 0, as_stream(stream), s->main.S, steps);
    HIPC(hipGetLastError());
    return 0;
}

int mg_enable_timing(mg_sim *s, int max_steps) {
    if (!s) return set_err(-22, "mg_enable_timing: null sim");
    HIPC(hipSetDevice(s->device));
    for (hipEvent_t e : s->ev) HIPC(hipEventDestroy(e));
    s->ev.clear();
    s->ev_used = 0;
    s->timing = max_steps > 0;
    for (int i = 0; i < 4 * max_steps; i++) {
        hipEvent_t e;
        HIPC(hipEventCreate(&e));
        s->ev.push_back(e);
    }
    return 0;
}

int mg_read_timing(mg_sim *s, double *out) {
    if (!s || !out) return set_err(-22, "mg_read_timing: null argument");
    double t_step = 0.0, t_render = 0.0, t_reset = 0.0;
    int n = (int)(s->ev_used / 4);
    for (int i = 0; i < n; i++) {
        float a = 0.f, b = 0.f, c = 0.f;
        const hipEvent_t *ev = &s->ev[4 * i];
        HIPC(hipEventSynchronize(ev[3]));
        HIPC(hipEventElapsedTime(&a, ev[0], ev[1]));
        HIPC(hipEventElapsedTime(&c, ev[1], ev[2]));
        HIPC(hipEventElapsedTime(&b, ev[2], ev[3]));
        t_step += a; t_render += b; t_reset += c;
    }
    out[0] = t_step; out[1] = t_render; out[2] = n; out[3] = t_reset;
    s->ev_used = 0;
    return 0;
}

// also a partly built sim (mg_create's failure paths): every member is null or zero until it is set
void mg_destroy(mg_sim *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (hipEvent_t e : s->ev) (void)hipEventDestroy(e);
    if (s->side) {
        (void)hipStreamSynchronize(s->side);
        (void)hipStreamDestroy(s->side);
    }
    if (s->ev_snap) (void)hipEventSynchronize(s->ev_snap);
    for (hipEvent_t e : {s->ev_copied, s->ev_prepared, s->ev_snap})
        if (e) (void)hipEventDestroy(e);
    (void)hipHostFree(s->snap_stage);
    for (void *p : {(void *)s->rows, (void *)s->pend, (void *)s->snap_dev, (void *)s->srows, (void *)s->dlib, (void *)s->reset_mask,
                    (void *)s->scene_built})
        (void)hipFree(p);
    for (StatePool *p : {&s->main, &s->shadow, &s->look.P, &s->fan.P}) pool_free(*p);
    delete s;
}

} // extern "C"
