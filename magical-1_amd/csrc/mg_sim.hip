// mg_sim.hip -- gfx950 kernels and the C ABI (include/magical_sim.h).
//
// Per env-step (mg_step): step_kernel (mg_physics.hip: one env per lane: action
// decode, 10 x [Robot.update + cpSpaceStep], episode counter, score, in-place
// reset of finished episodes) then render_kernel (mg_raster.hip: one workgroup
// per (env, view): 384^2 raster in LDS bands -> 96^2 area downsample -> LoRes
// frame stack).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/magical_sim.h"
#include "mg_launch.h"
#include "mg_phys.h"
#include "mg_philox.h"
#include "mg_plan.h"
#include "mg_cem.h"
#include "mg_snapshot.h"

static thread_local std::string g_err;
static int set_err(int code, const std::string &msg) {
    g_err = msg;
    return code;
}
#define HIPC(x)                                                                                        \
    do {                                                                                               \
        hipError_t _e = (x);                                                                           \
        if (_e != hipSuccess) return set_err(-5, std::string(#x) + ": " + hipGetErrorString(_e));      \
    } while (0)

// one [slot][N] row of the per-env state: env e's element is at pool + off + e * esize
struct StateRow { uint64_t off; uint32_t esize, pad; };

struct mg_sim {
    MGState S;
    // Next-layout shadow (reset prefetch).  BaseEnv.reset draws the whole layout from the env's RNG and
    // nothing else (mg_reset.h reset_env), so the layout of an env's NEXT episode is known as soon as its
    // current one starts.  SH is a second copy of the per-env state (same layout, no frame rings): right
    // after an env resets, reset_kernel runs on SH for it on a side stream, overlapping the step and render
    // kernels; when the episode ends the auto-reset is a copy SH -> S of that env (reset_copy_kernel).
    MGState SH;
    void *shadow_pool;
    StateRow *rows;        // device table of the per-env state rows (both pools)
    int nrows;
    uint8_t *pend;         // device u8[N]: envs whose shadow the side stream is preparing
    hipStream_t side;
    hipEvent_t ev_copied, ev_prepared;
    int shadow_ok;         // every env's shadow holds its next layout (set by a full mg_reset)
    int shadow_pending;    // a reset_kernel on SH is in flight on the side stream
    int reset_waves;          // auto-reset launches: wavefronts cap (0: one per env; MG_RESET_WAVES, A/B)
    int no_fused_reset;       // MG_FUSED_RESET=0: the robot scenes' auto-reset as its own launch (A/B, tests)
    int reset_waves_shadow;   // the shadow's next-layout launches: the same (MG_RESET_WAVES_SHADOW)
    int copy_wg;              // reset_copy_kernel's workgroups cap (MG_COPY_WG: tests, A/B)
    int force_render_retry;   // tests: the first k render classes of the chain hand every (env, view) on
    int scache_mode;          // tests: RenderOut::scache_mode
    mg_library *dlib;
    void *pool;
    size_t pool_bytes;
    int task, flags, preproc, max_steps, device, auto_reset;
    mg_buffers out;
    int bound;
    // window rings of the stacked views (mg_bind_window; null: materialised stacks), their period, and the step
    // counter that picks the slot (advanced by every mg_step before its render; resets do not advance it)
    uint8_t *wring[2];
    int wK;
    long long wstep;
    StepCaps caps;     // the task's per-env slot caps
    int step_form;     // step kernel form and envs per workgroup: a compiled pair of mg_stepforms.h
    int step_blk;
    uint8_t *reset_mask; // device u8[N]: envs to auto-reset after the step
    // snapshots (mg_snapshot / mg_restore; layout: mg_snapshot.h)
    SnapRow *srows;            // device table of a record's rows: the state rows and the per-env items layout() keeps out of them
    int nsrows;
    int64_t snap_state_bytes;  // a record's state section bytes (rounded up to 16)
    // index arrays of a call (env list, record list, restore mask): pinned host staging and its device copy, allocated
    // by the first call that passes a list; ev_snap marks the end of the last call that used them
    char *snap_stage, *snap_dev;
    hipEvent_t ev_snap;
    int snap_inflight;
    // lookahead (mg_lookahead): LK is a third copy of the per-env state (the shadow's layout: no frame rings), the
    // scratch its rollouts run on; allocated by the first call.  look_rows: the state rows a rollout needs copied
    // (every row but the MT19937 key -- physics and scoring draw no numbers -- plus the error flags); the host
    // table is built in mg_create, its device copy with the pool
    MGState LK;
    void *look_pool;
    StateRow *look_rows;
    std::vector<StateRow> look_rows_host;
    // plan (mg_plan): FP is the fan pool, a state of plan_cap >= K * num_envs rollout envs laid out as LK is (no frame
    // rings); rollout k * num_envs + e starts as a copy of env e.  One allocation (plan_pool) holds the state rows,
    // the rollouts' scores (plan_scores f64[plan_cap]: the reduction's input also when the caller wants no scores) and
    // the device table of the fan-out's rows (plan_rows: look_rows_host's rows with their place in FP).  Allocated by
    // the first call, re-allocated by a call that needs more rollouts.  mg_plan_cem's per-env scratch, the elite
    // threshold (cem_thr f64[num_envs], cem_kthr i32[num_envs]), is part of the same allocation
    MGState FP;
    void *plan_pool;
    int plan_cap;
    double *plan_scores;
    PlanRow *plan_rows;
    double *cem_thr;
    int32_t *cem_kthr;
    // optional per-kernel timing (hipEvents on the launch stream)
    int timing;
    std::vector<hipEvent_t> ev;   // quadruples: before step_kernel, after it, after the auto-reset, after render_kernel
    size_t ev_used;
};

// ---------------------------------------------------------------------------
// kernels
__global__ void __launch_bounds__(64) bodies_kernel(MGState S, double *out, int32_t *counts) {
    int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= S.n_envs) return;
    for (int b = 0; b < MG_MAX_BODIES; b++) {
        double *o = out + ((size_t)e * MG_MAX_BODIES + b) * 6;
        if (b < S.nbodies[e]) {
            o[0] = AT(S.bpx, b); o[1] = AT(S.bpy, b); o[2] = AT(S.ba, b);
            o[3] = AT(S.bvx, b); o[4] = AT(S.bvy, b); o[5] = AT(S.bw, b);
        } else {
            for (int k = 0; k < 6; k++) o[k] = 0.0;
        }
    }
    if (counts) {
        counts[4 * e + 0] = S.nbodies[e]; counts[4 * e + 1] = S.nshapes[e];
        counts[4 * e + 2] = S.ncons[e]; counts[4 * e + 3] = S.nactive[e];
    }
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
            switch (w.esize) {
            case 8: *(uint64_t *)(dst + o) = *(const uint64_t *)(src + o); break;
            case 4: *(uint32_t *)(dst + o) = *(const uint32_t *)(src + o); break;
            case 2: *(uint16_t *)(dst + o) = *(const uint16_t *)(src + o); break;
            default: dst[o] = src[o]; break;
            }
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

// every env's rows src -> dst (mg_lookahead: the sim's state into its scratch pool).  One thread per (row, env),
// envs fastest: a wavefront moves one contiguous segment of a [slot][N] row; a workgroup takes LOOK_ROWS_PER_WG rows
// of its 256 envs.
#define LOOK_ROWS_PER_WG 8
__global__ void __launch_bounds__(256) look_copy_kernel(const char *__restrict__ src, char *__restrict__ dst,
                                                        const StateRow *__restrict__ rows, int nrows, int n_envs) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_envs) return;
    const int r0 = blockIdx.y * LOOK_ROWS_PER_WG, r1 = r0 + LOOK_ROWS_PER_WG < nrows ? r0 + LOOK_ROWS_PER_WG : nrows;
    for (int r = r0; r < r1; r++) {
        const StateRow w = rows[r];   // uniform over the workgroup
        const size_t o = w.off + (size_t)e * w.esize;
        switch (w.esize) {
        case 8: *(uint64_t *)(dst + o) = *(const uint64_t *)(src + o); break;
        case 4: *(uint32_t *)(dst + o) = *(const uint32_t *)(src + o); break;
        case 2: *(uint16_t *)(dst + o) = *(const uint16_t *)(src + o); break;
        default: dst[o] = src[o]; break;
        }
    }
}

// ---------------------------------------------------------------------------
// allocation
struct Carver {
    char *base;
    size_t off;
    std::vector<StateRow> *rows = nullptr;   // records every take as [n / N] rows (n = slots x N)
    size_t N = 0;
    template <typename T> T *take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T *p = (T *)(base ? base + off : nullptr);
        if (rows)
            for (size_t k = 0; k < n / N; k++) rows->push_back(StateRow{off + k * N * sizeof(T), (uint32_t)sizeof(T), 0u});
        off += n * sizeof(T);
        return p;
    }
};

static void layout(MGState &S, Carver &c, bool frames = true) {
    size_t N = (size_t)S.N;
    c.N = N;
    size_t B = MG_MAX_BODIES * N, SH = MG_MAX_SHAPES * N, C = MG_MAX_CONS * N, A = MG_MAX_ARB * N, E = MG_MAX_ENTS * N;
    S.bpx = c.take<double>(B); S.bpy = c.take<double>(B); S.bvx = c.take<double>(B); S.bvy = c.take<double>(B);
    S.ba = c.take<double>(B); S.bw = c.take<double>(B); S.bvbx = c.take<double>(B); S.bvby = c.take<double>(B);
    S.bwb = c.take<double>(B); S.brc = c.take<double>(B); S.brs = c.take<double>(B); S.bminv = c.take<double>(B);
    S.biinv = c.take<double>(B); S.bacache = c.take<double>(B); S.bkin = c.take<int8_t>(B);
    S.nbodies = c.take<int32_t>(N);
    S.sbody = c.take<int8_t>(SH); S.spoly = c.take<int8_t>(SH); S.sent = c.take<int8_t>(SH);
    S.sgroup = c.take<int16_t>(SH); S.shash = c.take<int16_t>(SH); S.scat = c.take<uint8_t>(SH);
    S.sr = c.take<double>(SH); S.su = c.take<double>(SH); S.sbbl = c.take<double>(SH); S.sbbb = c.take<double>(SH);
    S.sbbr = c.take<double>(SH); S.sbbt = c.take<double>(SH);
    S.nshapes = c.take<int32_t>(N);
    S.ctype = c.take<int8_t>(C); S.ca = c.take<int8_t>(C); S.cb = c.take<int8_t>(C);
    S.cp = c.take<double>((size_t)CP_NUM * C);
    S.ncons = c.take<int32_t>(N);
    S.akey = c.take<int32_t>(A); S.astamp = c.take<uint32_t>(A); S.astate = c.take<int8_t>(A);
    S.acount = c.take<int8_t>(A); S.asa = c.take<int8_t>(A); S.asb = c.take<int8_t>(A);
    S.anx = c.take<double>(A); S.any = c.take<double>(A); S.au = c.take<double>(A);
    S.acon = c.take<double>((size_t)2 * AC_NUM * A); S.ahash = c.take<uint64_t>(2 * A);
    S.active = c.take<int8_t>(A); S.nactive = c.take<int32_t>(N); S.stamp = c.take<uint32_t>(N);
    S.curr_dt = c.take<double>(N);
    {   // not state rows: the error flags are merged by reset_copy_kernel, rg_retry is render scratch
        std::vector<StateRow> *r = c.rows;
        c.rows = nullptr;
        S.overflow = c.take<int32_t>(N); S.rg_retry = c.take<uint8_t>(2 * N);
        c.rows = r;
    }
    S.target_speed = c.take<double>(N); S.rel_turn = c.take<double>(N); S.target_finger = c.take<double>(N);
    S.robot_body0 = c.take<int32_t>(N); S.robot_cons0 = c.take<int32_t>(N); S.pv = c.take<double>(5 * N);
    S.ekind = c.take<int8_t>(E); S.etype = c.take<int8_t>(E); S.ecol = c.take<int8_t>(E); S.erole = c.take<int8_t>(E);
    S.ebody0 = c.take<int8_t>(E); S.eshape0 = c.take<int8_t>(E); S.enshapes = c.take<int8_t>(E);
    S.ex = c.take<double>(E); S.ey = c.take<double>(E); S.eang = c.take<double>(E); S.eh = c.take<double>(E);
    S.ew = c.take<double>(E); S.nents = c.take<int32_t>(N);
    S.goal_ent = c.take<int32_t>(N); S.episode_steps = c.take<int32_t>(N);
    S.tgt_ent = c.take<int32_t>(N); S.tgt_ids = c.take<int32_t>(2 * N);
    S.tgt_x = c.take<double>(N); S.tgt_y = c.take<double>(N);
    S.target_out = nullptr;
    S.mt_key = c.take<uint32_t>(624 * N); S.mt_pos = c.take<int32_t>(N);
    c.rows = nullptr;   // state rows end here (frames and render scratch below are not part of a layout)
    if (!frames) { S.hist_allo = S.hist_ego = S.scache = S.scache_ok = nullptr; S.hist_head = nullptr; return; }
    size_t FR = (size_t)MG_LORES * MG_LORES * 3;
    S.hist_allo = c.take<uint8_t>(4 * N * FR); S.hist_ego = c.take<uint8_t>(4 * N * FR);
    S.hist_head = c.take<int32_t>(2 * N);
    S.scache = c.take<uint8_t>(N * FR); S.scache_ok = c.take<uint8_t>(N);
}

// The rows of a snapshot record (mg_snapshot.h): layout()'s state rows plus the per-env items it keeps out of them
// -- the error flags, the render chain level of each view (rg_retry: [N][2], one 2-byte element per env), the frame
// rings' heads and the static layer's valid flag -- ordered by element size so that every element of the blob's
// [row][record] state section is naturally aligned for any record count.  S / pool null: sizes only.  Returns a
// record's state bytes, rounded up to 16 (the frames section after it moves as 16-byte words).
static int64_t snap_build_rows(const std::vector<StateRow> &rows, const MGState *S, const void *pool,
                               std::vector<SnapRow> &out) {
    std::vector<SnapRow> all;
    for (const StateRow &r : rows) all.push_back(SnapRow{r.off, r.esize, 0u});
    auto extra = [&](const void *p, size_t step, uint32_t esize) {
        all.push_back(SnapRow{S ? (uint64_t)((const char *)p - (const char *)pool) + step : 0u, esize, 0u});
    };
    const size_t N = S ? (size_t)S->N : 0;
    extra(S ? S->overflow : nullptr, 0, 4);
    extra(S ? S->rg_retry : nullptr, 0, 2);
    extra(S ? S->hist_head : nullptr, 0, 4);
    extra(S ? S->hist_head : nullptr, N * 4, 4);
    extra(S ? S->scache_ok : nullptr, 0, 1);
    out.clear();
    uint32_t pre = 0;
    for (uint32_t es : {8u, 4u, 2u, 1u})
        for (const SnapRow &r : all)
            if (r.esize == es) { out.push_back(SnapRow{r.off, es, pre}); pre += es; }
    return ((int64_t)pre + 15) / 16 * 16;
}

static hipStream_t as_stream(void *s) { return (hipStream_t)s; }

static int grid64(const mg_sim *s) { return (s->S.n_envs + 63) / 64; }

static int render_lores(mg_sim *s, hipStream_t st, const uint8_t *mask) {
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
    HIPC(mg_launch_render(s->S, s->dlib, ro, 0, st));
    if (s->preproc == MG_PREPROC_LORES3EA && !s->out.frames_only)
        HIPC(mg_launch_compose3ea(s->S, (const uint8_t *)s->out.obs_allo, mask, (uint8_t *)s->out.obs_past, st));
    return 0;
}

// hand the state of the envs in mask (null: all) from one pool to the other on st, then prepare their
// next layouts on the side stream (reset_kernel on the shadow)
static int shadow_handover(mg_sim *s, hipStream_t st, const uint8_t *mask, int to_main) {
    if (s->shadow_pending) HIPC(hipStreamWaitEvent(st, s->ev_prepared, 0));   // pend and the shadow are free
    const char *src = (const char *)(to_main ? s->shadow_pool : s->pool);
    char *dst = (char *)(to_main ? s->pool : s->shadow_pool);
    const int cgrid = (s->copy_wg > 0 && s->S.n_envs > s->copy_wg) ? s->copy_wg : s->S.n_envs;
    hipLaunchKernelGGL(reset_copy_kernel, dim3(cgrid), dim3(256), 0, st, src, dst, s->rows, s->nrows, mask,
                       s->pend, s->S, s->SH, to_main);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(s->ev_copied, st));
    HIPC(hipStreamWaitEvent(s->side, s->ev_copied, 0));
    TaskCfg cfg = {s->task, s->flags};
    HIPC(mg_launch_reset(s->SH, s->dlib, cfg, s->pend, s->side, s->reset_waves_shadow));
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
    memset(&s->S, 0, sizeof(MGState));
    s->timing = 0; s->ev_used = 0; s->bound = 0;
    s->wring[0] = s->wring[1] = nullptr; s->wK = 0; s->wstep = 0;
    s->task = cfg->task; s->flags = cfg->rand_flags; s->preproc = cfg->preproc;
    s->max_steps = cfg->max_episode_steps; s->device = cfg->device; s->auto_reset = cfg->auto_reset;
    s->S.n_envs = cfg->num_envs;
    s->S.cons_cap = MG_MAX_CONS;
    s->S.arb_cap = MG_MAX_ARB;
    s->S.max_tries = 10000; // geom.py:198
    if (const char *mt = getenv("MG_DEBUG_MAX_TRIES")) s->S.max_tries = atoi(mt) > 0 ? atoi(mt) : 10000; // tests only
    s->reset_waves = getenv("MG_RESET_WAVES") ? atoi(getenv("MG_RESET_WAVES")) : 0;
    s->no_fused_reset = getenv("MG_FUSED_RESET") && atoi(getenv("MG_FUSED_RESET")) == 0;
    // the shadow's next layouts run beside the step stream's kernels: 256 wavefronts scanning the pending mask
    // instead of one 352-VGPR wavefront per env, most of which only exit (512: ClusterColour 1.458 -> 1.468 M,
    // MatchRegions 1.329 -> 1.358 M env-steps/s, same box; the in-place robot-scene resets gained nothing).
    // Round 5: 256 -- fewer 352-VGPR wavefronts holding SIMDs beside the render -- MatchRegions 1.375 -> 1.393 M,
    // ClusterColour unchanged; 64 makes a wavefront's serial run of layouts outlast the step (MatchRegions 1.11 M)
    s->reset_waves_shadow = getenv("MG_RESET_WAVES_SHADOW") ? atoi(getenv("MG_RESET_WAVES_SHADOW")) : 256;
    s->copy_wg = getenv("MG_COPY_WG") ? atoi(getenv("MG_COPY_WG")) : 2048;
    if (const char *rr = getenv("MG_DEBUG_RENDER_RETRY")) s->force_render_retry = atoi(rr);                 // tests only
    else s->force_render_retry = 0;
    s->scache_mode = getenv("MG_DEBUG_SCACHE") ? atoi(getenv("MG_DEBUG_SCACHE")) : 0;                    // tests only
    s->S.N = (cfg->num_envs + 63) / 64 * 64;
    std::vector<StateRow> rows;
    Carver sizing = {nullptr, 0};
    sizing.rows = &rows;
    layout(s->S, sizing);
    s->pool_bytes = sizing.off + 256;
    hipError_t err = hipMalloc(&s->pool, s->pool_bytes);
    if (err != hipSuccess) { delete s; return set_err(-12, std::string("mg_create: hipMalloc pool: ") + hipGetErrorString(err)); }
    HIPC(hipMemset(s->pool, 0, s->pool_bytes));
    Carver real = {(char *)s->pool, 0};
    layout(s->S, real);
    err = hipMalloc((void **)&s->dlib, sizeof(mg_library));
    if (err != hipSuccess) { (void)hipFree(s->pool); delete s; return set_err(-12, "mg_create: hipMalloc library"); }
    HIPC(hipMemcpy(s->dlib, cfg->library, sizeof(mg_library), hipMemcpyHostToDevice));
    // the step kernel's form and envs per workgroup (mg_stepforms.h); MG_STEP_VARIANT, MG_STEP_BLK (LDS forms) and
    // MG_STEP_BLK0 (form 0) override them for experiments and tests
    auto env_int = [](const char *name, int unset) { const char *v = getenv(name); return v ? atoi(v) : unset; };
    s->caps = step_caps(cfg->task, cfg->rand_flags, ((const mg_library *)cfg->library)->block_nshapes[MG_SHAPE_STAR]);
    s->step_form = step_pick_form(s->caps, env_int("MG_STEP_VARIANT", -1));
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device);
    s->step_blk = step_pick_blk(s->step_form, cfg->num_envs, cus, env_int("MG_STEP_BLK", 0), env_int("MG_STEP_BLK0", 0));
    err = hipMalloc((void **)&s->reset_mask, (size_t)s->S.N);
    if (err != hipSuccess) { (void)hipFree(s->pool); (void)hipFree(s->dlib); delete s; return set_err(-12, "mg_create: hipMalloc mask"); }
    HIPC(hipMemset(s->reset_mask, 0, (size_t)s->S.N));
    // next-layout shadow: the many-block tasks, whose rejection-sampled layouts make a reset long (the
    // robot scenes reset in ~0.03 ms); MG_RESET_PREFETCH=0/1 overrides
    s->shadow_pool = nullptr; s->rows = nullptr; s->pend = nullptr; s->side = nullptr;
    s->shadow_ok = 0; s->shadow_pending = 0; s->nrows = 0;
    bool prefetch = s->auto_reset && s->task != MG_TASK_MOVE_TO_REGION && s->task != MG_TASK_MOVE_TO_CORNER;
    if (const char *pf = getenv("MG_RESET_PREFETCH")) prefetch = s->auto_reset && atoi(pf) != 0;
    if (prefetch) {
        s->SH = s->S;
        s->SH.target_out = nullptr;
        Carver ssz = {nullptr, 0};
        layout(s->SH, ssz, false);
        HIPC(hipMalloc(&s->shadow_pool, ssz.off + 256));
        HIPC(hipMemset(s->shadow_pool, 0, ssz.off + 256));
        Carver sreal = {(char *)s->shadow_pool, 0};
        layout(s->SH, sreal, false);
        s->nrows = (int)rows.size();
        HIPC(hipMalloc((void **)&s->rows, rows.size() * sizeof(StateRow)));
        HIPC(hipMemcpy(s->rows, rows.data(), rows.size() * sizeof(StateRow), hipMemcpyHostToDevice));
        HIPC(hipMalloc((void **)&s->pend, (size_t)s->S.N));
        HIPC(hipMemset(s->pend, 0, (size_t)s->S.N));
        HIPC(hipStreamCreateWithFlags(&s->side, hipStreamNonBlocking));
        HIPC(hipEventCreateWithFlags(&s->ev_copied, hipEventDisableTiming));
        HIPC(hipEventCreateWithFlags(&s->ev_prepared, hipEventDisableTiming));
    }
    {   // a snapshot record's row table (mg_snapshot / mg_restore)
        std::vector<SnapRow> srows;
        s->snap_state_bytes = snap_build_rows(rows, &s->S, s->pool, srows);
        s->nsrows = (int)srows.size();
        s->srows = nullptr; s->snap_stage = s->snap_dev = nullptr; s->ev_snap = nullptr; s->snap_inflight = 0;
        HIPC(hipMalloc((void **)&s->srows, srows.size() * sizeof(SnapRow)));
        HIPC(hipMemcpy(s->srows, srows.data(), srows.size() * sizeof(SnapRow), hipMemcpyHostToDevice));
    }
    {   // the rows a lookahead copies into its scratch pool (allocated by the first mg_lookahead)
        const uint64_t mt0 = (uint64_t)((const char *)s->S.mt_key - (const char *)s->pool);
        const uint64_t mt1 = (uint64_t)((const char *)s->S.mt_pos - (const char *)s->pool);
        for (const StateRow &r : rows)
            if (r.off < mt0 || r.off >= mt1) s->look_rows_host.push_back(r);
        s->look_rows_host.push_back(StateRow{(uint64_t)((const char *)s->S.overflow - (const char *)s->pool), 4u, 0u});
        s->look_pool = nullptr; s->look_rows = nullptr;
        s->plan_pool = nullptr; s->plan_cap = 0; s->plan_scores = nullptr; s->plan_rows = nullptr;
        s->cem_thr = nullptr; s->cem_kthr = nullptr;
    }
    std::vector<uint32_t> seeds(cfg->num_envs);
    for (int i = 0; i < cfg->num_envs; i++) seeds[i] = cfg->seeds ? cfg->seeds[i] : cfg->base_seed + (uint32_t)i;
    *out = s;
    return mg_seed(s, seeds.data());
}

int mg_seed(mg_sim *s, const uint32_t *seeds_host) {
    if (!s || !seeds_host) return set_err(-22, "mg_seed: null argument");
    HIPC(hipSetDevice(s->device));
    if (s->shadow_pending) HIPC(hipEventSynchronize(s->ev_prepared));
    s->shadow_pending = 0;
    s->shadow_ok = 0;   // the shadow's layouts came from the old seeds: valid again after a full mg_reset
    uint32_t *d = nullptr;
    HIPC(hipMalloc(&d, sizeof(uint32_t) * s->S.n_envs));
    HIPC(hipMemcpy(d, seeds_host, sizeof(uint32_t) * s->S.n_envs, hipMemcpyHostToDevice));
    HIPC(mg_launch_seed(s->S, d, 0));
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
    s->S.target_out = b->target;
    s->bound = 1;
    return 0;
}

int mg_reset(mg_sim *s, const uint8_t *mask, void *stream) {
    if (!s) return set_err(-22, "mg_reset: null sim");
    if (!s->bound && s->preproc != MG_PREPROC_NONE) return set_err(-22, "mg_reset: outputs not bound");
    HIPC(hipSetDevice(s->device));
    hipStream_t st = as_stream(stream);
    TaskCfg cfg = {s->task, s->flags};
    HIPC(mg_launch_reset(s->S, s->dlib, cfg, mask, st));
    if (s->shadow_pool) {
        const int rc = shadow_handover(s, st, mask, 0);
        if (rc) return rc;
        if (!mask) s->shadow_ok = 1;
    }
    if (s->preproc != MG_PREPROC_NONE) return render_lores(s, st, mask);
    return 0;
}

int mg_step(mg_sim *s, const uint8_t *actions, void *stream) {
    if (!s || !actions) return set_err(-22, "mg_step: null argument");
    if (!s->bound && s->preproc != MG_PREPROC_NONE) return set_err(-22, "mg_step: outputs not bound");
    HIPC(hipSetDevice(s->device));
    hipStream_t st = as_stream(stream);
    TaskCfg cfg = {s->task, s->flags};
    // robot scenes without layout randomisation: the step kernel runs the auto-reset itself (mg_stepk.h)
    const bool layout = (s->flags & (MG_RAND_LAYOUT_MINOR | MG_RAND_LAYOUT_FULL)) != 0;
    cfg.fused_reset = s->auto_reset && !s->shadow_ok && !layout && !s->no_fused_reset &&
                      ((s->task == MG_TASK_MOVE_TO_REGION && s->step_form == 5) ||
                       (s->task == MG_TASK_MOVE_TO_CORNER && s->step_form == 6));
    hipEvent_t *ev = nullptr;
    if (s->timing && s->ev_used + 4 <= s->ev.size()) { ev = &s->ev[s->ev_used]; s->ev_used += 4; }
    if (ev) HIPC(hipEventRecord(ev[0], st));
    HIPC(mg_launch_step(s->S, s->dlib, cfg, s->step_form, s->step_blk, s->max_steps, s->auto_reset, actions, s->out.reward,
                        s->out.done, s->out.eval_score, s->reset_mask, st));
    if (ev) HIPC(hipEventRecord(ev[1], st));
    if (s->auto_reset) {
        if (s->shadow_ok) {
            const int rc = shadow_handover(s, st, s->reset_mask, 1);
            if (rc) return rc;
        } else if (!cfg.fused_reset) {
            HIPC(mg_launch_reset(s->S, s->dlib, cfg, s->reset_mask, st, s->reset_waves));
        }
    }
    if (ev) HIPC(hipEventRecord(ev[2], st));
    int rc = 0;
    s->wstep++;   // this step's frame goes to the window rings' next slot
    if (s->preproc != MG_PREPROC_NONE) rc = render_lores(s, st, nullptr);
    if (ev) HIPC(hipEventRecord(ev[3], st));
    return rc;
}

hipError_t mg_launch_replay(const uint8_t *frames, int32_t nframes, const int32_t *episode_start, int32_t preproc,
                            uint8_t *scratch, uint8_t *out_allo, uint8_t *out_ego, uint8_t *out_past, hipStream_t st);

int mg_replay_lores(const uint8_t *frames, int32_t nframes, const int32_t *episode_start, int32_t preproc,
                    uint8_t *scratch, uint8_t *out_allo, uint8_t *out_ego, uint8_t *out_past, void *stream) {
    if (nframes <= 0 || !frames || !episode_start || !scratch || !out_allo || !out_ego)
        return set_err(-22, "mg_replay_lores: null argument or nframes <= 0");
    if (preproc != MG_PREPROC_LORES4E && preproc != MG_PREPROC_LORESSTACK && preproc != MG_PREPROC_LORES3EA &&
        preproc != MG_PREPROC_LORES4A)
        return set_err(-22, "mg_replay_lores: preproc must be 1 (LoRes4E), 2 (LoResStack), 3 (LoRes3EA) or 4 (LoRes4A)");
    if (preproc != MG_PREPROC_LORESSTACK && !out_past) return set_err(-22, "mg_replay_lores: out_past required");
    const void *ptrs[6] = {frames, scratch, out_allo, out_ego, out_past ? out_past : out_allo, episode_start};
    for (const void *p : ptrs)
        if (((uintptr_t)p & 15) != 0) return set_err(-22, "mg_replay_lores: buffers must be 16-byte aligned");
    HIPC(mg_launch_replay(frames, nframes, episode_start, preproc, scratch, out_allo, out_ego, out_past,
                          as_stream(stream)));
    return 0;
}

hipError_t mg_launch_restack(const uint8_t *recv, int32_t world, int32_t n, int64_t stride, int64_t off_a,
                             int64_t off_e, int64_t off_d, int32_t preproc, int64_t step, int32_t all_fresh,
                             uint8_t *ring, uint8_t *out_allo, uint8_t *out_ego, uint8_t *out_past, hipStream_t st);

int mg_restack(const uint8_t *recv, int32_t world, int32_t n, int64_t rank_stride, int64_t off_allo, int64_t off_ego,
               int64_t off_done, int32_t preproc, int64_t step, int32_t all_fresh, uint8_t *ring, uint8_t *out_allo,
               uint8_t *out_ego, uint8_t *out_past, void *stream) {
    if (!recv || !ring || world <= 0 || n <= 0 || step < 0) return set_err(-22, "mg_restack: null argument or bad size");
    const int64_t FR = (int64_t)MG_LORES * MG_LORES * 3;
    if ((int64_t)world * n * (MG_LORES * MG_LORES / 4) >= ((int64_t)1 << 31))
        return set_err(-22, "mg_restack: world * n too large for one launch");
    if (preproc == MG_PREPROC_LORESSTACK) {
        if (!out_allo || !out_ego) return set_err(-22, "mg_restack: LoResStack needs out_allo and out_ego");
    } else if (preproc == MG_PREPROC_LORES4E || preproc == MG_PREPROC_LORES4A || preproc == MG_PREPROC_LORES3EA) {
        if (!out_past) return set_err(-22, "mg_restack: out_past required for this preprocessor");
    } else {
        return set_err(-22, "mg_restack: preproc must be 1 (LoRes4E), 2 (LoResStack), 3 (LoRes3EA) or 4 (LoRes4A)");
    }
    if (off_allo < 0 || off_ego < 0 || off_done < 0 || off_allo + n * FR > rank_stride || off_ego + n * FR > rank_stride ||
        off_done + n > rank_stride)
        return set_err(-22, "mg_restack: a key of the rank block lies outside rank_stride");
    const int64_t al[4] = {(int64_t)(uintptr_t)recv, rank_stride, off_allo, off_ego};
    for (int64_t a : al)
        if (a & 15) return set_err(-22, "mg_restack: recv, rank_stride and frame offsets must be 16-byte aligned");
    const void *ptrs[4] = {ring, out_allo, out_ego, out_past};
    for (const void *p : ptrs)
        if (((uintptr_t)p & 15) != 0) return set_err(-22, "mg_restack: buffers must be 16-byte aligned");
    HIPC(mg_launch_restack(recv, world, n, rank_stride, off_allo, off_ego, off_done, preproc, step, all_fresh, ring,
                           out_allo, out_ego, out_past, as_stream(stream)));
    return 0;
}

hipError_t mg_launch_restack_window(const uint8_t *recv, int32_t world, int32_t n, int64_t stride, int64_t off_a,
                                    int64_t off_e, int64_t off_d, int32_t preproc, int64_t step, int32_t all_fresh,
                                    int32_t K, uint8_t *ring, hipStream_t st);

int mg_restack_window(const uint8_t *recv, int32_t world, int32_t n, int64_t rank_stride, int64_t off_allo,
                      int64_t off_ego, int64_t off_done, int32_t preproc, int64_t step, int32_t all_fresh, int32_t K,
                      uint8_t *ring, void *stream) {
    if (!recv || !ring || world <= 0 || n <= 0 || step < 0) return set_err(-22, "mg_restack_window: null argument or bad size");
    if (K < 4 || K > 64) return set_err(-22, "mg_restack_window: K must be in [4, 64]");
    if (preproc != MG_PREPROC_LORES4E && preproc != MG_PREPROC_LORESSTACK && preproc != MG_PREPROC_LORES4A)
        return set_err(-22, "mg_restack_window: preproc must be 1 (LoRes4E), 2 (LoResStack) or 4 (LoRes4A); "
                            "LoRes3EA's stack is not one ring's window (use mg_restack)");
    if ((int64_t)world * n * (MG_LORES * MG_LORES / 16) >= ((int64_t)1 << 31))
        return set_err(-22, "mg_restack_window: world * n too large for one launch");
    const int64_t FR = (int64_t)MG_LORES * MG_LORES * 3;
    if (off_allo < 0 || off_ego < 0 || off_done < 0 || off_allo + n * FR > rank_stride || off_ego + n * FR > rank_stride ||
        off_done + n > rank_stride)
        return set_err(-22, "mg_restack_window: a key of the rank block lies outside rank_stride");
    const int64_t al[5] = {(int64_t)(uintptr_t)recv, rank_stride, off_allo, off_ego, (int64_t)(uintptr_t)ring};
    for (int64_t a : al)
        if (a & 15) return set_err(-22, "mg_restack_window: recv, ring, rank_stride and frame offsets must be 16-byte aligned");
    HIPC(mg_launch_restack_window(recv, world, n, rank_stride, off_allo, off_ego, off_done, preproc, step, all_fresh, K,
                                  ring, as_stream(stream)));
    return 0;
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
    HIPC(mg_launch_render(s->S, s->dlib, ro, 1, as_stream(stream)));
    return 0;
}

int mg_get_bodies(mg_sim *s, double *out, int32_t *counts, void *stream) {
    if (!s || !out) return set_err(-22, "mg_get_bodies: null argument");
    HIPC(hipSetDevice(s->device));
    hipLaunchKernelGGL(bodies_kernel, dim3(grid64(s)), dim3(64), 0, as_stream(stream), s->S, out, counts);
    HIPC(hipGetLastError());
    return 0;
}

int mg_get_arbiters(mg_sim *s, double *out, uint64_t *hash, void *stream) {
    if (!s || !out || !hash) return set_err(-22, "mg_get_arbiters: null argument");
    HIPC(hipSetDevice(s->device));
    hipLaunchKernelGGL(arbiters_kernel, dim3(grid64(s)), dim3(64), 0, as_stream(stream), s->S, out, hash);
    HIPC(hipGetLastError());
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
    if (!s || env < 0 || env >= s->S.n_envs || body < 0 || body >= MG_MAX_BODIES)
        return set_err(-22, "mg_set_body_pose: bad argument");
    HIPC(hipSetDevice(s->device));
    hipLaunchKernelGGL(set_body_pose_kernel, dim3(1), dim3(1), 0, as_stream(stream), s->S, env, body, x, y, angle);
    HIPC(hipGetLastError());
    return 0;
}

int mg_get_errors(mg_sim *s, int32_t *out, void *stream) {
    if (!s || !out) return set_err(-22, "mg_get_errors: null argument");
    HIPC(hipSetDevice(s->device));
    hipLaunchKernelGGL(errors_kernel, dim3(grid64(s)), dim3(64), 0, as_stream(stream), s->S, out);
    HIPC(hipGetLastError());
    return 0;
}

int mg_random_actions(mg_sim *s, uint8_t *actions, uint64_t key, uint64_t step, void *stream) {
    if (!s || !actions) return set_err(-22, "mg_random_actions: null argument");
    HIPC(hipSetDevice(s->device));
    hipLaunchKernelGGL(actions_kernel, dim3((s->S.n_envs + 255) / 256), dim3(256), 0, as_stream(stream), actions,
                       s->S.n_envs, key, step);
    HIPC(hipGetLastError());
    return 0;
}

int mg_num_envs(const mg_sim *s) { return s ? s->S.n_envs : -22; }

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
    hipLaunchKernelGGL(set_episode_steps_kernel, dim3(grid64(s)), dim3(64), 0, as_stream(stream), s->S, steps);
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

// ---------------------------------------------------------------------------
// snapshots (layout: mg_snapshot.h)
static SnapHeader snap_header(int task, int flags, int preproc, int nrows, int64_t state_bytes, int64_t count) {
    SnapHeader h;
    memset(&h, 0, sizeof(h));
    h.magic = MG_SNAP_MAGIC; h.version = MG_SNAP_VERSION;
    h.task = task; h.rand_flags = flags; h.preproc = preproc;
    h.max_bodies = MG_MAX_BODIES; h.max_shapes = MG_MAX_SHAPES; h.max_cons = MG_MAX_CONS; h.max_arb = MG_MAX_ARB;
    h.max_ents = MG_MAX_ENTS;
    h.nrows = nrows; h.nframes = snap_frame_count(preproc);
    h.state_bytes = state_bytes;
    h.record_bytes = state_bytes + (int64_t)h.nframes * MG_SNAP_FRAME_BYTES;
    h.count = count;
    h.total_bytes = MG_SNAP_HEADER_BYTES + count * h.record_bytes;
    return h;
}

int64_t mg_snapshot_bytes(const mg_config *cfg, int32_t n) {
    if (!cfg || n < 0) return set_err(-22, "mg_snapshot_bytes: null config or negative record count");
    if (cfg->task < 0 || cfg->task > MG_TASK_PICK_AND_PLACE) return set_err(-22, "mg_snapshot_bytes: unknown task");
    if (cfg->preproc < MG_PREPROC_NONE || cfg->preproc > MG_PREPROC_LORES4A)
        return set_err(-22, "mg_snapshot_bytes: unknown preprocessor");
    MGState S;
    memset(&S, 0, sizeof(S));
    S.N = 64;
    std::vector<StateRow> rows;
    Carver sizing = {nullptr, 0};
    sizing.rows = &rows;
    layout(S, sizing);
    std::vector<SnapRow> srows;
    const int64_t sb = snap_build_rows(rows, nullptr, nullptr, srows);
    return snap_header(cfg->task, cfg->rand_flags, cfg->preproc, (int)srows.size(), sb, n).total_bytes;
}

// what both calls refuse: sims whose frame history is not in the pool
static int snap_check_mode(const mg_sim *s, const char *fn) {
    if (s->wring[0] || s->wring[1])
        return set_err(-22, std::string(fn) + ": not supported with window rings bound (mg_bind_window): the stacks' frames "
                                              "live in the caller's rings");
    if (s->bound && s->out.frames_only)
        return set_err(-22, std::string(fn) + ": not supported with frames_only outputs: the frame stacks live with the "
                                              "receivers (mg_restack)");
    if (!s->bound && s->preproc != MG_PREPROC_NONE) return set_err(-22, std::string(fn) + ": outputs not bound");
    return 0;
}

// the frames of a record (snap_frame_count): ring slots and static layer in the pool, plain current frames in the
// bound outputs
static SnapFrames snap_frames(const mg_sim *s) {
    SnapFrames F;
    memset(&F, 0, sizeof(F));
    const size_t slot = (size_t)s->S.N * MG_SNAP_FRAME_BYTES;
    auto ring = [&](uint8_t *r) { for (int k = 0; k < 4; k++) F.base[F.n++] = r + k * slot; };
    switch (s->preproc) {
    case MG_PREPROC_LORES4E: case MG_PREPROC_LORES3EA:
        ring(s->S.hist_ego); F.base[F.n++] = s->out.obs_allo; F.base[F.n++] = s->S.scache; break;
    case MG_PREPROC_LORESSTACK: ring(s->S.hist_allo); ring(s->S.hist_ego); break;
    case MG_PREPROC_LORES4A: ring(s->S.hist_allo); F.base[F.n++] = s->out.obs_ego; break;
    default: break;
    }
    return F;
}

// Stage the index arrays of a call on the device: envs / recs i32[n] (null: identity) and, for a restore, the u8[N]
// mask of the listed envs.  The staging buffers are the sim's own, so the previous call that used them must be done.
static int snap_stage_indices(mg_sim *s, hipStream_t st, const int32_t *envs, const int32_t *recs, int n, bool want_mask,
                              const int32_t **envs_dev, const int32_t **recs_dev, const uint8_t **mask_dev) {
    const size_t ne = (size_t)s->S.n_envs, bytes = 2 * ne * sizeof(int32_t) + (size_t)s->S.N;
    if (!s->ev_snap) {
        HIPC(hipHostMalloc((void **)&s->snap_stage, bytes, hipHostMallocDefault));
        HIPC(hipMalloc((void **)&s->snap_dev, bytes));
        HIPC(hipEventCreateWithFlags(&s->ev_snap, hipEventDisableTiming));
    }
    if (s->snap_inflight) HIPC(hipEventSynchronize(s->ev_snap));
    s->snap_inflight = 0;
    int32_t *he = (int32_t *)s->snap_stage, *hr = he + ne;
    uint8_t *hm = (uint8_t *)(hr + ne);
    for (int k = 0; k < n; k++) { he[k] = envs ? envs[k] : k; hr[k] = recs ? recs[k] : k; }
    if (want_mask) {
        memset(hm, 0, (size_t)s->S.N);
        for (int k = 0; k < n; k++) hm[he[k]] = 1;
    }
    HIPC(hipMemcpyAsync(s->snap_dev, s->snap_stage, bytes, hipMemcpyHostToDevice, st));
    *envs_dev = (const int32_t *)s->snap_dev;
    *recs_dev = *envs_dev + ne;
    if (mask_dev) *mask_dev = (const uint8_t *)(*recs_dev + ne);
    return 0;
}

int mg_snapshot(mg_sim *s, const int32_t *envs, int32_t n, uint8_t *blob, void *stream) {
    if (!s || !blob) return set_err(-22, "mg_snapshot: null argument");
    if ((uintptr_t)blob & 15) return set_err(-22, "mg_snapshot: the blob must be 16-byte aligned");
    if (int rc = snap_check_mode(s, "mg_snapshot")) return rc;
    if (n <= 0 || n > s->S.n_envs || (!envs && n != s->S.n_envs))
        return set_err(-22, "mg_snapshot: n must be in [1, num_envs], and num_envs when envs is null");
    for (int k = 0; envs && k < n; k++)
        if (envs[k] < 0 || envs[k] >= s->S.n_envs) return set_err(-22, "mg_snapshot: env index out of range");
    HIPC(hipSetDevice(s->device));
    hipStream_t st = as_stream(stream);
    const int32_t *de = nullptr, *dr = nullptr;
    if (envs) {
        if (int rc = snap_stage_indices(s, st, envs, nullptr, n, false, &de, &dr, nullptr)) return rc;
        dr = nullptr;   // record k of the blob
    }
    const SnapHeader h = snap_header(s->task, s->flags, s->preproc, s->nsrows, s->snap_state_bytes, n);
    HIPC(mg_launch_snap_header(h, blob, st));
    char *state = (char *)blob + MG_SNAP_HEADER_BYTES;
    HIPC(mg_launch_snap_state((char *)s->pool, state, s->srows, s->nsrows, de, dr, n, n, 1, st));
    HIPC(mg_launch_snap_frames(snap_frames(s), (uint8_t *)state + (int64_t)n * h.state_bytes, de, dr, n, 1, st));
    if (envs) { HIPC(hipEventRecord(s->ev_snap, st)); s->snap_inflight = 1; }
    return 0;
}

int mg_restore(mg_sim *s, const uint8_t *blob, const int32_t *envs, const int32_t *recs, int32_t n, void *stream) {
    if (!s || !blob) return set_err(-22, "mg_restore: null argument");
    if ((uintptr_t)blob & 15) return set_err(-22, "mg_restore: the blob must be 16-byte aligned");
    if (int rc = snap_check_mode(s, "mg_restore")) return rc;
    const int ne = s->S.n_envs;
    if (n <= 0 || n > ne) return set_err(-22, "mg_restore: n must be in [1, num_envs]");
    std::vector<uint8_t> seen((size_t)ne, 0);
    for (int k = 0; envs && k < n; k++) {
        if (envs[k] < 0 || envs[k] >= ne) return set_err(-22, "mg_restore: env index out of range");
        if (seen[envs[k]]) return set_err(-22, "mg_restore: an env is listed twice");
        seen[envs[k]] = 1;
    }
    HIPC(hipSetDevice(s->device));
    hipStream_t st = as_stream(stream);
    // the header, after whatever wrote the blob on this stream: one small copy, before any kernel is launched
    SnapHeader h;
    HIPC(hipMemcpyAsync(&h, blob, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPC(hipStreamSynchronize(st));
    if (h.magic != MG_SNAP_MAGIC) return set_err(-22, "mg_restore: not a snapshot blob (bad magic value)");
    if (h.version != MG_SNAP_VERSION)
        return set_err(-22, "mg_restore: blob layout version " + std::to_string(h.version) + ", this library reads " +
                                std::to_string(MG_SNAP_VERSION));
    const SnapHeader w = snap_header(s->task, s->flags, s->preproc, s->nsrows, s->snap_state_bytes, h.count);
    if (h.task != w.task || h.rand_flags != w.rand_flags || h.preproc != w.preproc)
        return set_err(-22, "mg_restore: the blob is of task " + std::to_string(h.task) + ", rand_flags " +
                                std::to_string(h.rand_flags) + ", preproc " + std::to_string(h.preproc) + "; this sim is " +
                                std::to_string(w.task) + ", " + std::to_string(w.rand_flags) + ", " + std::to_string(w.preproc));
    if (h.max_bodies != w.max_bodies || h.max_shapes != w.max_shapes || h.max_cons != w.max_cons ||
        h.max_arb != w.max_arb || h.max_ents != w.max_ents || h.nrows != w.nrows || h.nframes != w.nframes ||
        h.state_bytes != w.state_bytes || h.record_bytes != w.record_bytes)
        return set_err(-22, "mg_restore: the blob's record layout (slot caps, rows, frames, record size) is not this library's");
    if (h.count <= 0 || h.count > INT32_MAX || h.total_bytes != w.total_bytes)
        return set_err(-22, "mg_restore: bad record count or blob size in the header");
    for (int k = 0; k < n; k++) {
        const int64_t r = recs ? recs[k] : k;
        if (r < 0 || r >= h.count) return set_err(-22, "mg_restore: record index out of range (the blob holds " +
                                                            std::to_string(h.count) + ")");
    }
    const bool all = n == ne;   // the listed envs are distinct: every env is restored
    const int32_t *de = nullptr, *dr = nullptr;
    const uint8_t *dm = nullptr;
    const bool staged = envs || recs || !all;
    if (staged) {
        if (int rc = snap_stage_indices(s, st, envs, recs, n, true, &de, &dr, &dm)) return rc;
        if (all) dm = nullptr;
    }
    const char *state = (const char *)blob + MG_SNAP_HEADER_BYTES;
    HIPC(mg_launch_snap_state((char *)s->pool, (char *)state, s->srows, s->nsrows, de, dr, n, h.count, 0, st));
    HIPC(mg_launch_snap_frames(snap_frames(s), (uint8_t *)state + h.count * h.state_bytes, de, dr, n, 0, st));
    // the bound outputs from the restored frame history
    SnapRebuild R;
    memset(&R, 0, sizeof(R));
    R.N = s->S.N;
    const int pp = s->preproc;
    if (pp == MG_PREPROC_LORESSTACK || pp == MG_PREPROC_LORES4A) {
        R.ring[0] = s->S.hist_allo; R.head[0] = s->S.hist_head;
        R.plain[0] = pp == MG_PREPROC_LORES4A ? s->out.obs_allo : nullptr;
        R.stack[0] = pp == MG_PREPROC_LORES4A ? s->out.obs_past : s->out.obs_allo;
    }
    if (pp == MG_PREPROC_LORESSTACK || pp == MG_PREPROC_LORES4E || pp == MG_PREPROC_LORES3EA) {
        R.ring[1] = s->S.hist_ego; R.head[1] = s->S.hist_head + s->S.N;
        R.plain[1] = pp == MG_PREPROC_LORESSTACK ? nullptr : s->out.obs_ego;
        R.stack[1] = pp == MG_PREPROC_LORESSTACK ? s->out.obs_ego : pp == MG_PREPROC_LORES4E ? s->out.obs_past : nullptr;
    }
    HIPC(mg_launch_snap_rebuild(R, de, n, st));
    if (pp == MG_PREPROC_LORES3EA)
        HIPC(mg_launch_compose3ea(s->S, (const uint8_t *)s->out.obs_allo, dm, (uint8_t *)s->out.obs_past, st));
    if (s->S.target_out)
        HIPC(mg_launch_snap_target(s->S.tgt_ids, s->S.tgt_x, s->S.tgt_y, s->S.N, s->S.target_out, de, n, st));
    // the next-layout shadow of the restored envs: the RNG is advanced only by resets, so the restored mt_* rows are
    // the state right after the env's latest reset and the shadow is re-primed from them exactly as after a masked
    // explicit mg_reset
    if (s->shadow_pool) {
        if (int rc = shadow_handover(s, st, dm, 0)) return rc;
        if (all) s->shadow_ok = 1;
    }
    if (staged) { HIPC(hipEventRecord(s->ev_snap, st)); s->snap_inflight = 1; }
    return 0;
}

// ---------------------------------------------------------------------------
// lookahead (kernel: mg_lookahead.h)
static int look_alloc(mg_sim *s) {
    s->LK = s->S;
    s->LK.target_out = nullptr;   // nothing of a rollout reaches the bound outputs
    Carver sz = {nullptr, 0};
    layout(s->LK, sz, false);
    void *pool = nullptr;
    hipError_t err = hipMalloc(&pool, sz.off + 256);
    if (err != hipSuccess) return set_err(-12, std::string("mg_lookahead: hipMalloc scratch pool: ") + hipGetErrorString(err));
    StateRow *rows = nullptr;
    const size_t rb = s->look_rows_host.size() * sizeof(StateRow);
    err = hipMalloc((void **)&rows, rb);
    if (err == hipSuccess) err = hipMemset(pool, 0, sz.off + 256);
    if (err == hipSuccess) err = hipMemcpy(rows, s->look_rows_host.data(), rb, hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        (void)hipFree(pool); (void)hipFree(rows);
        return set_err(-12, std::string("mg_lookahead: scratch pool setup: ") + hipGetErrorString(err));
    }
    Carver real = {(char *)pool, 0};
    layout(s->LK, real, false);
    s->look_pool = pool; s->look_rows = rows;
    return 0;
}

int mg_lookahead(mg_sim *s, const uint8_t *actions, int32_t H, const mg_lookahead_out *out, void *stream) {
    if (!s || !out || !out->score) return set_err(-22, "mg_lookahead: null sim, out or out->score");
    if (H < 0 || H > 4096) return set_err(-22, "mg_lookahead: H must be in [0, 4096]");
    if (!actions && H > 0) return set_err(-22, "mg_lookahead: null actions with H > 0");
    HIPC(hipSetDevice(s->device));
    if (!s->look_pool)
        if (int rc = look_alloc(s)) return rc;
    hipStream_t st = as_stream(stream);
    const int nrows = (int)s->look_rows_host.size();
    hipLaunchKernelGGL(look_copy_kernel, dim3((s->S.n_envs + 255) / 256, (nrows + LOOK_ROWS_PER_WG - 1) / LOOK_ROWS_PER_WG),
                       dim3(256), 0, st, (const char *)s->pool, (char *)s->look_pool, s->look_rows, nrows, s->S.n_envs);
    HIPC(hipGetLastError());
    const LookOut lo = {out->score, out->steps, out->bodies, out->counts, out->errors};
    HIPC(mg_launch_lookahead(s->LK, s->dlib, s->task, s->step_form, s->step_blk, s->max_steps, actions, H, lo, st));
    return 0;
}

// ---------------------------------------------------------------------------
// plan (kernels: mg_plan.hip; the rollouts: the lookahead kernel on the fan pool)
static int plan_check_sizes(const mg_sim *s, const char *fn, int32_t H, int32_t K) {
    if (H < 0 || H > 4096) return set_err(-22, std::string(fn) + ": H must be in [0, 4096]");
    if (K < 1 || K > 4096) return set_err(-22, std::string(fn) + ": K must be in [1, 4096]");
    if ((int64_t)K * s->S.n_envs > MG_PLAN_MAX_ROLLOUTS)
        return set_err(-22, std::string(fn) + ": K * num_envs = " + std::to_string((int64_t)K * s->S.n_envs) +
                                " rollouts, more than MG_PLAN_MAX_ROLLOUTS = " + std::to_string(MG_PLAN_MAX_ROLLOUTS));
    return 0;
}

// (re)allocate the fan pool for M rollouts.  The device is synchronised first: an earlier call's kernels may still be
// running on the pool that is freed here.  On failure the sim has no fan pool and stays usable (the next mg_plan
// allocates again)
static int plan_alloc(mg_sim *s, int M) {
    HIPC(hipDeviceSynchronize());
    (void)hipFree(s->plan_pool);
    s->plan_pool = nullptr; s->plan_cap = 0; s->plan_scores = nullptr; s->plan_rows = nullptr;
    s->cem_thr = nullptr; s->cem_kthr = nullptr;
    MGState F = s->S;
    F.target_out = nullptr;   // nothing of a rollout reaches the bound outputs
    F.N = (M + 63) / 64 * 64;
    const size_t nrows = s->look_rows_host.size();
    double *thr = nullptr;     // mg_plan_cem's elite threshold, per env
    int32_t *kthr = nullptr;
    auto carve = [&](char *base, std::vector<StateRow> *rows, double **scores, PlanRow **table) {
        Carver c = {base, 0};
        c.rows = rows;
        layout(F, c, false);
        *scores = c.take<double>((size_t)F.N);
        *table = c.take<PlanRow>(nrows);
        thr = c.take<double>((size_t)s->S.n_envs);
        kthr = c.take<int32_t>((size_t)s->S.n_envs);
        return c.off + 256;
    };
    double *scores = nullptr;
    PlanRow *table = nullptr;
    const size_t bytes = carve(nullptr, nullptr, &scores, &table);
    void *pool = nullptr;
    hipError_t err = hipMalloc(&pool, bytes);
    if (err != hipSuccess)
        return set_err(-12, std::string("mg_plan: hipMalloc fan pool of ") + std::to_string(bytes) + " bytes for " +
                                std::to_string(M) + " rollouts: " + hipGetErrorString(err));
    std::vector<StateRow> rows;
    carve((char *)pool, &rows, &scores, &table);
    // the fan-out's rows: look_rows_host's choice (every state row but the MT19937 key, then the error flags) of the
    // fan pool's rows, which layout() lists in the same order as the sim's
    std::vector<PlanRow> pr;
    const uint64_t mt0 = (uint64_t)((const char *)F.mt_key - (const char *)pool);
    const uint64_t mt1 = (uint64_t)((const char *)F.mt_pos - (const char *)pool);
    for (const StateRow &r : rows)
        if (r.off < mt0 || r.off >= mt1) pr.push_back(PlanRow{0u, r.off, r.esize, 0u});
    pr.push_back(PlanRow{0u, (uint64_t)((const char *)F.overflow - (const char *)pool), 4u, 0u});
    bool same = pr.size() == nrows;
    for (size_t i = 0; same && i < nrows; i++) {
        pr[i].src = s->look_rows_host[i].off;
        same = pr[i].esize == s->look_rows_host[i].esize;
    }
    if (!same) {
        (void)hipFree(pool);
        return set_err(-5, "mg_plan: the fan pool's rows do not match the sim's (layout() changed?)");
    }
    err = hipMemset(pool, 0, bytes);
    if (err == hipSuccess) err = hipMemcpy(table, pr.data(), nrows * sizeof(PlanRow), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        (void)hipFree(pool);
        return set_err(-12, std::string("mg_plan: fan pool setup: ") + hipGetErrorString(err));
    }
    s->FP = F;
    s->plan_pool = pool; s->plan_cap = M; s->plan_scores = scores; s->plan_rows = table;
    s->cem_thr = thr; s->cem_kthr = kthr;
    return 0;
}

int mg_plan(mg_sim *s, const uint8_t *actions, int32_t H, int32_t K, const mg_plan_out *out, void *stream) {
    if (!s || !out || !out->best) return set_err(-22, "mg_plan: null sim, out or out->best");
    if (int rc = plan_check_sizes(s, "mg_plan", H, K)) return rc;
    if (!actions && H > 0) return set_err(-22, "mg_plan: null actions with H > 0");
    HIPC(hipSetDevice(s->device));
    const int n = s->S.n_envs, M = K * n;
    if (M > s->plan_cap)
        if (int rc = plan_alloc(s, M)) return rc;
    hipStream_t st = as_stream(stream);
    // the pool may be larger than this call needs: its rows keep the stride it was laid out with, the launch covers M
    MGState F = s->FP;
    F.n_envs = M;
    HIPC(mg_launch_plan_fan((const char *)s->pool, (char *)s->plan_pool, s->plan_rows, (int)s->look_rows_host.size(), n, K, st));
    double *scores = out->scores ? out->scores : s->plan_scores;
    const LookOut lo = {scores, out->steps, nullptr, nullptr, out->errors};
    HIPC(mg_launch_lookahead(F, s->dlib, s->task, s->step_form, s->step_blk, s->max_steps, actions, H, lo, st));
    HIPC(mg_launch_plan_reduce(scores, actions, H, n, K, out->best, out->best_score, out->first_action, st));
    return 0;
}

int mg_plan_sample(mg_sim *s, uint8_t *actions, int32_t H, int32_t K, int32_t repeat, uint64_t key, uint64_t step,
                   void *stream) {
    if (!s || !actions) return set_err(-22, "mg_plan_sample: null argument");
    if (repeat < 1) return set_err(-22, "mg_plan_sample: repeat must be at least 1");
    if (int rc = plan_check_sizes(s, "mg_plan_sample", H, K)) return rc;
    if (H == 0) return 0;
    HIPC(hipSetDevice(s->device));
    HIPC(mg_launch_plan_sample(actions, s->S.n_envs, H, K, repeat, key, step, as_stream(stream)));
    return 0;
}

int mg_plan_cem(mg_sim *s, uint8_t *actions, uint16_t *weights, int32_t warm, int32_t H, int32_t K, int32_t iters,
                int32_t elites, int32_t alpha, int32_t repeat, uint64_t key, uint64_t step, const mg_plan_cem_out *out,
                void *stream) {
    if (!s || !actions || !weights || !out || !out->best)
        return set_err(-22, "mg_plan_cem: null sim, actions_dev, weights_dev, out or out->best");
    if (H < 1 || H > 4096) return set_err(-22, "mg_plan_cem: H must be in [1, 4096]");
    if (int rc = plan_check_sizes(s, "mg_plan_cem", H, K)) return rc;
    if (iters < 1 || iters > 64) return set_err(-22, "mg_plan_cem: iters must be in [1, 64]");
    if (elites < 1 || elites > K) return set_err(-22, "mg_plan_cem: elites must be in [1, K]");
    if (alpha < 0 || alpha > 1024) return set_err(-22, "mg_plan_cem: alpha must be in [0, 1024]");
    if (repeat < 1) return set_err(-22, "mg_plan_cem: repeat must be at least 1");
    if (warm != 0 && warm != 1) return set_err(-22, "mg_plan_cem: warm must be 0 or 1");
    HIPC(hipSetDevice(s->device));
    const int n = s->S.n_envs, M = K * n, J = (H + repeat - 1) / repeat;
    if (M > s->plan_cap)
        if (int rc = plan_alloc(s, M)) return rc;
    hipStream_t st = as_stream(stream);
    MGState F = s->FP;
    F.n_envs = M;
    double *scores = out->scores ? out->scores : s->plan_scores;
    const LookOut lo = {scores, out->steps, nullptr, nullptr, out->errors};
    CemUpdate u = {actions, weights, scores, s->cem_thr, s->cem_kthr, out->best, n, H, K, J, repeat, alpha,
                   /*refit*/ 0, /*uniform*/ warm ? 0 : 1, /*draw*/ 1, /*incumbent*/ 0, key, step};
    HIPC(mg_launch_cem_update(u, st));   // iteration 0's candidates
    u.refit = 1; u.uniform = 0; u.incumbent = 1;
    for (int i = 0; i < iters; i++) {
        const bool last = i == iters - 1;
        HIPC(mg_launch_plan_fan((const char *)s->pool, (char *)s->plan_pool, s->plan_rows, (int)s->look_rows_host.size(), n, K, st));
        HIPC(mg_launch_lookahead(F, s->dlib, s->task, s->step_form, s->step_blk, s->max_steps, actions, H, lo, st));
        double *bs = out->iter_best ? out->iter_best + (size_t)i * n : last ? out->best_score : nullptr;
        HIPC(mg_launch_plan_reduce(scores, actions, H, n, K, out->best, bs, out->first_action, st));
        if (last && out->iter_best && out->best_score)
            HIPC(hipMemcpyAsync(out->best_score, bs, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIPC(mg_launch_cem_threshold(scores, n, K, elites, s->cem_thr, s->cem_kthr, st));
        // refit to this iteration's elites; unless it is the last, draw the next one's candidates over them
        u.draw = last ? 0 : 1;
        u.counter = step + (uint64_t)(i + 1) * (uint64_t)K * (uint64_t)J;
        HIPC(mg_launch_cem_update(u, st));
    }
    return 0;
}

void mg_destroy(mg_sim *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (hipEvent_t e : s->ev) (void)hipEventDestroy(e);
    if (s->side) {
        (void)hipStreamSynchronize(s->side);
        (void)hipEventDestroy(s->ev_copied); (void)hipEventDestroy(s->ev_prepared);
        (void)hipStreamDestroy(s->side);
        (void)hipFree(s->shadow_pool); (void)hipFree(s->rows); (void)hipFree(s->pend);
    }
    if (s->ev_snap) {
        (void)hipEventSynchronize(s->ev_snap);
        (void)hipEventDestroy(s->ev_snap);
        (void)hipHostFree(s->snap_stage); (void)hipFree(s->snap_dev);
    }
    (void)hipFree(s->srows);
    (void)hipFree(s->look_pool); (void)hipFree(s->look_rows);
    (void)hipFree(s->plan_pool);
    (void)hipFree(s->pool);
    (void)hipFree(s->dlib);
    (void)hipFree(s->reset_mask);
    delete s;
}

} // extern "C"
