// mg_snapshot.hip -- mg_snapshot_bytes / mg_snapshot / mg_restore and their data movement (layout: mg_snapshot.h).
//
// Two phases, both pure copies between the simulator's pool and a blob:
//  * state rows: one thread per (row, record).  The blob keeps the pool's orientation ([row][record]), so the 64
//    lanes of a wavefront touch one contiguous segment of the blob, and one contiguous segment of the pool
//    whenever the env list is a run (all envs, a pool chunk);
//  * frames: 27648-byte frames moved as 16-byte words, one workgroup of 192 threads per (record, frame) at a time
//    (1728 words = 9 per thread, all loaded before the first store).
// Grids are capped at 2048 workgroups (8 per CU) and stride over the rest.
#include <cstring>

#include "mg_sim.h"

#define SNAP_MAX_WG 2048
#define SNAP_ROWS_PER_WG 8

__global__ void __launch_bounds__(64) snap_header_kernel(SnapHeader h, uint32_t *blob) {
    blob[threadIdx.x] = ((const uint32_t *)&h)[threadIdx.x];   // 64 lanes x 4 bytes = the 256-byte header
}

template <bool TO_BLOB>
__global__ void __launch_bounds__(256) snap_state_kernel(char *__restrict__ pool, char *__restrict__ state,
                                                         const SnapRow *__restrict__ rows, int nrows,
                                                         const int32_t *__restrict__ envs, const int32_t *__restrict__ recs,
                                                         int n, int64_t count) {
    const int nrb = (n + 255) / 256, nrg = (nrows + SNAP_ROWS_PER_WG - 1) / SNAP_ROWS_PER_WG;
    for (int64_t item = blockIdx.x; item < (int64_t)nrb * nrg; item += gridDim.x) {
        const int k = (int)(item % nrb) * 256 + threadIdx.x;
        if (k >= n) continue;
        const size_t e = envs ? envs[k] : k, rec = recs ? recs[k] : k;
        const int r0 = (int)(item / nrb) * SNAP_ROWS_PER_WG, r1 = r0 + SNAP_ROWS_PER_WG < nrows ? r0 + SNAP_ROWS_PER_WG : nrows;
        for (int r = r0; r < r1; r++) {
            const SnapRow w = rows[r];   // uniform over the workgroup
            char *p = pool + w.off + e * w.esize;
            char *b = state + (size_t)w.pre * (size_t)count + rec * w.esize;
            if (TO_BLOB) copy_elem(b, p, w.esize);
            else copy_elem(p, b, w.esize);
        }
    }
}

template <bool TO_BLOB>
__global__ void __launch_bounds__(192) snap_frames_kernel(SnapFrames F, uint8_t *__restrict__ frames,
                                                          const int32_t *__restrict__ envs, const int32_t *__restrict__ recs,
                                                          int n) {
    constexpr int W = MG_SNAP_FRAME_BYTES / 16 / 192;   // 16-byte words per thread
    static_assert(W * 192 * 16 == MG_SNAP_FRAME_BYTES, "a frame is a whole number of 16-byte words per thread");
    for (int64_t item = blockIdx.x; item < (int64_t)n * F.n; item += gridDim.x) {
        const int k = (int)(item / F.n), f = (int)(item % F.n);
        const size_t e = envs ? envs[k] : k, rec = recs ? recs[k] : k;
        uint4 *p = (uint4 *)(F.base[f] + e * MG_SNAP_FRAME_BYTES);
        uint4 *b = (uint4 *)(frames + (rec * F.n + f) * MG_SNAP_FRAME_BYTES);
        uint4 *dst = TO_BLOB ? b : p;
        const uint4 *src = TO_BLOB ? p : b;
        uint4 v[W];
#pragma unroll
        for (int i = 0; i < W; i++) v[i] = src[i * 192 + threadIdx.x];
#pragma unroll
        for (int i = 0; i < W; i++) dst[i * 192 + threadIdx.x] = v[i];
    }
}

// FlattenFrameStack / EagerDictFrameStack of a restored env from its ring, as render_kernel's tail writes it: one
// thread per 4 pixels, 3 dwords of each of the 4 frames (oldest first: slots head + 1 .. head + 4, mod 4) in, the
// pixels' 48 stack bytes out as 3 x 16 B; the view's plain current frame is slot `head`
__global__ void __launch_bounds__(256) snap_rebuild_kernel(SnapRebuild R, const int32_t *__restrict__ envs, int n) {
    constexpr int Q = MG_LORES * MG_LORES / 4;   // pixel quads per frame
    const size_t FR = MG_SNAP_FRAME_BYTES;
    const int view = blockIdx.y;
    if (!R.ring[view]) return;
    for (int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x; gid < (int64_t)n * Q; gid += (int64_t)gridDim.x * 256) {
        const int k = (int)(gid / Q), q = (int)(gid % Q);
        const size_t e = envs ? envs[k] : k;
        const int head = R.head[view][e] & 3;
        uint32_t f[4][3];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t *src = (const uint32_t *)(R.ring[view] + ((size_t)((head + 1 + j) & 3) * R.N + e) * FR);
#pragma unroll
            for (int w = 0; w < 3; w++) f[j][w] = src[3 * q + w];
        }
        if (R.plain[view]) {
            uint32_t *o = (uint32_t *)(R.plain[view] + e * FR) + 3 * q;
            o[0] = f[3][0]; o[1] = f[3][1]; o[2] = f[3][2];
        }
        if (R.stack[view]) {
            uint32_t o[12];
#pragma unroll
            for (int b = 0; b < 48; b++) {   // output byte b: pixel b / 12, frame (b % 12) / 3, channel b % 3
                const int px = b / 12, j = (b % 12) / 3, sb = 3 * px + b % 3;   // source byte within 12
                const uint32_t byte = (f[j][sb / 4] >> (8 * (sb % 4))) & 255u;
                if (b % 4 == 0) o[b / 4] = byte; else o[b / 4] |= byte << (8 * (b % 4));
            }
            uint4 *dst = (uint4 *)(R.stack[view] + e * FR * 4) + 3 * q;
            dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
            dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
            dst[2] = make_uint4(o[8], o[9], o[10], o[11]);
        }
    }
}

__global__ void __launch_bounds__(64) snap_target_kernel(const int32_t *__restrict__ tgt_ids, const double *__restrict__ tgt_x,
                                                         const double *__restrict__ tgt_y, int N, double *__restrict__ out,
                                                         const int32_t *__restrict__ envs, int n) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n) return;
    const size_t e = envs ? envs[k] : k;
    double *t = out + 4 * e;
    t[0] = tgt_ids[e]; t[1] = tgt_ids[N + e]; t[2] = tgt_x[e]; t[3] = tgt_y[e];
}

static unsigned capped(int64_t items) { return (unsigned)(items < SNAP_MAX_WG ? (items > 0 ? items : 1) : SNAP_MAX_WG); }

hipError_t mg_launch_snap_header(const SnapHeader &h, uint8_t *blob, hipStream_t st) {
    hipLaunchKernelGGL(snap_header_kernel, dim3(1), dim3(64), 0, st, h, (uint32_t *)blob);
    return hipGetLastError();
}

hipError_t mg_launch_snap_state(char *pool, char *state, const SnapRow *rows, int nrows, const int32_t *envs,
                                const int32_t *recs, int n, int64_t count, int to_blob, hipStream_t st) {
    if (n <= 0 || nrows <= 0) return hipSuccess;
    const int64_t items = (int64_t)((n + 255) / 256) * ((nrows + SNAP_ROWS_PER_WG - 1) / SNAP_ROWS_PER_WG);
    if (to_blob)
        hipLaunchKernelGGL(snap_state_kernel<true>, dim3(capped(items)), dim3(256), 0, st, pool, state, rows, nrows, envs,
                           recs, n, count);
    else
        hipLaunchKernelGGL(snap_state_kernel<false>, dim3(capped(items)), dim3(256), 0, st, pool, state, rows, nrows, envs,
                           recs, n, count);
    return hipGetLastError();
}

hipError_t mg_launch_snap_frames(const SnapFrames &F, uint8_t *frames, const int32_t *envs, const int32_t *recs, int n,
                                 int to_blob, hipStream_t st) {
    if (n <= 0 || F.n <= 0) return hipSuccess;
    const int64_t items = (int64_t)n * F.n;
    if (to_blob)
        hipLaunchKernelGGL(snap_frames_kernel<true>, dim3(capped(items)), dim3(192), 0, st, F, frames, envs, recs, n);
    else
        hipLaunchKernelGGL(snap_frames_kernel<false>, dim3(capped(items)), dim3(192), 0, st, F, frames, envs, recs, n);
    return hipGetLastError();
}

hipError_t mg_launch_snap_rebuild(const SnapRebuild &R, const int32_t *envs, int n, hipStream_t st) {
    if (n <= 0 || (!R.ring[0] && !R.ring[1])) return hipSuccess;
    const int64_t blocks = ((int64_t)n * (MG_LORES * MG_LORES / 4) + 255) / 256;
    hipLaunchKernelGGL(snap_rebuild_kernel, dim3(capped(blocks), 2), dim3(256), 0, st, R, envs, n);
    return hipGetLastError();
}

hipError_t mg_launch_snap_target(const int32_t *tgt_ids, const double *tgt_x, const double *tgt_y, int N,
                                 double *target_out, const int32_t *envs, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(snap_target_kernel, dim3((n + 63) / 64), dim3(64), 0, st, tgt_ids, tgt_x, tgt_y, N, target_out,
                       envs, n);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// C ABI
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

int snap_init(mg_sim *s) {
    std::vector<SnapRow> srows;
    s->snap_state_bytes = snap_build_rows(s->main.rows, &s->main.S, s->main.mem, srows);
    s->nsrows = (int)srows.size();
    HIPC(hipMalloc((void **)&s->srows, srows.size() * sizeof(SnapRow)));
    HIPC(hipMemcpy(s->srows, srows.data(), srows.size() * sizeof(SnapRow), hipMemcpyHostToDevice));
    return 0;
}

extern "C" {

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
    const size_t slot = (size_t)s->main.S.N * MG_SNAP_FRAME_BYTES;
    auto ring = [&](uint8_t *r) { for (int k = 0; k < 4; k++) F.base[F.n++] = r + k * slot; };
    switch (s->preproc) {
    case MG_PREPROC_LORES4E: case MG_PREPROC_LORES3EA:
        ring(s->main.S.hist_ego); F.base[F.n++] = s->out.obs_allo; F.base[F.n++] = s->main.S.scache; break;
    case MG_PREPROC_LORESSTACK: ring(s->main.S.hist_allo); ring(s->main.S.hist_ego); break;
    case MG_PREPROC_LORES4A: ring(s->main.S.hist_allo); F.base[F.n++] = s->out.obs_ego; break;
    default: break;
    }
    return F;
}

// Stage the index arrays of a call on the device: envs / recs i32[n] (null: identity) and, for a restore, the u8[N]
// mask of the listed envs.  The staging buffers are the sim's own, so the previous call that used them must be done.
static int snap_stage_indices(mg_sim *s, hipStream_t st, const int32_t *envs, const int32_t *recs, int n, bool want_mask,
                              const int32_t **envs_dev, const int32_t **recs_dev, const uint8_t **mask_dev) {
    const size_t ne = (size_t)s->main.S.n_envs, bytes = 2 * ne * sizeof(int32_t) + (size_t)s->main.S.N;
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
        memset(hm, 0, (size_t)s->main.S.N);
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
    if (n <= 0 || n > s->main.S.n_envs || (!envs && n != s->main.S.n_envs))
        return set_err(-22, "mg_snapshot: n must be in [1, num_envs], and num_envs when envs is null");
    for (int k = 0; envs && k < n; k++)
        if (envs[k] < 0 || envs[k] >= s->main.S.n_envs) return set_err(-22, "mg_snapshot: env index out of range");
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
    HIPC(mg_launch_snap_state((char *)s->main.mem, state, s->srows, s->nsrows, de, dr, n, n, 1, st));
    HIPC(mg_launch_snap_frames(snap_frames(s), (uint8_t *)state + (int64_t)n * h.state_bytes, de, dr, n, 1, st));
    if (envs) { HIPC(hipEventRecord(s->ev_snap, st)); s->snap_inflight = 1; }
    return 0;
}

int mg_restore(mg_sim *s, const uint8_t *blob, const int32_t *envs, const int32_t *recs, int32_t n, void *stream) {
    if (!s || !blob) return set_err(-22, "mg_restore: null argument");
    if ((uintptr_t)blob & 15) return set_err(-22, "mg_restore: the blob must be 16-byte aligned");
    if (int rc = snap_check_mode(s, "mg_restore")) return rc;
    const int ne = s->main.S.n_envs;
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
    HIPC(mg_launch_snap_state((char *)s->main.mem, (char *)state, s->srows, s->nsrows, de, dr, n, h.count, 0, st));
    HIPC(mg_launch_snap_frames(snap_frames(s), (uint8_t *)state + h.count * h.state_bytes, de, dr, n, 0, st));
    // the bound outputs from the restored frame history
    SnapRebuild R;
    memset(&R, 0, sizeof(R));
    R.N = s->main.S.N;
    const int pp = s->preproc;
    if (pp == MG_PREPROC_LORESSTACK || pp == MG_PREPROC_LORES4A) {
        R.ring[0] = s->main.S.hist_allo; R.head[0] = s->main.S.hist_head;
        R.plain[0] = pp == MG_PREPROC_LORES4A ? s->out.obs_allo : nullptr;
        R.stack[0] = pp == MG_PREPROC_LORES4A ? s->out.obs_past : s->out.obs_allo;
    }
    if (pp == MG_PREPROC_LORESSTACK || pp == MG_PREPROC_LORES4E || pp == MG_PREPROC_LORES3EA) {
        R.ring[1] = s->main.S.hist_ego; R.head[1] = s->main.S.hist_head + s->main.S.N;
        R.plain[1] = pp == MG_PREPROC_LORESSTACK ? nullptr : s->out.obs_ego;
        R.stack[1] = pp == MG_PREPROC_LORESSTACK ? s->out.obs_ego : pp == MG_PREPROC_LORES4E ? s->out.obs_past : nullptr;
    }
    HIPC(mg_launch_snap_rebuild(R, de, n, st));
    if (pp == MG_PREPROC_LORES3EA)
        HIPC(mg_launch_compose3ea(s->main.S, (const uint8_t *)s->out.obs_allo, dm, (uint8_t *)s->out.obs_past, st));
    if (s->main.S.target_out)
        HIPC(mg_launch_snap_target(s->main.S.tgt_ids, s->main.S.tgt_x, s->main.S.tgt_y, s->main.S.N, s->main.S.target_out, de, n, st));
    // the next-layout shadow of the restored envs: the RNG is advanced only by resets, so the restored mt_* rows are
    // the state right after the env's latest reset and the shadow is re-primed from them exactly as after a masked
    // explicit mg_reset
    if (s->shadow.mem) {
        if (int rc = shadow_handover(s, st, dm, 0)) return rc;
        if (all) s->shadow_ok = 1;
    }
    if (staged) { HIPC(hipEventRecord(s->ev_snap, st)); s->snap_inflight = 1; }
    return 0;
}

} // extern "C"
