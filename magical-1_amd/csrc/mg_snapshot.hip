// mg_snapshot.hip -- data movement of mg_snapshot / mg_restore (layout: mg_snapshot.h; the C ABI is in mg_sim.hip).
//
// Two phases, both pure copies between the simulator's pool and a blob:
//  * state rows: one thread per (row, record).  The blob keeps the pool's orientation ([row][record]), so the 64
//    lanes of a wavefront touch one contiguous segment of the blob, and one contiguous segment of the pool
//    whenever the env list is a run (all envs, a pool chunk);
//  * frames: 27648-byte frames moved as 16-byte words, one workgroup of 192 threads per (record, frame) at a time
//    (1728 words = 9 per thread, all loaded before the first store).
// Grids are capped at 2048 workgroups (8 per CU) and stride over the rest.
#include "mg_snapshot.h"

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
            char *dst = TO_BLOB ? b : p;
            const char *src = TO_BLOB ? p : b;
            switch (w.esize) {
            case 8: *(uint64_t *)dst = *(const uint64_t *)src; break;
            case 4: *(uint32_t *)dst = *(const uint32_t *)src; break;
            case 2: *(uint16_t *)dst = *(const uint16_t *)src; break;
            default: *dst = *src; break;
            }
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
