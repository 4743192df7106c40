// mg_snapshot.h -- env state snapshots (mg_snapshot / mg_restore): blob layout and the launchers of mg_snapshot.hip.
//
// A blob holds `count` env records behind a 256-byte header:
//
//   [0, 256)                              SnapHeader (little-endian, zero padded)
//   [256, 256 + count * state_bytes)      state section: every row of the snapshot row table in the pool's own
//                                         orientation, [row][record], records fastest.  The rows are ordered by
//                                         element size (8, 4, 2, 1 bytes), so row r starts at pre[r] * count (pre[r] =
//                                         the element bytes of the rows before it, a multiple of its own element
//                                         size) and every element is naturally aligned for any count, with no padding
//                                         between rows; state_bytes is the per-record sum rounded up to 16.
//   [.., + count * nframes * 27648)       frames section: [record][frame][96 * 96 * 3], 16-byte aligned; which frames
//                                         a record carries depends on the preprocessor (snap_frame_count).
//
// So the blob's size is 256 + count * record_bytes exactly, record_bytes = state_bytes + nframes * 27648, and record k
// is addressable on its own (element k of each row, frame block k).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mg_common.h"

#define MG_SNAP_MAGIC 0x4E53474Du   // "MGSN"
#define MG_SNAP_VERSION 1
#define MG_SNAP_HEADER_BYTES 256
#define MG_SNAP_FRAME_BYTES (MG_LORES * MG_LORES * 3)
#define MG_SNAP_MAX_FRAMES 8

struct SnapHeader {
    uint32_t magic, version;
    int32_t task, rand_flags, preproc;
    int32_t max_bodies, max_shapes, max_cons, max_arb, max_ents;   // the MG_MAX_* caps the rows were laid out with
    int32_t nrows, nframes;
    int64_t state_bytes, record_bytes, count, total_bytes;
    uint8_t zero[MG_SNAP_HEADER_BYTES - 12 * 4 - 4 * 8];
};
static_assert(sizeof(SnapHeader) == MG_SNAP_HEADER_BYTES, "SnapHeader is the blob's first 256 bytes");

// one [slot][N] row of the pool in a record: env e's element at pool + off + e * esize, record k's at
// state section + pre * count + k * esize
struct SnapRow { uint64_t off; uint32_t esize, pre; };

// the frames of a record, in order: env e's frame f is the 27648 bytes at base[f] + e * 27648 (ring slots and the
// static layer in the pool; a plain current-frame view in the bound output buffer itself)
struct SnapFrames { int n; uint8_t *base[MG_SNAP_MAX_FRAMES]; };

// frames a record carries for a preprocessor (materialised stacks): LoRes4E / LoRes3EA: the ego ring (4), the
// current allo frame, the allo static layer; LoResStack: both rings; LoRes4A: the allo ring and the current ego frame
static inline int snap_frame_count(int preproc) {
    switch (preproc) {
    case MG_PREPROC_LORES4E: case MG_PREPROC_LORES3EA: return 6;
    case MG_PREPROC_LORESSTACK: return 8;
    case MG_PREPROC_LORES4A: return 5;
    default: return 0;
    }
}

// Both index arrays are device i32[n] or null (identity); the host has validated them (envs < live env count,
// recs < count) before any launch.  to_blob: record recs[k] <- env envs[k]; else env envs[k] <- record recs[k].
hipError_t mg_launch_snap_header(const SnapHeader &h, uint8_t *blob, hipStream_t st);
hipError_t mg_launch_snap_state(char *pool, char *state, const SnapRow *rows, int nrows, const int32_t *envs,
                                const int32_t *recs, int n, int64_t count, int to_blob, hipStream_t st);
hipError_t mg_launch_snap_frames(const SnapFrames &F, uint8_t *frames, const int32_t *envs, const int32_t *recs, int n,
                                 int to_blob, hipStream_t st);
// the bound outputs of the restored envs from their restored frame rings (no render: it would push a frame):
// ring[v] u8[4][N][27648] / head[v] i32[N] of view v (null: the view keeps no ring), plain[v] its current-frame
// output u8[.][27648] or null, stack[v] its [96][96][12] stack output or null
struct SnapRebuild { const uint8_t *ring[2]; const int32_t *head[2]; uint8_t *plain[2]; uint8_t *stack[2]; int N; };
hipError_t mg_launch_snap_rebuild(const SnapRebuild &R, const int32_t *envs, int n, hipStream_t st);
// PickAndPlace's target output of the restored envs from their tgt_* rows (as reset_env writes it)
hipError_t mg_launch_snap_target(const int32_t *tgt_ids, const double *tgt_x, const double *tgt_y, int N,
                                 double *target_out, const int32_t *envs, int n, hipStream_t st);
