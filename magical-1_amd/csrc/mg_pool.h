// mg_pool.h -- the per-env state's layout and its pools.  Every copy of the state a sim keeps (the main pool, the
// next-layout shadow, the rollout pools of mg_lookahead and mg_plan) is a StatePool: one device allocation carved by
// layout(), which is a pure function of the padded env count, so row i of any two pools is the same field.
#pragma once
#include <hip/hip_runtime.h>
#include <functional>
#include <vector>
#include "mg_state.h"

// one [slot][N] row of the per-env state: env e's element is at pool + off + e * esize
enum { ROW_STATE = 0, ROW_RNG = 1 };   // ROW_RNG: the MT19937 key, which only resets read (physics and scoring draw nothing)
struct StateRow { uint64_t off; uint32_t esize, kind; };

// the element of a row, 8, 4, 2 or 1 bytes
__device__ __forceinline__ void copy_elem(char *dst, const char *src, uint32_t esize) {
    switch (esize) {
    case 8: *(uint64_t *)dst = *(const uint64_t *)src; break;
    case 4: *(uint32_t *)dst = *(const uint32_t *)src; break;
    case 2: *(uint16_t *)dst = *(const uint16_t *)src; break;
    default: *dst = *src; break;
    }
}

struct Carver {
    char *base;
    size_t off;
    std::vector<StateRow> *rows = nullptr;   // records every take as [n / N] rows (n = slots x N) of `kind`
    size_t N = 0;
    uint32_t kind = ROW_STATE;
    template <typename T> T *take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T *p = (T *)(base ? base + off : nullptr);
        if (rows)
            for (size_t k = 0; k < n / N; k++) rows->push_back(StateRow{off + k * N * sizeof(T), (uint32_t)sizeof(T), kind});
        off += n * sizeof(T);
        return p;
    }
};

inline void layout(MGState &S, Carver &c, bool frames = true) {
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
    S.target_out = nullptr;   // nothing reaches a bound output unless mg_bind_outputs says so (the main pool only)
    c.kind = ROW_RNG;
    S.mt_key = c.take<uint32_t>(624 * N);
    c.kind = ROW_STATE;
    S.mt_pos = c.take<int32_t>(N);
    c.rows = nullptr;   // state rows end here (frames and render scratch below are not part of a layout)
    if (!frames) { S.hist_allo = S.hist_ego = S.scache = S.scache_ok = nullptr; S.hist_head = nullptr; return; }
    size_t FR = (size_t)MG_LORES * MG_LORES * 3;
    S.hist_allo = c.take<uint8_t>(4 * N * FR); S.hist_ego = c.take<uint8_t>(4 * N * FR);
    S.hist_head = c.take<int32_t>(2 * N);
    S.scache = c.take<uint8_t>(N * FR); S.scache_ok = c.take<uint8_t>(N);
}

// a copy of the per-env state: S's arrays are carved out of mem (zeroed), rows lists layout()'s state rows
struct StatePool { MGState S = {}; void *mem = nullptr; size_t bytes = 0; std::vector<StateRow> rows; };

inline void pool_free(StatePool &p) {
    (void)hipFree(p.mem);
    p = StatePool();
}

// p (empty) <- a pool of N (padded) envs with proto's scalars, with or without the frame rings; extra carves the
// caller's own arrays behind the state, and runs twice (sizing pass: null base).  A failure leaves p empty
inline hipError_t pool_create(StatePool &p, const MGState &proto, int N, bool frames,
                              const std::function<void(Carver &)> &extra = nullptr) {
    p.S = proto;
    p.S.N = N;
    Carver sizing = {nullptr, 0};
    layout(p.S, sizing, frames);
    if (extra) extra(sizing);
    p.bytes = sizing.off + 256;
    hipError_t err = hipMalloc(&p.mem, p.bytes);
    if (err == hipSuccess) err = hipMemset(p.mem, 0, p.bytes);
    if (err != hipSuccess) { pool_free(p); return err; }
    Carver real = {(char *)p.mem, 0};
    real.rows = &p.rows;
    layout(p.S, real, frames);
    if (extra) extra(real);
    return hipSuccess;
}

// the rows a rollout needs copied: every state row but the MT19937 key, then the error flags
inline std::vector<StateRow> pool_rollout_rows(const StatePool &p) {
    std::vector<StateRow> out;
    for (const StateRow &r : p.rows)
        if (r.kind == ROW_STATE) out.push_back(r);
    out.push_back(StateRow{(uint64_t)((const char *)p.S.overflow - (const char *)p.mem), 4u, ROW_STATE});
    return out;
}
