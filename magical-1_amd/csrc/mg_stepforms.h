// mg_stepforms.h -- the step kernel's compiled forms, stated once for host and device: which (form, envs per
// workgroup) pairs exist, each form's per-env slot caps, the arrays of the LDS env view (carved by the kernel,
// counted by the launch) and which pair a scene runs.  Plain C++17 without the HIP runtime, so a host compiler
// takes the header alone (tests/step_forms_probe.cpp).
//
//   form 0: state in HBM, one env per lane (scenes beyond every LDS form's caps; runtime lists)
//   form 4: LDS view, one env per 64-lane wavefront, order-free phases across lanes (cooperative; runtime lists)
//   form 5: LDS view, robot only (MoveToRegion), compile-time constraint list, 64 / blk lanes per env ("quad")
//   form 6: the same with one single-shape block (MoveToCorner)
#pragma once
#include <stddef.h>
#include "mg_state.h"

#ifdef __HIPCC__
#define MG_HD __host__ __device__ __forceinline__
#else
#define MG_HD inline
#endif

// Every compiled (form, envs per workgroup) pair, one row per translation unit (mg_step_v4.hip, mg_step_quad.hip,
// mg_step_hbm.hip instantiate their row; they are separate units to compile in parallel).  8 envs per workgroup:
// robot-scene grids below 16 envs per CU (step_pick_blk).  4 envs per workgroup was removed in round 6
// (profiles/r06_blk4).
#define MG_STEP_FORMS_COOP(X) X(4, 1)
#define MG_STEP_FORMS_QUAD(X) X(5, 16) X(6, 16) X(5, 8) X(6, 8)
#define MG_STEP_FORMS_HBM(X) X(0, 1) X(0, 8) X(0, 64)
#define MG_STEP_FORMS(X) MG_STEP_FORMS_COOP(X) MG_STEP_FORMS_QUAD(X) MG_STEP_FORMS_HBM(X)

MG_HD constexpr bool mg_step_blk_ok(int form, int blk) {
#define MG_STEP_IS(F, B) if (form == F && blk == B) return true;
    MG_STEP_FORMS(MG_STEP_IS)
#undef MG_STEP_IS
    return false;
}

// per-env slot caps: bodies, shapes, constraints, arbiter slots
struct StepCaps { int nb, ns, nc, na; };

// Caps of the LDS forms (compile-time, so every LDS address folds to a constant offset from the lane's column);
// zeros for form 0, whose state stays in HBM.
MG_HD constexpr StepCaps step_form_caps(int form) {
    return form == 5 ? StepCaps{6, 5, 10, 20}      // robot only
         : form == 6 ? StepCaps{7, 6, 12, 32}      // robot + one single-shape block
         : form == 4 ? StepCaps{14, 53, 26, 48}    // up to 8 blocks incl. stars (Cluster*, MatchRegions)
         : StepCaps{0, 0, 0, 0};
}

// ---- the LDS env view ------------------------------------------------------
// The 10 substeps of an env-step touch only the env's bodies, shapes, constraints, arbiters and a few scalars.
// They are copied once per env-step from HBM ([slot][N] arrays) into LDS ([slot][blk] arrays, one column per env)
// and the MGState "view" V points there with V.N = blk, so the same device code runs against LDS.
// X(field, element type, multiplier, per-env rows): the array holds multiplier * rows * blk elements and starts
// 16-byte aligned, in this order.
#define MG_STEP_VIEW(X) \
    X(bpx, double, 1, nb) X(bpy, double, 1, nb) X(bvx, double, 1, nb) X(bvy, double, 1, nb) X(ba, double, 1, nb) \
    X(bw, double, 1, nb) X(bvbx, double, 1, nb) X(bvby, double, 1, nb) X(bwb, double, 1, nb) X(brc, double, 1, nb) \
    X(brs, double, 1, nb) X(bminv, double, 1, nb) X(biinv, double, 1, nb) X(bacache, double, 1, nb) \
    X(sr, double, 1, ns) X(su, double, 1, ns) X(sbbl, double, 1, ns) X(sbbb, double, 1, ns) X(sbbr, double, 1, ns) \
    X(sbbt, double, 1, ns) \
    X(cp, double, CP_NUM, nc) \
    X(anx, double, 1, na) X(any, double, 1, na) X(au, double, 1, na) X(acon, double, 2 * AC_NUM, na) \
    X(ahash, uint64_t, 2, na) \
    X(curr_dt, double, 1, one) X(target_speed, double, 1, one) X(rel_turn, double, 1, one) \
    X(target_finger, double, 1, one) \
    X(akey, int32_t, 1, na) X(astamp, uint32_t, 1, na) \
    X(nbodies, int32_t, 1, one) X(nshapes, int32_t, 1, one) X(ncons, int32_t, 1, one) X(nactive, int32_t, 1, one) \
    X(stamp, uint32_t, 1, one) X(overflow, int32_t, 1, one) X(robot_body0, int32_t, 1, one) \
    X(robot_cons0, int32_t, 1, one) \
    X(sgroup, int16_t, 1, ns) X(shash, int16_t, 1, ns) X(sbody, int8_t, 1, ns) X(spoly, int8_t, 1, ns) \
    X(ctype, int8_t, 1, nc) X(ca, int8_t, 1, nc) X(cb, int8_t, 1, nc) \
    X(astate, int8_t, 1, na) X(acount, int8_t, 1, na) X(asa, int8_t, 1, na) X(asb, int8_t, 1, na) \
    X(active, int8_t, 1, na)

struct StepViewRows { int nb, ns, nc, na, one; };
#define MG_STEP_VIEW_COUNT(mult, rows) ((size_t)(mult) * (size_t)d.rows * (size_t)blk)

// the next `count` elements of T, 16-byte aligned (a function of its own, as it has always been: written out in
// carve_view's macro the quad kernels come out with swapped operands in three commutative instructions)
template <typename T>
MG_HD T *step_carve(unsigned char *base, size_t &off, size_t count) {
    off = (off + 15) & ~(size_t)15;
    T *p = (T *)(base + off);
    off += count * sizeof(T);
    return p;
}

// point the view's arrays into smem: the kernel side of the table
MG_HD void carve_view(MGState &V, unsigned char *smem, const StepCaps &c, int blk) {
    const StepViewRows d = {c.nb, c.ns, c.nc, c.na, 1};
    size_t off = 0;
#define MG_STEP_CARVE(f, T, mult, rows) V.f = step_carve<T>(smem, off, MG_STEP_VIEW_COUNT(mult, rows));
    MG_STEP_VIEW(MG_STEP_CARVE)
#undef MG_STEP_CARVE
    V.N = blk;
    V.cons_cap = c.nc;
    V.arb_cap = c.na;
}

// bytes of the view: the dynamic LDS the launch asks for
MG_HD constexpr size_t mg_step_lds_bytes(const StepCaps &c, int blk) {
    const StepViewRows d = {c.nb, c.ns, c.nc, c.na, 1};
    size_t off = 0;
#define MG_STEP_TAKE(f, T, mult, rows) off = ((off + 15) & ~(size_t)15) + MG_STEP_VIEW_COUNT(mult, rows) * sizeof(T);
    MG_STEP_VIEW(MG_STEP_TAKE)
#undef MG_STEP_TAKE
    return (off + 15) & ~(size_t)15;
}
#undef MG_STEP_VIEW_COUNT

// a workgroup may have 160 KB of LDS (form 6 at 16 envs takes 159,104 B of it)
#define MG_STEP_FITS(F, B) \
    static_assert(F == 0 || mg_step_lds_bytes(step_form_caps(F), B) <= 160 * 1024, "LDS view beyond a workgroup's LDS");
MG_STEP_FORMS(MG_STEP_FITS)
#undef MG_STEP_FITS

// ---- which pair a scene runs -----------------------------------------------
// Slot caps of a task's scenes; star_shapes: shapes of a star block (the most of any block type).
MG_HD constexpr StepCaps step_caps(int task, int flags, int star_shapes) {
    int nblk = 0, per_blk = star_shapes;
    switch (task) {
    case MG_TASK_MOVE_TO_REGION: nblk = 0; break;
    case MG_TASK_MOVE_TO_CORNER: nblk = 1; per_blk = (flags & MG_RAND_SHAPE_TYPE) ? star_shapes : 1; break;
    case MG_TASK_CLUSTER_COLOUR:
    case MG_TASK_CLUSTER_SHAPE: nblk = (flags & MG_RAND_SHAPE_COUNT) ? 10 : 8; break;
    case MG_TASK_MAKE_LINE: nblk = 4; break;
    case MG_TASK_FIND_DUPE: nblk = 7; break;
    case MG_TASK_FIX_COLOUR: nblk = 3; break;
    case MG_TASK_PICK_AND_PLACE: nblk = 3; break;
    default: nblk = (flags & MG_RAND_SHAPE_COUNT) ? 8 : 5; break;
    }
    const int ns = 5 + nblk * per_blk;
    const int pairs = 4 * ns + 5 * (ns - 5) + ((ns - 5) * (ns - 6)) / 2; // walls, robot-block, block-block
    return StepCaps{6 + nblk, ns, 10 + 2 * nblk, pairs < MG_MAX_ARB ? (pairs + 3) / 4 * 4 : MG_MAX_ARB};
}

// The form of a scene with these caps (measured on MI355X, 8192 envs, ms per env-step of physics):
// * compiled constraint lists (robot only / robot + one block): forms 5 / 6 (4096 envs: MoveToRegion 0.62 ms,
//   MoveToCorner 1.15; one env per lane, deleted in round 5: 0.73 / 1.42);
// * every other scene within form 4's caps: the cooperative form -- MatchRegions-TestAll 6.0 ms (one env per
//   single-lane workgroup, deleted in round 5: 10.6; form 0: 21.1), ClusterColour-Demo 8.6 ms (15.1; form 0: 10.7).
//   Its arbiter slots must match exactly: the HBM slots beyond the task's cap are never initialised.
MG_HD constexpr int step_scene_form(const StepCaps &c) {
    for (int f = 5; f <= 6; f++) {
        const StepCaps k = step_form_caps(f);
        if (c.nb == k.nb && c.ns == k.ns && c.nc == k.nc && c.na == k.na) return f;
    }
    const StepCaps k = step_form_caps(4);
    return c.nb <= k.nb && c.ns <= k.ns && c.nc <= k.nc && c.na == k.na ? 4 : 0;
}

// ... unless MG_STEP_VARIANT asks for another (want; -1: unset).  Experiments and tests: 0 and 4 run any scene
// (a scene beyond form 4's caps raises its error flag), 5 / 6 only their own.
MG_HD constexpr int step_pick_form(const StepCaps &c, int want) {
    const int own = step_scene_form(c);
    return want == 0 || want == 4 || ((want == 5 || want == 6) && want == own) ? want : own;
}

// Envs per workgroup.  The quad forms below 16 envs x CUs run 8: the grid then still reaches every CU, and a
// workgroup takes half a CU's LDS, so render workgroups of another env chunk fit beside it (the pipelined pool's
// 2048-env chunks: MoveToRegion 2.82 -> 2.84 M env-steps/s, profiles/r04_check7/).  At 4096 envs and more, 16
// (8 measured slower there: two workgroups per CU, 0.83 vs 0.61 ms).  want_blk / want_blk0: MG_STEP_BLK (LDS
// forms) / MG_STEP_BLK0 (form 0), taken when the pair is compiled (0: unset).
MG_HD constexpr int step_pick_blk(int form, int n_envs, int cus, int want_blk, int want_blk0) {
    const int want = form == 0 ? want_blk0 : want_blk;
    if (mg_step_blk_ok(form, want)) return want;
    return form == 0 ? 64 : form == 4 ? 1 : n_envs < 16 * cus ? 8 : 16;
}

// what mg_step_form reports: the caps the kernel runs with
MG_HD constexpr StepCaps step_reported_caps(int form, const StepCaps &task) {
    return form == 0 ? task : step_form_caps(form);
}
