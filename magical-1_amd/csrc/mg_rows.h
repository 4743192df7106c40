// mg_rows.h -- the sequential-impulse solver's rows as functions of values.
//
// One body of each row for the step forms: a form gathers the two bodies' velocities and the row's terms from
// wherever it keeps them (HBM, the LDS view, registers, lanes), calls the row and scatters what the row changed
// (the adapters in mg_step.h).  Nothing here touches MGState or a storage macro.  The arithmetic is Chipmunk's,
// operation for operation; bit parity with the oracle rests on it.
//
// Three places in mg_step.h keep a text of their own, for a register, scratch or speed bound that the shared row
// broke there ("Shared solver rows"), and must be edited in step with the rows here:
//   contact_row / contact_cached: harb_apply / harb_cached (the one-hot select form of forms 5 / 6)
//   joint_row / joint_cached:     cons_apply_impl / cons_cached_impl (form 0), lground_apply / lground_cached (form 4)
#pragma once
#include "mg_phys.h"

// one body's side of a row: velocities, bias velocities, inverse mass and moment
struct Side { double vx, vy, w, vbx, vby, wb, minv, iinv; };

// cpBody apply_impulse / apply_bias_impulse
MG_DEV void side_impulse(Side &X, V2 j, V2 r) {
    X.vx = X.vx + j.x * X.minv;
    X.vy = X.vy + j.y * X.minv;
    X.w = X.w + X.iinv * vcross(r, j);
}
MG_DEV void side_bias_impulse(Side &X, V2 j, V2 r) {
    X.vbx = X.vbx + j.x * X.minv;
    X.vby = X.vby + j.y * X.minv;
    X.wb = X.wb + X.iinv * vcross(r, j);
}

// ---- contact rows ----------------------------------------------------------
// one contact's pre-stepped terms (constant over the sweep) and the impulses the row accumulates
struct ContactTerms { double r1x, r1y, r2x, r2y, nMass, tMass, bias; };
struct ContactAcc { double jb, jn, jt; };

// cpArbiterApplyImpulse for one contact (a second text: harb_apply, mg_step.h).  LA / LB: the side is live; a static
// side (the static body, known at compile time) contributes velocity +0.0 and receives nothing.
template <bool LA, bool LB>
MG_DEV void contact_row(Side &A, Side &B, const ContactTerms &c, ContactAcc &acc, V2 n, double friction) {
    const double nMass = c.nMass;
    V2 r1 = v2(c.r1x, c.r1y), r2 = v2(c.r2x, c.r2y);
    V2 vb1 = v2(0.0, 0.0), v1 = v2(0.0, 0.0), vb2 = v2(0.0, 0.0), v2_ = v2(0.0, 0.0);
    if constexpr (LA) {
        vb1 = vadd(v2(A.vbx, A.vby), vmult(vperp(r1), A.wb));
        v1 = vadd(v2(A.vx, A.vy), vmult(vperp(r1), A.w));
    }
    if constexpr (LB) {
        vb2 = vadd(v2(B.vbx, B.vby), vmult(vperp(r2), B.wb));
        v2_ = vadd(v2(B.vx, B.vy), vmult(vperp(r2), B.w));
    }
    V2 vr = vsub(v2_, v1);
    double vbn = vdot(vsub(vb2, vb1), n);
    double vrn = vdot(vr, n);
    double vrt = vdot(vr, vperp(n));
    double jbn = (c.bias - vbn) * nMass;
    double jbnOld = acc.jb;
    double jBias = cpmax(jbnOld + jbn, 0.0);
    acc.jb = jBias;
    double jn = -(0.0 + vrn) * nMass;
    double jnOld = acc.jn;
    double jnAcc = cpmax(jnOld + jn, 0.0);
    acc.jn = jnAcc;
    double jtMax = friction * jnAcc;
    double jt = -vrt * c.tMass;
    double jtOld = acc.jt;
    double jtAcc = cpclamp(jtOld + jt, -jtMax, jtMax);
    acc.jt = jtAcc;
    V2 jb = vmult(n, jBias - jbnOld);
    if constexpr (LA) side_bias_impulse(A, vneg(jb), r1);
    if constexpr (LB) side_bias_impulse(B, jb, r2);
    V2 j = vrotate(n, v2(jnAcc - jnOld, jtAcc - jtOld));
    if constexpr (LA) side_impulse(A, vneg(j), r1);
    if constexpr (LB) side_impulse(B, j, r2);
}

// applyCachedImpulse of one contact (the arbiter's warm start)
template <bool LA, bool LB>
MG_DEV void contact_cached(Side &A, Side &B, const ContactTerms &c, const ContactAcc &acc, V2 n, double dt_coef) {
    V2 j = vmult(vrotate(n, v2(acc.jn, acc.jt)), dt_coef);
    if constexpr (LA) side_impulse(A, vneg(j), v2(c.r1x, c.r1y));
    if constexpr (LB) side_impulse(B, j, v2(c.r2x, c.r2y));
}

// ---- joint rows ------------------------------------------------------------
// a joint row's pre-stepped terms (constant over the sweep) and what the row writes
struct RegCons {
    double r1x, r1y, r2x, r2y, k11, k12, k21, k22, bias, bias2, jmax, ratio, ratio_inv, isum, rate, wcoef;
};
struct RegAcc { double jacc, jacc2, twrn; };

// applyImpulse of cpPivotJoint, cpGearJoint, cpRotaryLimitJoint, cpSimpleMotor and cpDampedRotarySpring (further
// texts: cons_apply_impl and lground_apply, mg_step.h).  A static side (LA / LB false) reads as zero velocities and
// receives nothing.  Where `type` is a compile-time constant the switch folds.
template <bool LA, bool LB>
MG_DEV void joint_row(int type, const RegCons &q, RegAcc &acc, Side &A, Side &B) {
    const double avx = LA ? A.vx : 0.0, avy = LA ? A.vy : 0.0, aw = LA ? A.w : 0.0;
    const double bvx = LB ? B.vx : 0.0, bvy = LB ? B.vy : 0.0, bw = LB ? B.w : 0.0;
    switch (type) {
    case MG_C_PIVOT: {
        V2 r1 = v2(q.r1x, q.r1y), r2 = v2(q.r2x, q.r2y);
        V2 v1 = vadd(v2(avx, avy), vmult(vperp(r1), aw));
        V2 v2_ = vadd(v2(bvx, bvy), vmult(vperp(r2), bw));
        V2 vr = vsub(v2_, v1);
        V2 d = vsub(v2(q.bias, q.bias2), vr);
        V2 j = v2(d.x * q.k11 + d.y * q.k12, d.x * q.k21 + d.y * q.k22);
        V2 jOld = v2(acc.jacc, acc.jacc2);
        V2 jAcc = vclamp(vadd(jOld, j), q.jmax);
        acc.jacc = jAcc.x; acc.jacc2 = jAcc.y;
        V2 dj = vsub(jAcc, jOld);
        if constexpr (LA) side_impulse(A, vneg(dj), r1);
        if constexpr (LB) side_impulse(B, dj, r2);
        break;
    }
    case MG_C_GEAR: {
        double wr = bw * q.ratio - aw;
        double j = (q.bias - wr) * q.isum;
        double jOld = acc.jacc;
        double jAcc = cpclamp(jOld + j, -q.jmax, q.jmax);
        acc.jacc = jAcc;
        j = jAcc - jOld;
        if constexpr (LA) A.w = A.w - j * A.iinv * q.ratio_inv;
        if constexpr (LB) B.w = B.w + j * B.iinv;
        break;
    }
    case MG_C_ROTLIMIT: {
        double bias = q.bias;
        if (!bias) return;
        double wr = bw - aw;
        double j = -(bias + wr) * q.isum;
        double jOld = acc.jacc;
        double jAcc = bias < 0.0 ? cpclamp(jOld + j, 0.0, q.jmax) : cpclamp(jOld + j, -q.jmax, 0.0);
        acc.jacc = jAcc;
        j = jAcc - jOld;
        if constexpr (LA) A.w = A.w - j * A.iinv;
        if constexpr (LB) B.w = B.w + j * B.iinv;
        break;
    }
    case MG_C_MOTOR: {
        double wr = bw - aw + q.rate;
        double j = -wr * q.isum;
        double jOld = acc.jacc;
        double jAcc = cpclamp(jOld + j, -q.jmax, q.jmax);
        acc.jacc = jAcc;
        j = jAcc - jOld;
        if constexpr (LA) A.w = A.w - j * A.iinv;
        if constexpr (LB) B.w = B.w + j * B.iinv;
        break;
    }
    case MG_C_SPRING: {
        double wrn = aw - bw;
        double w_damp = (acc.twrn - wrn) * q.wcoef;
        acc.twrn = wrn + w_damp;
        double j_damp = w_damp * q.isum;
        acc.jacc = acc.jacc + j_damp;
        if constexpr (LA) A.w = A.w + j_damp * A.iinv;
        if constexpr (LB) B.w = B.w - j_damp * B.iinv;
        break;
    }
    }
}

// applyCachedImpulse of the same joints (the spring has none)
template <bool LA, bool LB>
MG_DEV void joint_cached(int type, const RegCons &q, const RegAcc &acc, Side &A, Side &B, double dt_coef) {
    switch (type) {
    case MG_C_PIVOT: {
        V2 j = vmult(v2(acc.jacc, acc.jacc2), dt_coef);
        if constexpr (LA) side_impulse(A, vneg(j), v2(q.r1x, q.r1y));
        if constexpr (LB) side_impulse(B, j, v2(q.r2x, q.r2y));
        break;
    }
    case MG_C_GEAR: {
        double j = acc.jacc * dt_coef;
        if constexpr (LA) A.w = A.w - j * A.iinv * q.ratio_inv;
        if constexpr (LB) B.w = B.w + j * B.iinv;
        break;
    }
    case MG_C_ROTLIMIT:
    case MG_C_MOTOR: {
        double j = acc.jacc * dt_coef;
        if constexpr (LA) A.w = A.w - j * A.iinv;
        if constexpr (LB) B.w = B.w + j * B.iinv;
        break;
    }
    default: break;
    }
}
