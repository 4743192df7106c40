// mg_lookahead.hip -- mg_lookahead / mg_lookahead_obj and the lookahead-kernel dispatch: the launch of a compiled (form,
// envs per workgroup) pair, the one the sim's mg_step runs (mg_stepforms.h), plain or traced.  The kernels live in
// mg_look_*.hip, one translation unit per row of the form table; the kernel itself: mg_lookahead.h.  The rollouts run on
// the sim's `look` pool, a rollout pool of one candidate per env (mg_plan.h), filled by mg_plan's fan-out copy with K = 1.
#include <cmath>

#include "mg_sim.h"

static_assert(LOOK_OBJ_FINAL == MG_OBJ_FINAL && LOOK_OBJ_RETURN == MG_OBJ_RETURN && LOOK_OBJ_PEAK == MG_OBJ_PEAK,
              "mg_launch.h restates the header's objective kinds");

hipError_t mg_launch_lookahead(const MGState &S, const mg_library *L, int task, int form, int blk, int max_steps,
                               const uint8_t *actions, int H, const LookOut &out, const LookObj *obj, hipStream_t st) {
#define MG_LOOK_CASE(F, B) \
    if (form == F && blk == B) \
        return obj ? launch_look<F, B, true>(S, L, task, max_steps, actions, H, out, *obj, st) \
                   : launch_look<F, B, false>(S, L, task, max_steps, actions, H, out, LookObj{}, st);
    MG_STEP_FORMS(MG_LOOK_CASE)
#undef MG_LOOK_CASE
    return hipErrorInvalidValue;
}

int objective_check(const mg_objective *o, const char *fn) {
    const std::string f(fn);
    if (!o) return set_err(-22, f + ": null objective");
    if (o->kind < MG_OBJ_FINAL || o->kind > MG_OBJ_PEAK) return set_err(-22, f + ": objective kind must be 0, 1 or 2");
    if (o->reserved != 0) return set_err(-22, f + ": objective.reserved must be 0");
    if (!(o->gamma > 0.0 && o->gamma <= 1.0)) return set_err(-22, f + ": objective.gamma must be in (0, 1]");
    if (!(std::isfinite(o->tail) && o->tail >= 0.0)) return set_err(-22, f + ": objective.tail must be finite and >= 0");
    return 0;
}

LookObj objective_args(const mg_sim *s, const mg_objective *o) {
    LookObj a = {};
    a.kind = o->kind;
    a.debug = (s->flags & MG_DEBUG_REWARD) ? 1 : 0;
    a.gamma = o->gamma;
    a.tail = o->tail;
    return a;
}

// obj null: mg_lookahead.  The traced kernel runs for any kind but FINAL and for any requested objective output
static int lookahead_run(mg_sim *s, const char *fn, const uint8_t *actions, int32_t H, const mg_objective *obj,
                         const mg_lookahead_out *out, const mg_objective_out *oo, void *stream) {
    const std::string f(fn);
    if (!s || !out || !out->score) return set_err(-22, f + ": null sim, out or out->score");
    if (H < 0 || H > 4096) return set_err(-22, f + ": H must be in [0, 4096]");
    if (!actions && H > 0) return set_err(-22, f + ": null actions with H > 0");
    HIPC(hipSetDevice(s->device));
    const int n = s->main.S.n_envs;
    RolloutPool &R = s->look;
    if (int rc = rollout_reserve(s, R, n, fn)) return rc;
    hipStream_t st = as_stream(stream);
    HIPC(mg_launch_plan_fan((const char *)s->main.mem, (char *)R.P.mem, R.rows, R.nrows, n, /*K*/ 1, st));
    const LookOut lo = {out->score, out->steps, out->bodies, out->counts, out->errors};
    const bool wanted = oo && (oo->value || oo->peak || oo->peak_step || oo->score_trace || oo->reward_trace);
    if (!obj || (obj->kind == MG_OBJ_FINAL && !wanted)) {
        HIPC(mg_launch_lookahead(R.P.S, s->dlib, s->task, s->step_form, s->step_blk, s->max_steps, actions, H, lo, nullptr, st));
        return 0;
    }
    LookObj a = objective_args(s, obj);
    if (oo) {
        a.value = oo->value; a.peak = oo->peak; a.peak_step = oo->peak_step;
        a.score_trace = oo->score_trace; a.reward_trace = oo->reward_trace;
    }
    HIPC(mg_launch_lookahead(R.P.S, s->dlib, s->task, s->step_form, s->step_blk, s->max_steps, actions, H, lo, &a, st));
    return 0;
}

extern "C" int mg_lookahead(mg_sim *s, const uint8_t *actions, int32_t H, const mg_lookahead_out *out, void *stream) {
    return lookahead_run(s, "mg_lookahead", actions, H, nullptr, out, nullptr, stream);
}

extern "C" int mg_lookahead_obj(mg_sim *s, const uint8_t *actions, int32_t H, const mg_objective *obj,
                                const mg_lookahead_out *out, const mg_objective_out *obj_out, void *stream) {
    if (int rc = objective_check(obj, "mg_lookahead_obj")) return rc;
    return lookahead_run(s, "mg_lookahead_obj", actions, H, obj, out, obj_out, stream);
}
