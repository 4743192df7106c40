// mg_lookahead.hip -- mg_lookahead and the lookahead-kernel dispatch: the launch of a compiled (form, envs per
// workgroup) pair, the one the sim's mg_step runs (mg_stepforms.h).  The kernels live in mg_look_*.hip, one translation
// unit per row of the form table; the kernel itself: mg_lookahead.h.  The rollouts run on the sim's `look` pool, a
// rollout pool of one candidate per env (mg_plan.h), filled by mg_plan's fan-out copy with K = 1.
#include "mg_sim.h"

hipError_t mg_launch_lookahead(const MGState &S, const mg_library *L, int task, int form, int blk, int max_steps,
                               const uint8_t *actions, int H, const LookOut &out, hipStream_t st) {
#define MG_LOOK_CASE(F, B) \
    if (form == F && blk == B) return launch_lookahead_var<F, B>(S, L, task, max_steps, actions, H, out, st);
    MG_STEP_FORMS(MG_LOOK_CASE)
#undef MG_LOOK_CASE
    return hipErrorInvalidValue;
}

extern "C" int mg_lookahead(mg_sim *s, const uint8_t *actions, int32_t H, const mg_lookahead_out *out, void *stream) {
    if (!s || !out || !out->score) return set_err(-22, "mg_lookahead: null sim, out or out->score");
    if (H < 0 || H > 4096) return set_err(-22, "mg_lookahead: H must be in [0, 4096]");
    if (!actions && H > 0) return set_err(-22, "mg_lookahead: null actions with H > 0");
    HIPC(hipSetDevice(s->device));
    const int n = s->main.S.n_envs;
    RolloutPool &R = s->look;
    if (int rc = rollout_reserve(s, R, n, "mg_lookahead")) return rc;
    hipStream_t st = as_stream(stream);
    HIPC(mg_launch_plan_fan((const char *)s->main.mem, (char *)R.P.mem, R.rows, R.nrows, n, /*K*/ 1, st));
    const LookOut lo = {out->score, out->steps, out->bodies, out->counts, out->errors};
    HIPC(mg_launch_lookahead(R.P.S, s->dlib, s->task, s->step_form, s->step_blk, s->max_steps, actions, H, lo, st));
    return 0;
}
