// mg_physics.hip -- step-kernel dispatch: the launch of a compiled (form, envs per workgroup) pair.  The pairs,
// what each form is and which one a scene runs: mg_stepforms.h; the kernels live in mg_step_*.hip (one translation
// unit per row of the form table).  The one-lane-per-env LDS forms that 5/6/4 superseded were deleted in round 5
// (their A/B results are in DESIGN.md).  mg_step_seq's kernels (mg_seq.h, mg_seq_*.hip) are dispatched here likewise.
#include "mg_launch.h"

hipError_t mg_launch_step(const MGState &S, const mg_library *L, TaskCfg cfg, int form, int blk, int max_steps,
                          int auto_reset, const uint8_t *actions, float *reward, uint8_t *done, double *eval_score,
                          uint8_t *reset_mask, hipStream_t st) {
#define MG_STEP_CASE(F, B) \
    if (form == F && blk == B) \
        return launch_step_var<F, B>(S, L, cfg, max_steps, auto_reset, actions, reward, done, eval_score, reset_mask, st);
    MG_STEP_FORMS(MG_STEP_CASE)
#undef MG_STEP_CASE
    return hipErrorInvalidValue;
}

hipError_t mg_launch_step_seq(const MGState &S, const mg_library *L, TaskCfg cfg, int form, int blk, int max_steps,
                              int auto_reset, const uint8_t *actions, int R, float *reward, uint8_t *done,
                              double *eval_score, int32_t *steps, uint8_t *reset_mask, hipStream_t st) {
#define MG_SEQ_CASE(F, B) \
    if (form == F && blk == B) \
        return launch_step_seq_var<F, B>(S, L, cfg, max_steps, auto_reset, actions, R, reward, done, eval_score, steps, \
                                         reset_mask, st);
    MG_STEP_FORMS(MG_SEQ_CASE)
#undef MG_SEQ_CASE
    return hipErrorInvalidValue;
}

hipError_t mg_prof_read_physics(unsigned long long *out) {
    hipError_t e;
    if ((e = mg_prof_read_reset(out)) != hipSuccess) return e;
    if ((e = mg_prof_read_step_v4(out)) != hipSuccess) return e;
    if ((e = mg_prof_read_step_quad(out)) != hipSuccess) return e;
    return mg_prof_read_step_hbm(out);
}
