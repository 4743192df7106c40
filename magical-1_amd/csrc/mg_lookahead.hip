// mg_lookahead.hip -- lookahead-kernel dispatch: the launch of a compiled (form, envs per workgroup) pair, the one
// the sim's mg_step runs (mg_stepforms.h).  The kernels live in mg_look_*.hip, one translation unit per row of the
// form table; the kernel itself: mg_lookahead.h; the C ABI (mg_lookahead) and the scratch pool: mg_sim.hip.
#include "mg_launch.h"

hipError_t mg_launch_lookahead(const MGState &S, const mg_library *L, int task, int form, int blk, int max_steps,
                               const uint8_t *actions, int H, const LookOut &out, hipStream_t st) {
#define MG_LOOK_CASE(F, B) \
    if (form == F && blk == B) return launch_lookahead_var<F, B>(S, L, task, max_steps, actions, H, out, st);
    MG_STEP_FORMS(MG_LOOK_CASE)
#undef MG_LOOK_CASE
    return hipErrorInvalidValue;
}
