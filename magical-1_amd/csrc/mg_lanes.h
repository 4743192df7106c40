// mg_lanes.h -- the lane map of step_kernel (mg_stepk.h), step_seq_kernel (mg_seq.h) and lookahead_kernel
// (mg_lookahead.h): text included at the top of each kernel body, after `using F = StepForm<VAR, BLK>`.  It defines
// lane (the env's column in the view; in the cooperative form the lane's share of the rows), sub (QUAD: the lane's share
// of its env's rows), e (the env) and shadow.  QUAD: lanes without an env of their own (past n_envs, or a scene the form
// cannot hold) still take part in the workgroup barriers as shadows of a valid env; they never write HBM.  A lane of
// another form past n_envs has no barrier to meet and returns.  (Why text and not a function: DESIGN.md, "One workgroup
// skeleton".)
    const int lane = F::COOP ? (int)threadIdx.x : F::QUAD ? (int)threadIdx.x / F::QL : BLK == 1 ? 0 : (int)threadIdx.x;
    const int sub = F::QUAD ? (int)threadIdx.x % F::QL : 0;
    int e = xcd_block(blockIdx.x, gridDim.x) * BLK + (F::COOP ? 0 : lane);
    bool shadow = false;
    if (e >= S.n_envs) {
        if (!F::QUAD) return;
        shadow = true;
        e = S.n_envs - 1;
    }
