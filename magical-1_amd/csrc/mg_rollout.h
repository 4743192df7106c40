// mg_rollout.h -- the env-step loop of step_seq_kernel (mg_seq.h) and lookahead_kernel (mg_lookahead.h): the text of the
// middle of both kernel bodies, from the scene check to the return of every lane but the env's scoring lane.  It is
// included INSIDE each kernel, after the lane map (mg_lanes.h) and the kernel's own n, and is followed by the kernel's
// tail.  (Why text and not a function: DESIGN.md, "One workgroup skeleton".)
//
// Both kernels are step_kernel (mg_stepk.h) with `for h < n` inside: step_kernel's scene check, ONE load of the LDS view,
// the env_substeps_* calls in step_kernel's order with no HBM traffic between them, the env's column written back, and
// then the kernel's tail on the env's scoring lane from the HBM column.  So an env's state after h iterations has the
// bits that h calls of mg_step give it: everything is compiled with -ffp-contract=off, and what the view does not carry
// from one env-step to the next (cached shape BBs, the constraints' pre-step products, the robot's targets and motor
// rates) is recomputed before use in every env-step.
//
// From the kernel: F = StepForm<VAR, BLK>; S, L, smem; lane, sub, e, shadow (mg_lanes.h); int n, the env's env-steps
// (set to 0 here for a shadow or a refused env); act and astride, step h's action being act[h * astride], in range for
// h < the launch's step count and e < n_envs; and these macros, each a single statement or expression, all undefined
// again at the end:
//   MG_ROLLOUT_EVERY           false: the env's column goes back to HBM once, at its own last step.  true: after every
//                              env-step of its n, and the scoring lane then runs MG_ROLLOUT_AFTER_STEP(h), x_{h+1} in HBM
//   MG_ROLLOUT_REFUSE()        on the scoring lane of an env whose scene the form cannot hold (never expected), after
//                              the `overflow` bit is set
//   MG_ROLLOUT_REFUSED_COOP()  on every lane of such an env's workgroup in the cooperative form, which then returns
//   MG_ROLLOUT_REFUSED_TAIL    true: a refused env reaches the kernel's tail as well, with n = 0
//   MG_ROLLOUT_IF_BOTH(a, b)   `if (a) if (b)` or `if ((a) && (b))`: the head of the bit-32 refusal.  The same test; the
//                              two kernels wrote it in these two shapes and the compiler lays the whole kernel out
//                              differently for each, so each keeps its own
//
// Barriers.  QUAD: all 64 lanes must meet every workgroup barrier, and the envs of a workgroup end at different h, so
// nothing returns before the loop's end and the workgroup loops to hw, the maximum n of its envs (all 64 lanes take part
// in the butterfly).  An env's column goes back from its own lanes between env_substeps_quad's closing barrier and the
// next barrier (no lane writes the view there: the next env-step writes it only behind its opening barrier).  An env past
// its n, like a shadow, goes on in LDS and touches neither its HBM column nor its outputs again: both are guarded by
// own && h < n.  EVERY adds a fence and a barrier per iteration, which publish the rows to the env's sub-lane 0; the hook
// reads HBM only, so the other lanes run on into the next env-step's opening barrier and wait there.  hw is uniform and
// nothing returns or breaks inside the loop, so all 64 lanes reach that barrier exactly hw times, as they do those of
// env_substeps_quad.  The closing fence and barrier order the rows the sibling lanes wrote before the scoring lane's
// reads by the memory model, not by one wavefront's in-order memory pipe (as step_kernel).  COOP: one env per workgroup,
// so n is uniform; all 64 lanes write the view back; the hook on lane 0 needs no barrier behind it, because the view is
// next written behind the next env-step's first barrier, which waits for lane 0.
    MGProf P;
    MG_PP_INIT(P);
    if constexpr (F::LDS) {
        constexpr StepCaps C = F::C;
        bool fits = true;
        if (S.nbodies[e] > C.nb || S.nshapes[e] > C.ns || S.ncons[e] > C.nc) {
            if (!shadow && sub == 0) {
                S.overflow[e] |= 16; // scene larger than the variant's LDS caps
                MG_ROLLOUT_REFUSE();
            }
            if (!F::QUAD) {
                MG_ROLLOUT_REFUSED_COOP();
                return;
            }
            fits = false;
        }
        // (COOP: NCS = 0, so ok is true)
        bool ok = F::NCS == 0 || (S.ncons[e] == C.nc && S.robot_body0[e] == 0 && S.robot_cons0[e] == 0);
        for (int c = 0; c < F::NCS; c++) {
            const ConsDesc d = static_cons(c);
            ok = ok && AT(S.ctype, c) == d.type && AT(S.ca, c) == d.a && AT(S.cb, c) == d.b;
        }
        for (int k = 0; k < S.nshapes[e] && k < C.ns && F::NCS > 0; k++) ok = ok && shape_body_slot(AT(S.sbody, k)); // arb_body
        MG_ROLLOUT_IF_BOTH(!ok && fits, !shadow && sub == 0) {
            S.overflow[e] |= 32; // the compiled constraint list does not describe this scene
            MG_ROLLOUT_REFUSE();
        }
        // the view is built from the LDS carve only, as step_kernel's
        MGState V = S;
        carve_view(V, smem, C, BLK);
        if constexpr (F::QUAD) {
            const bool own = !shadow && fits && ok;
            if (!own) n = 0;
            xfer_state_quad<C.nb, C.ns, C.nc, C.na, F::QL>(S, V, lane, e, sub);
            if (!fits && sub == 0) { // an empty scene in the env's column: nothing indexes past the caps
                V.nbodies[lane] = 0; V.nshapes[lane] = 0; V.ncons[lane] = 0; V.nactive[lane] = 0;
            }
            int hw = n;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const int o = __shfl_xor(hw, off, 64);
                hw = o > hw ? o : hw;
            }
            for (int h = 0; h < hw; h++) {
                env_substeps_quad<F::NCS, F::QL>(V, L, lane, sub, act[h * astride], P);   // ends with a workgroup barrier
                if constexpr (MG_ROLLOUT_EVERY) {
                    if (own && h < n) xfer_state(S, V, C, lane, e, false, false, sub, F::QL);
                    __threadfence_block();
                    __syncthreads();
                    if (own && sub == 0 && h < n) MG_ROLLOUT_AFTER_STEP(h);
                } else {
                    if (own && h + 1 == n) xfer_state(S, V, C, lane, e, false, false, sub, F::QL);
                }
            }
            __threadfence_block();
            __syncthreads();
            if (!(MG_ROLLOUT_REFUSED_TAIL ? !shadow : own) || sub != 0) return;
        } else {   // COOP
            xfer_state(S, V, C, 0, e, true, true, lane, 64);
            __syncthreads();
            for (int h = 0; h < n; h++) {
                env_substeps_coop(V, L, lane, act[h * astride], P);   // ends with a workgroup barrier
                if constexpr (MG_ROLLOUT_EVERY) {
                    xfer_state(S, V, C, 0, e, false, true, lane, 64);
                    __threadfence_block();
                    __syncthreads();
                    if (lane == 0) MG_ROLLOUT_AFTER_STEP(h);
                }
            }
            // (EVERY: HBM holds x_n already -- the last step's write-back, or the untouched column when n = 0)
            if constexpr (!MG_ROLLOUT_EVERY) xfer_state(S, V, C, 0, e, false, true, lane, 64);
            __threadfence_block();
            __syncthreads();
            if (lane != 0) return;
        }
    } else {   // form 0 steps S itself
        for (int h = 0; h < n; h++) {
            env_substeps(S, L, e, act[h * astride], P);
            if constexpr (MG_ROLLOUT_EVERY) MG_ROLLOUT_AFTER_STEP(h);
        }
    }
#undef MG_ROLLOUT_EVERY
#undef MG_ROLLOUT_REFUSE
#undef MG_ROLLOUT_REFUSED_COOP
#undef MG_ROLLOUT_AFTER_STEP
#undef MG_ROLLOUT_REFUSED_TAIL
#undef MG_ROLLOUT_IF_BOTH
