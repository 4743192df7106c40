// mg_lookahead.h -- the lookahead kernel template (mg_lookahead: H env-steps of physics on a scratch copy of the
// state, then the task's score) and its launcher.  One instantiation per (form, envs per workgroup) pair of the
// step kernel's table (mg_stepforms.h), in translation units of their own (mg_look_quad.hip: 5 / 6, mg_look_v4.hip:
// 4, mg_look_hbm.hip: 0); mg_lookahead.hip dispatches.
//
// The kernel is step_kernel (mg_stepk.h) with the env-step loop inside: the same workgroup map, the same scene
// checks, the same LDS view and transfers, the same env_substeps_* calls in the same order -- so an env's state
// after h iterations has the bits that h calls of mg_step give it (everything is compiled with -ffp-contract=off,
// and what the view does not carry from one env-step to the next -- cached shape BBs, the constraints' pre-step
// products, the robot's targets and motor rates -- is recomputed before use in every env-step, here as there).
// What differs: the view is loaded once and written back once, S is the sim's scratch pool (never its own state),
// and there is no episode counter, reward, done flag or reset -- only the outputs of LookOut.
#pragma once
#include "mg_stepk.h"

// the outputs (LookOut: mg_launch.h) of env e from the scratch state S after its n simulated env-steps (one lane per env)
MG_DEV void look_emit(const MGState &S, const mg_library *L, int e, int task, int n, const LookOut &o) {
    o.score[e] = score_env(S, L, e, task);
    if (o.steps) o.steps[e] = n;
    if (o.errors) o.errors[e] = S.overflow[e];
    if (o.bodies) {   // as bodies_kernel (mg_get_bodies)
        const int nb = S.nbodies[e];
        for (int b = 0; b < MG_MAX_BODIES; b++) {
            double *q = o.bodies + ((size_t)e * MG_MAX_BODIES + b) * 6;
            const bool live = b < nb;
            q[0] = live ? AT(S.bpx, b) : 0.0; q[1] = live ? AT(S.bpy, b) : 0.0; q[2] = live ? AT(S.ba, b) : 0.0;
            q[3] = live ? AT(S.bvx, b) : 0.0; q[4] = live ? AT(S.bvy, b) : 0.0; q[5] = live ? AT(S.bw, b) : 0.0;
        }
    }
    if (o.counts) {
        o.counts[4 * e + 0] = S.nbodies[e]; o.counts[4 * e + 1] = S.nshapes[e];
        o.counts[4 * e + 2] = S.ncons[e]; o.counts[4 * e + 3] = S.nactive[e];
    }
}

// S: the scratch pool, holding a copy of every env's state.  actions: u8[H][n_envs], step-major.  Env e runs
// n = min(H, max_steps - episode_steps) env-steps (H when max_steps <= 0).
template <int VAR, int BLK>
__global__ void __launch_bounds__(64) lookahead_kernel(MGState S, const mg_library *__restrict__ L, int task, int max_steps,
                                                       const uint8_t *__restrict__ actions, int H, LookOut out) {
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr StepCaps C = step_form_caps(VAR);
    static_assert(mg_step_blk_ok(VAR, BLK), "not a pair of MG_STEP_FORMS (mg_stepforms.h)");
    constexpr bool LDS = VAR != 0;
    constexpr bool COOP = VAR == 4;            // one env per workgroup of 64 lanes
    constexpr bool QUAD = VAR == 5 || VAR == 6; // QL lanes per env, BLK envs in one 64-lane workgroup
    constexpr int QL = QUAD ? 64 / BLK : 1;
    constexpr int NCS = VAR == 4 ? 0 : C.nc;   // compile-time constraint list (0: the env's runtime list)
    const int lane = COOP ? (int)threadIdx.x : QUAD ? (int)threadIdx.x / QL : BLK == 1 ? 0 : (int)threadIdx.x;
    const int sub = QUAD ? (int)threadIdx.x % QL : 0;
    int e = xcd_block(blockIdx.x, gridDim.x) * BLK + (COOP ? 0 : lane);
    // QUAD: lanes without an env of their own (past n_envs, or a scene the form cannot hold) take part in the
    // workgroup barriers as shadows of a valid env and never write HBM: step_kernel's convention, unchanged
    bool shadow = false;
    if (e >= S.n_envs) {
        if (!QUAD) return;
        shadow = true;
        e = S.n_envs - 1;
    }
    const uint8_t *act = actions + e;   // step h: act[h * n_envs], h < H and e < n_envs
    const size_t astride = (size_t)S.n_envs;
    int n = H;
    if (max_steps > 0) {
        const int left = max_steps - S.episode_steps[e];
        n = left < 0 ? 0 : left < H ? left : H;
    }
    MGProf P;
    MG_PP_INIT(P);
    if constexpr (LDS) {
        bool fits = true;
        if (S.nbodies[e] > C.nb || S.nshapes[e] > C.ns || S.ncons[e] > C.nc) {
            if (!shadow && sub == 0) S.overflow[e] |= 16; // scene larger than the variant's LDS caps (never expected)
            fits = false;
        }
        bool ok = NCS == 0 || (S.ncons[e] == C.nc && S.robot_body0[e] == 0 && S.robot_cons0[e] == 0);
        for (int c = 0; c < NCS; c++) {
            const ConsDesc d = static_cons(c);
            ok = ok && AT(S.ctype, c) == d.type && AT(S.ca, c) == d.a && AT(S.cb, c) == d.b;
        }
        for (int k = 0; k < S.nshapes[e] && k < C.ns && NCS > 0; k++) ok = ok && shape_body_slot(AT(S.sbody, k)); // arb_body
        if (!ok && fits && !shadow && sub == 0) S.overflow[e] |= 32; // the compiled constraint list does not describe this scene
        if (!QUAD && !(fits && ok)) {   // COOP, uniform over the workgroup: nothing is simulated
            if (lane == 0) look_emit(S, L, e, task, 0, out);
            return;
        }
        MGState V = S;
        carve_view(V, smem, C, BLK);
        if constexpr (QUAD) {
            const bool own = !shadow && fits && ok;
            if (!own) n = 0;
            xfer_state_quad<C.nb, C.ns, C.nc, C.na, QL>(S, V, lane, e, sub, true);
            if (!fits && sub == 0) { // an empty scene in the env's column: nothing indexes past the caps
                V.nbodies[lane] = 0; V.nshapes[lane] = 0; V.ncons[lane] = 0; V.nactive[lane] = 0;
            }
            // every lane meets the workgroup barriers until the workgroup's longest env is done (all 64 lanes are
            // here: nothing has returned)
            int hw = n;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const int o = __shfl_xor(hw, off, 64);
                hw = o > hw ? o : hw;
            }
            for (int h = 0; h < hw; h++) {
                env_substeps_quad<NCS, QL>(V, L, lane, sub, act[h * astride], P);   // ends with a workgroup barrier
                // the env's last step: its column goes back to scratch from its own lanes, between that barrier and
                // the next env-step's opening one (no lane writes the view there); afterwards the env goes on in LDS
                // as a shadow does and never writes HBM again
                if (own && h + 1 == n) xfer_state(S, V, C, lane, e, false, false, sub, QL);
            }
            // the env's lane 0 reads scratch rows its sibling lanes wrote back: ordered by the memory model (as
            // step_kernel)
            __threadfence_block();
            __syncthreads();
            if (shadow || sub != 0) return;
        } else {   // COOP
            xfer_state(S, V, C, 0, e, true, true, lane, 64);
            __syncthreads();
            for (int h = 0; h < n; h++) env_substeps_coop(V, L, lane, act[h * astride], P);   // ends with a workgroup barrier
            xfer_state(S, V, C, 0, e, false, true, lane, 64);
            __threadfence_block();
            __syncthreads();
            if (lane != 0) return;
        }
    } else {
        for (int h = 0; h < n; h++) env_substeps(S, L, e, act[h * astride], P);
    }
    look_emit(S, L, e, task, n, out);
}

template <int VAR, int BLK>
hipError_t launch_lookahead_var(const MGState &S, const mg_library *L, int task, int max_steps, const uint8_t *actions,
                                int H, const LookOut &out, hipStream_t st) {
    constexpr size_t lds = VAR == 0 ? 0 : mg_step_lds_bytes(step_form_caps(VAR), BLK);
    static bool attr_set = false;
    if (VAR != 0 && !attr_set) {
        hipError_t err = hipFuncSetAttribute((const void *)lookahead_kernel<VAR, BLK>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err != hipSuccess) {
            fprintf(stderr, "lookahead form %d/%d: LDS attribute %zu B: %s\n", VAR, BLK, lds, hipGetErrorString(err));
            return err;
        }
        attr_set = true;
    }
    hipLaunchKernelGGL((lookahead_kernel<VAR, BLK>), dim3((S.n_envs + BLK - 1) / BLK), dim3(VAR == 0 ? BLK : 64), lds, st, S,
                       L, task, max_steps, actions, H, out);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess)
        fprintf(stderr, "lookahead form %d/%d: launch of %d workgroups, LDS %zu B: %s\n", VAR, BLK,
                (S.n_envs + BLK - 1) / BLK, lds, hipGetErrorString(err));
    return err;
}

// a translation unit instantiates its row of the form table: MG_STEP_FORMS_QUAD(MG_LOOK_INSTANTIATE)
#define MG_LOOK_INSTANTIATE(F, B) \
    template hipError_t launch_lookahead_var<F, B>(const MGState &, const mg_library *, int, int, const uint8_t *, int, \
                                                   const LookOut &, hipStream_t);
