// mg_beam.hip -- mg_plan_beam, its segment loop, and its survivor selection, in-pool resample and output kernels
// (mg_beam.h; the rollouts, the fan-out, the reduction and the fan pool are mg_plan's, the threshold mg_plan_cem's).
#include "mg_sim.h"
#include "mg_beam.h"
#include "mg_cem.h"

// One thread per env, every read and write of a [K][n] array coalesced along e (as plan_reduce_kernel).  Two passes
// over k: the first lists the env's B survivors in ascending k (surv[i][e]) and advances every slot's episode counter,
// the second gives every slot its parent -- a loser the next entry of that list, round and round.
__global__ void __launch_bounds__(256) beam_select_kernel(const double *__restrict__ values, const double *__restrict__ thr,
                                                          const int32_t *__restrict__ k_thr,
                                                          const int32_t *__restrict__ seg_steps,
                                                          int32_t *__restrict__ episode_steps, int n_envs, int K, int B,
                                                          int32_t *__restrict__ surv, int32_t *__restrict__ parent) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_envs) return;
    const size_t n = (size_t)n_envs;
    const double t = thr[e];
    const int kt = k_thr[e];
    int ns = 0;
    for (int k = 0; k < K; k++) {
        const size_t r = (size_t)k * n + e;
        episode_steps[r] += seg_steps[r];
        const double s = values[r];
        if ((s > t || (s == t && k <= kt)) && ns < B) surv[(size_t)ns++ * n + e] = k;   // (ns < B always holds)
    }
    int next = 0, j = 0;   // surv[next][e] is the next survivor in line; surv[j][e] the next one to meet in ascending k
    for (int k = 0; k < K; k++) {
        const size_t r = (size_t)k * n + e;
        if (j < ns && surv[(size_t)j * n + e] == k) {
            parent[r] = k;
            j++;
        } else {
            parent[r] = ns ? surv[(size_t)next * n + e] : k;   // (ns = B >= 1; a parent is always a slot below K)
            next = next + 1 >= ns ? 0 : next + 1;
        }
    }
}

hipError_t mg_launch_beam_select(const double *values, const double *thr, const int32_t *k_thr, const int32_t *seg_steps,
                                 int32_t *episode_steps, int n_envs, int K, int B, int32_t *surv, int32_t *parent,
                                 hipStream_t st) {
    hipLaunchKernelGGL(beam_select_kernel, dim3((n_envs + 255) / 256), dim3(256), 0, st, values, thr, k_thr, seg_steps,
                       episode_steps, n_envs, K, B, surv, parent);
    return hipGetLastError();
}

// The resample.  The grid is plan_fan_kernel's: a workgroup takes BEAM_ROWS_PER_WG rows of its 256 envs, envs fastest
// across lanes, and walks the K slots; a lane whose slot lost (parent != k) loads its env's element from the parent's
// column and stores it to its own, so the stores of a wavefront lie in one contiguous segment of a [slot][Mpad] row and
// its loads in at most B of them.  A survivor's lane moves nothing, and no column is both source and destination
// (parents are survivors), so the copy is in place and no lane waits for another.
//
// Rows of 1- and 2-byte elements, the fan-out's way: a lane carries 4 or 2 neighbouring envs of slot k as one 4-byte
// word (such a row occupies the workgroup's first 64 or 128 lanes).  Rows start on 4-byte boundaries, so the word at
// column k * n_envs + e0 is aligned when k * n_envs elements are a whole number of words and it does not run past the
// slot's last env; the lane then reads the destination word, replaces the losers' elements -- each from its own
// parent's column -- and writes the word back: the survivors' elements in it are rewritten with the values they have,
// and no other lane writes any of its bytes.  Otherwise the lane stores the losers' elements one by one.
#define BEAM_ROWS_PER_WG 8
__global__ void __launch_bounds__(256) beam_clone_kernel(char *__restrict__ pool, const PlanRow *__restrict__ rows, int nrows,
                                                         const int32_t *__restrict__ parent, int n_envs, int K) {
    const int tid = threadIdx.x, r0 = blockIdx.y * BEAM_ROWS_PER_WG, eb = blockIdx.x * 256;
    PlanRow w[BEAM_ROWS_PER_WG];   // uniform over the workgroup
    bool small = false;
#pragma unroll
    for (int i = 0; i < BEAM_ROWS_PER_WG; i++) {
        w[i].esize = 0;
        if (r0 + i >= nrows) continue;
        w[i] = rows[r0 + i];
        small = small || w[i].esize < 4;
    }
    const int e = eb + tid;
    for (int k = 0; k < K; k++) {
        const size_t col = (size_t)k * (size_t)n_envs;
        const int p1 = e < n_envs ? parent[col + e] : k;
        // the parents of the envs the lane carries in a row of 1-byte (q4, from env eb + 4 * tid) and of 2-byte
        // elements (q2, from env eb + 2 * tid); k: nothing to move (a survivor, or no such env)
        int q4[4] = {k, k, k, k}, q2[2] = {k, k};
        if (small) {   // uniform
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (tid < 64 && eb + 4 * tid + j < n_envs) q4[j] = parent[col + eb + 4 * tid + j];
#pragma unroll
            for (int j = 0; j < 2; j++)
                if (tid < 128 && eb + 2 * tid + j < n_envs) q2[j] = parent[col + eb + 2 * tid + j];
        }
#pragma unroll
        for (int i = 0; i < BEAM_ROWS_PER_WG; i++) {
            const uint32_t es = w[i].esize;
            if (es == 0) continue;
            char *row = pool + w[i].dst;
            if (es >= 4) {
                if (p1 == k) continue;
                const size_t d = (col + (size_t)e) * es, s = ((size_t)p1 * (size_t)n_envs + (size_t)e) * es;
                if (es == 8) *(uint64_t *)(row + d) = *(const uint64_t *)(row + s);
                else *(uint32_t *)(row + d) = *(const uint32_t *)(row + s);
            } else if (es == 2) {
                const int e0 = eb + 2 * tid;
                if (q2[0] == k && q2[1] == k) continue;
                uint16_t *d = (uint16_t *)row + col + (size_t)e0;
                const uint16_t *src = (const uint16_t *)row + (size_t)e0;
                if (((col * 2) & 3) == 0 && e0 + 2 <= n_envs) {
                    uint32_t v = *(const uint32_t *)d;
#pragma unroll
                    for (int j = 0; j < 2; j++)
                        if (q2[j] != k)
                            v = (v & ~(0xffffu << (16 * j))) | ((uint32_t)src[(size_t)q2[j] * (size_t)n_envs + j] << (16 * j));
                    *(uint32_t *)d = v;
                } else {
#pragma unroll
                    for (int j = 0; j < 2; j++)
                        if (q2[j] != k) d[j] = src[(size_t)q2[j] * (size_t)n_envs + j];
                }
            } else {
                const int e0 = eb + 4 * tid;
                if (q4[0] == k && q4[1] == k && q4[2] == k && q4[3] == k) continue;
                uint8_t *d = (uint8_t *)row + col + (size_t)e0;
                const uint8_t *src = (const uint8_t *)row + (size_t)e0;
                if ((col & 3) == 0 && e0 + 4 <= n_envs) {
                    uint32_t v = *(const uint32_t *)d;
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (q4[j] != k)
                            v = (v & ~(0xffu << (8 * j))) | ((uint32_t)src[(size_t)q4[j] * (size_t)n_envs + j] << (8 * j));
                    *(uint32_t *)d = v;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (q4[j] != k) d[j] = src[(size_t)q4[j] * (size_t)n_envs + j];
                }
            }
        }
    }
}

hipError_t mg_launch_beam_clone(char *pool, const PlanRow *rows_dev, int nrows, const int32_t *parent, int n_envs, int K,
                                hipStream_t st) {
    hipLaunchKernelGGL(beam_clone_kernel, dim3((n_envs + 255) / 256, (nrows + BEAM_ROWS_PER_WG - 1) / BEAM_ROWS_PER_WG),
                       dim3(256), 0, st, pool, rows_dev, nrows, parent, n_envs, K);
    return hipGetLastError();
}

// one thread per byte of plans[0 .. hend), envs fastest; as the clone, a survivor's byte is never written
__global__ void __launch_bounds__(256) beam_history_kernel(uint8_t *__restrict__ plans, const int32_t *__restrict__ parent,
                                                           int hend, int n_envs, int K) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t kn = (uint64_t)K * (uint64_t)n_envs;
    if (i >= (uint64_t)hend * kn) return;
    const uint64_t r = i % kn, e = r % (uint64_t)n_envs, k = r / (uint64_t)n_envs;
    const int p = parent[r];
    if (p != (int)k) plans[i] = plans[i - r + (uint64_t)p * (uint64_t)n_envs + e];
}

hipError_t mg_launch_beam_history(uint8_t *plans, const int32_t *parent, int hend, int n_envs, int K, hipStream_t st) {
    const uint64_t total = (uint64_t)hend * K * n_envs;   // <= 4096 * MG_PLAN_MAX_ROLLOUTS = 2^30
    hipLaunchKernelGGL(beam_history_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, plans, parent, hend,
                       n_envs, K);
    return hipGetLastError();
}

__global__ void __launch_bounds__(256) beam_steps_kernel(const int32_t *__restrict__ pool_episode_steps,
                                                         const int32_t *__restrict__ seg_steps,
                                                         const int32_t *__restrict__ env_episode_steps, int n_envs, int K,
                                                         int32_t *__restrict__ steps) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= K * n_envs) return;
    steps[r] = pool_episode_steps[r] + seg_steps[r] - env_episode_steps[r % n_envs];
}

hipError_t mg_launch_beam_steps(const int32_t *pool_episode_steps, const int32_t *seg_steps, const int32_t *env_episode_steps,
                                int n_envs, int K, int32_t *steps, hipStream_t st) {
    hipLaunchKernelGGL(beam_steps_kernel, dim3((K * n_envs + 255) / 256), dim3(256), 0, st, pool_episode_steps, seg_steps,
                       env_episode_steps, n_envs, K, steps);
    return hipGetLastError();
}

// one thread per (h, e), envs fastest
__global__ void __launch_bounds__(256) beam_gather_kernel(const uint8_t *__restrict__ plans, const int32_t *__restrict__ best,
                                                          int H, int n_envs, int K, uint8_t *__restrict__ best_plan) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= H * n_envs) return;
    const int e = i % n_envs, h = i / n_envs;
    best_plan[i] = plans[((size_t)h * K + (size_t)best[e]) * (size_t)n_envs + e];
}

hipError_t mg_launch_beam_gather(const uint8_t *plans, const int32_t *best, int H, int n_envs, int K, uint8_t *best_plan,
                                 hipStream_t st) {
    hipLaunchKernelGGL(beam_gather_kernel, dim3((H * n_envs + 255) / 256), dim3(256), 0, st, plans, best, H, n_envs, K,
                       best_plan);   // H * n_envs <= 4096 * 262144 / K: within int for every K >= 1
    return hipGetLastError();
}

extern "C" int mg_plan_beam(mg_sim *s, const uint8_t *actions, uint8_t *plans, int32_t H, int32_t K, int32_t seg,
                            int32_t survivors, const mg_objective *obj, const mg_plan_beam_out *out, void *stream) {
    const std::string f("mg_plan_beam");
    if (!s || !actions || !plans || !out || !out->best)
        return set_err(-22, f + ": null sim, actions_dev, plans_dev, out or out->best");
    if (H < 1 || H > 4096) return set_err(-22, f + ": H must be in [1, 4096]");
    if (int rc = plan_check_sizes(s, "mg_plan_beam", H, K)) return rc;
    if (seg < 1 || seg > H) return set_err(-22, f + ": seg must be in [1, H]");
    if (survivors < 1 || survivors > K) return set_err(-22, f + ": survivors must be in [1, K]");
    if (obj)
        if (int rc = objective_check(obj, "mg_plan_beam")) return rc;
    HIPC(hipSetDevice(s->device));
    const int n = s->main.S.n_envs, M = K * n, D = (H + seg - 1) / seg;
    RolloutPool &R = s->fan;
    if (int rc = rollout_reserve(s, R, M, "mg_plan_beam")) return rc;
    hipStream_t st = as_stream(stream);
    MGState F = R.P.S;
    F.n_envs = M;
    const bool traced = obj && obj->kind != MG_OBJ_FINAL;
    LookCarry carry = {R.beam_G, R.beam_P, R.beam_g, R.beam_kp, R.beam_k, R.beam_ended, 0};
    const int nrows = traced ? R.beam_nrows : R.beam_nrows - 6;   // FINAL keeps no carry
    const size_t kn = (size_t)K * n;
    if (plans != actions) HIPC(hipMemcpyAsync(plans, actions, (size_t)H * kn, hipMemcpyDeviceToDevice, st));
    HIPC(mg_launch_plan_fan((const char *)s->main.mem, (char *)R.P.mem, R.rows, R.nrows, n, K, st));
    double *values = nullptr;
    for (int d = 0; d < D; d++) {
        const bool last = d == D - 1;
        const int h0 = d * seg, h1 = last ? H : h0 + seg;
        values = out->depth_values ? out->depth_values + (size_t)d * kn : last && out->values ? out->values : R.scores;
        carry.load = d > 0;
        if (int rc = plan_rollouts(s, F, actions + (size_t)h0 * kn, h1 - h0, obj, values, R.beam_steps, out->errors, st,
                                   traced ? &carry : nullptr))
            return rc;
        if (last) break;
        int32_t *parent = out->parents ? out->parents + (size_t)d * kn : R.beam_parent;
        HIPC(mg_launch_cem_threshold(values, n, K, survivors, R.cem_thr, R.cem_kthr, st));
        HIPC(mg_launch_beam_select(values, R.cem_thr, R.cem_kthr, R.beam_steps, F.episode_steps, n, K, survivors, R.beam_surv,
                                   parent, st));
        HIPC(mg_launch_beam_clone((char *)R.P.mem, R.beam_rows, nrows, parent, n, K, st));
        HIPC(mg_launch_beam_history(plans, parent, h1, n, K, st));
    }
    if (out->steps)
        HIPC(mg_launch_beam_steps(F.episode_steps, R.beam_steps, s->main.S.episode_steps, n, K, out->steps, st));
    if (out->depth_values && out->values)
        HIPC(hipMemcpyAsync(out->values, values, kn * sizeof(double), hipMemcpyDeviceToDevice, st));
    HIPC(mg_launch_plan_reduce(values, plans, H, n, K, out->best, out->best_value, out->first_action, st));
    if (out->best_plan) HIPC(mg_launch_beam_gather(plans, out->best, H, n, K, out->best_plan, st));
    return 0;
}
