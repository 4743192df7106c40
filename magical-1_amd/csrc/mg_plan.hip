// mg_plan.hip -- mg_plan / mg_plan_sample, the rollout pools' allocation, and mg_plan's fan-out copy, best-of-K
// reduction and candidate sampler (mg_plan.h; the rollouts are the lookahead kernel on the fan pool).
#include <cassert>

#include "mg_sim.h"
#include "mg_philox.h"

// Fan-out: a workgroup takes PLAN_ROWS_PER_WG rows of its 256 envs, reads each source element once into registers
// and stores it K times, envs fastest across lanes -- source traffic does not grow with K, and every store of a
// wavefront is one contiguous segment of a [slot][Mpad] row.  Rows of 1- and 2-byte elements move as 4-byte words
// (a lane carries 4 or 2 neighbouring envs, so such a row occupies the workgroup's first 64 or 128 lanes): the source
// word is always aligned (rows start on 4-byte boundaries and are padded to 64 envs), the destination word of candidate
// k is when k * n_envs elements are a whole number of words -- every k when n_envs is a multiple of 4 -- and otherwise,
// or where the word would run past the candidate's last env, the lane stores its elements one by one.
//
// ONE (K = 1, mg_lookahead's copy): nothing is stored twice, so a lane moves its own env's element of each row and
// nothing is packed -- the fan path with one candidate measured 0.035 ms (MoveToRegion, 4096 envs) and 0.06 ms
// (ClusterColour, 8192 envs) slower per lookahead than this plain copy.
#define PLAN_ROWS_PER_WG 8
template <bool ONE>
__global__ void __launch_bounds__(256) plan_fan_kernel(const char *__restrict__ src, char *__restrict__ dst,
                                                       const PlanRow *__restrict__ rows, int nrows, int n_envs, int K) {
    const int tid = threadIdx.x, r0 = blockIdx.y * PLAN_ROWS_PER_WG;
    if (ONE) {
        const int e = blockIdx.x * 256 + tid;
        if (e >= n_envs) return;
        for (int r = r0; r < r0 + PLAN_ROWS_PER_WG && r < nrows; r++) {
            const PlanRow w = rows[r];   // uniform over the workgroup
            copy_elem(dst + w.dst + (size_t)e * w.esize, src + w.src + (size_t)e * w.esize, w.esize);
        }
        return;
    }
    PlanRow w[PLAN_ROWS_PER_WG];   // uniform over the workgroup
    uint64_t v[PLAN_ROWS_PER_WG];
    int e0[PLAN_ROWS_PER_WG];      // the lane's first env of the row; -1: none
#pragma unroll
    for (int i = 0; i < PLAN_ROWS_PER_WG; i++) {
        e0[i] = -1;
        v[i] = 0;
        if (r0 + i >= nrows) continue;
        w[i] = rows[r0 + i];
        const int pack = w[i].esize >= 4 ? 1 : 4 / (int)w[i].esize;
        const int e = blockIdx.x * 256 + tid * pack;
        if (tid * pack >= 256 || e >= n_envs) continue;
        e0[i] = e;
        const char *p = src + w[i].src + (size_t)e * w[i].esize;
        v[i] = w[i].esize == 8 ? *(const uint64_t *)p : (uint64_t)(*(const uint32_t *)p);
    }
    for (int k = 0; k < K; k++) {
        const size_t col = (size_t)k * (size_t)n_envs;
#pragma unroll
        for (int i = 0; i < PLAN_ROWS_PER_WG; i++) {
            if (e0[i] < 0) continue;
            const uint32_t es = w[i].esize;
            char *p = dst + w[i].dst + (col + (size_t)e0[i]) * es;
            if (es == 8) {
                *(uint64_t *)p = v[i];
            } else if (es == 4) {
                *(uint32_t *)p = (uint32_t)v[i];
            } else {
                const int pack = 4 / (int)es;
                if (((col * es) & 3) == 0 && e0[i] + pack <= n_envs) {
                    *(uint32_t *)p = (uint32_t)v[i];
                } else {
                    for (int j = 0; j < pack && e0[i] + j < n_envs; j++) {
                        if (es == 2) *(uint16_t *)(p + 2 * j) = (uint16_t)(v[i] >> (16 * j));
                        else p[j] = (char)(uint8_t)(v[i] >> (8 * j));
                    }
                }
            }
        }
    }
}

hipError_t mg_launch_plan_fan(const char *src_pool, char *dst_pool, const PlanRow *rows_dev, int nrows, int n_envs, int K,
                              hipStream_t st) {
    hipLaunchKernelGGL(K == 1 ? plan_fan_kernel<true> : plan_fan_kernel<false>,
                       dim3((n_envs + 255) / 256, (nrows + PLAN_ROWS_PER_WG - 1) / PLAN_ROWS_PER_WG), dim3(256), 0, st,
                       src_pool, dst_pool, rows_dev, nrows, n_envs, K);
    return hipGetLastError();
}

// one thread per env over its K candidates' scores, each read coalesced along e; strict >: the lowest k wins a tie
// (scores are never NaN)
__global__ void __launch_bounds__(256) plan_reduce_kernel(const double *__restrict__ scores,
                                                          const uint8_t *__restrict__ actions, int H, int n_envs, int K,
                                                          int32_t *__restrict__ best, double *__restrict__ best_score,
                                                          uint8_t *__restrict__ first_action) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_envs) return;
    double bs = scores[e];
    int b = 0;
    for (int k = 1; k < K; k++) {
        const double s = scores[(size_t)k * n_envs + e];
        if (s > bs) { bs = s; b = k; }
    }
    best[e] = b;
    if (best_score) best_score[e] = bs;
    if (first_action && actions && H > 0) first_action[e] = actions[(size_t)b * n_envs + e];   // step 0 of candidate b
}

hipError_t mg_launch_plan_reduce(const double *scores, const uint8_t *actions, int H, int n_envs, int K, int32_t *best,
                                 double *best_score, uint8_t *first_action, hipStream_t st) {
    hipLaunchKernelGGL(plan_reduce_kernel, dim3((n_envs + 255) / 256), dim3(256), 0, st, scores, actions, H, n_envs, K,
                       best, best_score, first_action);
    return hipGetLastError();
}

// one thread per action byte of u8[H][K][n_envs], envs fastest
__global__ void __launch_bounds__(256) plan_sample_kernel(uint8_t *__restrict__ out, int n_envs, int H, int K, int repeat,
                                                          uint64_t key, uint64_t step) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint64_t)H * K * n_envs) return;
    const int e = (int)(i % (uint64_t)n_envs);
    const uint64_t hk = i / (uint64_t)n_envs;
    const uint64_t h = hk / (uint64_t)K, k = hk % (uint64_t)K;
    const uint64_t J = ((uint64_t)H + repeat - 1) / repeat;
    out[i] = philox_action(key, step + k * J + h / (uint64_t)repeat, e);
}

hipError_t mg_launch_plan_sample(uint8_t *out, int n_envs, int H, int K, int repeat, uint64_t key, uint64_t step,
                                 hipStream_t st) {
    const uint64_t total = (uint64_t)H * K * n_envs;   // <= 4096 * MG_PLAN_MAX_ROLLOUTS = 2^30
    hipLaunchKernelGGL(plan_sample_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, out, n_envs, H, K,
                       repeat, key, step);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// C ABI
int plan_check_sizes(const mg_sim *s, const char *fn, int32_t H, int32_t K) {
    if (H < 0 || H > 4096) return set_err(-22, std::string(fn) + ": H must be in [0, 4096]");
    if (K < 1 || K > 4096) return set_err(-22, std::string(fn) + ": K must be in [1, 4096]");
    if ((int64_t)K * s->main.S.n_envs > MG_PLAN_MAX_ROLLOUTS)
        return set_err(-22, std::string(fn) + ": K * num_envs = " + std::to_string((int64_t)K * s->main.S.n_envs) +
                                " rollouts, more than MG_PLAN_MAX_ROLLOUTS = " + std::to_string(MG_PLAN_MAX_ROLLOUTS));
    return 0;
}

// (Re)allocate R for M rollouts unless it holds as many.  The device is synchronised first: an earlier call's kernels
// may still be running on the pool that is freed here.  On failure the sim is without this pool and stays usable (the
// next call allocates again)
int rollout_reserve(mg_sim *s, RolloutPool &R, int M, const char *fn) {
    if (M <= R.cap) return 0;
    HIPC(hipDeviceSynchronize());
    pool_free(R.P);
    R = RolloutPool();
    const std::vector<StateRow> src = pool_rollout_rows(s->main);
    RolloutPool T;
    hipError_t err = pool_create(T.P, s->main.S, (M + 63) / 64 * 64, false, [&](Carver &c) {
        T.scores = c.take<double>((size_t)T.P.S.N);
        T.rows = c.take<PlanRow>(src.size());
        T.cem_thr = c.take<double>((size_t)s->main.S.n_envs);
        T.cem_kthr = c.take<int32_t>((size_t)s->main.S.n_envs);
        const size_t N = (size_t)T.P.S.N;
        T.beam_G = c.take<double>(N); T.beam_P = c.take<double>(N); T.beam_g = c.take<double>(N);
        T.beam_kp = c.take<int32_t>(N); T.beam_k = c.take<int32_t>(N); T.beam_ended = c.take<int32_t>(N);
        T.beam_steps = c.take<int32_t>(N); T.beam_surv = c.take<int32_t>(N); T.beam_parent = c.take<int32_t>(N);
        T.beam_rows = c.take<PlanRow>(src.size() + 6);
    });
    if (err != hipSuccess)
        return set_err(-12, std::string(fn) + ": rollout pool for " + std::to_string(M) + " rollouts: " + hipGetErrorString(err));
    // layout() lists every pool's rows in the same order: row i of both lists is the same field
    const std::vector<StateRow> dst = pool_rollout_rows(T.P);
    assert(dst.size() == src.size());
    std::vector<PlanRow> pr;
    for (size_t i = 0; i < src.size(); i++) pr.push_back(PlanRow{src[i].off, dst[i].off, src[i].esize, 0u});
    err = hipMemcpy(T.rows, pr.data(), pr.size() * sizeof(PlanRow), hipMemcpyHostToDevice);
    if (err == hipSuccess) {   // a resample's rows (mg_plan_beam): the same rows within this pool, then the carry's
        std::vector<PlanRow> br;
        for (const StateRow &r : dst) br.push_back(PlanRow{r.off, r.off, r.esize, 0u});
        const auto own = [&](const void *p, uint32_t esize) {
            const uint64_t off = (uint64_t)((const char *)p - (const char *)T.P.mem);
            br.push_back(PlanRow{off, off, esize, 0u});
        };
        own(T.beam_G, 8u); own(T.beam_P, 8u); own(T.beam_g, 8u);
        own(T.beam_kp, 4u); own(T.beam_k, 4u); own(T.beam_ended, 4u);
        err = hipMemcpy(T.beam_rows, br.data(), br.size() * sizeof(PlanRow), hipMemcpyHostToDevice);
        T.beam_nrows = (int)br.size();
    }
    if (err != hipSuccess) {
        pool_free(T.P);
        return set_err(-12, std::string(fn) + ": rollout pool setup: " + hipGetErrorString(err));
    }
    T.nrows = (int)pr.size();
    T.cap = M;
    R = T;
    return 0;
}

int plan_rollouts(mg_sim *s, const MGState &F, const uint8_t *actions, int H, const mg_objective *obj, double *scores,
                  int32_t *steps, int32_t *errors, hipStream_t st, const LookCarry *carry) {
    if (!obj || obj->kind == MG_OBJ_FINAL) {
        const LookOut lo = {scores, steps, nullptr, nullptr, errors};
        HIPC(mg_launch_lookahead(F, s->dlib, s->task, s->step_form, s->step_blk, s->max_steps, actions, H, lo, nullptr, st));
        return 0;
    }
    // the traced kernel with `value` pointed at the [K][N] scores and no s_n output
    const LookOut lo = {nullptr, steps, nullptr, nullptr, errors};
    LookObj a = objective_args(s, obj);
    a.value = scores;
    if (carry) a.carry = *carry;
    HIPC(mg_launch_lookahead(F, s->dlib, s->task, s->step_form, s->step_blk, s->max_steps, actions, H, lo, &a, st));
    return 0;
}

// obj null: mg_plan
static int plan_run(mg_sim *s, const char *fn, const uint8_t *actions, int32_t H, int32_t K, const mg_objective *obj,
                    const mg_plan_out *out, void *stream) {
    const std::string f(fn);
    if (!s || !out || !out->best) return set_err(-22, f + ": null sim, out or out->best");
    if (int rc = plan_check_sizes(s, fn, H, K)) return rc;
    if (!actions && H > 0) return set_err(-22, f + ": null actions with H > 0");
    HIPC(hipSetDevice(s->device));
    const int n = s->main.S.n_envs, M = K * n;
    RolloutPool &R = s->fan;
    if (int rc = rollout_reserve(s, R, M, fn)) return rc;
    hipStream_t st = as_stream(stream);
    // the pool may be larger than this call needs: its rows keep the stride it was laid out with, the launch covers M
    MGState F = R.P.S;
    F.n_envs = M;
    HIPC(mg_launch_plan_fan((const char *)s->main.mem, (char *)R.P.mem, R.rows, R.nrows, n, K, st));
    double *scores = out->scores ? out->scores : R.scores;
    if (int rc = plan_rollouts(s, F, actions, H, obj, scores, out->steps, out->errors, st)) return rc;
    HIPC(mg_launch_plan_reduce(scores, actions, H, n, K, out->best, out->best_score, out->first_action, st));
    return 0;
}

extern "C" {

int mg_plan(mg_sim *s, const uint8_t *actions, int32_t H, int32_t K, const mg_plan_out *out, void *stream) {
    return plan_run(s, "mg_plan", actions, H, K, nullptr, out, stream);
}

int mg_plan_obj(mg_sim *s, const uint8_t *actions, int32_t H, int32_t K, const mg_objective *obj, const mg_plan_out *out,
                void *stream) {
    if (int rc = objective_check(obj, "mg_plan_obj")) return rc;
    return plan_run(s, "mg_plan_obj", actions, H, K, obj, out, stream);
}

int mg_plan_sample(mg_sim *s, uint8_t *actions, int32_t H, int32_t K, int32_t repeat, uint64_t key, uint64_t step,
                   void *stream) {
    if (!s || !actions) return set_err(-22, "mg_plan_sample: null argument");
    if (repeat < 1) return set_err(-22, "mg_plan_sample: repeat must be at least 1");
    if (int rc = plan_check_sizes(s, "mg_plan_sample", H, K)) return rc;
    if (H == 0) return 0;
    HIPC(hipSetDevice(s->device));
    HIPC(mg_launch_plan_sample(actions, s->main.S.n_envs, H, K, repeat, key, step, as_stream(stream)));
    return 0;
}

} // extern "C"
