// mg_cem.hip -- mg_plan_cem, its iteration loop, and its elite threshold and per-slot update kernels (mg_cem.h; the
// rollouts, the fan-out, the reduction and the fan pool are mg_plan's).
#include "mg_sim.h"
#include "mg_cem.h"
#include "mg_philox.h"

// a score as an unsigned key with the same order; -0.0 is made +0.0 first, so equal scores have equal keys
__device__ __forceinline__ uint64_t cem_key(double s) {
    const uint64_t u = (uint64_t)__double_as_longlong(s + 0.0);
    return u ^ ((u >> 63) ? ~0ull : (1ull << 63));
}

__device__ __forceinline__ double cem_unkey(uint64_t k) {
    return __longlong_as_double((long long)((k >> 63) ? k ^ (1ull << 63) : ~k));
}

// One thread per env, every read of scores[k * n + e] coalesced along e.  The E-th largest key is found bit by bit
// from the top (a radix select: of the keys that share the prefix chosen so far, either at least `need` have the
// next bit set, or those that have it rank above and are counted off), over the bits in which the env's keys differ
// at all: a first pass takes the AND and OR of the keys, and the bits they agree in are the prefix's already.  Graded
// scores in [0, 1] differ in the mantissa and a few exponent bits, binary ones in ten bits.  What is left of `need`
// is the rank of the threshold candidate among the candidates with the threshold's score, in ascending k.
__global__ void __launch_bounds__(256) cem_threshold_kernel(const double *__restrict__ scores, int n_envs, int K, int E,
                                                            double *__restrict__ thr, int32_t *__restrict__ k_thr) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_envs) return;
    const double *col = scores + e;
    uint64_t all = ~0ull, any = 0;
    for (int k = 0; k < K; k++) {
        const uint64_t key = cem_key(col[(size_t)k * n_envs]);
        all &= key;
        any |= key;
    }
    uint64_t prefix = all, diff = all ^ any;
    int need = E;
    while (diff) {
        const int b = 63 - __clzll((long long)diff);
        diff &= ~(1ull << b);
        const uint64_t want = (prefix | (1ull << b)) >> b;
        int c = 0;
        for (int k = 0; k < K; k++) c += (cem_key(col[(size_t)k * n_envs]) >> b) == want;
        if (need <= c) prefix |= 1ull << b;
        else need -= c;
    }
    int kt = 0;
    for (int k = 0, seen = 0; k < K; k++) {
        if (cem_key(col[(size_t)k * n_envs]) != prefix) continue;
        if (++seen == need) { kt = k; break; }
    }
    thr[e] = cem_unkey(prefix);
    k_thr[e] = kt;
}

hipError_t mg_launch_cem_threshold(const double *scores, int n_envs, int K, int E, double *thr, int32_t *k_thr,
                                   hipStream_t st) {
    hipLaunchKernelGGL(cem_threshold_kernel, dim3((n_envs + 255) / 256), dim3(256), 0, st, scores, n_envs, K, E, thr, k_thr);
    return hipGetLastError();
}

// The thread of (slot j, env e) owns column (rows of slot j, every k, e) of the candidates and w[j][:][e]: it reads
// the column's first row before it writes the column, so no thread waits for another, and for a fixed (row, k) or
// (j, a) the lanes' bytes are one contiguous segment.  The 18 weights -- counts of at most K <= 4096 elites plus alpha
// <= 1024 -- live in registers, two 16-bit halves per word, indexed only by unrolled loops.
#define CEM_WORDS (MG_CEM_ACTIONS / 2)
__global__ void __launch_bounds__(256) cem_update_kernel(CemUpdate u) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n = (size_t)u.n_envs;
    if (idx >= (uint64_t)u.J * n) return;
    const int e = (int)(idx % n), j = (int)(idx / n);
    const int h0 = j * u.repeat, h1 = min(u.H, h0 + u.repeat);
    const int K = u.K;
    uint32_t w[CEM_WORDS];
    uint8_t inc = 0;
    uint16_t *wcol = u.weights + (size_t)j * MG_CEM_ACTIONS * n + e;
    if (u.refit) {
#pragma unroll
        for (int q = 0; q < CEM_WORDS; q++) w[q] = (uint32_t)u.alpha * 0x00010001u;
        const double t = u.thr[e];
        const int kt = u.k_thr[e];
        const uint8_t *row = u.actions + (size_t)h0 * K * n + e;
        for (int k = 0; k < K; k++) {
            const double s = u.scores[(size_t)k * n + e];
            const uint32_t a = row[(size_t)k * n];
            if (!(s > t || (s == t && k <= kt))) continue;
            const uint32_t one = 1u << (16 * (a & 1u));
#pragma unroll
            for (int q = 0; q < CEM_WORDS; q++) w[q] += (a >> 1) == (uint32_t)q ? one : 0u;
        }
        inc = row[(size_t)u.best[e] * n];
#pragma unroll
        for (int q = 0; q < CEM_WORDS; q++) {
            wcol[(size_t)(2 * q) * n] = (uint16_t)w[q];
            wcol[(size_t)(2 * q + 1) * n] = (uint16_t)(w[q] >> 16);
        }
    } else if (u.uniform) {
#pragma unroll
        for (int q = 0; q < CEM_WORDS; q++) w[q] = 0x00010001u;
    } else {
#pragma unroll
        for (int q = 0; q < CEM_WORDS; q++)
            w[q] = (uint32_t)wcol[(size_t)(2 * q) * n] | ((uint32_t)wcol[(size_t)(2 * q + 1) * n] << 16);
    }
    if (!u.draw) return;
    uint32_t T = 0;
#pragma unroll
    for (int q = 0; q < CEM_WORDS; q++) T += (w[q] & 0xffffu) + (w[q] >> 16);
    if (T == 0) {   // (caller-supplied warm weights only) draws as if every weight were 1
        T = MG_CEM_ACTIONS;
#pragma unroll
        for (int q = 0; q < CEM_WORDS; q++) w[q] = 0x00010001u;
    }
    for (int k = 0; k < K; k++) {
        const uint32_t r = philox_word(u.key, u.counter + (uint64_t)k * u.J + j, e) % T;
        // the smallest a whose cumulative weight exceeds r = the number of cumulative weights that do not (r < T)
        uint32_t cum = 0, a = 0;
#pragma unroll
        for (int q = 0; q < CEM_WORDS; q++) {
            cum += w[q] & 0xffffu;
            a += cum <= r;
            cum += w[q] >> 16;
            a += cum <= r;
        }
        if (u.incumbent && k == 0) a = inc;
        for (int h = h0; h < h1; h++) u.actions[((size_t)h * K + k) * n + e] = (uint8_t)a;
    }
}

hipError_t mg_launch_cem_update(const CemUpdate &u, hipStream_t st) {
    const uint64_t total = (uint64_t)u.J * u.n_envs;   // <= 4096 * num_envs <= 2^30
    hipLaunchKernelGGL(cem_update_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, u);
    return hipGetLastError();
}

// obj null: mg_plan_cem
static int cem_run(mg_sim *s, const char *fn, uint8_t *actions, uint16_t *weights, int32_t warm, int32_t H, int32_t K,
                   int32_t iters, int32_t elites, int32_t alpha, int32_t repeat, uint64_t key, uint64_t step,
                   const mg_objective *obj, const mg_plan_cem_out *out, void *stream) {
    const std::string f(fn);
    if (!s || !actions || !weights || !out || !out->best)
        return set_err(-22, f + ": null sim, actions_dev, weights_dev, out or out->best");
    if (H < 1 || H > 4096) return set_err(-22, f + ": H must be in [1, 4096]");
    if (int rc = plan_check_sizes(s, fn, H, K)) return rc;
    if (iters < 1 || iters > 64) return set_err(-22, f + ": iters must be in [1, 64]");
    if (elites < 1 || elites > K) return set_err(-22, f + ": elites must be in [1, K]");
    if (alpha < 0 || alpha > 1024) return set_err(-22, f + ": alpha must be in [0, 1024]");
    if (repeat < 1) return set_err(-22, f + ": repeat must be at least 1");
    if (warm != 0 && warm != 1) return set_err(-22, f + ": warm must be 0 or 1");
    HIPC(hipSetDevice(s->device));
    const int n = s->main.S.n_envs, M = K * n, J = (H + repeat - 1) / repeat;
    RolloutPool &R = s->fan;
    if (int rc = rollout_reserve(s, R, M, fn)) return rc;
    hipStream_t st = as_stream(stream);
    MGState F = R.P.S;
    F.n_envs = M;
    double *scores = out->scores ? out->scores : R.scores;
    CemUpdate u = {actions, weights, scores, R.cem_thr, R.cem_kthr, out->best, n, H, K, J, repeat, alpha,
                   /*refit*/ 0, /*uniform*/ warm ? 0 : 1, /*draw*/ 1, /*incumbent*/ 0, key, step};
    HIPC(mg_launch_cem_update(u, st));   // iteration 0's candidates
    u.refit = 1; u.uniform = 0; u.incumbent = 1;
    for (int i = 0; i < iters; i++) {
        const bool last = i == iters - 1;
        HIPC(mg_launch_plan_fan((const char *)s->main.mem, (char *)R.P.mem, R.rows, R.nrows, n, K, st));
        if (int rc = plan_rollouts(s, F, actions, H, obj, scores, out->steps, out->errors, st)) return rc;
        double *bs = out->iter_best ? out->iter_best + (size_t)i * n : last ? out->best_score : nullptr;
        HIPC(mg_launch_plan_reduce(scores, actions, H, n, K, out->best, bs, out->first_action, st));
        if (last && out->iter_best && out->best_score)
            HIPC(hipMemcpyAsync(out->best_score, bs, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIPC(mg_launch_cem_threshold(scores, n, K, elites, R.cem_thr, R.cem_kthr, st));
        // refit to this iteration's elites; unless it is the last, draw the next one's candidates over them
        u.draw = last ? 0 : 1;
        u.counter = step + (uint64_t)(i + 1) * (uint64_t)K * (uint64_t)J;
        HIPC(mg_launch_cem_update(u, st));
    }
    return 0;
}

extern "C" int mg_plan_cem(mg_sim *s, uint8_t *actions, uint16_t *weights, int32_t warm, int32_t H, int32_t K,
                           int32_t iters, int32_t elites, int32_t alpha, int32_t repeat, uint64_t key, uint64_t step,
                           const mg_plan_cem_out *out, void *stream) {
    return cem_run(s, "mg_plan_cem", actions, weights, warm, H, K, iters, elites, alpha, repeat, key, step, nullptr, out,
                   stream);
}

extern "C" int mg_plan_cem_obj(mg_sim *s, uint8_t *actions, uint16_t *weights, int32_t warm, int32_t H, int32_t K,
                               int32_t iters, int32_t elites, int32_t alpha, int32_t repeat, uint64_t key, uint64_t step,
                               const mg_objective *obj, const mg_plan_cem_out *out, void *stream) {
    if (int rc = objective_check(obj, "mg_plan_cem_obj")) return rc;
    return cem_run(s, "mg_plan_cem_obj", actions, weights, warm, H, K, iters, elites, alpha, repeat, key, step, obj, out,
                   stream);
}
