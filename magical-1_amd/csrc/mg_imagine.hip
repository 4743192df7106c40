// mg_imagine.hip -- mg_imagine: the LoRes frames of a lookahead rollout.  The segment loop (a lookahead launch and a
// frame-less render per segment on mg_lookahead's scratch pool), and the two kernels of its own (mg_imagine.h).
#include "mg_sim.h"
#include "mg_imagine.h"

__global__ void __launch_bounds__(256) imagine_advance_kernel(int32_t *__restrict__ pool_steps,
                                                              const int32_t *__restrict__ seg_steps,
                                                              const int32_t *__restrict__ env_steps,
                                                              const int32_t *__restrict__ pool_errors, int n_envs,
                                                              int32_t *__restrict__ steps, int32_t *__restrict__ errors) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n_envs) return;
    const int k = pool_steps[e] + seg_steps[e];
    pool_steps[e] = k;
    if (steps) steps[e] = k - env_steps[e];
    if (errors) errors[e] = pool_errors[e];
}

hipError_t mg_launch_imagine_advance(int32_t *pool_steps, const int32_t *seg_steps, const int32_t *env_steps,
                                     const int32_t *pool_errors, int n_envs, int32_t *steps, int32_t *errors, hipStream_t st) {
    hipLaunchKernelGGL(imagine_advance_kernel, dim3((n_envs + 255) / 256), dim3(256), 0, st, pool_steps, seg_steps,
                       env_steps, pool_errors, n_envs, steps, errors);
    return hipGetLastError();
}

// The stack pass: a streaming kernel without LDS, compose3ea_kernel's shape (mg_raster.hip).  One thread per 4 pixels of
// one (f, env): 3 dwords of each of the four source frames in (a wavefront reads 768 contiguous bytes of each), the
// bytes interleaved in registers, 3 x 16 B out (a wavefront writes 3072 contiguous bytes).  blockIdx.y = f
__global__ void __launch_bounds__(256) imagine_stack_kernel(const uint8_t *__restrict__ frames, const uint8_t *__restrict__ lead,
                                                            const uint8_t *__restrict__ ring, const int32_t *__restrict__ head,
                                                            int n_envs, int Npad, uint8_t *__restrict__ stacks) {
    constexpr int Q = MG_LORES * MG_LORES / 4;   // pixel quads per frame
    const size_t FR = (size_t)MG_LORES * MG_LORES * 3;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int e = (int)(gid / Q), q = (int)(gid % Q), f = blockIdx.y;
    if (e >= n_envs) return;
    const int nh = head[e];
    const uint32_t *src[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int j = f - 3 + k;
        const uint8_t *p = (k == 0 && lead) ? lead + ((size_t)f * n_envs + e) * FR
                         : j >= 0           ? frames + ((size_t)j * n_envs + e) * FR
                                            : ring + ((size_t)((nh + j + 1) & 3) * Npad + e) * FR;
        src[k] = (const uint32_t *)p;
    }
    uint32_t g[4][3];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int w = 0; w < 3; w++) g[k][w] = src[k][3 * q + w];
    uint32_t o[12];
#pragma unroll
    for (int b = 0; b < 48; b++) {   // output byte b: pixel b / 12, source (b % 12) / 3, channel b % 3
        const int px = b / 12, k = (b % 12) / 3, sb = 3 * px + b % 3;
        const uint32_t byte = (g[k][sb / 4] >> (8 * (sb % 4))) & 255u;
        if (b % 4 == 0) o[b / 4] = byte; else o[b / 4] |= byte << (8 * (b % 4));
    }
    uint4 *dst = (uint4 *)(stacks + ((size_t)f * n_envs + e) * FR * 4) + 3 * q;
    dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
    dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
    dst[2] = make_uint4(o[8], o[9], o[10], o[11]);
}

hipError_t mg_launch_imagine_stack(const uint8_t *frames, const uint8_t *lead, const uint8_t *ring, const int32_t *head,
                                   int F, int n_envs, int Npad, uint8_t *stacks, hipStream_t st) {
    const int64_t n = (int64_t)n_envs * (MG_LORES * MG_LORES / 4);
    hipLaunchKernelGGL(imagine_stack_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)F), dim3(256), 0, st, frames, lead,
                       ring, head, n_envs, Npad, stacks);   // F <= 4096: within a grid's y extent
    return hipGetLastError();
}

extern "C" int mg_imagine(mg_sim *s, const uint8_t *actions, int32_t H, int32_t every, const mg_lookahead_out *out,
                          const mg_imagine_out *fr, void *stream) {
    const std::string f("mg_imagine");
    if (!s || !actions || !fr) return set_err(-22, f + ": null sim, actions_dev or frames");
    if (!fr->allo && !fr->ego && !fr->stack_allo && !fr->stack_ego) return set_err(-22, f + ": no frame output requested");
    if (H < 1 || H > 4096) return set_err(-22, f + ": H must be in [1, 4096]");
    if (every < 1 || every > H) return set_err(-22, f + ": every must be in [1, H]");
    const int pp = s->preproc;
    if (pp == MG_PREPROC_NONE) return set_err(-22, f + ": the unwrapped surface has no LoRes frame");
    const bool sa = fr->stack_allo != nullptr, se = fr->stack_ego != nullptr;
    if ((sa && pp != MG_PREPROC_LORESSTACK && pp != MG_PREPROC_LORES4A) || (se && pp == MG_PREPROC_LORES4A))
        return set_err(-22, f + ": this preprocessor keeps no stack of that view (LoResStack: allo and ego; LoRes4E and "
                                "LoRes3EA: ego; LoRes4A: allo)");
    if ((sa && !fr->allo) || (se && !fr->ego) || (se && pp == MG_PREPROC_LORES3EA && !fr->allo))
        return set_err(-22, f + ": a stack needs the plain frame buffer(s) it is built from (LoRes3EA: allo and ego)");
    if ((sa || se) && (s->wring[0] || s->wring[1] || (s->bound && s->out.frames_only)))
        return set_err(-22, f + ": stacks need the sim's own frame history, which a handle with window rings or "
                                "frames_only outputs does not keep");
    if (((uintptr_t)fr->allo | (uintptr_t)fr->ego | (uintptr_t)fr->stack_allo | (uintptr_t)fr->stack_ego) & 15)
        return set_err(-22, f + ": frame buffers must be 16-byte aligned");
    HIPC(hipSetDevice(s->device));
    const int n = s->main.S.n_envs, F = (H + every - 1) / every;
    RolloutPool &R = s->look;
    if (int rc = rollout_reserve(s, R, n, "mg_imagine")) return rc;
    hipStream_t st = as_stream(stream);
    const MGState &P = R.P.S;
    HIPC(mg_launch_plan_fan((const char *)s->main.mem, (char *)R.P.mem, R.rows, R.nrows, n, /*K*/ 1, st));
    RenderOut ro = {};
    ro.preproc = pp;
    ro.frames_only = 1;
    ro.small = s->task == MG_TASK_MOVE_TO_REGION || s->task == MG_TASK_MOVE_TO_CORNER;
    ro.first_level = s->task == MG_TASK_CLUSTER_COLOUR ? 0 : 1;
    ro.force_retry = s->force_render_retry;
    // the class chain's levels are render scratch, not state rows, so the fan-out leaves the pool's stale: they are
    // copied with the state (u8[2 * e + view]; DESIGN.md, "Imagined observations", says why not reset)
    if (!ro.small) HIPC(hipMemcpyAsync(P.rg_retry, s->main.S.rg_retry, 2 * (size_t)n, hipMemcpyDeviceToDevice, st));
    const size_t FR = (size_t)MG_LORES * MG_LORES * 3;
    for (int k = 0; k < F; k++) {
        const bool last = k == F - 1;
        const int h0 = k * every, h1 = last ? H : h0 + every;
        // a segment is a plain lookahead launch on the pool as the last one left it; the call's outputs are the last one's
        const LookOut lo = {last && out && out->score ? out->score : R.scores, R.beam_steps, last && out ? out->bodies : nullptr,
                            last && out ? out->counts : nullptr, nullptr};
        HIPC(mg_launch_lookahead(P, s->dlib, s->task, s->step_form, s->step_blk, s->max_steps, actions + (size_t)h0 * n,
                                 h1 - h0, lo, nullptr, st));
        ro.obs_allo = fr->allo ? fr->allo + (size_t)k * n * FR : nullptr;
        ro.obs_ego = fr->ego ? fr->ego + (size_t)k * n * FR : nullptr;
        HIPC(mg_launch_render(P, s->dlib, ro, 3, st));
        HIPC(mg_launch_imagine_advance(P.episode_steps, R.beam_steps, s->main.S.episode_steps, P.overflow, n,
                                       last && out ? out->steps : nullptr, last && out ? out->errors : nullptr, st));
    }
    const MGState &M = s->main.S;
    if (sa)
        HIPC(mg_launch_imagine_stack(fr->allo, nullptr, M.hist_allo, M.hist_head, F, n, M.N, fr->stack_allo, st));
    if (se)
        HIPC(mg_launch_imagine_stack(fr->ego, pp == MG_PREPROC_LORES3EA ? fr->allo : nullptr, M.hist_ego, M.hist_head + M.N, F,
                                     n, M.N, fr->stack_ego, st));
    return 0;
}
