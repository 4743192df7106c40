// mg_scene.hip -- explicit scenes in the C ABI (include/magical_sim.h): mg_get_scene reads every env's layout into
// mg_scene records, mg_reset_scene starts envs from records (device code: mg_scene.h).
// As in mg_reset.hip, one out-of-line collide() for the overlap check's shape queries bounds this unit's compile time.
#define MG_COLLIDE_ATTR __device__ __attribute__((noinline))
#include "mg_sim.h"
#include "mg_scene.h"

// One wavefront per env.  The env's record goes to LDS in 16-byte loads, is validated there, and only a record with
// status 0 reaches the build: an env that is not selected or is refused has had nothing written.  built[e] (the render's
// mask) and status[e] are written for every env.
__global__ void __launch_bounds__(64) scene_build_kernel(MGState S, const mg_library *__restrict__ L, SceneCfg cfg,
                                                         const mg_scene *__restrict__ scenes,
                                                         const uint8_t *__restrict__ mask, int32_t *__restrict__ status,
                                                         uint8_t *__restrict__ built) {
    __shared__ __attribute__((aligned(16))) uint64_t row[MG_SCENE_WORDS + 1];
    const int e = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (e >= S.n_envs) return;
    if (mask && !mask[e]) {   // uniform over the wavefront
        if (lane == 0) { status[e] = MG_SCENE_UNSELECTED; built[e] = 0; }
        return;
    }
    scene_load_row(scenes, e, row, lane);
    __syncthreads();
    const mg_scene &R = *(const mg_scene *)row;
    const int st = scene_status(R, L, cfg);
    if (lane == 0) { status[e] = st; built[e] = st == MG_SCENE_OK ? 1 : 0; }
    if (st != MG_SCENE_OK) return;
    scene_build(S, L, e, R, cfg);
}

// check = 1: one wavefront per built env runs the layout sampler's overlap queries on the scene as built
__global__ void __launch_bounds__(64) scene_check_kernel(MGState S, const mg_library *__restrict__ L, int task,
                                                         const uint8_t *__restrict__ built) {
    const int e = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (e >= S.n_envs || !built[e]) return;
    const bool hit = scene_overlaps(S, L, e, task, lane);
    if (hit && lane == 0) S.overflow[e] |= 2 | 64;   // PlacementError, as randomise_all raises it
}

__global__ void __launch_bounds__(64) scene_read_kernel(MGState S, int task, mg_scene *__restrict__ out) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= S.n_envs) return;
    scene_read(S, e, task, out + e);
}

extern "C" {

int mg_get_scene(mg_sim *s, mg_scene *scenes, void *stream) {
    if (!s || !scenes) return set_err(-22, "mg_get_scene: null argument");
    if ((uintptr_t)scenes & 7) return set_err(-22, "mg_get_scene: scenes_dev must be 8-byte aligned");
    HIPC(hipSetDevice(s->device));
    hipLaunchKernelGGL(scene_read_kernel, dim3((s->main.S.n_envs + 63) / 64), dim3(64), 0, as_stream(stream), s->main.S,
                       s->task, scenes);
    HIPC(hipGetLastError());
    return 0;
}

int mg_reset_scene(mg_sim *s, const mg_scene *scenes, const uint8_t *mask, int32_t check, int32_t *status, void *stream) {
    if (!s || !scenes || !status) return set_err(-22, "mg_reset_scene: null argument");
    if ((uintptr_t)scenes & 7) return set_err(-22, "mg_reset_scene: scenes_dev must be 8-byte aligned");
    if (check != 0 && check != 1) return set_err(-22, "mg_reset_scene: check must be 0 or 1");
    if (!s->bound && s->preproc != MG_PREPROC_NONE) return set_err(-22, "mg_reset_scene: outputs not bound");
    HIPC(hipSetDevice(s->device));
    hipStream_t st = as_stream(stream);
    const SceneCfg cfg = {s->task, s->flags, s->caps, s->step_form == 5 || s->step_form == 6};
    const int n = s->main.S.n_envs;
    hipLaunchKernelGGL(scene_build_kernel, dim3(n), dim3(64), 0, st, s->main.S, s->dlib, cfg, scenes, mask, status,
                       s->scene_built);
    HIPC(hipGetLastError());
    if (check) {
        hipLaunchKernelGGL(scene_check_kernel, dim3(n), dim3(64), 0, st, s->main.S, s->dlib, s->task, s->scene_built);
        HIPC(hipGetLastError());
    }
    // the shadow keeps the env's next layout and the RNG rows were not touched: nothing to hand over
    if (s->preproc != MG_PREPROC_NONE) return render_lores(s, st, s->scene_built);
    return 0;
}

} // extern "C"
