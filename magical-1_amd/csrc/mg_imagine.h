// mg_imagine.h -- mg_imagine's own kernels (mg_imagine.hip, with mg_imagine and its segment loop): the per-segment
// advance of the scratch pool's episode counter and the stack pass.  The rollouts are the lookahead kernel, launched
// unchanged on mg_lookahead's scratch pool once per segment (mg_lookahead.h); the frames are render_kernel's mode 3
// (mg_render.h), drawn from that pool; the fan-out copy is mg_plan's (mg_plan.h).
//
// Layouts (n = num_envs, FR = 96 * 96 * 3): frames u8[F][n][FR], stacks u8[F][n][4 * FR]; the sim's frame rings
// u8[4][Npad][FR] with the newest slot of env e in head[e] (hist_head + view * Npad).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// After a segment's rollout and render: pool_steps[e] += seg_steps[e] -- the pool's episode counter, which the
// lookahead kernel does not keep (mg_plan_beam's carry between segments, mg_beam.h), so the next segment's launch gives
// env e min(its length, what is left of the episode) env-steps and a stopped env stays stopped.  steps / errors (either
// may be null; passed after the last segment): the env-steps of the whole call, pool_steps[e] - env_steps[e] with
// env_steps the sim's own counter, and the pool's error flags with the render's capacity bits in them
hipError_t mg_launch_imagine_advance(int32_t *pool_steps, const int32_t *seg_steps, const int32_t *env_steps,
                                     const int32_t *pool_errors, int n_envs, int32_t *steps, int32_t *errors, hipStream_t st);
// stack[f][e] = (g_f-3, g_f-2, g_f-1, g_f) per pixel, 12 bytes, oldest first: g_j = frames[j][e] for j >= 0 and the
// ring's slot (head[e] + j + 1) & 3 for j < 0 (newest = -1).  lead not null (LoRes3EA): the first of the four is
// lead[f][e] instead (allo_f | ego_f-2 | ego_f-1 | ego_f, compose3ea_kernel's layout).  The ring is only read
hipError_t mg_launch_imagine_stack(const uint8_t *frames, const uint8_t *lead, const uint8_t *ring, const int32_t *head,
                                   int F, int n_envs, int Npad, uint8_t *stacks, hipStream_t st);
