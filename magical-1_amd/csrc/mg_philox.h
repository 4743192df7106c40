// mg_philox.h -- the device generator of random actions: Philox4x32-10 (Salmon et al. 2011), counter = (step lo,
// step hi, env, 0), key = (k lo, k hi); the action is the first output word mod 18.  Shared by mg_random_actions
// (mg_sim.hip) and mg_plan_sample (mg_plan.hip), which is defined through it, and by mg_plan_cem's weighted draw
// (mg_cem.hip), which reduces the same word modulo its weights' total.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ uint32_t mulhilo(uint32_t a, uint32_t b, uint32_t &hi) {
    uint64_t p = (uint64_t)a * b;
    hi = (uint32_t)(p >> 32);
    return (uint32_t)p;
}

// the first output word for (key, step, env e)
__device__ __forceinline__ uint32_t philox_word(uint64_t key, uint64_t step, int e) {
    uint32_t c0 = (uint32_t)step, c1 = (uint32_t)(step >> 32), c2 = (uint32_t)e, c3 = 0;
    uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
    for (int r = 0; r < 10; r++) {
        uint32_t hi0, hi1;
        uint32_t lo0 = mulhilo(0xD2511F53u, c0, hi0);
        uint32_t lo1 = mulhilo(0xCD9E8D57u, c2, hi1);
        uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

__device__ __forceinline__ uint8_t philox_action(uint64_t key, uint64_t step, int e) {
    return (uint8_t)(philox_word(key, step, e) % 18u);
}
