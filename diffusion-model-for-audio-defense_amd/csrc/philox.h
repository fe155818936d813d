// Philox4x32-10 counter-based generator (Salmon et al. 2011) and its Box-Muller normals, shared by the kernels that draw noise in
// registers (elementwise.hip, m5.hip).  counter = (block, sample_lo, sample_hi, stream), key = (seed_lo, seed_hi): sample i's noise
// is a pure function of (seed, i, stream) -> Monte Carlo votes do not depend on batch size or on the number of ranks.
#pragma once
#include "dmad_common.h"

namespace dmad {

__host__ __device__ inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

__device__ inline void philox_normal4(uint64_t seed, uint64_t sample, uint32_t stream, uint32_t block, float z[4]) {
    uint32_t c[4] = {block, (uint32_t)sample, (uint32_t)(sample >> 32), stream};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    // Box-Muller on (0,1) uniforms with 24 random bits each
    const float u0 = ((float)(c[0] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float u1 = ((float)(c[1] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float u2 = ((float)(c[2] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float u3 = ((float)(c[3] >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float r0 = sqrtf(-2.f * logf(u0)), r1 = sqrtf(-2.f * logf(u2));
    float s0, c0, s1, c1;
    sincosf(6.283185307179586f * u1, &s0, &c0);
    sincosf(6.283185307179586f * u3, &s1, &c1);
    z[0] = r0 * c0; z[1] = r0 * s0; z[2] = r1 * c1; z[3] = r1 * s1;
}

// One float4 of a Monte Carlo sample's input, certified_robust.py:46-47: x + delta, where delta is the caller's noise (d != nullptr) or
// sigma * the Philox normals keyed (seed, sample, stream 0, block).  Multiply, then add, each rounded: no FMA contraction, so the bits
// are those of torch's x + sigma * z on the same normals.  (mc_noise_scale_kernel states the same sum with its scale factor and is left
// as it was: it is on the benchmark's path.)
__device__ inline float4 noisy4(float4 x, const float* __restrict__ d, float sigma, uint64_t seed, uint64_t sample, uint32_t block) {
    float n[4];
    if (d) {
        const float4 dv = *(const float4*)d;
        n[0] = dv.x; n[1] = dv.y; n[2] = dv.z; n[3] = dv.w;
    } else {
        philox_normal4(seed, sample, 0u, block, n);
#pragma unroll
        for (int j = 0; j < 4; ++j) n[j] = __fmul_rn(sigma, n[j]);
    }
    return float4{__fadd_rn(x.x, n[0]), __fadd_rn(x.y, n[1]), __fadd_rn(x.z, n[2]), __fadd_rn(x.w, n[3])};
}

}  // namespace dmad
