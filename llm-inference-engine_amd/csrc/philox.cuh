// Philox4x32-10 uniform in (0, 1]: seed = the decode step, stream = the counter (the batch row for llmie_sampling, the
// request's seed for llmie_sample_logits).  oracle.uniform_philox reproduces it bit for bit.
#pragma once
#include "device_utils.cuh"

namespace llmie {

__device__ __forceinline__ float uniform_philox(uint32_t seed, uint32_t stream) {
    uint32_t c0 = stream, c1 = 0, c2 = 0, c3 = 0;
    uint32_t k0 = seed, k1 = 0x4c4c4d49u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return static_cast<float>((c0 >> 8) + 1u) * (1.0f / 16777216.0f);
}

// The laned form: counter (stream, lane, 0, 0), returned as the 24-bit integer U = (c0 >> 8) + 1 in [1, 2^24].  Lane 0 is the
// draw above (uniform_philox == U / 2^24); llmie_spec_verify_sampled takes its accept draw from lane 1 and its residual draw from
// lane 2, independent of the sampler's own pick at the same (seed, stream) and of each other.
__device__ __forceinline__ uint32_t philox_u24(uint32_t seed, uint32_t stream, uint32_t lane) {
    uint32_t c0 = stream, c1 = lane, c2 = 0, c3 = 0;
    uint32_t k0 = seed, k1 = 0x4c4c4d49u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return (c0 >> 8) + 1u;
}

}  // namespace llmie
