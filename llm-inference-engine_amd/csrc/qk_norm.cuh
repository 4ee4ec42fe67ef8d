// Per-head q/k RMSNorm (include/llmie.h, llmie_qk_norm): the arithmetic shared by the stand-alone operator (qk_norm.hip), the QKN
// instantiations of the decode split kernel (attention_decode.hip) and of the prefill RoPE + append kernel (prefill.hip), so that
// all of them give the same bits for the same head row.
//
// The ONE summation order of the sum of squares of a head row x[0 .. hs), hs in {64, 128}:
//   1. inside each aligned group of 8 consecutive elements: ss_g = fmaf(x_d, x_d, ss_g) in ascending d, from 0 (qkn_group_ss);
//   2. the hs / 8 group sums are combined by a butterfly over the bits of the group index, lowest bit first, plain fp32 adds
//      (a + b is commutative, so every member of a pair holds the same bits after its stage).
// Where the groups of a head lie in the lanes decides which stage is an add inside a lane and which a lane exchange:
//   operator, decode over the fp16 cache: lane j of the head holds group j                 -> exchanges xor 1, 2, 4 (, 8)
//   decode over the e4m3 cache:           lane j holds groups 2j, 2j + 1 (bit 0)           -> in-lane add FIRST, then xor 1, 2 (, 4)
//   prefill RoPE + append:                item j holds groups j, j + hs / 16 (highest bit) -> xor 1, 2 (, 4) on both sums, in-lane add LAST
#pragma once
#include "device_utils.cuh"

namespace llmie {

// step 1: the sum of squares of one aligned group of 8 consecutive elements (explicit fma, nothing left to contraction)
template <typename T> __device__ __forceinline__ float qkn_group_ss(const T *x8) {
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float f = to_f32(x8[e]);
        ss = __builtin_fmaf(f, f, ss);
    }
    return ss;
}
// step 2 across LANES adjacent lanes (a power of two <= 16), lowest distance first; every lane of the wave must be active
template <int LANES> __device__ __forceinline__ float qkn_lane_butterfly(float v) {
    static_assert(LANES == 1 || LANES == 2 || LANES == 4 || LANES == 8 || LANES == 16, "lanes of one head");
    if constexpr (LANES >= 2) v = lane_xor_sum<1>(v);
    if constexpr (LANES >= 4) v = lane_xor_sum<2>(v);
    if constexpr (LANES >= 8) v = lane_xor_sum<4>(v);
    if constexpr (LANES >= 16) v = lane_xor_sum<8>(v);
    return v;
}
// 1 / sqrt(mean square + eps): the form of norm.hip
__device__ __forceinline__ float qkn_inv(float ss, int hs, float eps) { return rsqrtf(ss / static_cast<float>(hs) + eps); }
// one element: (x * inv) * gamma, ONE rounding to the activation type
template <typename T> __device__ __forceinline__ T qkn_apply(float x, float inv, float g) {
    const float xi = x * inv;
    return from_f32<T>(xi * g);
}

// the host-side launch of the operator for the engine-less callers and the C entry (qk_norm.hip)
int qk_norm_f16(half_t *qkv, int rows, int head_num, int kv_head_num, int head_size, const half_t *q_gamma, const half_t *k_gamma, float eps,
                hipStream_t st);

}  // namespace llmie
