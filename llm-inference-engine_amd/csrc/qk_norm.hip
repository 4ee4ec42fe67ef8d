// llmie_qk_norm: per-head RMSNorm of the q and k heads of packed QKV rows, in place (Qwen3 `self_attn.q_norm` / `k_norm`), the
// operator on its own -- the per-kernel path runs it between llmie_linear and llmie_qkv_bias_transpose_rope; the engine's decode
// and prefill attention launches apply the same arithmetic themselves (qk_norm.cuh states it and its summation order).
//
// One head = HS / 8 adjacent lanes, one 16-byte vector per lane: the sum of squares is a lane butterfly, no LDS and no barrier.
// Memory-bound: every q / k element is read once and written once; v columns are never touched.
#include "qk_norm.cuh"

#include <cmath>

namespace llmie {

template <int HS>
__global__ __launch_bounds__(256) void qk_norm_kernel(half_t *__restrict__ qkv, long long items, int head_num, int kv_head_num,
                                                      const half_t *__restrict__ q_gamma, const half_t *__restrict__ k_gamma, float eps) {
    constexpr int LPH = HS / 8;   // lanes of one head; 256 % LPH == 0 and items % LPH == 0: a head's lanes are in one wave
    // the lanes past the last head of a partial last workgroup redo the last item and store nothing: every lane stays active for the
    // exchanges, and every address is one of an item inside the buffer
    const long long id = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    const bool live = id < items;
    const long long item = live ? id : items - 1;
    const int normed = head_num + kv_head_num;
    const int j = static_cast<int>(item % LPH);
    const long long hr = item / LPH;
    const int h = static_cast<int>(hr % normed);   // q heads, then k heads: the column order of a packed row
    const long long row = hr / normed;
    half_t *p = qkv + (static_cast<size_t>(row) * (head_num + 2 * kv_head_num) + h) * HS + j * 8;
    const half8_t x = *reinterpret_cast<const half8_t *>(p);
    const half8_t g = *reinterpret_cast<const half8_t *>((h < head_num ? q_gamma : k_gamma) + j * 8);
    half_t xe[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) xe[e] = x[e];
    const float inv = qkn_inv(qkn_lane_butterfly<LPH>(qkn_group_ss(xe)), HS, eps);
    half8_t y;
#pragma unroll
    for (int e = 0; e < 8; ++e) y[e] = qkn_apply<half_t>(to_f32(xe[e]), inv, to_f32(g[e]));
    if (live) *reinterpret_cast<half8_t *>(p) = y;
}

int qk_norm_f16(half_t *qkv, int rows, int head_num, int kv_head_num, int head_size, const half_t *q_gamma, const half_t *k_gamma, float eps,
                hipStream_t st) {
    const long long items = static_cast<long long>(rows) * (head_num + kv_head_num) * (head_size / 8);
    const long long blocks = (items + 255) / 256;
    if (blocks > 0x7fffffffLL) {
        set_error("qk_norm: %d rows of %d heads are more than one grid holds", rows, head_num + kv_head_num);
        return LLMIE_ERR_UNSUPPORTED;
    }
    if (head_size == 128) qk_norm_kernel<128><<<static_cast<unsigned>(blocks), 256, 0, st>>>(qkv, items, head_num, kv_head_num, q_gamma, k_gamma, eps);
    else qk_norm_kernel<64><<<static_cast<unsigned>(blocks), 256, 0, st>>>(qkv, items, head_num, kv_head_num, q_gamma, k_gamma, eps);
    return launch_status("qk_norm");
}

}  // namespace llmie

using namespace llmie;

extern "C" int llmie_qk_norm(void *qkv, int rows, int head_num, int kv_head_num, int head_size, const void *q_gamma, const void *k_gamma,
                             float eps, llmie_dtype dtype, llmie_stream stream) {
    LLMIE_REQUIRE(qkv && q_gamma && k_gamma, "qk_norm: NULL pointer");
    LLMIE_REQUIRE(rows > 0 && head_num > 0 && kv_head_num > 0 && head_size > 0, "qk_norm: bad shape rows=%d head_num=%d kv_head_num=%d head_size=%d",
                  rows, head_num, kv_head_num, head_size);
    LLMIE_REQUIRE(head_num % kv_head_num == 0, "qk_norm: kv_head_num must divide head_num");
    LLMIE_REQUIRE(eps >= 0.f && !std::isnan(eps), "qk_norm: eps must be a number >= 0");
    LLMIE_REQUIRE((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(q_gamma) | reinterpret_cast<uintptr_t>(k_gamma)) % 16 == 0,
                  "qk_norm: qkv and the gammas must be 16-byte aligned");
    if (dtype != LLMIE_F16) LLMIE_UNSUPPORTED("qk_norm: fp16 only (dtype %d)", (int)dtype);
    if (head_size != 64 && head_size != 128) LLMIE_UNSUPPORTED("qk_norm: head_size 64 / 128 only (head_size=%d)", head_size);
    return qk_norm_f16(static_cast<half_t *>(qkv), rows, head_num, kv_head_num, head_size, static_cast<const half_t *>(q_gamma),
                       static_cast<const half_t *>(k_gamma), eps, as_stream(stream));
}
