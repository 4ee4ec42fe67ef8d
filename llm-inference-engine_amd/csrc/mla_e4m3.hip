// Multi-head Latent Attention on an e4m3 latent cache (include/llmie.h, llmie_mla_*_e4m3): a token is 640 bytes -- 512 OCP e4m3fn
// codes of the latent, code = e4m3(c / c_scale) with one static fp32 c_scale per cache, then the 64 rotated k_pe halves in fp16 --
// against the 1152 of the fp16 cache.  The append and the decode are the E4 instantiations of the fp16 cache's kernel templates
// (mla.hip: mla_kv_append_kernel -- the fp16 row, quantised --, mla_decode_kernel -- the same work split behind a staging path that
// turns codes into halves, c_scale joining in fp32 --, reached through mla_append_launch and mla_decode_run); the split partials are
// one format, so the one mla_merge_kernel merges them.  This file holds the format's entries and its one kernel of its own:
//   mla_dequant_e4m3_kernel    rows t < ctx of one layer -> an fp16 latent cache of the same geometry            (the prompt path's bridge)
// The chunking depends on ctx alone: a sequence's bits do not depend on the batch, its slot or the grid; dense = paged bit for bit.
#include "mla_common.cuh"

namespace llmie {

namespace {

// ---- dequant: grid (tiles of 32 tokens, batch), 5 pieces per thread; rows t < ctx of one layer, e4m3 -> fp16 ----
__global__ __launch_bounds__(256) void mla_dequant_e4m3_kernel(const unsigned char *__restrict__ src, half_t *__restrict__ dst, size_t src_off,
                                                               size_t dst_off, int max_seq_len, int max_ctx, float c_scale,
                                                               const int32_t *__restrict__ ctx_len, const int32_t *__restrict__ table,
                                                               int max_pages) {
    const int t0 = blockIdx.x * kMlaTile, b = blockIdx.y, tid = threadIdx.x;
    const int ctx = ctx_len[b];
    if (!mla_live(ctx, max_ctx) || t0 >= ctx) return;
    const size_t row0 = mla_tile_row0(table, max_pages, b, t0, max_seq_len);
    const unsigned char *sp = src + src_off + row0 * kRowE4;
    half_t *dp = dst + dst_off + row0 * kRow;
    constexpr int P = kLatPieces + kPePieces;
#pragma unroll
    for (int i = 0; i < kMlaTile * P / 256; ++i) {
        const int id = tid + 256 * i, row = id / P, piece = id - row * P;
        if (t0 + row >= ctx) continue;
        const uint4_t v = *reinterpret_cast<const uint4_t *>(sp + row * kRowE4 + 16 * piece);
        if (piece >= kLatPieces) {
            *reinterpret_cast<uint4_t *>(dp + row * kRow + kLat + 8 * (piece - kLatPieces)) = v;
            continue;
        }
        half_t h[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(v[k], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(v[k], true);
            h[4 * k] = from_f32<half_t>(lo[0] * c_scale), h[4 * k + 1] = from_f32<half_t>(lo[1] * c_scale);
            h[4 * k + 2] = from_f32<half_t>(hi[0] * c_scale), h[4 * k + 3] = from_f32<half_t>(hi[1] * c_scale);
        }
        half_t *o = dp + row * kRow + 16 * piece;
        *reinterpret_cast<half8_t *>(o) = half8_t{h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]};
        *reinterpret_cast<half8_t *>(o + 8) = half8_t{h[8], h[9], h[10], h[11], h[12], h[13], h[14], h[15]};
    }
}

}  // namespace

}  // namespace llmie

using namespace llmie;

extern "C" const char *llmie_mla_decode_e4m3_plan(int batch, int head_num, int max_seq_len, int max_ctx, int paged, int max_pages, int num_pages,
                                                  long long workspace_bytes, int *status) {
    static thread_local char text[176];
    const MlaDecodeCall c{batch, head_num, max_seq_len, max_ctx, paged != 0, max_pages, num_pages, workspace_bytes >= 0,
                          workspace_bytes >= 0 ? static_cast<size_t>(workspace_bytes) : 0, true};
    return mla_decode_plan_text("mla_decode_e4m3_plan", c, text, sizeof(text), status);
}

extern "C" int llmie_mla_kv_append_e4m3(const void *kv_a, const void *gamma, float eps, const void *rope_table, void *cache, float c_scale,
                                        int layer, int batch, int max_seq_len, const int32_t *ctx_len_dev, const int32_t *block_table,
                                        int max_pages, int num_pages, llmie_stream stream) {
    LLMIE_REQUIRE(kv_a && gamma && rope_table && cache && ctx_len_dev, "mla_kv_append_e4m3: NULL operand");
    LLMIE_REQUIRE(batch >= 1 && layer >= 0, "mla_kv_append_e4m3: batch=%d should be >= 1 and layer=%d >= 0", batch, layer);
    LLMIE_REQUIRE(eps > 0.f, "mla_kv_append_e4m3: eps should be > 0");
    LLMIE_REQUIRE(mla_scale_ok(c_scale), "mla_kv_append_e4m3: c_scale should be positive and finite");
    const int rc = mla_cache_check("mla_kv_append_e4m3", max_seq_len, block_table != nullptr, max_pages, num_pages);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(mis16(kv_a) == 0 && mis16(gamma) == 0 && mis16(cache) == 0, "mla_kv_append_e4m3: kv_a, gamma and the cache should be 16-byte aligned");
    mla_append_launch(MlaAppendCall{kv_a, gamma, eps, rope_table, cache, layer, batch, max_seq_len, ctx_len_dev, nullptr, nullptr, 0, 0, block_table,
                                    max_pages, num_pages, true, c_scale},
                      batch, as_stream(stream));
    return launch_status("mla_kv_append_e4m3");
}

extern "C" int llmie_mla_kv_append_rows_e4m3(const void *kv_a, const void *gamma, float eps, const void *rope_table, void *cache, float c_scale,
                                             int layer, int batch, int total_tokens, int max_q_len, int kv_span, int max_seq_len,
                                             const int32_t *cum_dev, const int32_t *hist_dev, const int32_t *block_table, int max_pages,
                                             int num_pages, llmie_stream stream) {
    LLMIE_REQUIRE(kv_a && gamma && rope_table && cache && cum_dev && hist_dev, "mla_kv_append_rows_e4m3: NULL operand");
    LLMIE_REQUIRE(layer >= 0 && total_tokens >= 1, "mla_kv_append_rows_e4m3: layer=%d should be >= 0 and total_tokens=%d >= 1", layer, total_tokens);
    LLMIE_REQUIRE(eps > 0.f, "mla_kv_append_rows_e4m3: eps should be > 0");
    LLMIE_REQUIRE(mla_scale_ok(c_scale), "mla_kv_append_rows_e4m3: c_scale should be positive and finite");
    MlaPrefillPlan p{};
    const int rc = plan_mla_prefill("mla_kv_append_rows_e4m3",
                                    MlaPrefillCall{batch, 0, total_tokens, max_q_len, kv_span, max_seq_len, block_table != nullptr, max_pages, num_pages}, &p);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(mis16(kv_a) == 0 && mis16(gamma) == 0 && mis16(cache) == 0,
                  "mla_kv_append_rows_e4m3: kv_a, gamma and the cache should be 16-byte aligned");
    mla_append_launch(MlaAppendCall{kv_a, gamma, eps, rope_table, cache, layer, batch, max_seq_len, nullptr, cum_dev, hist_dev, max_q_len, kv_span,
                                    block_table, max_pages, num_pages, true, c_scale},
                      p.append_grid, as_stream(stream));
    return launch_status("mla_kv_append_rows_e4m3");
}

extern "C" int llmie_mla_decode_e4m3(const void *q_lat, const void *cache, void *o_lat, int layer, int batch, int head_num, int max_seq_len,
                                     int max_ctx, const int32_t *ctx_len_dev, float softmax_scale, void *workspace, size_t workspace_bytes,
                                     const int32_t *block_table, int max_pages, int num_pages, float c_scale, llmie_stream stream) {
    const MlaDecodeCall c{batch, head_num, max_seq_len, max_ctx, block_table != nullptr, max_pages, num_pages, workspace != nullptr, workspace_bytes, true};
    return mla_decode_run("mla_decode_e4m3", c, MlaDecodeIo{q_lat, cache, o_lat, layer, ctx_len_dev, block_table, softmax_scale, workspace, c_scale},
                          as_stream(stream));
}

extern "C" int llmie_mla_cache_dequant_e4m3(const void *cache_e4m3, void *cache_f16, float c_scale, int layer, int batch, int max_seq_len,
                                            int max_ctx, const int32_t *ctx_len_dev, const int32_t *block_table, int max_pages, int num_pages,
                                            llmie_stream stream) {
    LLMIE_REQUIRE(cache_e4m3 && cache_f16 && ctx_len_dev, "mla_cache_dequant_e4m3: NULL operand");
    LLMIE_REQUIRE(batch >= 1 && batch <= 65535 && layer >= 0, "mla_cache_dequant_e4m3: batch=%d should be in [1, 65535] and layer=%d >= 0", batch, layer);
    LLMIE_REQUIRE(mla_scale_ok(c_scale), "mla_cache_dequant_e4m3: c_scale should be positive and finite");
    const bool paged = block_table != nullptr;
    const int rc = mla_cache_check("mla_cache_dequant_e4m3", max_seq_len, paged, max_pages, num_pages);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(max_ctx >= 0 && max_ctx <= max_seq_len, "mla_cache_dequant_e4m3: max_ctx=%d should be 0 or in [1, max_seq_len=%d]", max_ctx, max_seq_len);
    LLMIE_REQUIRE(mis16(cache_e4m3) == 0 && mis16(cache_f16) == 0, "mla_cache_dequant_e4m3: both caches should be 16-byte aligned");
    const int span = max_ctx > 0 ? max_ctx : max_seq_len;
    hipLaunchKernelGGL(mla_dequant_e4m3_kernel, dim3((span + kMlaTile - 1) / kMlaTile, batch), dim3(256), 0, as_stream(stream),
                       static_cast<const unsigned char *>(cache_e4m3), static_cast<half_t *>(cache_f16),
                       mla_layer_off(layer, batch, max_seq_len, paged, num_pages, kRowE4), mla_layer_off(layer, batch, max_seq_len, paged, num_pages, kRow),
                       max_seq_len, span, c_scale, ctx_len_dev, block_table, max_pages);
    return launch_status("mla_cache_dequant_e4m3");
}
