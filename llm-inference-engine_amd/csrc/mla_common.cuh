// What the MLA translation units (mla.hip: the decode step; mla_prefill.hip: the prompt) share: the fixed geometry, where a latent
// cache row lives, and the host checks every entry makes.
#pragma once
#include "llmie_internal.h"

namespace llmie {

constexpr int kLat = LLMIE_MLA_KV_LORA_RANK, kRope = LLMIE_MLA_QK_ROPE_HEAD_DIM, kRow = LLMIE_MLA_ROW;
constexpr int kNope = LLMIE_MLA_QK_NOPE_HEAD_DIM, kVd = LLMIE_MLA_V_HEAD_DIM, kQ = kNope + kRope, kPage = LLMIE_MLA_PAGE_TOKENS;
static_assert(kLat == 512 && kRope == 64 && kRow == 576 && kNope == 128 && kVd == 128, "the kernels are written for this geometry");
// the e4m3 row (mla_e4m3.hip): 512 e4m3 latent bytes, then the 64 k_pe halves: 40 pieces of 16 bytes, 32 latent and 8 rope
constexpr int kRowE4 = LLMIE_MLA_ROW_E4M3_BYTES, kLatPieces = kLat / 16, kPePieces = kRope * 2 / 16;
static_assert(kRowE4 == kLat + 2 * kRope && kRowE4 == 16 * (kLatPieces + kPePieces), "the e4m3 row: 640 bytes");
// the decode split both cache formats share (plan_mla_decode): heads per workgroup, keys per staged tile, tokens per split, merge block
constexpr int kMlaHeads = 16, kMlaTile = 32, kMlaChunk = 256, kMlaMergeBlock = 128;

typedef __fp16 fp16x4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef __attribute__((address_space(3))) fp16x4_t *lds_fp16x4_ptr;
struct Tr8 { fp16x4_t lo, hi; };   // two transposed reads side by side are the 8-half MFMA operand

__device__ __forceinline__ bool mla_live(int ctx, int max_ctx) { return ctx >= 1 && ctx <= max_ctx; }

// where the cache row of (sequence b, position t) begins, in halves
__device__ __forceinline__ size_t mla_row_off(const int32_t *__restrict__ table, int max_pages, size_t layer_off, int b, int t, int max_seq_len) {
    return table ? layer_off + (static_cast<size_t>(table[static_cast<size_t>(b) * max_pages + t / kPage]) * kPage + t % kPage) * kRow
                 : layer_off + (static_cast<size_t>(b) * max_seq_len + t) * kRow;
}

// the same place in an e4m3 cache, in bytes (layer_off in bytes: mla_layer_off_bytes)
__device__ __forceinline__ size_t mla_row_off_bytes(const int32_t *__restrict__ table, int max_pages, size_t layer_off, int b, int t, int max_seq_len) {
    return table ? layer_off + (static_cast<size_t>(table[static_cast<size_t>(b) * max_pages + t / kPage]) * kPage + t % kPage) * kRowE4
                 : layer_off + (static_cast<size_t>(b) * max_seq_len + t) * kRowE4;
}

inline int mla_heads_check(const char *who, int batch, int head_num) {
    LLMIE_REQUIRE(batch >= 1, "%s: batch=%d should be >= 1", who, batch);
    if (head_num < 16 || head_num > 128 || head_num % 16 != 0)
        LLMIE_UNSUPPORTED("%s: head_num=%d: the MLA kernels take a multiple of 16 in [16, 128] (kv_lora_rank 512, rope 64, nope 128, v 128)", who,
                          head_num);
    return LLMIE_OK;
}

inline int mla_cache_check(const char *who, int max_seq_len, bool paged, int max_pages, int num_pages) {
    LLMIE_REQUIRE(max_seq_len >= 1, "%s: max_seq_len=%d should be >= 1", who, max_seq_len);
    if (paged) {
        LLMIE_REQUIRE(num_pages >= 1 && max_pages >= 1, "%s: paged cache: max_pages=%d and num_pages=%d should be >= 1", who, max_pages, num_pages);
        LLMIE_REQUIRE(static_cast<long long>(max_pages) * kPage >= max_seq_len, "%s: paged cache: max_pages=%d pages of %d tokens do not hold max_seq_len=%d",
                      who, max_pages, kPage, max_seq_len);
    }
    return LLMIE_OK;
}

inline size_t mla_layer_off(int layer, int batch, int max_seq_len, bool paged, int num_pages) {
    return static_cast<size_t>(layer) * (paged ? static_cast<size_t>(num_pages) * kPage : static_cast<size_t>(batch) * max_seq_len) * kRow;
}

inline size_t mla_layer_off_bytes(int layer, int batch, int max_seq_len, bool paged, int num_pages) {
    return static_cast<size_t>(layer) * (paged ? static_cast<size_t>(num_pages) * kPage : static_cast<size_t>(batch) * max_seq_len) * kRowE4;
}

}  // namespace llmie
