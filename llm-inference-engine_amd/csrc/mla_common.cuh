// What the five MLA translation units (mla.hip: the decode step, both cache formats, and the one append; mla_prefill.hip: the prompt;
// mla_verify.hip: several query rows; mla_e4m3.hip: the e4m3 cache's entries and its dequant; mla_sparse.hip: the indexer and the
// decode over a selection) share: the fixed geometry, where a latent cache row lives, the append's row arithmetic, the split partial's
// store, the host checks every entry makes and the host split plan.  The split-KV tile loop itself, which mla.hip and mla_sparse.hip
// alone run, is in mla_tile_loop.cuh.
#pragma once
#include "llmie_internal.h"

#include <cmath>
#include <cstdio>

namespace llmie {

constexpr int kLat = LLMIE_MLA_KV_LORA_RANK, kRope = LLMIE_MLA_QK_ROPE_HEAD_DIM, kRow = LLMIE_MLA_ROW;
constexpr int kNope = LLMIE_MLA_QK_NOPE_HEAD_DIM, kVd = LLMIE_MLA_V_HEAD_DIM, kQ = kNope + kRope, kPage = LLMIE_MLA_PAGE_TOKENS;
static_assert(kLat == 512 && kRope == 64 && kRow == 576 && kNope == 128 && kVd == 128, "the kernels are written for this geometry");
// the e4m3 row: 512 e4m3 latent bytes, then the 64 k_pe halves: 40 pieces of 16 bytes, 32 latent and 8 rope
constexpr int kRowE4 = LLMIE_MLA_ROW_E4M3_BYTES, kLatPieces = kLat / 16, kPePieces = kRope * 2 / 16;
static_assert(kRowE4 == kLat + 2 * kRope && kRowE4 == 16 * (kLatPieces + kPePieces), "the e4m3 row: 640 bytes");
// the split decode (both cache formats) and verify share (plan_mla_decode, plan_mla_verify): heads per workgroup, keys per staged
// tile, tokens per split, merge block, and the staged tile's padded LDS row
constexpr int kMlaHeads = 16, kMlaTile = 32, kMlaChunk = 256, kMlaMergeBlock = 128, kMlaStride = kRow + 16;
static_assert(kPage % kMlaTile == 0 && kMlaChunk % kMlaTile == 0, "a tile never crosses a page or a chunk");
static_assert((kMlaStride * 2) % 64 == 32, "row stride = an odd multiple of 32 bytes: conflict-free transposed reads");
constexpr float kLog2e = 1.44269504088896341f;   // the kernels' softmax runs in the log2 domain: scale2 = softmax_scale * kLog2e

typedef __fp16 fp16x4_t __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef __attribute__((address_space(3))) fp16x4_t *lds_fp16x4_ptr;
struct Tr8 { fp16x4_t lo, hi; };   // two transposed reads side by side are the 8-half MFMA operand

__device__ __forceinline__ bool mla_live(int ctx, int max_ctx) { return ctx >= 1 && ctx <= max_ctx; }

__device__ __forceinline__ bool mla_prefill_live(int len, int history, int max_q_len, int kv_span) {
    return len >= 1 && len <= max_q_len && history >= 0 && history <= kv_span - len;
}

// verify: the sequence's extent, or false where the call leaves it untouched
__device__ __forceinline__ bool verify_live(const int32_t *__restrict__ hist_dev, const int32_t *__restrict__ count_dev, int b, int rows, int span,
                                            int *hist, int *count) {
    *hist = hist_dev[b];
    *count = count_dev ? count_dev[b] : rows;
    return *hist >= 0 && *count >= 1 && *count <= rows && *hist <= span - *count;
}

// where the cache row of (sequence b, position t) begins, in units of ROW's: ROW = kRow (halves, fp16 cache) or kRowE4 (bytes, e4m3)
template <int ROW>
__device__ __forceinline__ size_t mla_row_off(const int32_t *__restrict__ table, int max_pages, size_t layer_off, int b, int t, int max_seq_len) {
    return table ? layer_off + (static_cast<size_t>(table[static_cast<size_t>(b) * max_pages + t / kPage]) * kPage + t % kPage) * ROW
                 : layer_off + (static_cast<size_t>(b) * max_seq_len + t) * ROW;
}

// the row index, inside a layer, of the first row of the tile that starts at position t0 of sequence b (a tile never crosses a page):
// one block-table read, made wave-uniform
__device__ __forceinline__ size_t mla_tile_row0(const int32_t *__restrict__ table, int max_pages, int b, int t0, int max_seq_len) {
    return table ? static_cast<size_t>(__builtin_amdgcn_readfirstlane(table[static_cast<size_t>(b) * max_pages + t0 / kPage])) * kPage + t0 % kPage
                 : static_cast<size_t>(b) * max_seq_len + t0;
}

// 8 e4m3 codes (two words, memory order) -> the 8 halves of their exact values
__device__ __forceinline__ half8_t e4m3x8_to_f16(unsigned w0, unsigned w1) {
    const half2_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, true);
    const half2_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, true);
    return half8_t{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// ---- the append's row, one wave per token (include/llmie.h states this order).  Lane i holds c[8 i .. 8 i + 7]; sum of squares:
// ss = fma(c_j, c_j, ss) over j = 0 .. 7 in that order from ss = 0, then the xor butterfly over lane distances 32, 16, 8, 4, 2, 1 ----
__device__ __forceinline__ half8_t mla_append_latent(const half_t *__restrict__ src, const half_t *__restrict__ gamma, float eps, int lane) {
    const half8_t x = *reinterpret_cast<const half8_t *>(src + 8 * lane);
    const half8_t g = *reinterpret_cast<const half8_t *>(gamma + 8 * lane);
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss = __builtin_fmaf(to_f32(x[j]), to_f32(x[j]), ss);
    ss = lane_xor_sum<32>(ss);
    ss = lane_xor_sum<16>(ss);
    ss = lane_xor_sum<8>(ss);
    ss = lane_xor_sum<4>(ss);
    ss = lane_xor_sum<2>(ss);
    ss = lane_xor_sum<1>(ss);
    const float inv = 1.f / sqrtf(ss * (1.f / kLat) + eps);
    half8_t y;
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = from_f32<half_t>(to_f32(x[j]) * inv * to_f32(g[j]));
    return y;
}

// the rotated k_pe pair (lane, lane + 32) of the token at position pos, lane < 32, into pe[0 .. 63]
__device__ __forceinline__ void mla_append_rope(const half_t *__restrict__ src, const float2 *__restrict__ rope, int pos, int lane, half_t *pe) {
    const float2 cs = rope[static_cast<size_t>(pos) * (kRope / 2) + lane];
    const float x0 = to_f32(src[kLat + lane]), x1 = to_f32(src[kLat + kRope / 2 + lane]);
    pe[lane] = from_f32<half_t>(x0 * cs.x - x1 * cs.y);
    pe[kRope / 2 + lane] = from_f32<half_t>(x1 * cs.x + x0 * cs.y);
}

// the sequence and cache position of packed token tok (cum[batch + 1] = exclusive prefix of the new-token counts, hist[b] = tokens
// already cached), or false where the token is past the last or its sequence is left untouched
__device__ __forceinline__ bool mla_packed_locate(const int32_t *__restrict__ cum, const int32_t *__restrict__ hist, int batch, int tok,
                                                  int max_q_len, int kv_span, int *seq, int *pos) {
    if (tok >= cum[batch]) return false;
    int b = 0;   // the last sequence that begins at or in front of the token: an empty one shares its begin with its successor
    for (int hi = batch; hi - b > 1;) {
        const int mid = (b + hi) >> 1;
        if (cum[mid] <= tok) b = mid;
        else hi = mid;
    }
    const int history = hist[b];
    if (!mla_prefill_live(cum[b + 1] - cum[b], history, max_q_len, kv_span)) return false;
    *seq = b, *pos = history + tok - cum[b];
    return true;
}

// a split's result for one (query row, head), o = this lane's dims 128 wave + 16 dt + 4 q + e: the only split stores the output
// itself, o / l in fp16; one of several its fp32 partial and (m, l) at slot bh * splits + split for mla_merge_kernel
__device__ __forceinline__ void mla_store_split(const floatx4 (&o)[8], float m, float l, size_t bh, int split, int splits, int wave, int q,
                                                half_t *__restrict__ o_lat, float *__restrict__ ws_o, float2 *__restrict__ ws_ml) {
    if (splits == 1) {
        const float inv = 1.f / l;
        half_t *op = o_lat + bh * kLat + 128 * wave + 4 * q;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
            const half4_t v = {from_f32<half_t>(o[dt][0] * inv), from_f32<half_t>(o[dt][1] * inv), from_f32<half_t>(o[dt][2] * inv),
                               from_f32<half_t>(o[dt][3] * inv)};
            *reinterpret_cast<half4_t *>(op + 16 * dt) = v;
        }
    } else {
        float *op = ws_o + (bh * splits + split) * kLat + 128 * wave + 4 * q;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) *reinterpret_cast<floatx4 *>(op + 16 * dt) = o[dt];
        if (wave == 0 && q == 0) ws_ml[bh * splits + split] = make_float2(m, l);
    }
}

inline bool mla_scale_ok(float scale) { return scale > 0.f && std::isfinite(scale); }   // softmax_scale, c_scale: positive and finite

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

inline int mla_max_ctx_check(const char *who, int max_ctx, int max_seq_len) {
    LLMIE_REQUIRE(max_ctx >= 0 && max_ctx <= max_seq_len, "%s: max_ctx=%d should be 0 (lengths known to the device only) or in [1, max_seq_len=%d]", who,
                  max_ctx, max_seq_len);
    return LLMIE_OK;
}

inline int mla_top_k_check(const char *who, int top_k) {
    LLMIE_REQUIRE(top_k >= 1 && top_k <= LLMIE_MLA_SPARSE_MAX_TOPK, "%s: top_k=%d should be in [1, %d]", who, top_k, LLMIE_MLA_SPARSE_MAX_TOPK);
    return LLMIE_OK;
}

// ---- the split plan the decode, the sparse decode and verify share (MlaSplitPlan, llmie_internal.h) ----
inline int mla_splits(int units) { return (units + kMlaChunk - 1) / kMlaChunk; }   // units: a context span, or top_k

// the partials of `slots` (sequence, query row) slots: per head and split o[512] in fp32, then (m, l); nothing with one split
inline size_t mla_partials_bytes(size_t slots, int head_num, int splits) {
    return splits > 1 ? slots * head_num * splits * (kLat + 2) * sizeof(float) : 0;
}

// fills the plan: `units` in chunks of kMlaChunk, one merge row per slot, grid z as given; false where the caller's workspace does
// not hold the partials (the caller words the refusal)
inline bool mla_split_plan(MlaSplitPlan *p, int units, int head_num, int slots, int grid_z, bool workspace, size_t workspace_bytes) {
    p->heads = kMlaHeads, p->tile = kMlaTile, p->chunk = kMlaChunk;
    p->grid[0] = mla_splits(units), p->grid[1] = head_num / kMlaHeads, p->grid[2] = grid_z;
    p->merge = p->grid[0] > 1;
    p->merge_grid[0] = head_num, p->merge_grid[1] = slots, p->merge_block = kMlaMergeBlock;
    p->workspace_bytes = mla_partials_bytes(slots, head_num, p->grid[0]);
    return p->workspace_bytes == 0 || (workspace && workspace_bytes >= p->workspace_bytes);
}

// the (m, l) pairs lie behind the slots x head_num x splits partial outputs; null with one split
inline float2 *mla_ws_ml(float *ws_o, const MlaSplitPlan &p) {
    return p.merge ? reinterpret_cast<float2 *>(ws_o + static_cast<size_t>(p.merge_grid[1]) * p.merge_grid[0] * p.grid[0] * kLat) : nullptr;
}

// the tail of the three plan texts: "merge 16x2/128", or "merge none"
inline void mla_merge_text(char *text, size_t size, const MlaSplitPlan &p) {
    if (p.merge) snprintf(text, size, "merge %dx%d/%d", p.merge_grid[0], p.merge_grid[1], p.merge_block);
    else snprintf(text, size, "merge none");
}

// where a layer begins, in units of row's: row = kRow (halves) or kRowE4 (bytes)
inline size_t mla_layer_off(int layer, int batch, int max_seq_len, bool paged, int num_pages, int row) {
    return static_cast<size_t>(layer) * (paged ? static_cast<size_t>(num_pages) * kPage : static_cast<size_t>(batch) * max_seq_len) * row;
}

}  // namespace llmie
