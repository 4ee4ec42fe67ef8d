// Multi-head Latent Attention, SPARSE decode step (DeepSeek-V3.2, "DeepSeek Sparse Attention"; include/llmie.h llmie_mla_index_topk,
// llmie_mla_decode_sparse): a small indexer scores every cached token, I_t = sum_h w_h relu(q_idx_h . k_idx_t) over 64 index heads of
// 128 dims, and the attention of mla.hip runs over the top_k best-scoring latent rows only.  Three kernels:
//   mla_index_logits_kernel   I_t of every position t < ctx into an fp32 workspace row                (MFMA, no LDS, HBM-bound)
//   mla_index_select_kernel   exact top_k of a row: radix select, then one ordered compaction          (one workgroup per sequence)
//   mla_sparse_attend_kernel  the split-KV flash decode of mla_decode_kernel over sel[b, 0 .. count)    (MFMA, the hot path)
// and the merge is mla.hip's (mla_merge_launch, with sel_count as the length array and ctx_len for the liveness).
//
// mla_index_logits_kernel.  Grid (ceil(span / 64), batch), 4 waves of 16 keys.  The key rows are the A operand straight from global
// memory -- lane (r, q) reads row r at halves 32 s + 8 q .. for the 4 steps --, q_idx[b] is the B operand: 16 fragments (4 head blocks
// x 4 steps, 64 VGPRs) loaded once and kept.  16 MFMAs leave acc[cb][e] = key 4 q + e . head 16 cb + r.  The summation order is FIXED
// and does not depend on where a key sits: v = max(acc[0], 0) * w[r], then v = fma(max(acc[cb], 0), w[16 cb + r], v) for cb = 1, 2, 3,
// then the xor butterfly v += v[lane ^ d] over d = 8, 4, 2, 1.  So equal key rows give equal logit bits, whatever their positions.
// 16 divides 128: a wave's keys never cross a page, one wave-uniform page lookup per 16 keys.  Keys at or past ctx re-read row ctx - 1
// and are not stored; waves past the context, and sequences with ctx <= top_k (their selection is the identity), exit.
//
// mla_index_select_kernel.  1024 threads per sequence.  A logit becomes an order-preserving unsigned key (NaN below every number,
// -0 = +0); four 8-bit passes, most significant byte first, histogram the keys that share the prefix found so far (LDS atomics on 8
// bank-staggered copies of the 256 bins) and fix the next byte of the threshold key T and `need`, the number of keys equal to T to
// admit.  One more pass emits, in ascending position, every key > T and the first `need` keys = T: a workgroup prefix scan of the packed
// pair (count of keys > T, count of keys = T) over 4096 positions at a time.  No global atomics, plain stores.
//
// mla_sparse_attend_kernel.  Grid (ceil(top_k / 256), head_num / 16, batch): the kernel runs the tile loop of mla_decode_kernel, the
// one text of it (mla_split_tiles in mla_tile_loop.cuh; mla.hip says how it works), with the gathered row source, over entries
// j < count = min(sel_count[b], top_k) instead of positions t < ctx.  What is the kernel's own is the row locate: the 32
// rows of a staged tile no longer share a base, so at its start a workgroup resolves its chunk's up to 256 row numbers inside the layer
// ONCE, into 1 KB of LDS (one sel read and one block-table read per row), and the tile loop's fetch has one LDS read in front of each
// 16-byte global load, no dependent sel -> table -> row chain.  Every position is clamped into [0, ctx - 1]: a negative entry or one
// >= ctx inside count is the caller's error, it attends the clamped row and nothing faults.  Entries at or past count re-read entry
// count - 1 and are masked to -inf in the last tile only.  With sel = 0 .. ctx - 1 the result has the bits of llmie_mla_decode.
#include "mla_tile_loop.cuh"

namespace llmie {

namespace {

constexpr int kIdxHeads = LLMIE_MLA_INDEX_HEADS, kIdxDim = LLMIE_MLA_INDEX_DIM, kIdxKeys = 64, kIdxPad = 256;
constexpr int kSelThreads = 1024, kSelSpan = 4 * kSelThreads, kSelCopies = 8, kSelBins = 256;
static_assert(kIdxHeads == 64 && kIdxDim == 128, "the indexer kernel is written for 64 heads of 128 dims");
static_assert(kPage % 16 == 0 && kIdxPad % 4 == 0, "a wave's 16 keys share a page; the select reads 4 logits at a time");

__global__ __launch_bounds__(256) void mla_index_logits_kernel(const half_t *__restrict__ q_idx, const float *__restrict__ w_idx,
                                                               const half_t *__restrict__ k_idx, float *__restrict__ logits,
                                                               float *__restrict__ logits_out, const int32_t *__restrict__ ctx_len,
                                                               const int32_t *__restrict__ table, int max_pages, size_t layer_off,
                                                               int max_seq_len, int span, size_t pitch, int top_k) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int ctx = ctx_len[b];
    if (!mla_live(ctx, span) || ctx <= top_k) return;
    const int k0 = blockIdx.x * kIdxKeys + 16 * wave;
    if (k0 >= ctx) return;

    half8_t qf[4][4];   // q_idx[b][head 16 cb + r][32 s + 8 q ..]
    float w[4];
    {
        const half_t *qp = q_idx + (static_cast<size_t>(b) * kIdxHeads + r) * kIdxDim + 8 * q;
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) {
#pragma unroll
            for (int s = 0; s < 4; ++s) qf[cb][s] = *reinterpret_cast<const half8_t *>(qp + cb * 16 * kIdxDim + 32 * s);
            w[cb] = w_idx[b * kIdxHeads + 16 * cb + r];
        }
    }
    const int t = min(k0 + r, ctx - 1);   // >= k0: the same 16 keys, the same page
    const half_t *kp = k_idx + layer_off + (mla_tile_row0(table, max_pages, b, k0, max_seq_len) + (t - k0)) * kIdxDim + 8 * q;
    half8_t kf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) kf[s] = *reinterpret_cast<const half8_t *>(kp + 32 * s);
    floatx4 acc[4];
#pragma unroll
    for (int cb = 0; cb < 4; ++cb) {
        acc[cb] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[s], qf[cb][s], acc[cb], 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float v = fmaxf(acc[0][e], 0.f) * w[0];
#pragma unroll
        for (int cb = 1; cb < 4; ++cb) v = __builtin_fmaf(fmaxf(acc[cb][e], 0.f), w[cb], v);
        v = lane_xor_sum<8>(v);
        v = lane_xor_sum<4>(v);
        v = lane_xor_sum<2>(v);
        v = lane_xor_sum<1>(v);
        const int key = k0 + 4 * q + e;
        if (r == 0 && key < ctx) {
            logits[b * pitch + key] = v;
            if (logits_out) logits_out[static_cast<size_t>(b) * span + key] = v;
        }
    }
}

// larger logit <=> larger key; NaN = 0 lies below every number (the key of -inf is 0x007fffff), -0 and +0 share a key
__device__ __forceinline__ unsigned mla_index_key(float x) {
    unsigned u = __builtin_bit_cast(unsigned, x);
    if (x != x) return 0u;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(kSelThreads) void mla_index_select_kernel(const float *__restrict__ logits, int32_t *__restrict__ sel,
                                                                       int32_t *__restrict__ sel_count, const int32_t *__restrict__ ctx_len,
                                                                       int span, size_t pitch, int top_k) {
    __shared__ unsigned hist[kSelCopies * (kSelBins + 1)];   // copy c at c * 257: the same bin of two copies in two banks
    __shared__ unsigned bins[kSelBins], pick[2], wave_total[kSelThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ctx = ctx_len[b];
    int32_t *out = sel + static_cast<size_t>(b) * top_k;
    if (!mla_live(ctx, span)) {
        if (tid == 0) sel_count[b] = 0;
        return;
    }
    if (ctx <= top_k) {   // everything is selected: no logit is read
        for (int j = tid; j < top_k; j += kSelThreads) out[j] = j < ctx ? j : -1;
        if (tid == 0) sel_count[b] = ctx;
        return;
    }
    const float *lg = logits + b * pitch;   // positions 4 i .. 4 i + 3 < pitch are readable, those < ctx are written

    unsigned prefix = 0u, need = top_k;   // the threshold key's bytes found so far; how many keys of the remaining set to take
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < kSelCopies * (kSelBins + 1); i += kSelThreads) hist[i] = 0u;
        __syncthreads();
        const unsigned himask = shift == 24 ? 0u : ~0u << (shift + 8);
        unsigned *mine = hist + (lane & (kSelCopies - 1)) * (kSelBins + 1);
        for (int t0 = 4 * tid; t0 < ctx; t0 += kSelSpan) {
            const floatx4 v = *reinterpret_cast<const floatx4 *>(lg + t0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned key = mla_index_key(v[e]);
                if (t0 + e < ctx && (key & himask) == prefix) atomicAdd(mine + ((key >> shift) & (kSelBins - 1)), 1u);
            }
        }
        __syncthreads();
        if (tid < kSelBins) {
            unsigned n = 0u;
#pragma unroll
            for (int c = 0; c < kSelCopies; ++c) n += hist[c * (kSelBins + 1) + tid];
            bins[tid] = n;
        }
        __syncthreads();
        if (tid < kSelBins) {   // the one bin d with count(bins > d) < need <= count(bins >= d)
            unsigned above = 0u;
            for (int j = tid + 1; j < kSelBins; ++j) above += bins[j];
            if (above < need && need <= above + bins[tid]) pick[0] = tid, pick[1] = need - above;
        }
        __syncthreads();
        prefix |= pick[0] << shift;
        need = pick[1];
    }

    // prefix = the threshold key T; need = how many of the keys equal to T are taken: those at the lowest positions
    unsigned gt_base = 0u, eq_base = 0u;   // keys > T / = T in front of this round's positions
    for (int c0 = 0; c0 < ctx; c0 += kSelSpan) {
        const int t0 = c0 + 4 * tid;
        bool gt[4] = {false, false, false, false}, eq[4] = {false, false, false, false};
        unsigned cnt = 0u;   // (keys > T) << 16 | (keys = T) of this thread's four positions
        if (t0 < ctx) {
            const floatx4 v = *reinterpret_cast<const floatx4 *>(lg + t0);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned key = mla_index_key(v[e]);
                gt[e] = t0 + e < ctx && key > prefix;
                eq[e] = t0 + e < ctx && key == prefix;
                cnt += (gt[e] ? 0x10000u : 0u) + (eq[e] ? 1u : 0u);
            }
        }
        unsigned inc = cnt;   // inclusive scan over the wave, then the waves in front
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(inc, d, 64);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wave_total[wave] = inc;
        __syncthreads();
        unsigned before = inc - cnt, total = 0u;
#pragma unroll
        for (int i = 0; i < kSelThreads / 64; ++i) {
            const unsigned x = wave_total[i];
            before += i < wave ? x : 0u;
            total += x;
        }
        unsigned g = gt_base + (before >> 16), q = eq_base + (before & 0xffffu);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (gt[e]) out[g + min(q, need)] = t0 + e, ++g;
            else if (eq[e]) {
                if (q < need) out[g + q] = t0 + e;
                ++q;
            }
        }
        gt_base += total >> 16, eq_base += total & 0xffffu;
        __syncthreads();   // wave_total is rewritten
    }
    if (tid == 0) sel_count[b] = top_k;
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void mla_sparse_attend_kernel(
    const half_t *__restrict__ q_lat, const half_t *__restrict__ cache, half_t *__restrict__ o_lat, float *__restrict__ ws_o,
    float2 *__restrict__ ws_ml, const int32_t *__restrict__ sel, const int32_t *__restrict__ sel_count, const int32_t *__restrict__ ctx_len,
    const int32_t *__restrict__ table, int max_pages, size_t layer_off, int head_num, int top_k, int max_seq_len,
    float scale2 /* softmax_scale * log2(e) */) {
    __shared__ int Rw[kMlaChunk];   // the chunk's row numbers inside the layer
    const int b = blockIdx.z, tid = threadIdx.x;
    const int ctx = ctx_len[b], count = min(sel_count[b], top_k);
    const int j_begin = blockIdx.x * kMlaChunk;
    // a dead context (the merge launch tests the same: nothing writes the row), or nothing to do (count < 1 included); one test
    // (`|`): both lengths are loaded side by side
    if (!mla_live(ctx, max_seq_len) | (j_begin >= count)) return;
    {   // locate: entry j_begin + tid, one past the last re-reads the last; the position is clamped into the sequence
        const int pos = min(max(sel[static_cast<size_t>(b) * top_k + min(j_begin + tid, count - 1)], 0), ctx - 1);
        Rw[tid] = table ? table[static_cast<size_t>(b) * max_pages + pos / kPage] * kPage + pos % kPage : b * max_seq_len + pos;
    }
    // (the barrier behind these writes is MlaGatheredRows::ready(), behind the loop's q loads)
    mla_split_tiles<false>(q_lat, MlaGatheredRows{cache + layer_off, Rw}, o_lat, ws_o, ws_ml, b, head_num, j_begin, count, scale2);
}

size_t index_pitch(int span) { return (static_cast<size_t>(span) + kIdxPad - 1) / kIdxPad * kIdxPad; }

}  // namespace

// The one planner of llmie_mla_index_topk: every check that needs no pointer, then the two launches.  Pure host code.
int plan_mla_index_topk(const char *who, const MlaIndexCall &c, MlaIndexPlan *p) {
    LLMIE_REQUIRE(c.batch >= 1 && c.batch <= 65535, "%s: batch=%d should be in [1, 65535]", who, c.batch);
    int rc = mla_top_k_check(who, c.top_k);
    if (rc == LLMIE_OK) rc = mla_cache_check(who, c.max_seq_len, c.paged, c.max_pages, c.num_pages);
    if (rc == LLMIE_OK) rc = mla_max_ctx_check(who, c.max_ctx, c.max_seq_len);
    if (rc != LLMIE_OK) return rc;
    p->keys = kIdxKeys;
    p->span = c.max_ctx > 0 ? c.max_ctx : c.max_seq_len;
    p->pitch = index_pitch(p->span);
    p->logits = p->span > c.top_k;   // no context above top_k: every selection is the identity
    p->grid[0] = (p->span + kIdxKeys - 1) / kIdxKeys, p->grid[1] = c.batch;
    p->select_grid = c.batch, p->select_block = kSelThreads;
    p->workspace_bytes = p->logits ? static_cast<size_t>(c.batch) * p->pitch * sizeof(float) : 0;
    if (p->workspace_bytes > 0 && (!c.workspace || c.workspace_bytes < p->workspace_bytes)) {
        set_error("%s: workspace of %zu bytes, %d rows of %zu logits need %zu (llmie_mla_index_topk_workspace_bytes)", who,
                  c.workspace ? c.workspace_bytes : static_cast<size_t>(0), c.batch, p->pitch, p->workspace_bytes);
        return LLMIE_ERR_WORKSPACE;
    }
    return LLMIE_OK;
}

// The one planner of llmie_mla_decode_sparse.  Pure host code.
int plan_mla_decode_sparse(const char *who, const MlaSparseCall &c, MlaSparsePlan *p) {
    int rc = mla_heads_check(who, c.batch, c.head_num);
    if (rc == LLMIE_OK) rc = mla_cache_check(who, c.max_seq_len, c.paged, c.max_pages, c.num_pages);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(c.batch <= 65535, "%s: batch=%d should be <= 65535", who, c.batch);
    rc = mla_top_k_check(who, c.top_k);
    if (rc != LLMIE_OK) return rc;
    const long long rows = c.paged ? static_cast<long long>(c.num_pages) * kPage : static_cast<long long>(c.batch) * c.max_seq_len;
    if (rows > 2147483647LL) LLMIE_UNSUPPORTED("%s: a layer of %lld cache rows: the row numbers of a selection are 32 bits, at most 2^31 - 1 rows", who, rows);
    if (!mla_split_plan(p, c.top_k, c.head_num, c.batch, c.batch, c.workspace, c.workspace_bytes)) {
        set_error("%s: workspace of %zu bytes, %d splits of %d entries need %zu (llmie_mla_decode_workspace_bytes with top_k)", who,
                  c.workspace ? c.workspace_bytes : static_cast<size_t>(0), p->grid[0], kMlaChunk, p->workspace_bytes);
        return LLMIE_ERR_WORKSPACE;
    }
    return LLMIE_OK;
}

}  // namespace llmie

using namespace llmie;

extern "C" size_t llmie_mla_index_topk_workspace_bytes(int batch, int max_seq_len) {
    if (batch < 1 || max_seq_len < 1) return 0;
    return static_cast<size_t>(batch) * index_pitch(max_seq_len) * sizeof(float);
}

extern "C" const char *llmie_mla_index_topk_plan(int batch, int top_k, int max_seq_len, int max_ctx, int paged, int max_pages, int num_pages,
                                                 long long workspace_bytes, int *status) {
    static thread_local char text[160];
    const MlaIndexCall c{batch, top_k, max_seq_len, max_ctx, paged != 0, max_pages, num_pages, workspace_bytes >= 0,
                         workspace_bytes >= 0 ? static_cast<size_t>(workspace_bytes) : 0};
    MlaIndexPlan p{};
    const int rc = plan_mla_index_topk("mla_index_topk_plan", c, &p);
    if (status) *status = rc;
    if (rc != LLMIE_OK) return nullptr;
    int n = snprintf(text, sizeof(text), "mla_index f16 ih%d id%d keys%d topk%d grid ", kIdxHeads, kIdxDim, p.keys, top_k);
    if (p.logits) n += snprintf(text + n, sizeof(text) - n, "%dx%d", p.grid[0], p.grid[1]);
    else n += snprintf(text + n, sizeof(text) - n, "none");
    snprintf(text + n, sizeof(text) - n, " select %dx%d", p.select_grid, p.select_block);
    return text;
}

extern "C" int llmie_mla_index_topk(const void *q_idx, const float *w_idx, const void *k_idx_cache, int32_t *sel, int32_t *sel_count,
                                    float *logits_out, int layer, int batch, int top_k, int max_seq_len, int max_ctx, const int32_t *ctx_len_dev,
                                    void *workspace, size_t workspace_bytes, const int32_t *block_table, int max_pages, int num_pages,
                                    llmie_stream stream) {
    LLMIE_REQUIRE(q_idx && w_idx && k_idx_cache && sel && sel_count && ctx_len_dev, "mla_index_topk: NULL operand");
    LLMIE_REQUIRE(layer >= 0, "mla_index_topk: layer=%d should be >= 0", layer);
    const bool paged = block_table != nullptr;
    MlaIndexPlan p{};
    const int rc = plan_mla_index_topk("mla_index_topk", MlaIndexCall{batch, top_k, max_seq_len, max_ctx, paged, max_pages, num_pages,
                                                                       workspace != nullptr, workspace_bytes}, &p);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(mis16(q_idx) == 0 && mis16(k_idx_cache) == 0 && (!p.logits || mis16(workspace) == 0),
                  "mla_index_topk: q_idx, the index cache and the workspace should be 16-byte aligned");
    float *logits = static_cast<float *>(workspace);
    const hipStream_t st = as_stream(stream);
    if (p.logits)
        hipLaunchKernelGGL(mla_index_logits_kernel, dim3(p.grid[0], p.grid[1]), dim3(256), 0, st, static_cast<const half_t *>(q_idx), w_idx,
                           static_cast<const half_t *>(k_idx_cache), logits, logits_out, ctx_len_dev, block_table, max_pages,
                           mla_layer_off(layer, batch, max_seq_len, paged, num_pages, kIdxDim), max_seq_len, p.span, p.pitch, top_k);
    hipLaunchKernelGGL(mla_index_select_kernel, dim3(p.select_grid), dim3(p.select_block), 0, st, logits, sel, sel_count, ctx_len_dev, p.span,
                       p.pitch, top_k);
    return launch_status("mla_index_topk");
}

extern "C" const char *llmie_mla_decode_sparse_plan(int batch, int head_num, int top_k, int max_seq_len, int paged, int max_pages, int num_pages,
                                                    long long workspace_bytes, int *status) {
    static thread_local char text[160];
    const MlaSparseCall c{batch, head_num, top_k, max_seq_len, paged != 0, max_pages, num_pages, workspace_bytes >= 0,
                          workspace_bytes >= 0 ? static_cast<size_t>(workspace_bytes) : 0};
    MlaSparsePlan p{};
    const int rc = plan_mla_decode_sparse("mla_decode_sparse_plan", c, &p);
    if (status) *status = rc;
    if (rc != LLMIE_OK) return nullptr;
    const int n = snprintf(text, sizeof(text), "mla_sparse f16 nh%d hb%d tile%d chunk%d topk%d grid %dx%dx%d ", head_num, p.heads, p.tile, p.chunk,
                           top_k, p.grid[0], p.grid[1], p.grid[2]);
    mla_merge_text(text + n, sizeof(text) - n, p);
    return text;
}

extern "C" int llmie_mla_decode_sparse(const void *q_lat, const void *cache, void *o_lat, const int32_t *sel, const int32_t *sel_count, int layer,
                                       int batch, int head_num, int top_k, int max_seq_len, const int32_t *ctx_len_dev, float softmax_scale,
                                       void *workspace, size_t workspace_bytes, const int32_t *block_table, int max_pages, int num_pages,
                                       llmie_stream stream) {
    LLMIE_REQUIRE(q_lat && cache && o_lat && sel && sel_count && ctx_len_dev, "mla_decode_sparse: NULL operand");
    LLMIE_REQUIRE(layer >= 0, "mla_decode_sparse: layer=%d should be >= 0", layer);
    LLMIE_REQUIRE(mla_scale_ok(softmax_scale), "mla_decode_sparse: softmax_scale should be positive and finite");
    const bool paged = block_table != nullptr;
    MlaSparsePlan p{};
    const int rc = plan_mla_decode_sparse("mla_decode_sparse", MlaSparseCall{batch, head_num, top_k, max_seq_len, paged, max_pages, num_pages,
                                                                             workspace != nullptr, workspace_bytes}, &p);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(mis16(q_lat) == 0 && mis16(cache) == 0 && mis16(o_lat) == 0 && (!p.merge || mis16(workspace) == 0),
                  "mla_decode_sparse: q_lat, the cache, o_lat and the workspace should be 16-byte aligned");
    half_t *out = static_cast<half_t *>(o_lat);
    float *ws_o = static_cast<float *>(workspace);
    float2 *ws_ml = mla_ws_ml(ws_o, p);
    const hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(mla_sparse_attend_kernel, dim3(p.grid[0], p.grid[1], p.grid[2]), dim3(256), 0, st, static_cast<const half_t *>(q_lat),
                       static_cast<const half_t *>(cache), out, ws_o, ws_ml, sel, sel_count, ctx_len_dev, block_table, max_pages,
                       mla_layer_off(layer, batch, max_seq_len, paged, num_pages, kRow), head_num, top_k, max_seq_len, softmax_scale * kLog2e);
    if (p.merge) mla_merge_launch(p, top_k, ws_o, out, sel_count, nullptr, 0, ctx_len_dev, max_seq_len, st);
    return launch_status("mla_decode_sparse");
}
