// Multi-head Latent Attention, decode step (DeepSeek-V2 / V3 / R1, Kimi-K2), in the absorbed form: the cache holds ONE row of
// 576 halves per token (512 latent dims c, 64 rotated k_pe dims), every query head attends over that row, and the per-head
// projections W_UK / W_UV are folded into the query and the output (include/llmie.h, llmie_mla_*).  Four launches per layer:
//   mla_kv_append_kernel    RMSNorm(c) * gamma  ||  rope(k_pe)  ->  cache row ctx - 1               (one wave per token)
//   mla_q_absorb_kernel     q_lat = (W_UK[h]^T q_nope) || rope(q_pe)                                (MFMA, W_UK staged once)
//   mla_decode_kernel       split-KV flash decode over the latent rows, 16 heads per workgroup      (MFMA, the hot path)
//   mla_merge_kernel        fixed-order merge of the split partials (only with more than one split)
//   mla_out_project_kernel  out[b, h] = W_UV[h] o_lat[b, h]                                         (MFMA, operands from registers)
//
// mla_decode_kernel.  Its tile loop, described here, is mla_split_tiles in mla_tile_loop.cuh, which mla_sparse_attend_kernel
// (mla_sparse.hip) runs too, over gathered rows.  Grid (splits, head_num / 16, batch), 4 waves.  A workgroup walks one chunk of kMlaChunk tokens of one
// sequence in tiles of kMlaTile = 32 keys.  A tile (32 rows x 576 halves) goes global -> registers -> LDS once and serves BOTH
// products from there: all 576 columns are the A operand of S^T = C . Q^T, the first 512 columns are -- read with the transposed
// LDS read ds_read_b64_tr_b16 -- the A operand of O^T += C^T . P^T.  Rows are padded to 592 halves (1184 bytes = 160 mod 256):
// the 4 rows x 32 bytes a 16-lane group of the transposed read addresses, and the 4 rows of the next group, fall into 8 different
// 32-byte bank groups.  Two tile buffers: tile t+1 is published while tile t is multiplied and tile t+2 is in flight in
// registers, one barrier per iteration for the staging (as prefill_flash_kernel) plus one for the logit exchange below.
//   S^T: wave (kh, kk) multiplies keys 16 kh .. +15 by dims 288 kk .. +287 (9 MFMA steps; its q fragments, 36 VGPRs, come from
//        global memory once) and leaves the partial logits in LDS (2 x 2 KB, fp32).
//   softmax: after the barrier EVERY wave adds the two partials of all 32 keys x 16 heads (8 values per lane, in exactly the
//        order the P^T operand wants them) and keeps the same running max / sum -- redundant, a few dozen VALU slots, and it
//        saves a second exchange of m, l and the fp16 P tile.
//   O^T: wave w accumulates output dims 128 w .. +127: 16 transposed reads, 8 MFMAs, 8 floatx4 accumulators.
// Rows of a tile at or past ctx re-read row ctx - 1 (same tile, same page) and their logits are -inf before the max; no load
// leaves the context and no block-table entry past (ctx - 1) / 128 is read.  The chunking depends on ctx alone, so a sequence's
// bits do not depend on the batch, its slot or the grid.  Plain softmax: out = sum p v / sum p, no epsilon in the denominator.
// The append, the decode and the merge kernel are templates that also serve the bulk append (mla_prefill.hip), the e4m3 cache
// (mla_e4m3.hip) and verify's merge (mla_verify.hip) through mla_append_launch, mla_decode_run and mla_merge_launch.
#include "mla_tile_loop.cuh"

#include <cstring>

namespace llmie {

namespace {

// ---- append: one wave per token.  cum == null: token = sequence b, row ctx_len[b] - 1; else the packed token blockIdx.x of the bulk
// form.  The row is mla_append_latent || mla_append_rope (mla_common.cuh) for both formats; E4: code = e4m3(fp16 / c_scale),
// saturated, the 640 bytes are put together in LDS and leave as 40 stores of 16 bytes. ----
template <bool E4, typename... Scale>
__global__ __launch_bounds__(64) void mla_kv_append_kernel(const half_t *__restrict__ kv_a, const half_t *__restrict__ gamma, float eps,
                                                           const float2 *__restrict__ rope, cache_elem_t<E4> *__restrict__ cache, size_t layer_off,
                                                           int max_seq_len, const int32_t *__restrict__ ctx_len, const int32_t *__restrict__ cum,
                                                           const int32_t *__restrict__ hist, int batch, int max_q_len, int kv_span,
                                                           const int32_t *__restrict__ table, int max_pages, const Scale... c_scale /* E4 */) {
    static_assert(sizeof...(Scale) == (E4 ? 1 : 0), "c_scale");
    const int tok = blockIdx.x, lane = threadIdx.x;
    int b = tok, pos;
    if (cum) {
        if (!mla_packed_locate(cum, hist, batch, tok, max_q_len, kv_span, &b, &pos)) return;
    } else {
        const int ctx = ctx_len[b];
        if (!mla_live(ctx, max_seq_len)) return;
        pos = ctx - 1;
    }
    const half_t *src = kv_a + static_cast<size_t>(tok) * kRow;
    const half8_t y = mla_append_latent(src, gamma, eps, lane);
    if constexpr (E4) {
        __shared__ __attribute__((aligned(16))) unsigned char Rs[kRowE4];
        float z[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = to_f32(y[j]) / pack_arg<0>(c_scale...);
        *reinterpret_cast<uint2 *>(Rs + 8 * lane) = make_uint2(pack4_e4m3(z[0], z[1], z[2], z[3]), pack4_e4m3(z[4], z[5], z[6], z[7]));
        if (lane < kRope / 2) mla_append_rope(src, rope, pos, lane, reinterpret_cast<half_t *>(Rs + kLat));
        __syncthreads();
        if (lane < kRowE4 / 16)
            *reinterpret_cast<uint4_t *>(cache + mla_row_off<kRowE4>(table, max_pages, layer_off, b, pos, max_seq_len) + 16 * lane) =
                *reinterpret_cast<const uint4_t *>(Rs + 16 * lane);
    } else {
        half_t *row = cache + mla_row_off<kRow>(table, max_pages, layer_off, b, pos, max_seq_len);
        *reinterpret_cast<half8_t *>(row + 8 * lane) = y;
        if (lane < kRope / 2) mla_append_rope(src, rope, pos, lane, row + kLat);
    }
}

// ---- q absorb: grid (4 column blocks of 128, head_num), 4 waves.  W_UK[h] (rows h * 256 .. + 127 of kv_b, [n][c]) is the
// [K, N] operand as stored: its 128 x 128 block goes to LDS once, each wave gathers the fragments of its 32 columns with the
// transposed read (8 fragments, kept in registers) and then walks the batch 16 rows at a time: O^T[c][b] = sum_n W[n][c] q[b][n].
// k index 8 q + j of a 32-step stands for n = 32 s + 16 (j >> 2) + 4 q + (j & 3) on both operands. ----
__global__ __launch_bounds__(256) void mla_q_absorb_kernel(const half_t *__restrict__ qin, const half_t *__restrict__ kv_b,
                                                           const float2 *__restrict__ rope, half_t *__restrict__ q_lat, int batch,
                                                           int head_num, int max_seq_len, const int32_t *__restrict__ ctx_len) {
    constexpr int WS = 128 + 16;   // 288-byte rows: 32 mod 256
    __shared__ __attribute__((aligned(16))) half_t Ws[kNope * WS];
    const int cb = blockIdx.x, h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const half_t *w = kv_b + static_cast<size_t>(h) * (kNope + kVd) * kLat + cb * 128;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int id = tid + 256 * i, n = id >> 4, ch = id & 15;
        *reinterpret_cast<half8_t *>(Ws + n * WS + ch * 8) = *reinterpret_cast<const half8_t *>(w + static_cast<size_t>(n) * kLat + ch * 8);
    }
    __syncthreads();
    half8_t wf[4][2];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            const half_t *blk = Ws + (32 * s + 4 * q + (r >> 2)) * WS + 32 * wave + 16 * dt + 4 * (r & 3);
            const fp16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(blk));
            const fp16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(blk + 16 * WS));
            wf[s][dt] = __builtin_bit_cast(half8_t, Tr8{lo, hi});
        }
    for (int bt = 0; bt < batch; bt += 16) {
        const int brow = min(bt + r, batch - 1);
        const half_t *qp = qin + (static_cast<size_t>(brow) * head_num + h) * kQ;
        half8_t pf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const half4_t lo = *reinterpret_cast<const half4_t *>(qp + 32 * s + 4 * q);
            const half4_t hi = *reinterpret_cast<const half4_t *>(qp + 32 * s + 16 + 4 * q);
            pf[s] = half8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
        const bool live = bt + r < batch && mla_live(ctx_len[brow], max_seq_len);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[s][dt], pf[s], acc, 0, 0, 0);
            if (live) {
                const half4_t v = {from_f32<half_t>(acc[0]), from_f32<half_t>(acc[1]), from_f32<half_t>(acc[2]), from_f32<half_t>(acc[3])};
                *reinterpret_cast<half4_t *>(q_lat + (static_cast<size_t>(brow) * head_num + h) * kRow + cb * 128 + 32 * wave + 16 * dt + 4 * q) = v;
            }
        }
    }
    if (cb == 0) {   // the rotated q_pe of this head, pairs (j, j + 32) at position ctx - 1
        for (int idx = tid; idx < batch * (kRope / 2); idx += 256) {
            const int b = idx / (kRope / 2), j = idx % (kRope / 2);
            const int ctx = ctx_len[b];
            if (!mla_live(ctx, max_seq_len)) continue;
            const float2 cs = rope[static_cast<size_t>(ctx - 1) * (kRope / 2) + j];
            const half_t *qp = qin + (static_cast<size_t>(b) * head_num + h) * kQ + kNope;
            half_t *dst = q_lat + (static_cast<size_t>(b) * head_num + h) * kRow + kLat;
            const float x0 = to_f32(qp[j]), x1 = to_f32(qp[j + kRope / 2]);
            dst[j] = from_f32<half_t>(x0 * cs.x - x1 * cs.y);
            dst[j + kRope / 2] = from_f32<half_t>(x1 * cs.x + x0 * cs.y);
        }
    }
}

// ---- out project: grid (head_num, 2), 4 waves of 16 value rows each.  W_UV[h] (rows h * 256 + 128 .. of kv_b, [v][c]) is the
// [N, K] operand as stored: a wave's 16 rows x 512 are 16 A fragments loaded straight into registers, once; the batch goes by
// 16 rows at a time (B fragments straight from o_lat).  No LDS. ----
__global__ __launch_bounds__(256) void mla_out_project_kernel(const half_t *__restrict__ o_lat, const half_t *__restrict__ kv_b,
                                                              half_t *__restrict__ out, int batch, int head_num) {
    const int h = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int vb = blockIdx.y * 64 + 16 * wave;
    const half_t *w = kv_b + (static_cast<size_t>(h) * (kNope + kVd) + kNope + vb + r) * kLat + 8 * q;
    half8_t af[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) af[s] = *reinterpret_cast<const half8_t *>(w + 32 * s);
    for (int bt = 0; bt < batch; bt += 16) {
        const int brow = min(bt + r, batch - 1);
        const half_t *op = o_lat + (static_cast<size_t>(brow) * head_num + h) * kLat + 8 * q;
        half8_t bf[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) bf[s] = *reinterpret_cast<const half8_t *>(op + 32 * s);
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[s], bf[s], acc, 0, 0, 0);
        if (bt + r < batch) {
            const half4_t v = {from_f32<half_t>(acc[0]), from_f32<half_t>(acc[1]), from_f32<half_t>(acc[2]), from_f32<half_t>(acc[3])};
            *reinterpret_cast<half4_t *>(out + (static_cast<size_t>(brow) * head_num + h) * kVd + vb + 4 * q) = v;
        }
    }
}

// ---- the attention: the tile loop is mla_split_tiles (mla_tile_loop.cuh, one template over the cache format and the row source) over
// the contiguous rows of positions t < ctx.  E4 = false: the fp16 cache, the argument list without c_scale; E4 = true: cache in bytes,
// layer_off in bytes.  The kernel decides what is its own: whether the sequence is live and which chunk this split walks. ----
template <bool E4, typename... Scale>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void mla_decode_kernel(
    const half_t *__restrict__ q_lat, const cache_elem_t<E4> *__restrict__ cache, half_t *__restrict__ o_lat, float *__restrict__ ws_o,
    float2 *__restrict__ ws_ml, const int32_t *__restrict__ ctx_len, const int32_t *__restrict__ table, int max_pages, size_t layer_off,
    int head_num, int max_seq_len, int max_ctx, float scale2 /* softmax_scale * log2(e) */, const Scale... c_scale /* E4 */) {
    const int b = blockIdx.z, ctx = ctx_len[b];
    if (!mla_live(ctx, max_ctx)) return;
    const int t_begin = blockIdx.x * kMlaChunk;
    if (t_begin >= ctx) return;
    mla_split_tiles<E4>(q_lat, MlaContiguousRows<E4>{cache + layer_off, table, max_pages, b, max_seq_len, t_begin, ctx}, o_lat, ws_o, ws_ml, b,
                        head_num, t_begin, ctx, scale2, c_scale...);
}

// merge: 128 threads x 4 dims per (query row, head).  Splits 0 .. ceil(ctx / chunk) - 1 in that order: M = max m_i,
// w_i = 2^(m_i - M), L = sum w_i l_i, out = (sum w_i o_i) / L.  One partial gives the bits of the one-split launch (w = 1).
// Decode: grid (head_num, batch), len_dev = ctx_len, no pack.  The sparse decode: len_dev = sel_count, span = top_k, the pack =
// (ctx_len, its bound max_seq_len), so that a sequence the attention kernel left alone for its dead context is left alone here.
// VERIFY: grid (head_num, batch x rows), len_dev = hist, the pack = (count_dev, rows); a partial that saw nothing (m = -inf, l = 0,
// o = 0) has weight 0, and the split that holds the row's own node is finite, so M is.
template <bool VERIFY, typename... Rows>
__global__ __launch_bounds__(kMlaMergeBlock) void mla_merge_kernel(const float *__restrict__ ws_o, const float2 *__restrict__ ws_ml,
                                                                   half_t *__restrict__ o_lat, const int32_t *__restrict__ len_dev, int head_num,
                                                                   int span, int splits,
                                                                   const Rows... vr /* VERIFY: count_dev, rows; sparse: live_dev, live_span */) {
    static_assert(sizeof...(Rows) == 2 || (!VERIFY && sizeof...(Rows) == 0), "count_dev, rows; or live_dev, live_span; or nothing");
    const int h = blockIdx.x, tid = threadIdx.x;
    int row = blockIdx.y, ctx;   // the (sequence, query row) slot, and the context its splits cover
    if constexpr (VERIFY) {
        const int rows = pack_arg<1>(vr...), b = row / rows;
        int hist, count;
        if (!verify_live(len_dev, pack_arg<0>(vr...), b, rows, span, &hist, &count) || row - b * rows >= count) return;
        ctx = hist + count;
    } else {
        ctx = len_dev[row];
        if (!mla_live(ctx, span)) return;
        if constexpr (sizeof...(Rows) == 2) {
            if (!mla_live(pack_arg<0>(vr...)[row], pack_arg<1>(vr...))) return;
        }
    }
    const int n = (ctx + kMlaChunk - 1) / kMlaChunk;   // <= splits (ctx <= span)
    const size_t bh = static_cast<size_t>(row) * head_num + h;
    float M = -INFINITY;
    for (int i = 0; i < n; ++i) M = fmaxf(M, ws_ml[bh * splits + i].x);
    float L = 0.f;
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < n; ++i) {
        const float2 ml = ws_ml[bh * splits + i];
        const float w = __builtin_amdgcn_exp2f(ml.x - M);
        L = __builtin_fmaf(w, ml.y, L);
        const floatx4 v = *reinterpret_cast<const floatx4 *>(ws_o + (bh * splits + i) * kLat + 4 * tid);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(w, v[e], acc[e]);
    }
    const float inv = 1.f / L;
    const half4_t v = {from_f32<half_t>(acc[0] * inv), from_f32<half_t>(acc[1] * inv), from_f32<half_t>(acc[2] * inv),
                       from_f32<half_t>(acc[3] * inv)};
    *reinterpret_cast<half4_t *>(o_lat + bh * kLat + 4 * tid) = v;
}

}  // namespace

// The one planner of llmie_mla_decode: every check that needs no pointer, then the launch.  Pure host code.
int plan_mla_decode(const char *who, const MlaDecodeCall &c, MlaDecodePlan *p) {
    int rc = mla_heads_check(who, c.batch, c.head_num);
    if (rc == LLMIE_OK) rc = mla_cache_check(who, c.max_seq_len, c.paged, c.max_pages, c.num_pages);
    if (rc == LLMIE_OK) rc = mla_max_ctx_check(who, c.max_ctx, c.max_seq_len);
    if (rc != LLMIE_OK) return rc;
    p->row_bytes = c.e4m3 ? kRowE4 : kRow * static_cast<int>(sizeof(half_t));
    p->span = c.max_ctx > 0 ? c.max_ctx : c.max_seq_len;
    if (!mla_split_plan(p, p->span, c.head_num, c.batch, c.batch, c.workspace, c.workspace_bytes)) {
        set_error("%s: workspace of %zu bytes, %d splits of %d tokens need %zu (llmie_mla_decode_workspace_bytes)", who,
                  c.workspace ? c.workspace_bytes : static_cast<size_t>(0), p->grid[0], kMlaChunk, p->workspace_bytes);
        return LLMIE_ERR_WORKSPACE;
    }
    return LLMIE_OK;
}

void mla_merge_launch(const MlaSplitPlan &p, int span, float *ws_o, half_t *o_lat, const int32_t *len_dev, const int32_t *count_dev, int rows,
                      const int32_t *live_dev, int live_span, hipStream_t st) {
    const dim3 grid(p.merge_grid[0], p.merge_grid[1]), block(p.merge_block);
    const int head_num = p.merge_grid[0], splits = p.grid[0];
    const float2 *ws_ml = mla_ws_ml(ws_o, p);
    if (rows)
        hipLaunchKernelGGL((mla_merge_kernel<true, const int32_t *, int>), grid, block, 0, st, ws_o, ws_ml, o_lat, len_dev, head_num, span, splits, count_dev,
                           rows);
    else if (live_dev)
        hipLaunchKernelGGL((mla_merge_kernel<false, const int32_t *, int>), grid, block, 0, st, ws_o, ws_ml, o_lat, len_dev, head_num, span, splits,
                           live_dev, live_span);
    else hipLaunchKernelGGL(mla_merge_kernel<false>, grid, block, 0, st, ws_o, ws_ml, o_lat, len_dev, head_num, span, splits);
}

void mla_append_launch(const MlaAppendCall &a, int tokens, hipStream_t st) {
    const size_t layer_off = mla_layer_off(a.layer, a.batch, a.max_seq_len, a.block_table != nullptr, a.num_pages, a.e4m3 ? kRowE4 : kRow);
    const half_t *kv_a = static_cast<const half_t *>(a.kv_a), *gamma = static_cast<const half_t *>(a.gamma);
    const float2 *rope = static_cast<const float2 *>(a.rope);
    if (a.e4m3)
        hipLaunchKernelGGL((mla_kv_append_kernel<true, float>), dim3(tokens), dim3(64), 0, st, kv_a, gamma, a.eps, rope, static_cast<unsigned char *>(a.cache),
                           layer_off, a.max_seq_len, a.ctx_len, a.cum, a.hist, a.batch, a.max_q_len, a.kv_span, a.block_table, a.max_pages, a.c_scale);
    else
        hipLaunchKernelGGL(mla_kv_append_kernel<false>, dim3(tokens), dim3(64), 0, st, kv_a, gamma, a.eps, rope, static_cast<half_t *>(a.cache), layer_off,
                           a.max_seq_len, a.ctx_len, a.cum, a.hist, a.batch, a.max_q_len, a.kv_span, a.block_table, a.max_pages);
}

int mla_decode_run(const char *who, const MlaDecodeCall &c, const MlaDecodeIo &io, hipStream_t st) {
    LLMIE_REQUIRE(io.q_lat && io.cache && io.o_lat && io.ctx_len, "%s: NULL operand", who);
    LLMIE_REQUIRE(io.layer >= 0, "%s: layer=%d should be >= 0", who, io.layer);
    LLMIE_REQUIRE(mla_scale_ok(io.softmax_scale), "%s: softmax_scale should be positive and finite", who);
    if (c.e4m3) LLMIE_REQUIRE(mla_scale_ok(io.c_scale), "%s: c_scale should be positive and finite", who);
    MlaDecodePlan p{};
    const int rc = plan_mla_decode(who, c, &p);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(mis16(io.q_lat) == 0 && mis16(io.cache) == 0 && mis16(io.o_lat) == 0 && (!p.merge || mis16(io.workspace) == 0),
                  "%s: q_lat, the cache, o_lat and the workspace should be 16-byte aligned", who);
    const half_t *q_lat = static_cast<const half_t *>(io.q_lat);
    half_t *o_lat = static_cast<half_t *>(io.o_lat);
    float *ws_o = static_cast<float *>(io.workspace);
    float2 *ws_ml = mla_ws_ml(ws_o, p);
    const size_t layer_off = mla_layer_off(io.layer, c.batch, c.max_seq_len, c.paged, c.num_pages, c.e4m3 ? kRowE4 : kRow);
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]);
    if (c.e4m3)
        hipLaunchKernelGGL((mla_decode_kernel<true, float>), grid, dim3(256), 0, st, q_lat, static_cast<const unsigned char *>(io.cache), o_lat, ws_o, ws_ml,
                           io.ctx_len, io.block_table, c.max_pages, layer_off, c.head_num, c.max_seq_len, p.span, io.softmax_scale * kLog2e, io.c_scale);
    else
        hipLaunchKernelGGL(mla_decode_kernel<false>, grid, dim3(256), 0, st, q_lat, static_cast<const half_t *>(io.cache), o_lat, ws_o, ws_ml, io.ctx_len,
                           io.block_table, c.max_pages, layer_off, c.head_num, c.max_seq_len, p.span, io.softmax_scale * kLog2e);
    if (p.merge) mla_merge_launch(p, p.span, ws_o, o_lat, io.ctx_len, nullptr, 0, nullptr, 0, st);
    return launch_status(who);
}

const char *mla_decode_plan_text(const char *who, const MlaDecodeCall &c, char *text, size_t size, int *status) {
    MlaDecodePlan p{};
    const int rc = plan_mla_decode(who, c, &p);
    if (status) *status = rc;
    if (rc != LLMIE_OK) return nullptr;
    int n = snprintf(text, size, "mla %s nh%d hb%d tile%d chunk%d ", c.e4m3 ? "e4m3" : "f16", c.head_num, p.heads, p.tile, p.chunk);
    if (c.e4m3) n += snprintf(text + n, size - n, "row%d ", p.row_bytes);
    n += snprintf(text + n, size - n, "grid %dx%dx%d ", p.grid[0], p.grid[1], p.grid[2]);
    mla_merge_text(text + n, size - n, p);
    return text;
}

}  // namespace llmie

using namespace llmie;

extern "C" size_t llmie_mla_decode_workspace_bytes(int batch, int head_num, int max_seq_len) {
    if (batch < 1 || head_num < 1 || max_seq_len < 1) return 0;
    return mla_partials_bytes(batch, head_num, mla_splits(max_seq_len));
}

extern "C" const char *llmie_mla_decode_plan(int batch, int head_num, int max_seq_len, int max_ctx, int paged, int max_pages, int num_pages,
                                             long long workspace_bytes, int *status) {
    static thread_local char text[160];
    const MlaDecodeCall c{batch, head_num, max_seq_len, max_ctx, paged != 0, max_pages, num_pages, workspace_bytes >= 0,
                          workspace_bytes >= 0 ? static_cast<size_t>(workspace_bytes) : 0};
    return mla_decode_plan_text("mla_decode_plan", c, text, sizeof(text), status);
}

extern "C" int llmie_mla_kv_append(const void *kv_a, const void *gamma, float eps, const void *rope_table, void *cache, int layer, int batch,
                                   int max_seq_len, const int32_t *ctx_len_dev, const int32_t *block_table, int max_pages, int num_pages,
                                   llmie_stream stream) {
    LLMIE_REQUIRE(kv_a && gamma && rope_table && cache && ctx_len_dev, "mla_kv_append: NULL operand");
    LLMIE_REQUIRE(batch >= 1 && layer >= 0, "mla_kv_append: batch=%d should be >= 1 and layer=%d >= 0", batch, layer);
    LLMIE_REQUIRE(eps > 0.f, "mla_kv_append: eps should be > 0");
    const int rc = mla_cache_check("mla_kv_append", max_seq_len, block_table != nullptr, max_pages, num_pages);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(mis16(kv_a) == 0 && mis16(gamma) == 0 && mis16(cache) == 0, "mla_kv_append: kv_a, gamma and the cache should be 16-byte aligned");
    mla_append_launch(MlaAppendCall{kv_a, gamma, eps, rope_table, cache, layer, batch, max_seq_len, ctx_len_dev, nullptr, nullptr, 0, 0, block_table,
                                    max_pages, num_pages},
                      batch, as_stream(stream));
    return launch_status("mla_kv_append");
}

extern "C" int llmie_mla_q_absorb(const void *q, const void *kv_b, const void *rope_table, void *q_lat, int batch, int head_num, int max_seq_len,
                                  const int32_t *ctx_len_dev, llmie_stream stream) {
    LLMIE_REQUIRE(q && kv_b && rope_table && q_lat && ctx_len_dev, "mla_q_absorb: NULL operand");
    const int rc = mla_heads_check("mla_q_absorb", batch, head_num);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(max_seq_len >= 1, "mla_q_absorb: max_seq_len=%d should be >= 1", max_seq_len);
    LLMIE_REQUIRE(mis16(q) == 0 && mis16(kv_b) == 0 && mis16(q_lat) == 0, "mla_q_absorb: q, kv_b and q_lat should be 16-byte aligned");
    hipLaunchKernelGGL(mla_q_absorb_kernel, dim3(kLat / 128, head_num), dim3(256), 0, as_stream(stream), static_cast<const half_t *>(q),
                       static_cast<const half_t *>(kv_b), static_cast<const float2 *>(rope_table), static_cast<half_t *>(q_lat), batch, head_num,
                       max_seq_len, ctx_len_dev);
    return launch_status("mla_q_absorb");
}

extern "C" int llmie_mla_decode(const void *q_lat, const void *cache, void *o_lat, int layer, int batch, int head_num, int max_seq_len, int max_ctx,
                                const int32_t *ctx_len_dev, float softmax_scale, void *workspace, size_t workspace_bytes,
                                const int32_t *block_table, int max_pages, int num_pages, llmie_stream stream) {
    const MlaDecodeCall c{batch, head_num, max_seq_len, max_ctx, block_table != nullptr, max_pages, num_pages, workspace != nullptr, workspace_bytes};
    return mla_decode_run("mla_decode", c, MlaDecodeIo{q_lat, cache, o_lat, layer, ctx_len_dev, block_table, softmax_scale, workspace}, as_stream(stream));
}

extern "C" int llmie_mla_out_project(const void *o_lat, const void *kv_b, void *out, int batch, int head_num, llmie_stream stream) {
    LLMIE_REQUIRE(o_lat && kv_b && out, "mla_out_project: NULL operand");
    const int rc = mla_heads_check("mla_out_project", batch, head_num);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(mis16(o_lat) == 0 && mis16(kv_b) == 0 && mis16(out) == 0, "mla_out_project: o_lat, kv_b and out should be 16-byte aligned");
    hipLaunchKernelGGL(mla_out_project_kernel, dim3(head_num, kVd / 64), dim3(256), 0, as_stream(stream), static_cast<const half_t *>(o_lat),
                       static_cast<const half_t *>(kv_b), static_cast<half_t *>(out), batch, head_num);
    return launch_status("mla_out_project");
}
