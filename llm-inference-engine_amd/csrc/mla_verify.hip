// Multi-head Latent Attention, speculative verify: several query rows per sequence -- a chain of draft tokens or a draft tree -- attend
// over the latent cache in the absorbed form, in ONE pass over the history (include/llmie.h, llmie_mla_verify).  The nodes' rows are
// already in the cache at slots hist + i; row i sees every key t < hist and the nodes hist + j whose bit j is set in its ancestor mask
// (the convention of llmie_decoder_set_tree; no mask array = the chain).  Two launches:
//   mla_verify_kernel        split-KV flash attention, 16 heads x kVerRows query rows = 64 MFMA columns per workgroup   (the hot path)
//   mla_merge_kernel         (mla.hip, mla_merge_launch) fixed-order merge of the split partials (only with more than one split)
//
// mla_verify_kernel.  Grid (splits, head_num / 16, batch x ceil(rows / kVerRows)), 4 waves, one workgroup per CU on the unified
// 512-register file.  A workgroup walks one chunk of kMlaChunk tokens of ONE sequence in tiles of 32 keys for a block of kVerRows query
// rows: a tile (32 rows x 576 halves, rows padded to 592) goes global -> registers -> LDS ONCE for all of them, two buffers, tile t + 1
// published while tile t is multiplied and tile t + 2 in flight in registers -- the staging of mla_decode_kernel.  What differs is
// what a staged fragment feeds.  Column block cb = query row kVerRows rb + cb, column r of it = head 16 hb + r:
//   S^T: wave (kh, kk) multiplies keys 16 kh .. +15 by dims 288 kk .. +287.  Each of its 9 row-wise K fragments is read from LDS once
//        and feeds kVerRows MFMAs, one per column block, against q fragments held in registers (kVerRows x 36 VGPRs, loaded once).
//        The partial logits meet in LDS (2 x 32 keys x 64 columns, fp32).
//   softmax: every wave adds the two partials of all 32 keys x 64 columns (8 values per lane and column block, in the k order of the
//        P^T operand) and keeps a running (max, sum) per column block.  Only the tiles that overlap [hist, ctx) -- a wave-uniform
//        test, at most ceil(rows / 32) + 1 tiles of a sequence -- apply the mask; a column whose keys so far are all masked keeps
//        (m = -inf, l = 0, o = 0): the subtrahend of the exponentials is 0 there, never -inf, so no NaN arises.
//   O^T: wave w accumulates output dims 128 w .. +127 of ALL column blocks: each of the 16 transposed reads (ds_read_b64_tr_b16) of a
//        tile feeds kVerRows MFMAs; kVerRows x 8 floatx4 accumulators.
// 17 x kVerRows MFMAs per wave between the two barriers of a tile for 25 fragment reads: 0.37 reads per MFMA at kVerRows = 4, against
// 25 / 17 = 1.47 in mla_decode_kernel.  Rows of a tile at or past ctx re-read row ctx - 1 (same tile, same page) and are masked; no
// load leaves the context and no block-table entry past (ctx - 1) / 128 is read.  Query rows at or past count[b] inside a live row
// block compute with the operands of row count[b] - 1 and write nothing.  The chunking depends on ctx alone and a column's arithmetic
// on nothing but its own q row, mask and the tiles: a row's bits do not depend on the batch, its slot, the grid or its neighbours.
#include "mla_common.cuh"

namespace llmie {

namespace {

constexpr int kVerRows = 4, kVerCols = kMlaHeads * kVerRows;   // heads, tile, chunk and the padded LDS row are the decode kernel's
static_assert(kVerRows >= 2 && LLMIE_SPEC_TREE_MAX_NODES <= 64, "at least two column blocks per fragment; the mask is one uint64");

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void mla_verify_kernel(
    const half_t *__restrict__ q_lat, const half_t *__restrict__ cache, half_t *__restrict__ o_lat, float *__restrict__ ws_o,
    float2 *__restrict__ ws_ml, const int32_t *__restrict__ hist_dev, const int32_t *__restrict__ count_dev, const uint64_t *__restrict__ anc,
    const int32_t *__restrict__ table, int max_pages, size_t layer_off, int rows, int row_blocks, int head_num, int max_seq_len, int span,
    float scale2 /* softmax_scale * log2(e) */) {
    __shared__ __attribute__((aligned(16))) half_t Ts[2][kMlaTile * kMlaStride];   // 2 x 37888 bytes
    __shared__ __attribute__((aligned(16))) float Sp[2 * 8 * kVerCols * 4];          // partial logits [kk][key / 4][column][key % 4]
    const int split = blockIdx.x, hb = blockIdx.y, b = blockIdx.z / row_blocks, rb = blockIdx.z - b * row_blocks, splits = gridDim.x;
    int hist, count;
    if (!verify_live(hist_dev, count_dev, b, rows, span, &hist, &count)) return;
    const int row0 = rb * kVerRows, ctx = hist + count;
    if (row0 >= count) return;
    const int t_begin = split * kMlaChunk;
    if (t_begin >= ctx) return;
    const int n_tiles = (min(ctx, t_begin + kMlaChunk) - t_begin + kMlaTile - 1) / kMlaTile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int kh = wave & 1, kk = wave >> 1;
    const int head = hb * kMlaHeads + r;

    half8_t qf[kVerRows][9];      // Q[row cb][head r][288 kk + 32 s + 8 q ..]: the B operands of this wave's 9 steps
    uint64_t vis[kVerRows];       // bit j: row cb sees node j (wave-uniform)
#pragma unroll
    for (int cb = 0; cb < kVerRows; ++cb) {
        const int i = min(row0 + cb, count - 1);
        const half_t *qp = q_lat + ((static_cast<size_t>(b) * rows + i) * head_num + head) * kRow + 288 * kk + 8 * q;
#pragma unroll
        for (int s = 0; s < 9; ++s) qf[cb][s] = *reinterpret_cast<const half8_t *>(qp + 32 * s);
        const uint64_t a = anc ? anc[static_cast<size_t>(b) * rows + i] : ~0ull;
        vis[cb] = (a & ((2ull << i) - 1ull)) | (1ull << i);
    }

    // staging: wave w moves rows 8 w .. 8 w + 7 of a tile.  A row is 72 sixteen-byte pieces: piece `lane` of each of the 8 rows (the row,
    // its clamp and its address are wave-uniform), then the 8 x 8 pieces left over, row 8 w + lane / 8, piece 64 + lane % 8
    constexpr int NCH = 9;
    half8_t treg[NCH];
    const int srow = 8 * wave, xrow = srow + (lane >> 3), xch = 64 + (lane & 7);
    auto fetch_tile = [&](int t0) {   // global -> registers; one page lookup per tile, wave-uniform
        const half_t *src = cache + layer_off + mla_tile_row0(table, max_pages, b, t0, max_seq_len) * kRow;
        const int last = ctx - 1 - t0;   // (0 <= last; last < 32 where the clamp acts: same tile, same page)
#pragma unroll
        for (int i = 0; i < 8; ++i)
            treg[i] = *reinterpret_cast<const half8_t *>(src + static_cast<size_t>(min(srow + i, last)) * kRow + lane * 8);
        treg[8] = *reinterpret_cast<const half8_t *>(src + static_cast<size_t>(min(xrow, last)) * kRow + xch * 8);
    };
    auto publish_tile = [&](int buf) {   // registers -> LDS, padded rows
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<half8_t *>(Ts[buf] + (srow + i) * kMlaStride + lane * 8) = treg[i];
        *reinterpret_cast<half8_t *>(Ts[buf] + xrow * kMlaStride + xch * 8) = treg[8];
    };

    floatx4 o[kVerRows][8];   // O^T: dims 128 wave + 16 dt + 4 q + e, column = (row cb, head r)
    float m_run[kVerRows], l_run[kVerRows];   // log2 domain, scale applied; l_run: this lane's 8 of a tile's 32 keys
#pragma unroll
    for (int cb = 0; cb < kVerRows; ++cb) {
        m_run[cb] = -INFINITY, l_run[cb] = 0.f;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) o[cb][dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    }

    fetch_tile(t_begin);
    publish_tile(0);
    if (1 < n_tiles) fetch_tile(t_begin + kMlaTile);
    for (int it = 0; it < n_tiles; ++it) {
        const int t0 = t_begin + it * kMlaTile;
        const half_t *Tt = Ts[it & 1];
        __syncthreads();   // tile `it` published; every wave done with tile it - 1 (the other buffer) and with its logits
        if (it + 1 < n_tiles) {
            publish_tile((it + 1) & 1);
            if (it + 2 < n_tiles) fetch_tile(t0 + 2 * kMlaTile);   // in flight under this iteration's MFMAs
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- S^T partial: keys 16 kh + r, dims 288 kk ..; one K fragment, kVerRows column blocks ----
        {
            half8_t kf[9];
            const half_t *kp = Tt + (16 * kh + r) * kMlaStride + 288 * kk + 8 * q;
#pragma unroll
            for (int s = 0; s < 9; ++s) kf[s] = *reinterpret_cast<const half8_t *>(kp + 32 * s);
            floatx4 sacc[kVerRows];
#pragma unroll
            for (int cb = 0; cb < kVerRows; ++cb) sacc[cb] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 9; ++s)
#pragma unroll
                for (int cb = 0; cb < kVerRows; ++cb) sacc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[s], qf[cb][s], sacc[cb], 0, 0, 0);
            // sacc[cb][e] = S[key 16 kh + 4 q + e][row cb, head r]
#pragma unroll
            for (int cb = 0; cb < kVerRows; ++cb)
                *reinterpret_cast<floatx4 *>(Sp + (((kk * 8 + 4 * kh + q) * kVerCols + 16 * cb + r) << 2)) = sacc[cb];
        }
        __syncthreads();   // both halves of every logit are there
        __builtin_amdgcn_sched_barrier(0);
        const bool masked = t0 + kMlaTile > hist;   // wave-uniform: the tile holds a node, or rows past ctx
        half8_t pf[kVerRows];
#pragma unroll
        for (int cb = 0; cb < kVerRows; ++cb) {
            float s8[8];   // keys t0 + 16 (j >> 2) + 4 q + (j & 3): the k index 8 q + j of the P^T operand
            {
                const floatx4 a0 = *reinterpret_cast<const floatx4 *>(Sp + (((0 * 8 + q) * kVerCols + 16 * cb + r) << 2));
                const floatx4 b0 = *reinterpret_cast<const floatx4 *>(Sp + (((1 * 8 + q) * kVerCols + 16 * cb + r) << 2));
                const floatx4 a1 = *reinterpret_cast<const floatx4 *>(Sp + (((0 * 8 + 4 + q) * kVerCols + 16 * cb + r) << 2));
                const floatx4 b1 = *reinterpret_cast<const floatx4 *>(Sp + (((1 * 8 + 4 + q) * kVerCols + 16 * cb + r) << 2));
#pragma unroll
                for (int e = 0; e < 4; ++e) s8[e] = a0[e] + b0[e], s8[4 + e] = a1[e] + b1[e];
            }
            if (masked) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int node = t0 + 16 * (j >> 2) + 4 * q + (j & 3) - hist;   // < 0: history
                    const bool see = (node < 0) | ((node < 64) & (static_cast<int>(vis[cb] >> (node & 63)) & 1));   // (no branch)
                    s8[j] = see ? s8[j] : -INFINITY;
                }
            }
            float mloc = -INFINITY;
#pragma unroll
            for (int j = 0; j < 8; ++j) mloc = fmaxf(mloc, s8[j]);
            mloc = lane_xor_max<16>(lane_xor_max<32>(mloc)) * scale2;   // over the 4 lanes of the column; scale2 > 0
            const float m_new = fmaxf(m_run[cb], mloc);
            const float m_sub = m_new == -INFINITY ? 0.f : m_new;   // nothing seen so far: every exponent below is -inf, not NaN
            const float alpha = __builtin_amdgcn_exp2f(m_run[cb] - m_sub);   // first seen tile: 2^(-inf) = 0
            float lsum = 0.f;
            typedef float float2v_t __attribute__((ext_vector_type(2)));
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s8[j], scale2, -m_sub));
                const float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s8[j + 1], scale2, -m_sub));
                lsum += p0 + p1;
                const half2_t hh = __builtin_convertvector(float2v_t{p0, p1}, half2_t);
                pf[cb][j] = hh[0];
                pf[cb][j + 1] = hh[1];
            }
            l_run[cb] = l_run[cb] * alpha + lsum;
            m_run[cb] = m_new;
            if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {
#pragma unroll
                for (int dt = 0; dt < 8; ++dt) o[cb][dt] *= alpha;
            }
            __builtin_amdgcn_sched_barrier(0);   // one column block's logits and accumulators pass through the VALU at a time
        }
        // ---- O^T += C^T . P^T: A fragment = C[key(q, j)][128 wave + 16 dt + r], gathered down a column by the transposed read; one
        // gather, kVerRows column blocks ----
        {
            const half_t *blk = Tt + (4 * q + (r >> 2)) * kMlaStride + 128 * wave + 4 * (r & 3);
#pragma unroll
            for (int d0 = 0; d0 < 8; d0 += 4) {   // in two halves: 16 fragment registers in flight, not 32
                fp16x4_t lo[4], hi[4];
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    lo[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(blk + (d0 + dt) * 16));
                    hi[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(blk + 16 * kMlaStride + (d0 + dt) * 16));
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const half8_t cf = __builtin_bit_cast(half8_t, Tr8{lo[dt], hi[dt]});
#pragma unroll
                    for (int cb = 0; cb < kVerRows; ++cb)
                        o[cb][d0 + dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cf, pf[cb], o[cb][d0 + dt], 0, 0, 0);
                }
            }
        }
    }
#pragma unroll
    for (int cb = 0; cb < kVerRows; ++cb) {
        const float l = lane_xor_sum<32>(lane_xor_sum<16>(l_run[cb]));
        if (row0 + cb >= count) continue;   // (wave-uniform) a row past the count: nothing is written
        const size_t bh = (static_cast<size_t>(b) * rows + row0 + cb) * head_num + head;
        // mla_store_split written out: called here, the helper costs this 512-register kernel three VGPRs spilled to scratch
        if (splits == 1) {   // the only split: the output itself (the self bit: l > 0)
            const float inv = 1.f / l;
            half_t *op = o_lat + bh * kLat + 128 * wave + 4 * q;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                const half4_t v = {from_f32<half_t>(o[cb][dt][0] * inv), from_f32<half_t>(o[cb][dt][1] * inv),
                                   from_f32<half_t>(o[cb][dt][2] * inv), from_f32<half_t>(o[cb][dt][3] * inv)};
                *reinterpret_cast<half4_t *>(op + 16 * dt) = v;
            }
        } else {
            float *op = ws_o + (bh * splits + split) * kLat + 128 * wave + 4 * q;
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) *reinterpret_cast<floatx4 *>(op + 16 * dt) = o[cb][dt];
            if (wave == 0 && q == 0) ws_ml[bh * splits + split] = make_float2(m_run[cb], l);
        }
    }
}

}  // namespace

// The one planner of llmie_mla_verify: every check that needs no pointer, then the launch.  Pure host code.
int plan_mla_verify(const char *who, const MlaVerifyCall &c, MlaVerifyPlan *p) {
    int rc = mla_heads_check(who, c.batch, c.head_num);
    if (rc == LLMIE_OK) rc = mla_cache_check(who, c.max_seq_len, c.paged, c.max_pages, c.num_pages);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(c.rows >= 1, "%s: rows=%d should be >= 1", who, c.rows);
    if (c.rows > LLMIE_SPEC_TREE_MAX_NODES)
        LLMIE_UNSUPPORTED("%s: rows=%d: at most LLMIE_SPEC_TREE_MAX_NODES=%d query rows per sequence (one 64-bit ancestor mask per row)", who, c.rows,
                          LLMIE_SPEC_TREE_MAX_NODES);
    rc = mla_max_ctx_check(who, c.max_ctx, c.max_seq_len);
    if (rc != LLMIE_OK) return rc;
    p->rows = kVerRows;
    p->span = c.max_ctx > 0 ? c.max_ctx : c.max_seq_len;
    p->row_blocks = (c.rows + kVerRows - 1) / kVerRows;
    LLMIE_REQUIRE(static_cast<long long>(c.batch) * p->row_blocks <= 65535 && static_cast<long long>(c.batch) * c.rows <= 65535,
                  "%s: batch=%d x rows=%d does not fit one launch (batch x rows <= 65535)", who, c.batch, c.rows);
    if (!mla_split_plan(p, p->span, c.head_num, c.batch * c.rows, c.batch * p->row_blocks, c.workspace, c.workspace_bytes)) {
        set_error("%s: workspace of %zu bytes, %d rows x %d splits of %d tokens need %zu (llmie_mla_verify_workspace_bytes)", who,
                  c.workspace ? c.workspace_bytes : static_cast<size_t>(0), c.rows, p->grid[0], kMlaChunk, p->workspace_bytes);
        return LLMIE_ERR_WORKSPACE;
    }
    return LLMIE_OK;
}

}  // namespace llmie

using namespace llmie;

extern "C" size_t llmie_mla_verify_workspace_bytes(int batch, int rows, int head_num, int max_seq_len) {
    if (batch < 1 || rows < 1 || head_num < 1 || max_seq_len < 1) return 0;
    return mla_partials_bytes(static_cast<size_t>(batch) * rows, head_num, mla_splits(max_seq_len));
}

extern "C" const char *llmie_mla_verify_plan(int batch, int rows, int head_num, int max_seq_len, int max_ctx, int tree, int paged, int max_pages,
                                             int num_pages, long long workspace_bytes, int *status) {
    static thread_local char text[192];
    MlaVerifyPlan p{};
    const MlaVerifyCall c{batch, rows, head_num, max_seq_len, max_ctx, tree != 0, paged != 0, max_pages, num_pages, workspace_bytes >= 0,
                          workspace_bytes >= 0 ? static_cast<size_t>(workspace_bytes) : 0};
    const int rc = plan_mla_verify("mla_verify_plan", c, &p);
    if (status) *status = rc;
    if (rc != LLMIE_OK) return nullptr;
    const int n = snprintf(text, sizeof(text), "mla_verify f16 nh%d rows%d %s cols %dx%d tile%d chunk%d grid %dx%dx%d ", head_num, rows,
                           c.tree ? "tree" : "chain", p.heads, p.rows, p.tile, p.chunk, p.grid[0], p.grid[1], p.grid[2]);
    mla_merge_text(text + n, sizeof(text) - n, p);
    return text;
}

extern "C" int llmie_mla_verify(const void *q_lat, const void *cache, void *o_lat, int layer, int batch, int rows, int head_num, int max_seq_len,
                                int max_ctx, const int32_t *hist_dev, const int32_t *count_dev, const uint64_t *anc_dev, float softmax_scale,
                                void *workspace, size_t workspace_bytes, const int32_t *block_table, int max_pages, int num_pages,
                                llmie_stream stream) {
    LLMIE_REQUIRE(q_lat && cache && o_lat && hist_dev, "mla_verify: NULL operand");
    LLMIE_REQUIRE(layer >= 0, "mla_verify: layer=%d should be >= 0", layer);
    LLMIE_REQUIRE(mla_scale_ok(softmax_scale), "mla_verify: softmax_scale should be positive and finite");
    MlaVerifyPlan p{};
    const MlaVerifyCall c{batch, rows, head_num, max_seq_len, max_ctx, anc_dev != nullptr, block_table != nullptr, max_pages, num_pages,
                          workspace != nullptr, workspace_bytes};
    const int rc = plan_mla_verify("mla_verify", c, &p);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(mis16(q_lat) == 0 && mis16(cache) == 0 && mis16(o_lat) == 0 && (!p.merge || mis16(workspace) == 0),
                  "mla_verify: q_lat, the cache, o_lat and the workspace should be 16-byte aligned");
    float *ws_o = static_cast<float *>(workspace);
    float2 *ws_ml = mla_ws_ml(ws_o, p);
    hipLaunchKernelGGL(mla_verify_kernel, dim3(p.grid[0], p.grid[1], p.grid[2]), dim3(256), 0, as_stream(stream),
                       static_cast<const half_t *>(q_lat), static_cast<const half_t *>(cache), static_cast<half_t *>(o_lat), ws_o, ws_ml, hist_dev,
                       count_dev, anc_dev, block_table, max_pages, mla_layer_off(layer, batch, max_seq_len, block_table != nullptr, num_pages, kRow), rows,
                       p.row_blocks, head_num, max_seq_len, p.span, softmax_scale * kLog2e);
    if (p.merge) mla_merge_launch(p, p.span, ws_o, static_cast<half_t *>(o_lat), hist_dev, count_dev, rows, nullptr, 0, as_stream(stream));
    return launch_status("mla_verify");
}
