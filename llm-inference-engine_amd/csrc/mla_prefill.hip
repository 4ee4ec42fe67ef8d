// Multi-head Latent Attention, prefill (DeepSeek-V2 / V3 / R1, Kimi-K2), in the UN-absorbed form: the prompt's latent rows are
// written to the cache in bulk, projected up once to per-head k_nope || v rows, and a flash kernel with q/k width 192 and v width
// 128 attends over them (include/llmie.h, llmie_mla_kv_append_rows / _kv_up / _prefill).  Per key and head that is 2 x (192 + 128)
// FLOP against the absorbed form's 2 x (576 + 512).  Sequences are packed as in prefill.hip: cum[batch + 1] = exclusive prefix of the
// new-token counts, hist[b] = tokens already cached.  A sequence with no new token, more than max_q_len of them, or a context above
// kv_span is left wholly untouched by all three launches.
//   mla_kv_append_kernel        (mla.hip, mla_append_launch) the single-token row at position hist[b] + i  (one wave per packed token)
//   mla_kv_up_kernel            kv_up[b, t, h, 0:256] = fp16(W[h] c_t), t < ctx                      (MFMA, latent tile staged once)
//   mla_prefill_flash_kernel    causal online-softmax attention, plain softmax                       (MFMA, the hot path)
//
// mla_kv_up_kernel.  Grid (token tiles of 64, head_num / 4, batch), 4 waves.  out^T[n][t] = sum_c W[h][n][c] c_t[c]: both operands
// are k-contiguous as stored, so W rows are the A operand straight from global memory in fragment layout (16 rows x 512 = 16
// fragments, 64 VGPRs, the next block's in flight under this block's MFMAs) and the latent rows are the B operand, staged in LDS
// once per workgroup (64 rows x 1056 bytes, an odd multiple of 32) and read 4 x 16 times per weight block: every weight fragment
// feeds 4 MFMAs.  Wave w owns the 16-row blocks 4 w .. 4 w + 3 of each head, so the 128 bytes of an output row that it fills over
// four steps are contiguous.  Weights are re-read once per token tile (256 KB per head), latents once per head block.
//
// mla_prefill_flash_kernel.  Grid (query tiles of 64, head_num, batch) walked longest-first, 4 waves x 16 query rows.  A key tile
// is 32 rows; a staged row is the 512 contiguous bytes kv_up[b, t, h] (k_nope || v) followed by the 128 bytes of k_pe from the cache
// row -- shared by all heads, never copied per head -- padded to 672 bytes (an odd multiple of 32: conflict-free transposed reads).
// Two tile buffers (2 x 21504 bytes, three workgroups per CU), tile t+1 published while tile t is multiplied and tile t+2 in flight
// in registers, one barrier per iteration.
//   S^T = K . Q^T: 2 key blocks x 6 k-steps; steps 0..3 read columns 0..127 (k_nope), steps 4..5 columns 256..319 (k_pe).  The q
//        fragments come from global memory once; fragments 4 and 5 hold the rotate-half pairs (j, j + 32) in the same lane and
//        element, so q_pe is rotated in place, in fp32 from the table, one rounding (as mla_q_absorb_kernel).
//   softmax: online, log2 domain, per lane the 8 logits of its query row, P^T straight from the S accumulators.
//   O^T += V^T . P^T: 16 transposed reads of columns 128..255, 8 MFMAs.
// Key 0 is visible to every query, so after tile 0 every running maximum is finite; a later tile wholly in a row's future gives
// alpha = 2^0 = 1 and p = 2^-inf = 0 and leaves the row's state as it was, and a wave skips a tile wholly in the future of all its
// rows.  Staged rows past the last key any query of the workgroup sees re-read that key's row (same tile, same page): no load leaves
// the context, no kv_up row at or past ctx and no block-table entry past (ctx - 1) / 128 is read.  A row's bits depend on its
// position and the rows it sees alone: not on the batch, the slot, the grid, or how the prompt was cut into calls.
#include "mla_common.cuh"

#include <cstdio>

namespace llmie {

namespace {

constexpr int kPfQ = 64, kPfTile = 32, kPfStride = kNope + kVd + kRope + 16;   // 336 halves: k_nope | v | k_pe | pad
constexpr int kPfPieces = (kNope + kVd + kRope) / 8;                           // 40 sixteen-byte pieces per staged row
constexpr int kUpTok = 64, kUpHeads = 4, kUpStride = kLat + 16;
static_assert(kPage % kPfTile == 0 && kPage % kUpTok == 0, "a tile never crosses a page");
static_assert((kPfStride * 2) % 64 == 32 && (kUpStride * 2) % 64 == 32, "row stride = an odd multiple of 32 bytes");
static_assert(kPfTile * kPfPieces % 256 == 0, "a tile is a whole number of pieces per thread");

// ---- up-projection ----
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void mla_kv_up_kernel(const half_t *__restrict__ cache, const half_t *__restrict__ kv_b,
                                                        half_t *__restrict__ kv_up, const int32_t *__restrict__ cum,
                                                        const int32_t *__restrict__ hist, const int32_t *__restrict__ table, int max_pages,
                                                        size_t layer_off, int head_num, int max_seq_len, int max_q_len, int kv_span) {
    __shared__ __attribute__((aligned(16))) half_t Ls[kUpTok * kUpStride];   // 67584 bytes
    const int t0 = blockIdx.x * kUpTok, hb = blockIdx.y, b = blockIdx.z;
    const int len = cum[b + 1] - cum[b], history = hist[b];
    if (!mla_prefill_live(len, history, max_q_len, kv_span)) return;
    const int ctx = history + len;
    if (t0 >= ctx) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    {   // the latent tile, global -> LDS; one page lookup per tile; rows at or past ctx re-read row ctx - 1 (same tile, same page)
        const half_t *base = cache + layer_off + mla_tile_row0(table, max_pages, b, t0, max_seq_len) * kRow;
        const int last = ctx - 1 - t0;   // >= 0
        half8_t lreg[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int id = tid + 256 * i, row = id >> 6, ch = id & 63;
            lreg[i] = *reinterpret_cast<const half8_t *>(base + min(row, last) * kRow + ch * 8);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int id = tid + 256 * i, row = id >> 6, ch = id & 63;
            *reinterpret_cast<half8_t *>(Ls + row * kUpStride + ch * 8) = lreg[i];
        }
    }
    // weight block `it` of the workgroup: head hb * 4 + (it >> 2), rows 16 (4 wave + (it & 3)) .. + 15 of its 256
    auto weight_rows = [&](int it) {
        return kv_b + ((static_cast<size_t>(hb) * kUpHeads + (it >> 2)) * (kNope + kVd) + 16 * (4 * wave + (it & 3)) + r) * kLat + 8 * q;
    };
    half8_t af[16], an[16];
    {
        const half_t *w = weight_rows(0);
#pragma unroll
        for (int s = 0; s < 16; ++s) an[s] = *reinterpret_cast<const half8_t *>(w + 32 * s);
    }
    __syncthreads();
    for (int it = 0; it < 4 * kUpHeads; ++it) {
#pragma unroll
        for (int s = 0; s < 16; ++s) af[s] = an[s];
        if (it + 1 < 4 * kUpHeads) {
            const half_t *w = weight_rows(it + 1);
#pragma unroll
            for (int s = 0; s < 16; ++s) an[s] = *reinterpret_cast<const half8_t *>(w + 32 * s);
        }
        const int h = hb * kUpHeads + (it >> 2), n0 = 16 * (4 * wave + (it & 3));
#pragma unroll
        for (int tt = 0; tt < kUpTok / 16; ++tt) {
            const half_t *bp = Ls + (16 * tt + r) * kUpStride + 8 * q;
            floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[s], *reinterpret_cast<const half8_t *>(bp + 32 * s), acc, 0, 0, 0);
            // acc[e] = out[token t0 + 16 tt + r][row n0 + 4 q + e]
            const int t = t0 + 16 * tt + r;
            if (t < ctx) {
                const half4_t v = {from_f32<half_t>(acc[0]), from_f32<half_t>(acc[1]), from_f32<half_t>(acc[2]), from_f32<half_t>(acc[3])};
                *reinterpret_cast<half4_t *>(kv_up + ((static_cast<size_t>(b) * kv_span + t) * head_num + h) * (kNope + kVd) + n0 + 4 * q) = v;
            }
            __builtin_amdgcn_sched_barrier(0);   // one token block's 16 fragments at a time: the reads of the next stay behind
        }
    }
}

// ---- the attention ----
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void mla_prefill_flash_kernel(
    const half_t *__restrict__ qin, const half_t *__restrict__ kv_up, const half_t *__restrict__ cache, const float2 *__restrict__ rope,
    half_t *__restrict__ out, const int32_t *__restrict__ cum, const int32_t *__restrict__ hist, const int32_t *__restrict__ table,
    int max_pages, size_t layer_off, int head_num, int max_seq_len, int max_q_len, int kv_span, float scale2 /* softmax_scale * log2(e) */) {
    __shared__ __attribute__((aligned(16))) half_t Ts[2][kPfTile * kPfStride];   // 2 x 21504 bytes
    // longest first (prefill_flash_kernel): the linear ids walk the query tiles from the last, heaviest one down, all heads and
    // sequences of a tile index together
    const int nx = gridDim.x, rows = gridDim.y * gridDim.z;
    const int lin = blockIdx.x + nx * (blockIdx.y + gridDim.y * blockIdx.z);
    const int kx = lin / rows, rowi = lin - kx * rows;
    const int xq = nx - 1 - kx, b = rowi / gridDim.y, h = rowi - b * gridDim.y;
    const int len = cum[b + 1] - cum[b], history = hist[b];
    if (!mla_prefill_live(len, history, max_q_len, kv_span)) return;
    const int q0 = xq * kPfQ;
    if (q0 >= len) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;

    // this lane's query row (clamped in the tail tile: computed, not stored) and its position; keys t <= qpos are visible
    const int qrow = q0 + 16 * wave + r, qrow_c = min(qrow, len - 1), qpos = history + qrow_c;
    half8_t qf[6];   // Q[row][32 s + 8 q ..]: the B operand of the 6 k-steps
    {
        const half_t *qp = qin + (static_cast<size_t>(cum[b] + qrow_c) * head_num + h) * kQ + 8 * q;
#pragma unroll
        for (int s = 0; s < 6; ++s) qf[s] = *reinterpret_cast<const half8_t *>(qp + 32 * s);
        // q_pe: element e of fragment 4 is rope dim 8 q + e, the same element of fragment 5 its partner 32 further
        const float2 *cp = rope + static_cast<size_t>(qpos) * (kRope / 2) + 8 * q;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float2 cs = cp[e];
            const float x0 = to_f32(qf[4][e]), x1 = to_f32(qf[5][e]);
            qf[4][e] = from_f32<half_t>(x0 * cs.x - x1 * cs.y);
            qf[5][e] = from_f32<half_t>(x1 * cs.x + x0 * cs.y);
        }
    }

    const int t_hi = history + min(q0 + kPfQ, len);   // keys [0, t_hi) are seen by some row of this workgroup; t_hi <= ctx
    const int n_tiles = (t_hi + kPfTile - 1) / kPfTile;
    constexpr int NCH = kPfTile * kPfPieces / 256;    // 5 sixteen-byte pieces of a tile per thread
    half8_t treg[NCH];
    const half_t *up_base = kv_up + (static_cast<size_t>(b) * kv_span * head_num + h) * (kNope + kVd);
    auto fetch_tile = [&](int t0) {   // global -> registers; one page lookup per tile, wave-uniform
        const size_t base = table ? layer_off + static_cast<size_t>(__builtin_amdgcn_readfirstlane(table[static_cast<size_t>(b) * max_pages + t0 / kPage])) * kPage * kRow
                                  : layer_off + static_cast<size_t>(b) * max_seq_len * kRow;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int id = tid + 256 * i, row = id / kPfPieces, ch = id - row * kPfPieces;
            const int t = min(t0 + row, t_hi - 1);   // (t0 <= t_hi - 1 < t0 + 32 where the clamp acts: same tile, same page)
            const half_t *src = ch < (kNope + kVd) / 8 ? up_base + static_cast<size_t>(t) * head_num * (kNope + kVd) + ch * 8
                                                       : cache + base + static_cast<size_t>(table ? t % kPage : t) * kRow + kLat + (ch * 8 - (kNope + kVd));
            treg[i] = *reinterpret_cast<const half8_t *>(src);
        }
    };
    auto publish_tile = [&](int buf) {   // registers -> LDS, padded rows: k_nope at 0, v at 128, k_pe at 256
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int id = tid + 256 * i, row = id / kPfPieces, ch = id - row * kPfPieces;
            *reinterpret_cast<half8_t *>(Ts[buf] + row * kPfStride + ch * 8) = treg[i];
        }
    };

    floatx4 o[8];   // O^T: value dims 16 dt + 4 q + e, column = this lane's query row
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) o[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;   // log2 domain, scale applied; l_run: this lane's 8 of a tile's 32 keys

    fetch_tile(0);
    publish_tile(0);
    if (1 < n_tiles) fetch_tile(kPfTile);
    for (int it = 0; it < n_tiles; ++it) {
        const int t0 = it * kPfTile;
        const half_t *Tt = Ts[it & 1];
        __syncthreads();   // tile `it` published by every thread; every wave done with tile it - 1 (the other buffer)
        if (it + 1 < n_tiles) {
            publish_tile((it + 1) & 1);
            if (it + 2 < n_tiles) fetch_tile(t0 + 2 * kPfTile);   // in flight under this iteration's MFMAs
        }
        __builtin_amdgcn_sched_barrier(0);
        // a tile wholly in the future of the wave's rows (never tile 0): the wave only takes part in the staging
        if (t0 > history + q0 + 16 * wave + 15) continue;
        // ---- S^T = K . Q^T: key blocks 16 tt + r, 6 k-steps ----
        floatx4 sacc[2];
#pragma unroll
        for (int sb = 0; sb < 2; ++sb) {   // two batches of 3 k-steps: 24 fragment registers instead of 48
            half8_t kf[2][3];
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
                const half_t *kp = Tt + (16 * tt + r) * kPfStride + 8 * q;
#pragma unroll
                for (int s = 0; s < 3; ++s) kf[tt][s] = *reinterpret_cast<const half8_t *>(kp + (3 * sb + s < 4 ? 32 * (3 * sb + s) : kVd + 32 * (3 * sb + s)));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int tt = 0; tt < 2; ++tt)
                    sacc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[tt][s], qf[3 * sb + s], sb + s == 0 ? floatx4{0.f, 0.f, 0.f, 0.f} : sacc[tt], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        // sacc[tt][e] = S[key t0 + 16 tt + 4 q + e][this lane's query row]: the k index 8 q + 4 tt + e of the P^T operand
        float mloc = -INFINITY;
        if (t0 + kPfTile - 1 > history + q0 + 16 * wave) {   // wave-uniform: the tile reaches past the wave's first query position
#pragma unroll
            for (int tt = 0; tt < 2; ++tt)
#pragma unroll
                for (int e = 0; e < 4; ++e) sacc[tt][e] = t0 + 16 * tt + 4 * q + e <= qpos ? sacc[tt][e] : -INFINITY;
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int e = 0; e < 4; ++e) mloc = fmaxf(mloc, sacc[tt][e]);
        mloc = lane_xor_max<16>(lane_xor_max<32>(mloc)) * scale2;   // over the 4 lanes of the query row; scale2 > 0
        const float m_new = fmaxf(m_run, mloc);                      // finite from tile 0 on: key 0 is visible to every row
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // first tile: 2^(-inf) = 0
        float lsum = 0.f;
        half8_t pf;
        typedef float float2v_t __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int tt = 0; tt < 2; ++tt)
#pragma unroll
            for (int e = 0; e < 4; e += 2) {
                const float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[tt][e], scale2, -m_new));
                const float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[tt][e + 1], scale2, -m_new));
                lsum += p0 + p1;
                const half2_t hh = __builtin_convertvector(float2v_t{p0, p1}, half2_t);
                pf[4 * tt + e] = hh[0];
                pf[4 * tt + e + 1] = hh[1];
            }
        l_run = l_run * alpha + lsum;
        m_run = m_new;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) o[dt] *= alpha;
        }
        // ---- O^T += V^T . P^T: A fragment = V[key(q, j)][16 dt + r], gathered down a column by the transposed read ----
        {
            const half_t *blk = Tt + (4 * q + (r >> 2)) * kPfStride + kNope + 4 * (r & 3);
            fp16x4_t lo[8], hi[8];
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                lo[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(blk + dt * 16));
                hi[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(blk + 16 * kPfStride + dt * 16));
            }
#pragma unroll
            for (int dt = 0; dt < 8; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, Tr8{lo[dt], hi[dt]}), pf, o[dt], 0, 0, 0);
        }
    }
    const float l = lane_xor_sum<32>(lane_xor_sum<16>(l_run));
    if (qrow < len) {
        const float inv = 1.f / l;
        half_t *op = out + (static_cast<size_t>(cum[b] + qrow) * head_num + h) * kVd + 4 * q;
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) {
            const half4_t v = {from_f32<half_t>(o[dt][0] * inv), from_f32<half_t>(o[dt][1] * inv), from_f32<half_t>(o[dt][2] * inv),
                               from_f32<half_t>(o[dt][3] * inv)};
            *reinterpret_cast<half4_t *>(op + 16 * dt) = v;
        }
    }
}

}  // namespace

// The one planner of the three prefill entries: every check that needs no pointer, then the launches.  Pure host code.
int plan_mla_prefill(const char *who, const MlaPrefillCall &c, MlaPrefillPlan *p) {
    int rc = c.head_num != 0 ? mla_heads_check(who, c.batch, c.head_num) : LLMIE_OK;
    if (rc == LLMIE_OK) rc = mla_cache_check(who, c.max_seq_len, c.paged, c.max_pages, c.num_pages);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(c.batch >= 1 && c.batch <= 65535, "%s: batch=%d should be in [1, 65535]", who, c.batch);
    LLMIE_REQUIRE(c.max_q_len >= 1, "%s: max_q_len=%d should be >= 1", who, c.max_q_len);
    LLMIE_REQUIRE(c.kv_span >= 1 && c.kv_span <= c.max_seq_len, "%s: kv_span=%d should be in [1, max_seq_len=%d]", who, c.kv_span, c.max_seq_len);
    LLMIE_REQUIRE(c.total_tokens >= 0 && c.total_tokens <= static_cast<long long>(c.batch) * c.max_q_len,
                  "%s: total_tokens=%d should be at most batch * max_q_len = %lld", who, c.total_tokens, static_cast<long long>(c.batch) * c.max_q_len);
    p->q_rows = kPfQ, p->key_tile = kPfTile;
    p->flash_grid[0] = (c.max_q_len + kPfQ - 1) / kPfQ, p->flash_grid[1] = c.head_num, p->flash_grid[2] = c.batch;
    p->up_tokens = kUpTok, p->up_heads = kUpHeads;
    p->up_grid[0] = (c.kv_span + kUpTok - 1) / kUpTok, p->up_grid[1] = c.head_num / kUpHeads, p->up_grid[2] = c.batch;
    p->append_grid = c.total_tokens;
    return LLMIE_OK;
}

}  // namespace llmie

using namespace llmie;

extern "C" const char *llmie_mla_prefill_plan(int batch, int head_num, int total_tokens, int max_q_len, int kv_span, int max_seq_len, int paged,
                                              int max_pages, int num_pages, int *status) {
    static thread_local char text[192];
    MlaPrefillPlan p{};
    int rc = LLMIE_OK;
    if (head_num == 0 || total_tokens < 1) {
        set_error("mla_prefill_plan: head_num=%d and total_tokens=%d should be >= 1", head_num, total_tokens);
        rc = LLMIE_ERR_INVALID_ARG;
    } else {
        rc = plan_mla_prefill("mla_prefill_plan", MlaPrefillCall{batch, head_num, total_tokens, max_q_len, kv_span, max_seq_len, paged != 0, max_pages, num_pages}, &p);
    }
    if (status) *status = rc;
    if (rc != LLMIE_OK) return nullptr;
    snprintf(text, sizeof(text), "mla_prefill f16 nh%d q%d kt%d flash %dx%dx%d up tt%d hb%d %dx%dx%d append %d", head_num, p.q_rows, p.key_tile,
             p.flash_grid[0], p.flash_grid[1], p.flash_grid[2], p.up_tokens, p.up_heads, p.up_grid[0], p.up_grid[1], p.up_grid[2], p.append_grid);
    return text;
}

extern "C" int llmie_mla_kv_append_rows(const void *kv_a, const void *gamma, float eps, const void *rope_table, void *cache, int layer, int batch,
                                        int total_tokens, int max_q_len, int kv_span, int max_seq_len, const int32_t *cum_dev,
                                        const int32_t *hist_dev, const int32_t *block_table, int max_pages, int num_pages, llmie_stream stream) {
    LLMIE_REQUIRE(kv_a && gamma && rope_table && cache && cum_dev && hist_dev, "mla_kv_append_rows: NULL operand");
    LLMIE_REQUIRE(layer >= 0 && total_tokens >= 1, "mla_kv_append_rows: layer=%d should be >= 0 and total_tokens=%d >= 1", layer, total_tokens);
    LLMIE_REQUIRE(eps > 0.f, "mla_kv_append_rows: eps should be > 0");
    MlaPrefillPlan p{};
    const int rc = plan_mla_prefill("mla_kv_append_rows", MlaPrefillCall{batch, 0, total_tokens, max_q_len, kv_span, max_seq_len, block_table != nullptr, max_pages, num_pages}, &p);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(mis16(kv_a) == 0 && mis16(gamma) == 0 && mis16(cache) == 0, "mla_kv_append_rows: kv_a, gamma and the cache should be 16-byte aligned");
    mla_append_launch(MlaAppendCall{kv_a, gamma, eps, rope_table, cache, layer, batch, max_seq_len, nullptr, cum_dev, hist_dev, max_q_len, kv_span,
                                    block_table, max_pages, num_pages},
                      p.append_grid, as_stream(stream));
    return launch_status("mla_kv_append_rows");
}

extern "C" int llmie_mla_kv_up(const void *cache, const void *kv_b, void *kv_up, int layer, int batch, int head_num, int max_q_len, int kv_span,
                               int max_seq_len, const int32_t *cum_dev, const int32_t *hist_dev, const int32_t *block_table, int max_pages,
                               int num_pages, llmie_stream stream) {
    LLMIE_REQUIRE(cache && kv_b && kv_up && cum_dev && hist_dev, "mla_kv_up: NULL operand");
    LLMIE_REQUIRE(layer >= 0, "mla_kv_up: layer=%d should be >= 0", layer);
    MlaPrefillPlan p{};
    const int rc = plan_mla_prefill("mla_kv_up", MlaPrefillCall{batch, head_num, 0, max_q_len, kv_span, max_seq_len, block_table != nullptr, max_pages, num_pages}, &p);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(mis16(cache) == 0 && mis16(kv_b) == 0 && mis16(kv_up) == 0, "mla_kv_up: the cache, kv_b and kv_up should be 16-byte aligned");
    hipLaunchKernelGGL(mla_kv_up_kernel, dim3(p.up_grid[0], p.up_grid[1], p.up_grid[2]), dim3(256), 0, as_stream(stream),
                       static_cast<const half_t *>(cache), static_cast<const half_t *>(kv_b), static_cast<half_t *>(kv_up), cum_dev, hist_dev, block_table,
                       max_pages, mla_layer_off(layer, batch, max_seq_len, block_table != nullptr, num_pages, kRow), head_num, max_seq_len, max_q_len, kv_span);
    return launch_status("mla_kv_up");
}

extern "C" int llmie_mla_prefill(const void *q, const void *kv_up, const void *cache, const void *rope_table, void *out, int layer, int batch,
                                 int head_num, int total_tokens, int max_q_len, int kv_span, int max_seq_len, const int32_t *cum_dev,
                                 const int32_t *hist_dev, float softmax_scale, const int32_t *block_table, int max_pages, int num_pages,
                                 llmie_stream stream) {
    LLMIE_REQUIRE(q && kv_up && cache && rope_table && out && cum_dev && hist_dev, "mla_prefill: NULL operand");
    LLMIE_REQUIRE(layer >= 0 && total_tokens >= 1, "mla_prefill: layer=%d should be >= 0 and total_tokens=%d >= 1", layer, total_tokens);
    LLMIE_REQUIRE(mla_scale_ok(softmax_scale), "mla_prefill: softmax_scale should be positive and finite");
    MlaPrefillPlan p{};
    const int rc = plan_mla_prefill("mla_prefill", MlaPrefillCall{batch, head_num, total_tokens, max_q_len, kv_span, max_seq_len, block_table != nullptr, max_pages, num_pages}, &p);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(mis16(q) == 0 && mis16(kv_up) == 0 && mis16(cache) == 0 && mis16(rope_table) == 0 && mis16(out) == 0,
                  "mla_prefill: q, kv_up, the cache, the rope table and out should be 16-byte aligned");
    hipLaunchKernelGGL(mla_prefill_flash_kernel, dim3(p.flash_grid[0], p.flash_grid[1], p.flash_grid[2]), dim3(256), 0, as_stream(stream),
                       static_cast<const half_t *>(q), static_cast<const half_t *>(kv_up), static_cast<const half_t *>(cache),
                       static_cast<const float2 *>(rope_table), static_cast<half_t *>(out), cum_dev, hist_dev, block_table, max_pages,
                       mla_layer_off(layer, batch, max_seq_len, block_table != nullptr, num_pages, kRow), head_num, max_seq_len, max_q_len, kv_span,
                       softmax_scale * kLog2e);
    return launch_status("mla_prefill");
}
