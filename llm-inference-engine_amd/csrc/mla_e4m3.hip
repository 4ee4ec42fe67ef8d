// Multi-head Latent Attention on an e4m3 latent cache (include/llmie.h, llmie_mla_*_e4m3): a token is 640 bytes -- 512 OCP e4m3fn
// codes of the latent, code = e4m3(c / c_scale) with one static fp32 c_scale per cache, then the 64 rotated k_pe halves in fp16 --
// against the 1152 of the fp16 cache.  Three kernels:
//   mla_kv_append_e4m3_kernel  the row of mla_kv_append_kernel, quantised: single token (row ctx - 1) and bulk   (one wave per token)
//   mla_decode_e4m3_kernel     split-KV flash decode over such rows, 16 heads per workgroup                      (MFMA, the hot path)
//   mla_dequant_e4m3_kernel    rows t < ctx of one layer -> an fp16 latent cache of the same geometry            (the prompt path's bridge)
// The split partials are those of mla_decode_kernel, so mla_merge_kernel (mla.hip, mla_merge_launch) merges them.
//
// mla_decode_e4m3_kernel is the work split of mla_decode_kernel -- grid (splits, head_num / 16, batch), 4 waves, chunks of 256
// tokens in tiles of 32 keys, two LDS tile buffers of 592-half rows, S^T row-wise and O^T through ds_read_b64_tr_b16, the redundant
// softmax, one staging barrier and one logit-exchange barrier per tile -- behind a different staging path:
//   fetch    a tile is 32 rows x 640 bytes = 1280 pieces of 16 bytes, 5 per thread (9 in the fp16 kernel: 20 VGPRs in flight, not
//            36).  A row is 32 latent pieces + 8 rope pieces, so wave w takes rows 8 w .. 8 w + 7: latent piece i = 0..3 of a lane is
//            row 8 w + 2 i + (lane >> 5), column lane & 31; its rope piece is row 8 w + (lane >> 3), column lane & 7.  The row
//            of a piece is a constant plus a lane bit: no division, the tile's base is wave-uniform (one page lookup), the lane's
//            offset is 32 bits.  Rows at or past ctx re-read row ctx - 1 (same tile, same page) and are masked to -inf.
//   publish  every latent piece becomes 16 halves with v_cvt_scalef32_pk_f16_fp8 at scale 1.0 (two codes per instruction): each half
//            IS the code's value -- every finite e4m3 value, the subnormal codes included, is an fp16 normal --, so no power-of-two
//            factor rides along and no MFMA operand is subnormal.  The rope piece is stored as it came.
//   scale    c_scale never touches an fp16 operand.  Wave kk = 0 (dims 0..287) multiplies its logit partial by c_scale; wave
//            kk = 1 keeps two accumulators -- steps 0..6 are latent dims 288..511, steps 7..8 are k_pe -- and leaves
//            c_scale * s_lat + s_pe.  o is multiplied by c_scale once, in front of the partial store / the fp16 store.
// The chunking depends on ctx alone: a sequence's bits do not depend on the batch, its slot or the grid; dense = paged bit for bit.
#include "mla_common.cuh"

#include <cmath>
#include <cstdio>

namespace llmie {

namespace {

constexpr int kE4Stride = kRow + 16;   // the fp16 kernel's padded LDS row
static_assert(kPage % kMlaTile == 0 && kMlaChunk % kMlaTile == 0, "a tile never crosses a page or a chunk");
static_assert((kE4Stride * 2) % 64 == 32, "row stride = an odd multiple of 32 bytes: conflict-free transposed reads");
static_assert(kMlaTile == 32 && kLatPieces == 32 && kPePieces == 8, "the fetch layout: 4 waves x 8 rows, 4 latent + 1 rope piece per lane");

// 8 e4m3 codes (two words, memory order) -> the 8 halves of their exact values
__device__ __forceinline__ half8_t e4m3x8_to_f16(unsigned w0, unsigned w1) {
    const half2_t a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, true);
    const half2_t c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, true);
    return half8_t{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// ---- append: one wave per token.  cum == null: token = sequence b, row ctx_len[b] - 1 (mla_kv_append_kernel); else the packed
// token blockIdx.x of the bulk form (mla_kv_append_rows_kernel).  The fp16 row is computed exactly as there (include/llmie.h:
// lane i holds c[8 i .. 8 i + 7], fma chain, xor butterfly 32 .. 1), then code = e4m3(fp16 / c_scale), saturated.  The 640 bytes
// are put together in LDS and leave as 40 stores of 16 bytes. ----
__global__ __launch_bounds__(64) void mla_kv_append_e4m3_kernel(const half_t *__restrict__ kv_a, const half_t *__restrict__ gamma, float eps,
                                                                const float2 *__restrict__ rope, unsigned char *__restrict__ cache,
                                                                size_t layer_off, int max_seq_len, float c_scale,
                                                                const int32_t *__restrict__ ctx_len, const int32_t *__restrict__ cum,
                                                                const int32_t *__restrict__ hist, int batch, int max_q_len, int kv_span,
                                                                const int32_t *__restrict__ table, int max_pages) {
    __shared__ __attribute__((aligned(16))) unsigned char Rs[kRowE4];
    const int tok = blockIdx.x, lane = threadIdx.x;
    int b = tok, pos;
    if (cum) {
        if (tok >= cum[batch]) return;
        b = 0;   // the last sequence that begins at or in front of the token: an empty one shares its begin with its successor
        for (int hi = batch; hi - b > 1;) {
            const int mid = (b + hi) >> 1;
            if (cum[mid] <= tok) b = mid;
            else hi = mid;
        }
        const int len = cum[b + 1] - cum[b], history = hist[b];
        if (!(len >= 1 && len <= max_q_len && history >= 0 && history <= kv_span - len)) return;
        pos = history + tok - cum[b];
    } else {
        const int ctx = ctx_len[b];
        if (!mla_live(ctx, max_seq_len)) return;
        pos = ctx - 1;
    }
    const half_t *src = kv_a + static_cast<size_t>(tok) * kRow;
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
    float z[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = to_f32(from_f32<half_t>(to_f32(x[j]) * inv * to_f32(g[j]))) / c_scale;
    *reinterpret_cast<uint2 *>(Rs + 8 * lane) = make_uint2(pack4_e4m3(z[0], z[1], z[2], z[3]), pack4_e4m3(z[4], z[5], z[6], z[7]));
    if (lane < kRope / 2) {
        const float2 cs = rope[static_cast<size_t>(pos) * (kRope / 2) + lane];
        const float x0 = to_f32(src[kLat + lane]), x1 = to_f32(src[kLat + kRope / 2 + lane]);
        half_t *pe = reinterpret_cast<half_t *>(Rs + kLat);
        pe[lane] = from_f32<half_t>(x0 * cs.x - x1 * cs.y);
        pe[kRope / 2 + lane] = from_f32<half_t>(x1 * cs.x + x0 * cs.y);
    }
    __syncthreads();
    if (lane < kRowE4 / 16)
        *reinterpret_cast<uint4_t *>(cache + mla_row_off_bytes(table, max_pages, layer_off, b, pos, max_seq_len) + 16 * lane) =
            *reinterpret_cast<const uint4_t *>(Rs + 16 * lane);
}

// ---- dequant: grid (tiles of 32 tokens, batch), 5 pieces per thread; rows t < ctx of one layer, e4m3 -> fp16 ----
__global__ __launch_bounds__(256) void mla_dequant_e4m3_kernel(const unsigned char *__restrict__ src, half_t *__restrict__ dst, size_t src_off,
                                                               size_t dst_off, int max_seq_len, int max_ctx, float c_scale,
                                                               const int32_t *__restrict__ ctx_len, const int32_t *__restrict__ table,
                                                               int max_pages) {
    const int t0 = blockIdx.x * kMlaTile, b = blockIdx.y, tid = threadIdx.x;
    const int ctx = ctx_len[b];
    if (!mla_live(ctx, max_ctx) || t0 >= ctx) return;
    const size_t row0 = table ? static_cast<size_t>(table[static_cast<size_t>(b) * max_pages + t0 / kPage]) * kPage + t0 % kPage
                              : static_cast<size_t>(b) * max_seq_len + t0;
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

// ---- the attention ----
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void mla_decode_e4m3_kernel(
    const half_t *__restrict__ q_lat, const unsigned char *__restrict__ cache, half_t *__restrict__ o_lat, float *__restrict__ ws_o,
    float2 *__restrict__ ws_ml, const int32_t *__restrict__ ctx_len, const int32_t *__restrict__ table, int max_pages,
    size_t layer_off /* bytes */, int head_num, int max_seq_len, int max_ctx, float scale2 /* softmax_scale * log2(e) */, float c_scale) {
    __shared__ __attribute__((aligned(16))) half_t Ts[2][kMlaTile * kE4Stride];   // 2 x 37888 bytes: the codes' values || k_pe, in fp16
    __shared__ __attribute__((aligned(16))) float Sp[2 * 8 * 16 * 4];              // partial logits [kk][key / 4][head][key % 4]
    const int split = blockIdx.x, hb = blockIdx.y, b = blockIdx.z, splits = gridDim.x;
    const int ctx = ctx_len[b];
    if (!mla_live(ctx, max_ctx)) return;
    const int t_begin = split * kMlaChunk;
    if (t_begin >= ctx) return;
    const int n_tiles = (min(ctx, t_begin + kMlaChunk) - t_begin + kMlaTile - 1) / kMlaTile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int kh = wave & 1, kk = wave >> 1;
    const int head = hb * kMlaHeads + r;

    half8_t qf[9];   // Q[head r][288 kk + 32 s + 8 q ..]: the B operand of this wave's 9 steps
    {
        const half_t *qp = q_lat + (static_cast<size_t>(b) * head_num + head) * kRow + 288 * kk + 8 * q;
#pragma unroll
        for (int s = 0; s < 9; ++s) qf[s] = *reinterpret_cast<const half8_t *>(qp + 32 * s);
    }

    // staging: wave w owns rows 8 w .. 8 w + 7 of a tile
    const int lrow = 8 * wave + (lane >> 5), lcol = lane & 31;   // latent piece i: row lrow + 2 i, codes 16 lcol ..
    const int prow = 8 * wave + (lane >> 3), pcol = lane & 7;    // rope piece: halves kLat + 8 pcol ..
    uint4_t lreg[4];
    half8_t preg;
    auto fetch_tile = [&](int t0) {   // global -> registers; one page lookup per tile, wave-uniform
        const size_t row0 = table ? static_cast<size_t>(__builtin_amdgcn_readfirstlane(table[static_cast<size_t>(b) * max_pages + t0 / kPage])) * kPage + t0 % kPage
                                  : static_cast<size_t>(b) * max_seq_len + t0;
        const unsigned char *base = cache + layer_off + row0 * kRowE4;
        const int last = ctx - 1 - t0;   // >= 0; a row past it re-reads it (same tile, same page)
#pragma unroll
        for (int i = 0; i < 4; ++i) lreg[i] = *reinterpret_cast<const uint4_t *>(base + min(lrow + 2 * i, last) * kRowE4 + 16 * lcol);
        preg = *reinterpret_cast<const half8_t *>(base + min(prow, last) * kRowE4 + kLat + 16 * pcol);
    };
    auto publish_tile = [&](int buf) {   // registers -> LDS: codes to halves, padded rows
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            half_t *dst = Ts[buf] + (lrow + 2 * i) * kE4Stride + 16 * lcol;
            *reinterpret_cast<half8_t *>(dst) = e4m3x8_to_f16(lreg[i][0], lreg[i][1]);
            *reinterpret_cast<half8_t *>(dst + 8) = e4m3x8_to_f16(lreg[i][2], lreg[i][3]);
        }
        *reinterpret_cast<half8_t *>(Ts[buf] + prow * kE4Stride + kLat + 8 * pcol) = preg;
    };

    floatx4 o[8];   // O^T in units of c_scale: dims 128 wave + 16 dt + 4 q + e, column = head r
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) o[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;   // log2 domain, scale applied; l_run: this lane's 8 of a tile's 32 keys

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
        // ---- S^T partial: keys 16 kh + r, dims 288 kk ..; c_scale joins in fp32 ----
        {
            half8_t kf[9];
            const half_t *kp = Tt + (16 * kh + r) * kE4Stride + 288 * kk + 8 * q;
#pragma unroll
            for (int s = 0; s < 9; ++s) kf[s] = *reinterpret_cast<const half8_t *>(kp + 32 * s);
            floatx4 s_lat = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 7; ++s) s_lat = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[s], qf[s], s_lat, 0, 0, 0);
            floatx4 s_end = kk ? floatx4{0.f, 0.f, 0.f, 0.f} : s_lat;   // kk = 0: latent dims 224..287; kk = 1: k_pe, an accumulator of its own
            s_end = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[7], qf[7], s_end, 0, 0, 0);
            s_end = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[8], qf[8], s_end, 0, 0, 0);
            floatx4 sacc;   // sacc[e] = S[key 16 kh + 4 q + e][head r]
#pragma unroll
            for (int e = 0; e < 4; ++e) sacc[e] = kk ? __builtin_fmaf(c_scale, s_lat[e], s_end[e]) : c_scale * s_end[e];
            *reinterpret_cast<floatx4 *>(Sp + (((kk * 8 + 4 * kh + q) * 16 + r) << 2)) = sacc;
        }
        __syncthreads();   // both halves of every logit are there
        float s8[8];       // keys t0 + 16 (j >> 2) + 4 q + (j & 3): the k index 8 q + j of the P^T operand
        {
            const floatx4 a0 = *reinterpret_cast<const floatx4 *>(Sp + (((0 * 8 + q) * 16 + r) << 2));
            const floatx4 b0 = *reinterpret_cast<const floatx4 *>(Sp + (((1 * 8 + q) * 16 + r) << 2));
            const floatx4 a1 = *reinterpret_cast<const floatx4 *>(Sp + (((0 * 8 + 4 + q) * 16 + r) << 2));
            const floatx4 b1 = *reinterpret_cast<const floatx4 *>(Sp + (((1 * 8 + 4 + q) * 16 + r) << 2));
#pragma unroll
            for (int e = 0; e < 4; ++e) s8[e] = a0[e] + b0[e], s8[4 + e] = a1[e] + b1[e];
        }
        float mloc = -INFINITY;
        if (t0 + kMlaTile > ctx) {   // wave-uniform: only the context's last tile masks
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int t = t0 + 16 * (j >> 2) + 4 * q + (j & 3);
                s8[j] = t < ctx ? s8[j] : -INFINITY;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) mloc = fmaxf(mloc, s8[j]);
        mloc = lane_xor_max<16>(lane_xor_max<32>(mloc)) * scale2;   // over the 4 lanes of head r; scale2 > 0; key t0 < ctx: finite
        const float m_new = fmaxf(m_run, mloc);
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);   // first tile: 2^(-inf) = 0
        float lsum = 0.f;
        half8_t pf;
        typedef float float2v_t __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
            const float p0 = __builtin_amdgcn_exp2f(__builtin_fmaf(s8[j], scale2, -m_new));
            const float p1 = __builtin_amdgcn_exp2f(__builtin_fmaf(s8[j + 1], scale2, -m_new));
            lsum += p0 + p1;
            const half2_t hh = __builtin_convertvector(float2v_t{p0, p1}, half2_t);
            pf[j] = hh[0];
            pf[j + 1] = hh[1];
        }
        l_run = l_run * alpha + lsum;
        m_run = m_new;
        if (__builtin_amdgcn_ballot_w64(alpha != 1.0f)) {
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) o[dt] *= alpha;
        }
        // ---- O^T += C^T . P^T: A fragment = C[key(q, j)][128 wave + 16 dt + r], gathered down a column by the transposed read ----
        {
            const half_t *blk = Tt + (4 * q + (r >> 2)) * kE4Stride + 128 * wave + 4 * (r & 3);
            fp16x4_t lo[8], hi[8];
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                lo[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(blk + dt * 16));
                hi[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(blk + 16 * kE4Stride + dt * 16));
            }
#pragma unroll
            for (int dt = 0; dt < 8; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, Tr8{lo[dt], hi[dt]}), pf, o[dt], 0, 0, 0);
        }
    }
    const float l = lane_xor_sum<32>(lane_xor_sum<16>(l_run));
    const size_t bh = static_cast<size_t>(b) * head_num + head;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) o[dt] *= c_scale;   // the one place the output meets c_scale
    if (splits == 1) {   // the only split: the output itself
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
        if (wave == 0 && q == 0) ws_ml[bh * splits + split] = make_float2(m_run, l);
    }
}

inline bool scale_ok(float c_scale) { return c_scale > 0.f && std::isfinite(c_scale); }

}  // namespace

}  // namespace llmie

using namespace llmie;

extern "C" const char *llmie_mla_decode_e4m3_plan(int batch, int head_num, int max_seq_len, int max_ctx, int paged, int max_pages, int num_pages,
                                                  long long workspace_bytes, int *status) {
    static thread_local char text[176];
    MlaDecodePlan p{};
    const MlaDecodeCall c{batch, head_num, max_seq_len, max_ctx, paged != 0, max_pages, num_pages, workspace_bytes >= 0,
                          workspace_bytes >= 0 ? static_cast<size_t>(workspace_bytes) : 0, true};
    const int rc = plan_mla_decode("mla_decode_e4m3_plan", c, &p);
    if (status) *status = rc;
    if (rc != LLMIE_OK) return nullptr;
    int n = snprintf(text, sizeof(text), "mla e4m3 nh%d hb%d tile%d chunk%d row%d grid %dx%dx%d merge ", head_num, p.heads, p.tile, p.chunk,
                     p.row_bytes, p.grid[0], p.grid[1], p.grid[2]);
    if (p.merge) snprintf(text + n, sizeof(text) - n, "%dx%d/%d", p.merge_grid[0], p.merge_grid[1], p.merge_block);
    else snprintf(text + n, sizeof(text) - n, "none");
    return text;
}

extern "C" int llmie_mla_kv_append_e4m3(const void *kv_a, const void *gamma, float eps, const void *rope_table, void *cache, float c_scale,
                                        int layer, int batch, int max_seq_len, const int32_t *ctx_len_dev, const int32_t *block_table,
                                        int max_pages, int num_pages, llmie_stream stream) {
    LLMIE_REQUIRE(kv_a && gamma && rope_table && cache && ctx_len_dev, "mla_kv_append_e4m3: NULL operand");
    LLMIE_REQUIRE(batch >= 1 && layer >= 0, "mla_kv_append_e4m3: batch=%d should be >= 1 and layer=%d >= 0", batch, layer);
    LLMIE_REQUIRE(eps > 0.f, "mla_kv_append_e4m3: eps should be > 0");
    LLMIE_REQUIRE(scale_ok(c_scale), "mla_kv_append_e4m3: c_scale should be positive and finite");
    const int rc = mla_cache_check("mla_kv_append_e4m3", max_seq_len, block_table != nullptr, max_pages, num_pages);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(mis16(kv_a) == 0 && mis16(gamma) == 0 && mis16(cache) == 0, "mla_kv_append_e4m3: kv_a, gamma and the cache should be 16-byte aligned");
    hipLaunchKernelGGL(mla_kv_append_e4m3_kernel, dim3(batch), dim3(64), 0, as_stream(stream), static_cast<const half_t *>(kv_a),
                       static_cast<const half_t *>(gamma), eps, static_cast<const float2 *>(rope_table), static_cast<unsigned char *>(cache),
                       mla_layer_off_bytes(layer, batch, max_seq_len, block_table != nullptr, num_pages), max_seq_len, c_scale, ctx_len_dev,
                       static_cast<const int32_t *>(nullptr), static_cast<const int32_t *>(nullptr), batch, 0, 0, block_table, max_pages);
    return launch_status("mla_kv_append_e4m3");
}

extern "C" int llmie_mla_kv_append_rows_e4m3(const void *kv_a, const void *gamma, float eps, const void *rope_table, void *cache, float c_scale,
                                             int layer, int batch, int total_tokens, int max_q_len, int kv_span, int max_seq_len,
                                             const int32_t *cum_dev, const int32_t *hist_dev, const int32_t *block_table, int max_pages,
                                             int num_pages, llmie_stream stream) {
    LLMIE_REQUIRE(kv_a && gamma && rope_table && cache && cum_dev && hist_dev, "mla_kv_append_rows_e4m3: NULL operand");
    LLMIE_REQUIRE(layer >= 0 && total_tokens >= 1, "mla_kv_append_rows_e4m3: layer=%d should be >= 0 and total_tokens=%d >= 1", layer, total_tokens);
    LLMIE_REQUIRE(eps > 0.f, "mla_kv_append_rows_e4m3: eps should be > 0");
    LLMIE_REQUIRE(scale_ok(c_scale), "mla_kv_append_rows_e4m3: c_scale should be positive and finite");
    MlaPrefillPlan p{};
    const int rc = plan_mla_prefill("mla_kv_append_rows_e4m3",
                                    MlaPrefillCall{batch, 0, total_tokens, max_q_len, kv_span, max_seq_len, block_table != nullptr, max_pages, num_pages}, &p);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(mis16(kv_a) == 0 && mis16(gamma) == 0 && mis16(cache) == 0,
                  "mla_kv_append_rows_e4m3: kv_a, gamma and the cache should be 16-byte aligned");
    hipLaunchKernelGGL(mla_kv_append_e4m3_kernel, dim3(p.append_grid), dim3(64), 0, as_stream(stream), static_cast<const half_t *>(kv_a),
                       static_cast<const half_t *>(gamma), eps, static_cast<const float2 *>(rope_table), static_cast<unsigned char *>(cache),
                       mla_layer_off_bytes(layer, batch, max_seq_len, block_table != nullptr, num_pages), max_seq_len, c_scale,
                       static_cast<const int32_t *>(nullptr), cum_dev, hist_dev, batch, max_q_len, kv_span, block_table, max_pages);
    return launch_status("mla_kv_append_rows_e4m3");
}

extern "C" int llmie_mla_decode_e4m3(const void *q_lat, const void *cache, void *o_lat, int layer, int batch, int head_num, int max_seq_len,
                                     int max_ctx, const int32_t *ctx_len_dev, float softmax_scale, void *workspace, size_t workspace_bytes,
                                     const int32_t *block_table, int max_pages, int num_pages, float c_scale, llmie_stream stream) {
    LLMIE_REQUIRE(q_lat && cache && o_lat && ctx_len_dev, "mla_decode_e4m3: NULL operand");
    LLMIE_REQUIRE(layer >= 0, "mla_decode_e4m3: layer=%d should be >= 0", layer);
    LLMIE_REQUIRE(softmax_scale > 0.f && std::isfinite(softmax_scale), "mla_decode_e4m3: softmax_scale should be positive and finite");
    LLMIE_REQUIRE(scale_ok(c_scale), "mla_decode_e4m3: c_scale should be positive and finite");
    MlaDecodePlan p{};
    const MlaDecodeCall c{batch, head_num, max_seq_len, max_ctx, block_table != nullptr, max_pages, num_pages, workspace != nullptr, workspace_bytes, true};
    const int rc = plan_mla_decode("mla_decode_e4m3", c, &p);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(mis16(q_lat) == 0 && mis16(cache) == 0 && mis16(o_lat) == 0 && (!p.merge || mis16(workspace) == 0),
                  "mla_decode_e4m3: q_lat, the cache, o_lat and the workspace should be 16-byte aligned");
    float *ws_o = static_cast<float *>(workspace);
    float2 *ws_ml = p.merge ? reinterpret_cast<float2 *>(ws_o + static_cast<size_t>(batch) * head_num * p.grid[0] * kLat) : nullptr;
    hipLaunchKernelGGL(mla_decode_e4m3_kernel, dim3(p.grid[0], p.grid[1], p.grid[2]), dim3(256), 0, as_stream(stream),
                       static_cast<const half_t *>(q_lat), static_cast<const unsigned char *>(cache), static_cast<half_t *>(o_lat), ws_o, ws_ml,
                       ctx_len_dev, block_table, max_pages, mla_layer_off_bytes(layer, batch, max_seq_len, block_table != nullptr, num_pages),
                       head_num, max_seq_len, p.span, softmax_scale * 1.44269504088896341f, c_scale);
    if (p.merge) mla_merge_launch(p, ws_o, ws_ml, static_cast<half_t *>(o_lat), ctx_len_dev, head_num, as_stream(stream));
    return launch_status("mla_decode_e4m3");
}

extern "C" int llmie_mla_cache_dequant_e4m3(const void *cache_e4m3, void *cache_f16, float c_scale, int layer, int batch, int max_seq_len,
                                            int max_ctx, const int32_t *ctx_len_dev, const int32_t *block_table, int max_pages, int num_pages,
                                            llmie_stream stream) {
    LLMIE_REQUIRE(cache_e4m3 && cache_f16 && ctx_len_dev, "mla_cache_dequant_e4m3: NULL operand");
    LLMIE_REQUIRE(batch >= 1 && batch <= 65535 && layer >= 0, "mla_cache_dequant_e4m3: batch=%d should be in [1, 65535] and layer=%d >= 0", batch, layer);
    LLMIE_REQUIRE(scale_ok(c_scale), "mla_cache_dequant_e4m3: c_scale should be positive and finite");
    const bool paged = block_table != nullptr;
    const int rc = mla_cache_check("mla_cache_dequant_e4m3", max_seq_len, paged, max_pages, num_pages);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(max_ctx >= 0 && max_ctx <= max_seq_len, "mla_cache_dequant_e4m3: max_ctx=%d should be 0 or in [1, max_seq_len=%d]", max_ctx, max_seq_len);
    LLMIE_REQUIRE(mis16(cache_e4m3) == 0 && mis16(cache_f16) == 0, "mla_cache_dequant_e4m3: both caches should be 16-byte aligned");
    const int span = max_ctx > 0 ? max_ctx : max_seq_len;
    hipLaunchKernelGGL(mla_dequant_e4m3_kernel, dim3((span + kMlaTile - 1) / kMlaTile, batch), dim3(256), 0, as_stream(stream),
                       static_cast<const unsigned char *>(cache_e4m3), static_cast<half_t *>(cache_f16),
                       mla_layer_off_bytes(layer, batch, max_seq_len, paged, num_pages), mla_layer_off(layer, batch, max_seq_len, paged, num_pages),
                       max_seq_len, span, c_scale, ctx_len_dev, block_table, max_pages);
    return launch_status("mla_cache_dequant_e4m3");
}
