// The split-KV tile loop of the MLA decode step, written once for mla_decode_kernel<E4> (mla.hip: positions t < ctx of a sequence) and
// mla_sparse_attend_kernel (mla_sparse.hip: entries j < count of a selection).  A workgroup of 4 waves walks one chunk of kMlaChunk
// units in tiles of kMlaTile rows for 16 heads: staging (two LDS buffers, the next-but-one tile in flight in registers), the S^T MFMA
// chain, the logit exchange, the log2-domain online softmax, the transposed-read O^T accumulation and the partial's store.  The head
// comment of mla.hip says how each works.  What the two kernels do not share is where a tile's 32 rows lie -- the row source below --
// and what the loop counts against: `n` units, ctx or count.  Only mla.hip and mla_sparse.hip include this file; mla_verify_kernel
// is another algorithm (several column blocks per staged fragment) and keeps its own loop.
#pragma once
#include "mla_common.cuh"

#include <type_traits>

namespace llmie {

template <bool E4> using cache_elem_t = std::conditional_t<E4, unsigned char, half_t>;   // the e4m3 cache is addressed in bytes

// ---- row sources: tile(it) is tile `it` of the chunk, its row(r) where row r = 0 .. 31 of that tile begins in the cache; ready()
// runs once, behind the loop's q loads and in front of its first tile() ----
// Contiguous: positions begin + 32 it + r of sequence b.  One page lookup per tile, wave-uniform; a row past the last of the n
// positions re-reads the last (same tile, same page); 32-bit offsets inside the tile.
template <bool E4>
struct MlaContiguousRows {
    const cache_elem_t<E4> *layer;
    const int32_t *table;
    int max_pages, b, max_seq_len, begin, n;
    struct Tile {
        const cache_elem_t<E4> *base;
        int last;   // >= 0
        __device__ __forceinline__ const cache_elem_t<E4> *row(int r) const { return base + min(r, last) * (E4 ? kRowE4 : kRow); }
    };
    __device__ __forceinline__ void ready() const {}
    __device__ __forceinline__ Tile tile(int it) const {
        const int t0 = begin + it * kMlaTile;
        return Tile{layer + mla_tile_row0(table, max_pages, b, t0, max_seq_len) * (E4 ? kRowE4 : kRow), n - 1 - t0};
    }
};
// Gathered: rw[32 it + r] in LDS is the row's number inside the layer; the kernel has written rw[0 .. kMlaChunk), one entry per
// thread, and ready() is the barrier behind those writes.  It stands behind the loop's q loads, not in the kernel: no q load may
// be scheduled among the tile loads, or the loop waits for every load in flight in front of its last S^T step.
// Every piece of a row sits behind one LDS read, no dependent chain of global loads.
struct MlaGatheredRows {
    const half_t *layer;
    const int *rw;
    struct Tile {
        const half_t *layer;
        const int *rw;
        __device__ __forceinline__ const half_t *row(int r) const { return layer + static_cast<size_t>(rw[r]) * kRow; }
    };
    __device__ __forceinline__ void ready() const { __syncthreads(); }
    __device__ __forceinline__ Tile tile(int it) const { return Tile{layer, rw + it * kMlaTile}; }
};

// ---- the loop, for split blockIdx.x of the 16 heads blockIdx.y of sequence b: units begin .. min(n, begin + kMlaChunk) - 1, begin < n.
// E4 = false: fp16 rows, no c_scale.  E4 = true (rows in bytes) differs in three places, each behind `if constexpr`:
//   fetch    a tile is 32 rows x 640 bytes = 1280 pieces of 16 bytes, 5 per thread (9 in the fp16 form: 20 VGPRs in flight, not 36).
//            A row is 32 latent pieces + 8 rope pieces, so wave w takes rows 8 w .. 8 w + 7: latent piece i = 0..3 of a lane is row
//            8 w + 2 i + (lane >> 5), column lane & 31; its rope piece is row 8 w + (lane >> 3), column lane & 7: no division.
//   publish  every latent piece becomes 16 halves with v_cvt_scalef32_pk_f16_fp8 at scale 1.0 (two codes per instruction): each half
//            IS the code's value -- every finite e4m3 value, the subnormal codes included, is an fp16 normal --, so no power-of-two
//            factor rides along and no MFMA operand is subnormal.  The rope piece is stored as it came.
//   scale    c_scale never touches an fp16 operand.  Wave kk = 0 (dims 0..287) multiplies its logit partial by c_scale; wave
//            kk = 1 keeps two accumulators -- steps 0..6 are latent dims 288..511, steps 7..8 are k_pe -- and leaves
//            c_scale * s_lat + s_pe.  o is multiplied by c_scale once, in front of the store. ----
template <bool E4, typename Rows, typename... Scale>
__device__ __forceinline__ void mla_split_tiles(const half_t *__restrict__ q_lat, const Rows &rows, half_t *__restrict__ o_lat,
                                                float *__restrict__ ws_o, float2 *__restrict__ ws_ml, int b, int head_num, int begin, int n,
                                                float scale2 /* softmax_scale * log2(e) */, const Scale... c_scale /* E4 */) {
    static_assert(sizeof...(Scale) == (E4 ? 1 : 0), "c_scale");
    static_assert(kMlaTile == 32 && kLatPieces == 32 && kPePieces == 8, "the e4m3 fetch layout: 4 waves x 8 rows, 4 latent + 1 rope piece per lane");
    __shared__ __attribute__((aligned(16))) half_t Ts[2][kMlaTile * kMlaStride];   // 2 x 37888 bytes (E4: the codes' values || k_pe, in fp16)
    __shared__ __attribute__((aligned(16))) float Sp[2 * 8 * 16 * 4];                // partial logits [kk][key / 4][head][key % 4]
    const int split = blockIdx.x, hb = blockIdx.y, splits = gridDim.x;
    const int n_tiles = (min(n, begin + kMlaChunk) - begin + kMlaTile - 1) / kMlaTile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int kh = wave & 1, kk = wave >> 1;
    const size_t bh = static_cast<size_t>(b) * head_num + hb * kMlaHeads + r;

    half8_t qf[9];   // Q[head r][288 kk + 32 s + 8 q ..]: the B operand of this wave's 9 steps
    {
        const half_t *qp = q_lat + bh * kRow + 288 * kk + 8 * q;
#pragma unroll
        for (int s = 0; s < 9; ++s) qf[s] = *reinterpret_cast<const half8_t *>(qp + 32 * s);
    }

    constexpr int NCH = E4 ? 5 : kMlaTile * kRow / 8 / 256;   // sixteen-byte pieces of a tile per thread (fp16: 9)
    half8_t treg[NCH];
    // E4 staging: wave w owns rows 8 w .. 8 w + 7 of a tile
    const int lrow = 8 * wave + (lane >> 5), lcol = lane & 31;   // latent piece i: row lrow + 2 i, codes 16 lcol ..
    const int prow = 8 * wave + (lane >> 3), pcol = lane & 7;    // rope piece: halves kLat + 8 pcol ..
    auto fetch_tile = [&](int it) {   // global -> registers
        const auto tile = rows.tile(it);
        if constexpr (E4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) treg[i] = *reinterpret_cast<const half8_t *>(tile.row(lrow + 2 * i) + 16 * lcol);
            treg[4] = *reinterpret_cast<const half8_t *>(tile.row(prow) + kLat + 16 * pcol);
        } else {
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int id = tid + 256 * i, row = id / (kRow / 8), ch = id - row * (kRow / 8);
                treg[i] = *reinterpret_cast<const half8_t *>(tile.row(row) + ch * 8);
            }
        }
    };
    auto publish_tile = [&](int buf) {   // registers -> LDS, padded rows (E4: codes to halves)
        if constexpr (E4) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint4_t w = __builtin_bit_cast(uint4_t, treg[i]);
                half_t *dst = Ts[buf] + (lrow + 2 * i) * kMlaStride + 16 * lcol;
                *reinterpret_cast<half8_t *>(dst) = e4m3x8_to_f16(w[0], w[1]);
                *reinterpret_cast<half8_t *>(dst + 8) = e4m3x8_to_f16(w[2], w[3]);
            }
            *reinterpret_cast<half8_t *>(Ts[buf] + prow * kMlaStride + kLat + 8 * pcol) = treg[4];
        } else {
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int id = tid + 256 * i, row = id / (kRow / 8), ch = id - row * (kRow / 8);
                *reinterpret_cast<half8_t *>(Ts[buf] + row * kMlaStride + ch * 8) = treg[i];
            }
        }
    };

    floatx4 o[8];   // O^T (E4: in units of c_scale): dims 128 wave + 16 dt + 4 q + e, column = head r
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) o[dt] = floatx4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;   // log2 domain, scale applied; l_run: this lane's 8 of a tile's 32 keys

    rows.ready();
    fetch_tile(0);
    publish_tile(0);
    if (1 < n_tiles) fetch_tile(1);
    for (int it = 0; it < n_tiles; ++it) {
        const int u0 = begin + it * kMlaTile;
        const half_t *Tt = Ts[it & 1];
        __syncthreads();   // tile `it` published; every wave done with tile it - 1 (the other buffer) and with its logits
        if (it + 1 < n_tiles) {
            publish_tile((it + 1) & 1);
            if (it + 2 < n_tiles) fetch_tile(it + 2);   // in flight under this iteration's MFMAs
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- S^T partial: keys 16 kh + r, dims 288 kk .. (E4: c_scale joins in fp32) ----
        {
            half8_t kf[9];
            const half_t *kp = Tt + (16 * kh + r) * kMlaStride + 288 * kk + 8 * q;
#pragma unroll
            for (int s = 0; s < 9; ++s) kf[s] = *reinterpret_cast<const half8_t *>(kp + 32 * s);
            floatx4 sacc = {0.f, 0.f, 0.f, 0.f};   // sacc[e] = S[key 16 kh + 4 q + e][head r]
#pragma unroll
            for (int s = 0; s < 7; ++s) sacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[s], qf[s], sacc, 0, 0, 0);
            if constexpr (E4) {
                const floatx4 s_lat = sacc;
                floatx4 s_end = kk ? floatx4{0.f, 0.f, 0.f, 0.f} : s_lat;   // kk = 0: latent dims 224..287; kk = 1: k_pe, an accumulator of its own
                s_end = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[7], qf[7], s_end, 0, 0, 0);
                s_end = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[8], qf[8], s_end, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    sacc[e] = kk ? __builtin_fmaf(pack_arg<0>(c_scale...), s_lat[e], s_end[e]) : pack_arg<0>(c_scale...) * s_end[e];
            } else {
                sacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[7], qf[7], sacc, 0, 0, 0);
                sacc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[8], qf[8], sacc, 0, 0, 0);
            }
            *reinterpret_cast<floatx4 *>(Sp + (((kk * 8 + 4 * kh + q) * 16 + r) << 2)) = sacc;
        }
        __syncthreads();   // both halves of every logit are there
        float s8[8];       // units u0 + 16 (j >> 2) + 4 q + (j & 3): the k index 8 q + j of the P^T operand
        {
            const floatx4 a0 = *reinterpret_cast<const floatx4 *>(Sp + (((0 * 8 + q) * 16 + r) << 2));
            const floatx4 b0 = *reinterpret_cast<const floatx4 *>(Sp + (((1 * 8 + q) * 16 + r) << 2));
            const floatx4 a1 = *reinterpret_cast<const floatx4 *>(Sp + (((0 * 8 + 4 + q) * 16 + r) << 2));
            const floatx4 b1 = *reinterpret_cast<const floatx4 *>(Sp + (((1 * 8 + 4 + q) * 16 + r) << 2));
#pragma unroll
            for (int e = 0; e < 4; ++e) s8[e] = a0[e] + b0[e], s8[4 + e] = a1[e] + b1[e];
        }
        float mloc = -INFINITY;
        if (u0 + kMlaTile > n) {   // wave-uniform: only the last tile of the n units masks
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int u = u0 + 16 * (j >> 2) + 4 * q + (j & 3);
                s8[j] = u < n ? s8[j] : -INFINITY;
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) mloc = fmaxf(mloc, s8[j]);
        mloc = lane_xor_max<16>(lane_xor_max<32>(mloc)) * scale2;   // over the 4 lanes of head r; scale2 > 0; unit u0 < n: finite
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
            const half_t *blk = Tt + (4 * q + (r >> 2)) * kMlaStride + 128 * wave + 4 * (r & 3);
            fp16x4_t lo[8], hi[8];
#pragma unroll
            for (int dt = 0; dt < 8; ++dt) {
                lo[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(blk + dt * 16));
                hi[dt] = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4_ptr)(blk + 16 * kMlaStride + dt * 16));
            }
#pragma unroll
            for (int dt = 0; dt < 8; ++dt)
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, Tr8{lo[dt], hi[dt]}), pf, o[dt], 0, 0, 0);
        }
    }
    const float l = lane_xor_sum<32>(lane_xor_sum<16>(l_run));
    if constexpr (E4) {
#pragma unroll
        for (int dt = 0; dt < 8; ++dt) o[dt] *= pack_arg<0>(c_scale...);   // the one place the output meets c_scale
    }
    mla_store_split(o, m_run, l, bh, split, splits, wave, q, o_lat, ws_o, ws_ml);
}

}  // namespace llmie
