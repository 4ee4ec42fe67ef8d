// Multi-LoRA: per-row adapters on top of a projection (llmie_lora_*; include/llmie.h states the semantics).  No reference launcher.
//
// Three kernels, gfx950:
//   plan    one workgroup per forward call: the effective slot of every row (for prefill: the sequence's slot expanded over the
//           lengths; -1 for rows without a loaded adapter), then the rows of each slot, in row order, cut into tiles of <= 16.  One
//           wave per slot walks the row slots 64 at a time (ballots): the row order inside a slot is the row order of the call.
//   shrink  grid (tiles, K slices), 4 waves: t = x . A^T of one tile over one K slice by v_mfma_f32_16x16x32_f16.  x rows and A rows
//           are both contiguous along K, so lane l loads row l & 15, k = 8 (l >> 4) .. + 7 of either operand as ONE 16-byte global
//           load and no LDS transposition is needed.  The waves take the slice's k-steps round robin, two steps of loads in flight
//           each, and their accumulators are summed through LDS in a fixed order.  The A matrix is read once per tile.
//   expand  grid (tiles, groups of 256 columns), 4 waves x 4 column tiles: sums the K slices' partials (fixed order), rounds t to
//           fp16 once and computes the TRANSPOSED product B . t^T (B rows as the A operand: 16-byte loads again), so a lane holds 4
//           consecutive output columns of one row: scale, then an 8-byte read-modify-write of y.  A row belongs to one tile: no race.
// Surplus tiles (the grids are sized to the host bound rows / 16 + min(slots, rows)) exit on the plan's tile count.
#include "llmie_internal.h"

namespace llmie {
namespace {

constexpr int kLoraMagic = 0x4c6f5241;
constexpr int kLoraTileRows = 16;
constexpr int kLoraMaxRankTotal = 3 * 64;
constexpr int kLoraPlanThreads = 256;
constexpr int kLoraWaves = 4;
constexpr int kLoraExpandCols = 256;   // columns per expand workgroup: 4 waves x 4 tiles of 16

struct LoraSlotHdr {
    int32_t rank;
    float scale;
    int32_t pad[2];
};
static_assert(sizeof(LoraSlotHdr) == 16, "table layout");

__host__ __device__ inline size_t lora_align(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }
__host__ __device__ inline int lora_tiles(int rows, int slots) { return rows / kLoraTileRows + (slots < rows ? slots : rows); }
inline bool lora_rank_ok(int r) { return r == 8 || r == 16 || r == 32 || r == 64; }

// the workspace: [header | row_slot[rows] | tile_slot[tiles] | tile_rows[tiles][16] | partials], offsets a function of (rows, slots)
struct LoraWs {
    size_t row_slot, tile_slot, tile_rows, partial, fixed;
    int tiles;
};
inline LoraWs lora_ws(int rows, int slots) {
    LoraWs w;
    w.tiles = lora_tiles(rows, slots);
    size_t off = 256;
    w.row_slot = off, off += lora_align(4 * static_cast<size_t>(rows));
    w.tile_slot = off, off += lora_align(4 * static_cast<size_t>(w.tiles));
    w.tile_rows = off, off += lora_align(64 * static_cast<size_t>(w.tiles));
    w.partial = off;
    w.fixed = off;
    return w;
}
inline size_t lora_partial_bytes(int tiles, int rank_total) {
    return lora_align(static_cast<size_t>(LLMIE_LORA_MAX_KSPLIT) * tiles * kLoraTileRows * rank_total * sizeof(float));
}
// K slices of the shrink launch: a function of K alone
inline int lora_ksplit(int K) {
    const int ks = K / 512;
    return ks < 1 ? 1 : (ks > LLMIE_LORA_MAX_KSPLIT ? LLMIE_LORA_MAX_KSPLIT : ks);
}

struct LoraSlotStore {   // one launch's worth of llmie_lora_slot_load, by value in the kernel arguments
    int slot, layers, layer0, count, write_hdr;
    LoraSlotHdr hdr;
    const void *ptr[16][8];
};

__global__ __launch_bounds__(128) void lora_slot_store_kernel(unsigned char *table, int slots, const LoraSlotStore s) {
    const int i = threadIdx.x;
    if (i == 0 && s.write_hdr) reinterpret_cast<LoraSlotHdr *>(table)[s.slot] = s.hdr;
    if (i < s.count * 8) {
        const void **ptrs = reinterpret_cast<const void **>(table + static_cast<size_t>(slots) * sizeof(LoraSlotHdr));
        ptrs[(static_cast<size_t>(s.slot) * s.layers + s.layer0) * 8 + i] = s.ptr[i / 8][i % 8];
    }
}

// hdr: {magic, rows, slots, tiles in use}
__global__ __launch_bounds__(kLoraPlanThreads) void lora_plan_kernel(const int32_t *__restrict__ slot, const int32_t *__restrict__ lengths, int batch,
                                                                      int rows, const unsigned char *__restrict__ table, int slots, int32_t *hdr,
                                                                      int32_t *row_slot, int32_t *tile_slot, int32_t *tile_rows, int tiles) {
    __shared__ int32_t s_base[LLMIE_LORA_MAX_SLOTS + 1];
    const LoraSlotHdr *th = reinterpret_cast<const LoraSlotHdr *>(table);
    // the effective slot of every row
    for (int t = threadIdx.x; t < rows; t += kLoraPlanThreads) {
        int s;
        if (lengths) {
            int b = 0, acc = 0;
            while (b < batch) {
                const int len = max(lengths[b], 0);
                if (t < acc + len) break;
                acc += len, ++b;
            }
            s = b < batch ? slot[b] : -1;
        } else {
            s = slot[t];
        }
        if (s < 0 || s >= slots) s = -1;
        if (s >= 0) {
            const int r = th[s].rank;
            if (r != 8 && r != 16 && r != 32 && r != 64) s = -1;
        }
        row_slot[t] = s;
    }
    __syncthreads();
    // rows per slot -> tiles per slot: one WAVE per slot walks the rows 64 at a time (a ballot counts the matches)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int s = wave; s < slots; s += kLoraPlanThreads / 64) {
        int n = 0;
        for (int t0 = 0; t0 < rows; t0 += 64) {
            const int t = t0 + lane;
            n += __popcll(__ballot(t < rows && row_slot[t] == s));
        }
        if (lane == 0) s_base[s + 1] = (n + kLoraTileRows - 1) / kLoraTileRows;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        s_base[0] = 0;
        for (int s = 0; s < slots; ++s) acc += s_base[s + 1], s_base[s + 1] = acc;
    }
    __syncthreads();
    const int used = min(s_base[slots], tiles);
    // the rows of a slot in row order: a row's place is the matches in front of it (earlier chunks, lower lanes of its own)
    for (int s = wave; s < slots; s += kLoraPlanThreads / 64) {
        const int base = s_base[s], end = s_base[s + 1];
        if (base == end || end > tiles) continue;
        int32_t *out = tile_rows + static_cast<size_t>(base) * kLoraTileRows;
        int i = 0;
        for (int t0 = 0; t0 < rows; t0 += 64) {
            const int t = t0 + lane;
            const bool hit = t < rows && row_slot[t] == s;
            const unsigned long long m = __ballot(hit);
            if (hit) out[i + __popcll(m & ((1ull << lane) - 1))] = t;
            i += __popcll(m);
        }
        for (int p = i + lane; p < (end - base) * kLoraTileRows; p += 64) out[p] = -1;
        for (int ti = base + lane; ti < end; ti += 64) tile_slot[ti] = s;
    }
    for (int ti = used + threadIdx.x; ti < tiles; ti += kLoraPlanThreads) tile_slot[ti] = -1;
    if (threadIdx.x == 0) {
        hdr[0] = kLoraMagic, hdr[1] = rows, hdr[2] = slots, hdr[3] = used;
    }
}

struct LoraApplyArgs {
    const half_t *x;
    half_t *y;
    int rows, K, N, blocks, col1, col2;   // column blocks: [0, col1), [col1, col2), [col2, N)
    const unsigned char *table;
    int slots, layers, layer, module;
    const int32_t *hdr, *tile_slot, *tile_rows;
    float *partial;
    int tiles, rt_max, ksplit, slice_steps;   // rt_max = blocks * 64: the row stride unit of the partials
};

// the tile's slot, or -1 (surplus tile; the plan in the workspace is not this call's; the adapter lacks the module)
__device__ __forceinline__ int lora_tile(const LoraApplyArgs &a, int ti, int *rank, float *scale, const half_t **A, const half_t **B) {
    if (a.hdr[0] != kLoraMagic || a.hdr[1] != a.rows || a.hdr[2] != a.slots || ti >= a.hdr[3]) return -1;
    const int s = a.tile_slot[ti];
    if (s < 0 || s >= a.slots) return -1;
    const LoraSlotHdr h = reinterpret_cast<const LoraSlotHdr *>(a.table)[s];
    if (h.rank != 8 && h.rank != 16 && h.rank != 32 && h.rank != 64) return -1;
    const half_t *const *p = reinterpret_cast<const half_t *const *>(a.table + static_cast<size_t>(a.slots) * sizeof(LoraSlotHdr)) +
                             ((static_cast<size_t>(s) * a.layers + a.layer) * 4 + a.module) * 2;
    *A = p[0], *B = p[1];
    if (!*A || !*B) return -1;
    *rank = h.rank, *scale = h.scale;
    return s;
}

// one wave, its k-steps of one slice: acc[nt] += x frag x A frag of column tile nt (NT tiles; A rows clamped to R - 1: the columns
// behind R are never read)
template <int NT>
__device__ __forceinline__ void lora_shrink_wave(const half_t *__restrict__ xrow, const half_t *__restrict__ A, int K, int R, int lane, int k_begin,
                                                 int k_end, float *red /* this wave's [16][NT * 16] */) {
    floatx4 acc[NT];
    const half_t *arow[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        acc[nt] = floatx4{0.f, 0.f, 0.f, 0.f};
        arow[nt] = A + static_cast<size_t>(min(nt * 16 + (lane & 15), R - 1)) * K + 8 * (lane >> 4);
    }
    const half_t *xp = xrow + 8 * (lane >> 4);
    constexpr int kStride = 32 * kLoraWaves;
    int k = k_begin;
    // two k-steps of loads in flight: the second step's fragments are requested before the first step's MFMAs issue
    for (; k + kStride < k_end; k += 2 * kStride) {
        half8_t x0 = *reinterpret_cast<const half8_t *>(xp + k), x1 = *reinterpret_cast<const half8_t *>(xp + k + kStride);
        half8_t a0[NT], a1[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) a0[nt] = *reinterpret_cast<const half8_t *>(arow[nt] + k);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) a1[nt] = *reinterpret_cast<const half8_t *>(arow[nt] + k + kStride);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x0, a0[nt], acc[nt], 0, 0, 0);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x1, a1[nt], acc[nt], 0, 0, 0);
    }
    if (k < k_end) {
        half8_t x0 = *reinterpret_cast<const half8_t *>(xp + k);
        half8_t a0[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) a0[nt] = *reinterpret_cast<const half8_t *>(arow[nt] + k);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(x0, a0[nt], acc[nt], 0, 0, 0);
    }
    // D: column (of t) = lane & 15, row = 4 (lane >> 4) + i
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int i = 0; i < 4; ++i) red[(4 * (lane >> 4) + i) * (NT * 16) + nt * 16 + (lane & 15)] = acc[nt][i];
}

__global__ __launch_bounds__(64 * kLoraWaves) void lora_shrink_kernel(const LoraApplyArgs a) {
    __shared__ float red[kLoraWaves][kLoraTileRows * kLoraMaxRankTotal];
    const int ti = blockIdx.x, ks = blockIdx.y;
    int rank;
    float scale;
    const half_t *A, *B;
    if (lora_tile(a, ti, &rank, &scale, &A, &B) < 0) return;
    const int R = a.blocks * rank, NT = (R + 15) / 16;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int first = a.tile_rows[static_cast<size_t>(ti) * kLoraTileRows];
    if (first < 0 || first >= a.rows) return;   // (the whole workgroup: a tile in use has a first row)
    int m = a.tile_rows[static_cast<size_t>(ti) * kLoraTileRows + (lane & 15)];
    if (m < 0 || m >= a.rows) m = first;        // padding: any row of the tile, the result is not used
    const half_t *xrow = a.x + static_cast<size_t>(m) * a.K;
    const int k_lo = ks * a.slice_steps * 32, k_hi = min(k_lo + a.slice_steps * 32, a.K);
    const int k_begin = k_lo + wave * 32;
    float *my = red[wave];
    int ntc;   // the instantiation's tile count, >= NT
    if (NT <= 1) ntc = 1, lora_shrink_wave<1>(xrow, A, a.K, R, lane, k_begin, k_hi, my);
    else if (NT <= 2) ntc = 2, lora_shrink_wave<2>(xrow, A, a.K, R, lane, k_begin, k_hi, my);
    else if (NT <= 4) ntc = 4, lora_shrink_wave<4>(xrow, A, a.K, R, lane, k_begin, k_hi, my);
    else if (NT <= 8) ntc = 8, lora_shrink_wave<8>(xrow, A, a.K, R, lane, k_begin, k_hi, my);
    else ntc = 12, lora_shrink_wave<12>(xrow, A, a.K, R, lane, k_begin, k_hi, my);
    __syncthreads();
    float *out = a.partial + (static_cast<size_t>(ks) * a.tiles + ti) * kLoraTileRows * a.rt_max;
    const int stride = ntc * 16;
    for (int e = threadIdx.x; e < kLoraTileRows * R; e += 64 * kLoraWaves) {
        const int row = e / R, col = e - row * R;
        const int src = row * stride + col;
        out[row * R + col] = ((red[0][src] + red[1][src]) + red[2][src]) + red[3][src];
    }
}

__global__ __launch_bounds__(64 * kLoraWaves) void lora_expand_kernel(const LoraApplyArgs a) {
    const int ti = blockIdx.x;
    int rank;
    float scale;
    const half_t *A, *B;
    if (lora_tile(a, ti, &rank, &scale, &A, &B) < 0) return;
    const int R = a.blocks * rank;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4;
    const int m = a.tile_rows[static_cast<size_t>(ti) * kLoraTileRows + (lane & 15)];
    const bool live = m >= 0 && m < a.rows;
    const float *part = a.partial + static_cast<size_t>(ti) * kLoraTileRows * a.rt_max + (lane & 15) * R;
    const size_t ks_stride = static_cast<size_t>(a.tiles) * kLoraTileRows * a.rt_max;
    half8_t t0 = half8_t{0, 0, 0, 0, 0, 0, 0, 0}, t1 = t0;   // t[m = lane & 15][r = 8 g .. + 7] and (rank 64) [32 + 8 g .. + 7] of the current column block, fp16
    int cur_j = -1;
#pragma unroll 1
    for (int q = 0; q < 4; ++q) {
        const int n0 = blockIdx.y * kLoraExpandCols + (wave * 4 + q) * 16;
        if (n0 >= a.N) break;
        const int j = n0 >= a.col2 ? 2 : (n0 >= a.col1 ? 1 : 0);
        if (j != cur_j) {
            cur_j = j;
#pragma unroll
            for (int hlf = 0; hlf < 2; ++hlf) {
                float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                const int r0 = 32 * hlf + 8 * g;
                if (r0 < rank) {
                    for (int ks = 0; ks < a.ksplit; ++ks) {
                        const float4_t *p = reinterpret_cast<const float4_t *>(part + ks * ks_stride + j * rank + r0);
                        const float4_t u = p[0], v = p[1];
                        s[0] += u.x, s[1] += u.y, s[2] += u.z, s[3] += u.w, s[4] += v.x, s[5] += v.y, s[6] += v.z, s[7] += v.w;
                    }
                }
                half8_t h;
#pragma unroll
                for (int i = 0; i < 8; ++i) h[i] = static_cast<half_t>(s[i]);
                if (hlf == 0) t0 = h;
                else t1 = h;
            }
        }
        // A operand: B rows n0 + (lane & 15), r = 8 g .. + 7 (zero behind the rank)
        const half_t *brow = B + static_cast<size_t>(n0 + (lane & 15)) * rank;
        half8_t b0 = half8_t{0, 0, 0, 0, 0, 0, 0, 0}, b1 = b0;
        if (8 * g < rank) b0 = *reinterpret_cast<const half8_t *>(brow + 8 * g);
        if (32 + 8 * g < rank) b1 = *reinterpret_cast<const half8_t *>(brow + 32 + 8 * g);
        floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(b0, t0, acc, 0, 0, 0);
        if (rank > 32) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(b1, t1, acc, 0, 0, 0);
        // D: row (output column) = n0 + 4 g + i, column (row of the tile) = lane & 15
        if (live) {
            half4_t *yp = reinterpret_cast<half4_t *>(a.y + static_cast<size_t>(m) * a.N + n0 + 4 * g);
            half4_t v = *yp;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = static_cast<half_t>(static_cast<float>(v[i]) + scale * acc[i]);
            *yp = v;
        }
    }
}

int lora_ws_check(const char *who, const void *workspace, size_t workspace_bytes, size_t need) {
    if (!workspace || workspace_bytes < need || reinterpret_cast<uintptr_t>(workspace) % 256) {
        set_error("%s: workspace missing, too small or not 256-byte aligned (%zu < %zu)", who, workspace ? workspace_bytes : size_t(0), need);
        return LLMIE_ERR_WORKSPACE;
    }
    return LLMIE_OK;
}

}  // namespace

static int lora_shape_check(const char *who, int K, int N, int blocks, const int *block_widths) {
    LLMIE_REQUIRE(K > 0 && N > 0, "%s: non-positive shape K=%d N=%d", who, K, N);
    LLMIE_REQUIRE(blocks >= 1 && blocks <= 3 && block_widths, "%s: %d column blocks outside [1, 3]", who, blocks);
    long long sum = 0;
    for (int j = 0; j < blocks; ++j) {
        LLMIE_REQUIRE(block_widths[j] > 0, "%s: column block %d has width %d", who, j, block_widths[j]);
        sum += block_widths[j];
    }
    LLMIE_REQUIRE(sum == N, "%s: the column blocks sum to %lld, not N=%d", who, sum, N);
    if (K % 32) LLMIE_UNSUPPORTED("%s: K=%d is not a multiple of 32", who, K);
    for (int j = 0; j < blocks; ++j)
        if (block_widths[j] % 16) LLMIE_UNSUPPORTED("%s: column block %d has width %d, not a multiple of 16", who, j, block_widths[j]);
    return LLMIE_OK;
}

}  // namespace llmie

using namespace llmie;

extern "C" size_t llmie_lora_table_bytes(int slots, int layers) {
    if (slots <= 0 || layers <= 0 || slots > LLMIE_LORA_MAX_SLOTS) return 0;
    return static_cast<size_t>(slots) * (sizeof(LoraSlotHdr) + 64 * static_cast<size_t>(layers));
}

extern "C" int llmie_lora_slot_load(void *table_dev, int slots, int layers, int slot, const llmie_lora_adapter *host_desc, llmie_stream stream) {
    LLMIE_REQUIRE(table_dev, "lora_slot_load: NULL pointer");
    LLMIE_REQUIRE(slots > 0 && layers > 0, "lora_slot_load: non-positive table shape slots=%d layers=%d", slots, layers);
    if (slots > LLMIE_LORA_MAX_SLOTS) LLMIE_UNSUPPORTED("lora_slot_load: %d slots above LLMIE_LORA_MAX_SLOTS (%d)", slots, LLMIE_LORA_MAX_SLOTS);
    LLMIE_REQUIRE(slot >= 0 && slot < slots, "lora_slot_load: slot %d outside [0, %d)", slot, slots);
    if (host_desc) {
        LLMIE_REQUIRE(lora_rank_ok(host_desc->rank), "lora_slot_load: rank %d outside {8, 16, 32, 64}", host_desc->rank);
        LLMIE_REQUIRE(host_desc->layers == layers && host_desc->layer, "lora_slot_load: the adapter describes %d layers, the table has %d",
                      host_desc->layer ? host_desc->layers : 0, layers);
        for (int l = 0; l < layers; ++l)
            for (int mo = 0; mo < 4; ++mo) {
                const void *A = host_desc->layer[l].a[mo], *B = host_desc->layer[l].b[mo];
                LLMIE_REQUIRE((A == nullptr) == (B == nullptr), "lora_slot_load: layer %d module %d has an A without its B (or the reverse)", l, mo);
                if (mis16(A) || mis16(B)) LLMIE_UNSUPPORTED("lora_slot_load: layer %d module %d: A / B not 16-byte aligned", l, mo);
            }
    }
    for (int l0 = 0; l0 < layers; l0 += 16) {
        LoraSlotStore s{};
        s.slot = slot, s.layers = layers, s.layer0 = l0, s.count = layers - l0 < 16 ? layers - l0 : 16, s.write_hdr = l0 == 0;
        // an emptied slot keeps rank 0 in front of null pointers; a loaded one gets its header with the first layers
        s.hdr = LoraSlotHdr{host_desc ? host_desc->rank : 0, host_desc ? host_desc->scale : 0.f, {0, 0}};
        for (int l = 0; l < s.count; ++l)
            for (int mo = 0; mo < 4; ++mo) {
                s.ptr[l][2 * mo] = host_desc ? host_desc->layer[l0 + l].a[mo] : nullptr;
                s.ptr[l][2 * mo + 1] = host_desc ? host_desc->layer[l0 + l].b[mo] : nullptr;
            }
        lora_slot_store_kernel<<<1, 128, 0, as_stream(stream)>>>(static_cast<unsigned char *>(table_dev), slots, s);
        if (int rc = launch_status("lora_slot_load")) return rc;
    }
    return LLMIE_OK;
}

extern "C" size_t llmie_lora_workspace_bytes(int max_rows, int slots, int max_rank_total) {
    if (max_rows <= 0 || slots <= 0 || slots > LLMIE_LORA_MAX_SLOTS || max_rank_total <= 0 || max_rank_total > kLoraMaxRankTotal) return 0;
    const LoraWs w = lora_ws(max_rows, slots);
    return w.fixed + lora_partial_bytes(w.tiles, max_rank_total);
}

extern "C" int llmie_lora_plan(const int32_t *slot_dev, const int32_t *lengths_dev, int batch, int rows, const void *table_dev, int slots,
                               void *workspace, size_t workspace_bytes, llmie_stream stream) {
    LLMIE_REQUIRE(slot_dev && table_dev, "lora_plan: NULL pointer");
    LLMIE_REQUIRE(rows > 0 && slots > 0 && (!lengths_dev || batch > 0), "lora_plan: non-positive size rows=%d slots=%d batch=%d", rows, slots, batch);
    if (slots > LLMIE_LORA_MAX_SLOTS) LLMIE_UNSUPPORTED("lora_plan: %d slots above LLMIE_LORA_MAX_SLOTS (%d)", slots, LLMIE_LORA_MAX_SLOTS);
    const LoraWs w = lora_ws(rows, slots);
    if (int rc = lora_ws_check("lora_plan", workspace, workspace_bytes, w.fixed)) return rc;
    char *base = static_cast<char *>(workspace);
    lora_plan_kernel<<<1, kLoraPlanThreads, 0, as_stream(stream)>>>(slot_dev, lengths_dev, batch, rows, static_cast<const unsigned char *>(table_dev), slots,
                                                                    reinterpret_cast<int32_t *>(base), reinterpret_cast<int32_t *>(base + w.row_slot),
                                                                    reinterpret_cast<int32_t *>(base + w.tile_slot),
                                                                    reinterpret_cast<int32_t *>(base + w.tile_rows), w.tiles);
    return launch_status("lora_plan");
}

extern "C" int llmie_lora_apply(const void *x, void *y, int rows, int K, int N, int blocks, const int *block_widths, const void *table_dev,
                                int slots, int layers, int layer, int module, void *workspace, size_t workspace_bytes, llmie_dtype dtype,
                                llmie_stream stream) {
    LLMIE_REQUIRE(x && y && table_dev, "lora_apply: NULL pointer");
    LLMIE_REQUIRE(rows > 0 && slots > 0 && layers > 0, "lora_apply: non-positive size rows=%d slots=%d layers=%d", rows, slots, layers);
    LLMIE_REQUIRE(layer >= 0 && layer < layers && module >= 0 && module < 4, "lora_apply: layer %d / module %d outside [0, %d) / [0, 4)", layer, module,
                  layers);
    if (int rc = lora_shape_check("lora_apply", K, N, blocks, block_widths)) return rc;
    if (dtype != LLMIE_F16) LLMIE_UNSUPPORTED("lora_apply: fp16 activations only");
    if (slots > LLMIE_LORA_MAX_SLOTS) LLMIE_UNSUPPORTED("lora_apply: %d slots above LLMIE_LORA_MAX_SLOTS (%d)", slots, LLMIE_LORA_MAX_SLOTS);
    if (mis16(x) || mis16(y)) LLMIE_UNSUPPORTED("lora_apply: x / y not 16-byte aligned");
    const LoraWs w = lora_ws(rows, slots);
    const int rt_max = blocks * 64;
    if (int rc = lora_ws_check("lora_apply", workspace, workspace_bytes, w.fixed + lora_partial_bytes(w.tiles, rt_max))) return rc;
    char *base = static_cast<char *>(workspace);
    LoraApplyArgs a{};
    a.x = static_cast<const half_t *>(x), a.y = static_cast<half_t *>(y);
    a.rows = rows, a.K = K, a.N = N, a.blocks = blocks;
    a.col1 = blocks > 1 ? block_widths[0] : N;
    a.col2 = blocks > 2 ? block_widths[0] + block_widths[1] : N;
    a.table = static_cast<const unsigned char *>(table_dev);
    a.slots = slots, a.layers = layers, a.layer = layer, a.module = module;
    a.hdr = reinterpret_cast<const int32_t *>(base);
    a.tile_slot = reinterpret_cast<const int32_t *>(base + w.tile_slot);
    a.tile_rows = reinterpret_cast<const int32_t *>(base + w.tile_rows);
    a.partial = reinterpret_cast<float *>(base + w.partial);
    a.tiles = w.tiles, a.rt_max = rt_max;
    a.ksplit = lora_ksplit(K);
    a.slice_steps = (K / 32 + a.ksplit - 1) / a.ksplit;
    hipStream_t st = as_stream(stream);
    lora_shrink_kernel<<<dim3(w.tiles, a.ksplit), 64 * kLoraWaves, 0, st>>>(a);
    if (int rc = launch_status("lora_apply(shrink)")) return rc;
    lora_expand_kernel<<<dim3(w.tiles, (N + kLoraExpandCols - 1) / kLoraExpandCols), 64 * kLoraWaves, 0, st>>>(a);
    return launch_status("lora_apply(expand)");
}
