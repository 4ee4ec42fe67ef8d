// Mixture-of-experts FFN (llmie_moe_*; include/llmie.h states the arithmetic).  No reference launcher.
//
// Kernels, gfx950:
//   route     one wave per row: the E router logits (16-byte loads of x and Wr, fp32 dot2 accumulation, DPP reduction), the k maxima
//             by (logit descending, expert id ascending) through wave maxima + ballots, the weights in fp32.
//   plan      one workgroup (the shape of lora_plan_kernel): pairs per expert, each expert's pairs in (row, rank) order cut into
//             tiles of <= 16 * RT, the tile list and the tile count.  The grids are sized to the host bound
//             pairs / (16 RT) + min(E, pairs); surplus workgroups exit on the device count.
//   GEMV      gate/up + SwiGLU: grid (blocks of 16 Ie columns, pair); the workgroup reads its pair's expert id and streams that
//             expert's gate and up rows in the manner of gemv_ksplit_kernel (activation row in registers, 16-byte non-temporal
//             loads, the next rows requested before the reduction, DPP + one LDS exchange).  down + combine: grid (blocks of 16 H
//             columns, row); the workgroup walks its row's k experts in rank order and sums w_j d_j in fp32 -- no partials.
//   grouped   v_mfma_f32_16x16x32_f16, expert rows as the A operand and the gathered rows of the tile's pairs as B, both fetched as
//             16-byte row-contiguous loads (no LDS), two k-steps per loop body.  Gate/up: a wave holds 16 gate columns and the
//             matching 16 up columns of RT row tiles: SwiGLU in registers, every weight fragment shared by the RT tiles.  Down: the
//             same arrangement, d[pair][H] in fp32 to the workspace; a combine launch applies the weights in rank order.
//   _ex       llmie_moe_ffn_ex / _route_ex: an expert descriptor with a router bias, gate/up and down biases and the clamped SwiGLU as
//             epilogues of the kernels above (a template flag on the fp16 expert kernels, uniform branches elsewhere), and MXFP4
//             experts on kernels of their own beside the fp16 ones: moe_mx4_gemv_* (waves own weight rows, a lane's 16-byte load is
//             one block of 32 codes) and moe_mx4_grouped_kernel (operands swapped: a lane owns one weight row and one scale).
//             llmie_moe_ffn is the _ex call of a descriptor with fp16 experts, no bias and the plain act; such a call (MoePlan::ex
//             false) launches the EX = false instantiations.
// Every output element is computed by one lane chain that depends on its row, the weights and the route only: no atomics, same bits
// wherever the row stands.
//
// Host side: a call is MoeCall + MoeOperands (llmie_internal.h).  plan_moe -- pure, the only producer of a MoePlan --
// decides the route, RT, the grids, the workspace carve and the kernel instantiations; the launcher (moe_launch), the plan text
// (llmie_moe_ffn_plan / _plan_ex) and the workspace rule read that plan.  moe_prepare makes every check of an entry in one fixed
// order, plans, carves and fills the kernel arguments once; moe_launch runs the stages asked for and does nothing else, each launch
// written once behind a dispatch helper that turns the plan's fields into template arguments.  llmie_moe_ffn / _ex are prepare +
// every stage; the engine plans once per forward / prefill call, prepares once per sparse layer and launches the three stages
// under its three op kinds.
#include "llmie_internal.h"

#include <cstring>
#include <new>
#include <type_traits>

namespace llmie {
namespace {

constexpr int kMoeMaxExperts = LLMIE_MOE_MAX_EXPERTS;
constexpr int kMoeMaxTopK = LLMIE_MOE_MAX_TOP_K;
constexpr int kMoeGemvRows = 4;         // plan_moe: the GEMV route up to this many rows (fp16 experts)
constexpr int kMoeGemvRowsMx4 = 16;     // MXFP4 experts: the GEMV route is ahead of the grouped one at 5, 8 and 16 rows
constexpr int kMoeGemvForceRows = 16;   // LLMIE_MOE_FORCE_GEMV up to this many rows
constexpr int kMoeRt4PairsPerExpert = 32;   // plan_moe: RT = 4 once pairs / E reaches this
constexpr int kMoeGemvCols = 16;        // output columns per GEMV workgroup
constexpr int kMoeGemvMaxK = 8 * 256 * 8;   // the GEMV kernels hold at most 8 chunks of the activation row per thread
constexpr int kMoeGroupCols = 64;       // output columns per grouped workgroup: 4 waves x 16
constexpr int kMoeCombineThreads = 256;
constexpr unsigned kMoeFlags = LLMIE_MOE_SOFTMAX_ALL | LLMIE_MOE_FORCE_GEMV | LLMIE_MOE_FORCE_GROUPED | LLMIE_MOE_FORCE_RT1 | LLMIE_MOE_FORCE_RT4;

__host__ __device__ inline size_t moe_align(size_t v) { return (v + 255) & ~static_cast<size_t>(255); }

// ---- plan_moe: a pure host function of a MoeCall (llmie_internal.h), and the only producer of a MoePlan ----
int moe_shape_check(const char *who, const MoeCall &c) {
    const int rows = c.rows, H = c.H, Ie = c.Ie, E = c.E, k = c.k;
    LLMIE_REQUIRE(rows > 0 && H > 0 && Ie > 0 && E > 0 && k > 0, "%s: non-positive size rows=%d hidden=%d inter=%d experts=%d top_k=%d", who, rows, H,
                  Ie, E, k);
    if (E > kMoeMaxExperts) LLMIE_UNSUPPORTED("%s: %d experts above LLMIE_MOE_MAX_EXPERTS (%d)", who, E, kMoeMaxExperts);
    if (k > E) LLMIE_UNSUPPORTED("%s: top_k=%d above the %d experts", who, k, E);
    if (k > kMoeMaxTopK) LLMIE_UNSUPPORTED("%s: top_k=%d above LLMIE_MOE_MAX_TOP_K (%d)", who, k, kMoeMaxTopK);
    if (H % 64) LLMIE_UNSUPPORTED("%s: hidden=%d is not a multiple of 64", who, H);
    if (Ie % 64) LLMIE_UNSUPPORTED("%s: inter=%d is not a multiple of 64", who, Ie);
    if (static_cast<long long>(rows) * k > (1ll << 24)) LLMIE_UNSUPPORTED("%s: rows * top_k = %lld above 2^24", who, static_cast<long long>(rows) * k);
    return LLMIE_OK;
}

inline int moe_tiles(int pairs, int E, int rt) { return pairs / (16 * rt) + (E < pairs ? E : pairs); }

MoeCarve moe_carve(const MoeCall &c, bool grouped, int tiles_max, size_t tile_pair_slots) {
    const size_t pairs = static_cast<size_t>(c.rows) * c.k;
    MoeCarve w{};
    size_t off = 256;   // the plan's header: {tiles in use}
    w.expert = off, off += moe_align(4 * pairs);
    w.weight = off, off += moe_align(4 * pairs);
    w.act = off, off += moe_align(2 * pairs * c.Ie);
    w.tile_expert = off, off += moe_align(4 * static_cast<size_t>(tiles_max));
    w.tile_pairs = off, off += moe_align(4 * tile_pair_slots);
    w.d = off, off += grouped ? moe_align(4 * pairs * c.H) : 0;
    w.bytes = off;
    return w;
}
// every section at the larger of its sizes over the routes and RT: covers the plan of every row count up to c.rows
MoeCarve moe_cover_carve(const MoeCall &c) {
    const int pairs = c.rows * c.k, t1 = moe_tiles(pairs, c.E, 1), t4 = moe_tiles(pairs, c.E, 4);
    const size_t s1 = static_cast<size_t>(t1) * 16, s4 = static_cast<size_t>(t4) * 64;
    return moe_carve(c, true, t1 > t4 ? t1 : t4, s1 > s4 ? s1 : s4);
}

// XC of the fp16 GEMV kernels: 16-byte chunks of a K-long row per thread
int moe_xc(int K) {
    const int need = (K / 8 + 255) / 256;
    return need <= 1 ? 1 : (need <= 2 ? 2 : (need <= 4 ? 4 : 8));
}
// the (XB, KW) of the MXFP4 GEMV kernels: 0 .. 3 = (1, 1), (2, 1), (2, 2), (2, 4)
int moe_mx4_cfg(int K) {
    const int nb = K / 32;
    return nb <= 64 ? 0 : (nb <= 128 ? 1 : (nb <= 256 ? 2 : 3));
}

// the shape has been checked (moe_shape_check)
// format: LLMIE_W_F16 or LLMIE_W_MXFP4 experts.  The GEMV row threshold is a per-format constant (tools/moebench.py --mxfp4 shows the
// MXFP4 crossover at the 16 rows the GEMV kernels stop at); RT = 4 from 32 pairs per expert in both (rt4 is ahead from 128 tokens in both)
int plan_moe(const char *who, const MoeCall &c, MoePlan *p) {
    const int rows = c.rows, H = c.H, Ie = c.Ie, E = c.E;
    const unsigned flags = c.flags;
    const bool mx4 = c.format == LLMIE_W_MXFP4;
    const int gemv_rows = mx4 ? kMoeGemvRowsMx4 : kMoeGemvRows;
    const bool fg = flags & LLMIE_MOE_FORCE_GEMV, fm = flags & LLMIE_MOE_FORCE_GROUPED;
    LLMIE_REQUIRE(!(fg && fm), "%s: LLMIE_MOE_FORCE_GEMV and LLMIE_MOE_FORCE_GROUPED together", who);
    LLMIE_REQUIRE(!(flags & ~kMoeFlags), "%s: unknown flags 0x%x", who, flags);
    LLMIE_REQUIRE(!((flags & LLMIE_MOE_FORCE_RT1) && (flags & LLMIE_MOE_FORCE_RT4)), "%s: LLMIE_MOE_FORCE_RT1 and LLMIE_MOE_FORCE_RT4 together", who);
    const bool gemv_fits = H <= kMoeGemvMaxK && Ie <= kMoeGemvMaxK;
    if (fg && rows > kMoeGemvForceRows) LLMIE_UNSUPPORTED("%s: LLMIE_MOE_FORCE_GEMV with %d rows, above %d", who, rows, kMoeGemvForceRows);
    if (fg && !gemv_fits) LLMIE_UNSUPPORTED("%s: LLMIE_MOE_FORCE_GEMV with hidden=%d / inter=%d above %d", who, H, Ie, kMoeGemvMaxK);
    *p = MoePlan{};
    p->call = c, p->ex = c.ex;
    p->pairs = rows * c.k;
    p->route = fg ? MOE_GEMV : (fm ? MOE_GROUPED : (rows <= gemv_rows && gemv_fits ? MOE_GEMV : MOE_GROUPED));
    p->route_grid = (rows + 3) / 4;
    if (p->route == MOE_GEMV) {
        const auto cfg = [&](int K) { return mx4 ? moe_mx4_cfg(K) : moe_xc(K); };
        p->gate_up_cfg = cfg(H), p->down_cfg = cfg(Ie);
        p->gate_up_grid[0] = Ie / kMoeGemvCols, p->gate_up_grid[1] = p->pairs;
        p->down_grid[0] = H / kMoeGemvCols, p->down_grid[1] = rows;
        p->ws = moe_carve(c, false, 0, 0);
    } else {
        p->rt = (flags & LLMIE_MOE_FORCE_RT1) ? 1 : ((flags & LLMIE_MOE_FORCE_RT4) || p->pairs / E >= kMoeRt4PairsPerExpert ? 4 : 1);
        p->tiles = moe_tiles(p->pairs, E, p->rt);
        p->gate_up_grid[0] = p->tiles, p->gate_up_grid[1] = Ie / kMoeGroupCols;
        p->down_grid[0] = p->tiles, p->down_grid[1] = H / kMoeGroupCols;
        p->combine_grid[0] = rows, p->combine_grid[1] = (H / 4 + kMoeCombineThreads - 1) / kMoeCombineThreads;   // rows on x: no 65535 limit
        p->ws = moe_carve(c, true, p->tiles, static_cast<size_t>(p->tiles) * 16 * p->rt);
    }
    return LLMIE_OK;
}

// ---- route ----
struct MoeRouteArgs {
    const half_t *x, *router;
    int rows, H, E, k, softmax_all;
    int32_t *expert;
    float *weight;
    const half_t *bias;   // [E] or null (llmie_moe_route_ex): one fp32 add to the summed logit
};

__global__ __launch_bounds__(256) void moe_route_kernel(const MoeRouteArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + wave;
    if (row >= a.rows) return;   // the whole wave
    const int nch = a.H >> 3;
    const half8_t *xr = reinterpret_cast<const half8_t *>(a.x + static_cast<size_t>(row) * a.H);
    const half8_t *wr = reinterpret_cast<const half8_t *>(a.router);
    // lane l keeps the logits of experts l and 64 + l; -inf behind E and for a NaN
    float v0 = -INFINITY, v1 = -INFINITY;
    for (int e0 = 0; e0 < a.E; e0 += 4) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = lane; c < nch; c += 64) {
            const half8_t xv = xr[c];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = min(e0 + i, a.E - 1);   // (a clamped expert's logit is not kept)
                acc[i] = dot8(xv, wr[static_cast<size_t>(e) * nch + c], acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float r = wave_sum(acc[i]);
            if (a.bias) r += to_f32(a.bias[min(e0 + i, a.E - 1)]);
            if (r != r) r = -INFINITY;
            const int e = e0 + i;
            if (e < a.E && (e & 63) == lane) {
                if (e < 64) v0 = r;
                else v1 = r;
            }
        }
    }
    // the k maxima: (logit descending, expert id ascending); an entry leaves the contest once taken
    bool open0 = lane < a.E, open1 = lane + 64 < a.E;
    float sel[kMoeMaxTopK];
    int sel_id[kMoeMaxTopK];
#pragma unroll
    for (int j = 0; j < kMoeMaxTopK; ++j) {
        sel[j] = -INFINITY, sel_id[j] = 0;
        if (j < a.k) {
            const float mine = fmaxf(open0 ? v0 : -INFINITY, open1 ? v1 : -INFINITY);
            const float m = wave_max(mine);
            const unsigned long long b0 = __ballot(open0 && v0 == m), b1 = __ballot(open1 && v1 == m);
            // k <= E: an open entry exists, and -inf == -inf finds it when nothing finite is left
            int id = b0 ? __builtin_ctzll(b0) : (b1 ? 64 + __builtin_ctzll(b1) : 0);
            id = min(id, a.E - 1);
            if (id == lane) open0 = false;
            if (id == lane + 64) open1 = false;
            sel[j] = m, sel_id[j] = id;
        }
    }
    float den = 0.f;
    if (a.softmax_all) {
        float t = (lane < a.E ? expf(v0 - sel[0]) : 0.f) + (lane + 64 < a.E ? expf(v1 - sel[0]) : 0.f);
        den = wave_sum(t);
    } else {
#pragma unroll
        for (int j = 0; j < kMoeMaxTopK; ++j)
            if (j < a.k) den += expf(sel[j] - sel[0]);
    }
#pragma unroll
    for (int j = 0; j < kMoeMaxTopK; ++j)
        if (j < a.k && lane == j) {
            a.expert[static_cast<size_t>(row) * a.k + j] = sel_id[j];
            a.weight[static_cast<size_t>(row) * a.k + j] = expf(sel[j] - sel[0]) / den;
        }
}

// ---- plan: hdr[0] = tiles in use; tile_expert[tiles]; tile_pairs[tiles][16 * RT] (-1 = padding) ----
__global__ __launch_bounds__(256) void moe_plan_kernel(const int32_t *__restrict__ expert, int pairs, int E, int rt, int32_t *hdr,
                                                       int32_t *tile_expert, int32_t *tile_pairs, int tiles) {
    __shared__ int32_t s_base[kMoeMaxExperts + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int slots = 16 * rt;
    // wave w owns the experts w, w + 4, ...: lane i counts expert w + 4 i (E <= 128: i < 32)
    const int mine = wave + 4 * lane;
    const int owned = wave < E ? (E - wave + 3) / 4 : 0;
    int n = 0;
    for (int p0 = 0; p0 < pairs; p0 += 64) {
        const int p = p0 + lane;
        const int e = p < pairs ? expert[p] : -1;
        for (int i = 0; i < owned; ++i) {
            const int c = __popcll(__ballot(e == wave + 4 * i));
            if (lane == i) n += c;
        }
    }
    if (lane < owned) s_base[mine + 1] = (n + slots - 1) / slots;
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        s_base[0] = 0;
        for (int e = 0; e < E; ++e) acc += s_base[e + 1], s_base[e + 1] = acc;
    }
    __syncthreads();
    const int used = min(s_base[E], tiles);
    // the pairs of an expert in pair order: a pair's place is the matches in front of it (earlier chunks, lower lanes of its own)
    int run = 0;   // lane i: pairs of expert wave + 4 i placed so far
    for (int p0 = 0; p0 < pairs; p0 += 64) {
        const int p = p0 + lane;
        const int e = p < pairs ? expert[p] : -1;
        for (int i = 0; i < owned; ++i) {
            const int ex = wave + 4 * i;
            const bool hit = e == ex;
            const unsigned long long m = __ballot(hit);
            if (!m) continue;
            const int before = __builtin_amdgcn_readlane(run, i);
            const int base = s_base[ex], end = s_base[ex + 1];
            const int at = before + __popcll(m & ((1ull << lane) - 1));
            if (hit && end <= tiles && at < (end - base) * slots) tile_pairs[static_cast<size_t>(base) * slots + at] = p;
            if (lane == i) run += __popcll(m);
        }
    }
    for (int i = 0; i < owned; ++i) {
        const int ex = wave + 4 * i;
        const int base = s_base[ex], end = s_base[ex + 1];
        if (base == end || end > tiles) continue;
        const int placed = __builtin_amdgcn_readlane(run, i);
        for (int q = placed + lane; q < (end - base) * slots; q += 64) tile_pairs[static_cast<size_t>(base) * slots + q] = -1;
        for (int ti = base + lane; ti < end; ti += 64) tile_expert[ti] = ex;
    }
    for (int ti = used + threadIdx.x; ti < tiles; ti += 256) tile_expert[ti] = -1;
    if (threadIdx.x == 0) hdr[0] = used;
}

// ---- GEMV route ----
struct MoeFfnArgs {
    const half_t *x, *gate_up, *down, *resid;
    half_t *y, *act;
    const int32_t *expert;
    const float *weight;
    int rows, H, Ie, E, k, pairs;
    // grouped
    const int32_t *hdr, *tile_expert, *tile_pairs;
    float *d;
    // llmie_moe_ffn_ex.  MXFP4 experts: gate_up / down point at the codes, these at the e8m0 bytes.  Biases: null = none.  act_kind: llmie_moe_act
    const uint8_t *gate_up_scale, *down_scale;
    const half_t *gate_up_bias, *down_bias;
    int act_kind;
    float alpha, limit;
};

__device__ __forceinline__ int moe_expert_of(const MoeFfnArgs &a, int pair) { return min(max(a.expert[pair], 0), a.E - 1); }
__device__ __forceinline__ float moe_silu_mul(float g, float u) { return (g / (1.0f + expf(-g))) * u; }
// the _ex epilogue of a (gate, up) pair of expert e at inter column n: the biases (a uniform branch), then the act
__device__ __forceinline__ float moe_act_ex(const MoeFfnArgs &a, int e, int n, float g, float u) {
    if (a.gate_up_bias) {
        const half_t *b = a.gate_up_bias + static_cast<size_t>(e) * 2 * a.Ie;
        g += to_f32(b[n]), u += to_f32(b[a.Ie + n]);
    }
    if (a.act_kind == LLMIE_MOE_ACT_SWIGLU_CLAMPED) {
        g = fminf(g, a.limit), u = fminf(fmaxf(u, -a.limit), a.limit);
        return (u + 1.0f) * g / (1.0f + expf(-a.alpha * g));
    }
    return moe_silu_mul(g, u);
}

// XC: 16-byte chunks of the activation row per thread (H <= XC * 2048).  EX: with the _ex epilogue (biases, act); false = llmie_moe_ffn
template <int XC, bool EX>
__global__ __launch_bounds__(256) void moe_gemv_gate_up_kernel(const MoeFfnArgs a) {
    constexpr int RP = 2;                      // (gate, up) row pairs per iteration: 4 rows x XC loads in flight per lane
    constexpr int ITERS = kMoeGemvCols / RP;
    __shared__ float red[2][4][2 * RP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = blockIdx.y, row = pair / a.k;
    const int H = a.H, Ie = a.Ie, nch = H >> 3;
    const int e = moe_expert_of(a, pair);
    const half_t *W = a.gate_up + static_cast<size_t>(e) * 2 * Ie * H;
    const int n_base = blockIdx.x * kMoeGemvCols;
    uint4_t wb[2 * RP][XC];
    auto load_rows = [&](int it) {
#pragma unroll
        for (int r = 0; r < 2 * RP; ++r) {
            const int n = n_base + it * RP + (r >> 1) + (r & 1) * Ie;
            const uint4_t *w = reinterpret_cast<const uint4_t *>(W + static_cast<size_t>(n) * H);
#pragma unroll
            for (int j = 0; j < XC; ++j) wb[r][j] = load_nt(w + min(j * 256 + tid, nch - 1));   // past the row end: meets a zero activation chunk
        }
    };
    half8_t xr[XC];
    const half8_t *xg = reinterpret_cast<const half8_t *>(a.x + static_cast<size_t>(row) * H);
#pragma unroll
    for (int j = 0; j < XC; ++j) xr[j] = j * 256 + tid < nch ? xg[j * 256 + tid] : half8_t{0, 0, 0, 0, 0, 0, 0, 0};
    load_rows(0);
#pragma unroll 1
    for (int it = 0; it < ITERS; ++it) {
        float acc[2 * RP];
#pragma unroll
        for (int r = 0; r < 2 * RP; ++r) {
            acc[r] = 0.f;
#pragma unroll
            for (int j = 0; j < XC; ++j) acc[r] = dot8(__builtin_bit_cast(half8_t, wb[r][j]), xr[j], acc[r]);
        }
        if (it + 1 < ITERS) load_rows(it + 1);   // in flight across the reduction
        float (*slot)[2 * RP] = red[it & 1];
#pragma unroll
        for (int r = 0; r < 2 * RP; ++r) {
            const float s = wave_sum(acc[r]);
            if (lane == 0) slot[wave][r] = s;
        }
        __syncthreads();
        if (tid < RP) {
            const float g = ((slot[0][2 * tid] + slot[1][2 * tid]) + slot[2][2 * tid]) + slot[3][2 * tid];
            const float u = ((slot[0][2 * tid + 1] + slot[1][2 * tid + 1]) + slot[2][2 * tid + 1]) + slot[3][2 * tid + 1];
            const int n = n_base + it * RP + tid;
            if constexpr (EX) a.act[static_cast<size_t>(pair) * Ie + n] = from_f32<half_t>(moe_act_ex(a, e, n, g, u));
            else a.act[static_cast<size_t>(pair) * Ie + n] = from_f32<half_t>(moe_silu_mul(g, u));
        }
    }
}

// XC: 16-byte chunks of the SwiGLU row per thread (Ie <= XC * 2048).  EX: with the down bias
template <int XC, bool EX>
__global__ __launch_bounds__(256) void moe_gemv_down_kernel(const MoeFfnArgs a) {
    constexpr int RPW = 4;
    constexpr int ITERS = kMoeGemvCols / RPW;
    __shared__ float red[2][4][RPW];
    __shared__ float ysum[kMoeGemvCols];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.y;
    const int H = a.H, Ie = a.Ie, nch = Ie >> 3;
    const int n_base = blockIdx.x * kMoeGemvCols;
    const int steps = a.k * ITERS;   // step s: expert rank s / ITERS, columns n_base + (s % ITERS) * RPW ..
    uint4_t wb[RPW][XC];
    half8_t ar[XC], ar_next[XC];
    auto load_rows = [&](int s) {
        const int pair = row * a.k + s / ITERS, it = s % ITERS;
        const half_t *W = a.down + static_cast<size_t>(moe_expert_of(a, pair)) * H * Ie;
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const uint4_t *w = reinterpret_cast<const uint4_t *>(W + static_cast<size_t>(n_base + it * RPW + r) * Ie);
#pragma unroll
            for (int j = 0; j < XC; ++j) wb[r][j] = load_nt(w + min(j * 256 + tid, nch - 1));
        }
        if (it == 0) {
            const half8_t *ag = reinterpret_cast<const half8_t *>(a.act + static_cast<size_t>(pair) * Ie);
#pragma unroll
            for (int j = 0; j < XC; ++j) ar_next[j] = j * 256 + tid < nch ? ag[j * 256 + tid] : half8_t{0, 0, 0, 0, 0, 0, 0, 0};
        }
    };
    if (tid < kMoeGemvCols) ysum[tid] = 0.f;
    load_rows(0);
#pragma unroll 1
    for (int s = 0; s < steps; ++s) {
        const int it = s % ITERS;
        if (it == 0) {
#pragma unroll
            for (int j = 0; j < XC; ++j) ar[j] = ar_next[j];
        }
        float acc[RPW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            acc[r] = 0.f;
#pragma unroll
            for (int j = 0; j < XC; ++j) acc[r] = dot8(__builtin_bit_cast(half8_t, wb[r][j]), ar[j], acc[r]);
        }
        if (s + 1 < steps) load_rows(s + 1);
        float (*slot)[RPW] = red[s & 1];
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            const float v = wave_sum(acc[r]);
            if (lane == 0) slot[wave][r] = v;
        }
        __syncthreads();
        if (tid < RPW) {   // thread t owns ysum[it * RPW + t] through the whole walk: rank order, no race
            float dj = ((slot[0][tid] + slot[1][tid]) + slot[2][tid]) + slot[3][tid];
            if constexpr (EX) {
                if (a.down_bias) dj += to_f32(a.down_bias[static_cast<size_t>(moe_expert_of(a, row * a.k + s / ITERS)) * H + n_base + it * RPW + tid]);
            }
            const float wj = a.weight[row * a.k + s / ITERS];
            ysum[it * RPW + tid] = ysum[it * RPW + tid] + wj * dj;
        }
    }
    __syncthreads();
    if (tid < kMoeGemvCols) {
        const size_t at = static_cast<size_t>(row) * H + n_base + tid;
        const float r = a.resid ? to_f32(a.resid[at]) : 0.f;
        a.y[at] = from_f32<half_t>(ysum[tid] + r);
    }
}

// ---- grouped MFMA route ----
// SWIGLU: A = the expert's gate rows n and up rows Ie + n (K = H), B = x rows of the tile's pairs; writes act[pair][Ie] fp16.
// else:   A = the expert's down rows n (K = Ie), B = act rows of the tile's pairs; writes d[pair][H] fp32.
// EX (SWIGLU only): with the _ex epilogue; the down bias of the grouped route is added by the combine launch
template <int RT, bool SWIGLU, bool EX>
__global__ __launch_bounds__(256) void moe_grouped_kernel(const MoeFfnArgs a) {
    constexpr int NA = SWIGLU ? 2 : 1;
    const int ti = blockIdx.x;
    if (ti >= a.hdr[0]) return;   // surplus tile (the whole workgroup)
    const int e = a.tile_expert[ti];
    if (e < 0 || e >= a.E) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    const int H = a.H, Ie = a.Ie;
    const int K = SWIGLU ? H : Ie;
    const int n0 = blockIdx.y * kMoeGroupCols + wave * 16;
    const half_t *W = SWIGLU ? a.gate_up + static_cast<size_t>(e) * 2 * Ie * H : a.down + static_cast<size_t>(e) * H * Ie;
    const half_t *wrow[NA];
    wrow[0] = W + static_cast<size_t>(n0 + c) * K + 8 * g;
    if constexpr (SWIGLU) wrow[1] = W + static_cast<size_t>(Ie + n0 + c) * K + 8 * g;
    const int32_t *tp = a.tile_pairs + static_cast<size_t>(ti) * 16 * RT;
    const int first = tp[0];
    if (first < 0 || first >= a.pairs) return;   // (a tile in use has a first pair)
    int pr[RT];
    bool live[RT];
    const half_t *brow[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        pr[t] = tp[t * 16 + c];
        live[t] = pr[t] >= 0 && pr[t] < a.pairs;
        if (!live[t]) pr[t] = first;   // padding: any pair of the tile, the result is not stored
        brow[t] = (SWIGLU ? a.x + static_cast<size_t>(pr[t] / a.k) * H : a.act + static_cast<size_t>(pr[t]) * Ie) + 8 * g;
    }
    floatx4 acc[RT][NA];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int i = 0; i < NA; ++i) acc[t][i] = floatx4{0.f, 0.f, 0.f, 0.f};
    // K % 64 == 0: two k-steps of loads per body, all requested before the first MFMA; the compiler's unroll puts four in flight
#pragma unroll 2
    for (int k = 0; k < K; k += 64) {
        half8_t w0[NA], w1[NA], b0[RT], b1[RT];
#pragma unroll
        for (int i = 0; i < NA; ++i) w0[i] = *reinterpret_cast<const half8_t *>(wrow[i] + k), w1[i] = *reinterpret_cast<const half8_t *>(wrow[i] + k + 32);
#pragma unroll
        for (int t = 0; t < RT; ++t) b0[t] = *reinterpret_cast<const half8_t *>(brow[t] + k), b1[t] = *reinterpret_cast<const half8_t *>(brow[t] + k + 32);
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int i = 0; i < NA; ++i) acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0[i], b0[t], acc[t][i], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int i = 0; i < NA; ++i) acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w1[i], b1[t], acc[t][i], 0, 0, 0);
    }
    // D: row (output column) = n0 + 4 g + i, column (pair of the tile) = lane & 15
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        if (!live[t]) continue;
        if constexpr (SWIGLU) {
            half4_t v;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (EX) v[i] = from_f32<half_t>(moe_act_ex(a, e, n0 + 4 * g + i, acc[t][0][i], acc[t][1][i]));
                else v[i] = from_f32<half_t>(moe_silu_mul(acc[t][0][i], acc[t][1][i]));
            }
            *reinterpret_cast<half4_t *>(a.act + static_cast<size_t>(pr[t]) * Ie + n0 + 4 * g) = v;
        } else {
            *reinterpret_cast<float4_t *>(a.d + static_cast<size_t>(pr[t]) * H + n0 + 4 * g) =
                float4_t{acc[t][0][0], acc[t][0][1], acc[t][0][2], acc[t][0][3]};
        }
    }
}

// y[row] = fp16(sum_j w_j d_j (rank order, fp32) + resid[row]); a thread owns 4 columns.  d_j gains the down bias of its expert here
// (a uniform branch; null: today's sum)
__global__ __launch_bounds__(kMoeCombineThreads) void moe_combine_kernel(const MoeFfnArgs a) {
    const int row = blockIdx.x, q = blockIdx.y * kMoeCombineThreads + threadIdx.x;
    if (4 * q >= a.H) return;
    float4_t s = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < a.k; ++j) {
        const size_t pair = static_cast<size_t>(row) * a.k + j;
        const float w = a.weight[pair];
        float4_t v = *reinterpret_cast<const float4_t *>(a.d + pair * a.H + 4 * q);
        if (a.down_bias) {
            const half_t *b = a.down_bias + static_cast<size_t>(moe_expert_of(a, static_cast<int>(pair))) * a.H + 4 * q;   // (2-byte aligned only)
            v.x += to_f32(b[0]), v.y += to_f32(b[1]), v.z += to_f32(b[2]), v.w += to_f32(b[3]);
        }
        s.x = s.x + w * v.x, s.y = s.y + w * v.y, s.z = s.z + w * v.z, s.w = s.w + w * v.w;
    }
    const size_t at = static_cast<size_t>(row) * a.H + 4 * q;
    if (a.resid) {
        const half4_t r = *reinterpret_cast<const half4_t *>(a.resid + at);
        s.x += to_f32(r[0]), s.y += to_f32(r[1]), s.z += to_f32(r[2]), s.w += to_f32(r[3]);
    }
    *reinterpret_cast<half4_t *>(a.y + at) = half4_t{from_f32<half_t>(s.x), from_f32<half_t>(s.y), from_f32<half_t>(s.z), from_f32<half_t>(s.w)};
}

// ---- MXFP4 experts (llmie_moe_ffn_ex, LLMIE_W_MXFP4): the layout of llmie_quantize_mxfp4 on the flattened [E * 2 Ie, H] / [E * H, Ie] ----
// GEMV route, the arrangement of mxfp4_gemv_kernel: a lane's 16-byte load is one block of 32 codes and KW waves share a weight row (lane
// l of part p takes blocks 64 p + l, 64 (p + KW) + l, ..: XB of them), so the 4 / KW wave groups of a workgroup walk their own
// columns of its 16.  The pair's activation blocks stay in registers; a block's 2^e scales the block's fp32 partial sum; the next
// rows are requested before the reduction.  K <= 64 KW XB blocks of 32: (XB, KW) = (1, 1), (2, 1), (2, 2), (2, 4) cover K <= 16384.
template <int XB, int KW>
__global__ __launch_bounds__(256) void moe_mx4_gemv_gate_up_kernel(const MoeFfnArgs a) {
    constexpr int GROUPS = 4 / KW, CPG = kMoeGemvCols / GROUPS;   // columns per wave group
    constexpr int RP = 4, ITERS = CPG / RP;                        // (gate, up) row pairs per iteration: 8 rows x XB loads in flight per lane
    __shared__ float red[2][4][2 * RP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, group = wave / KW, part = wave % KW;
    const int pair = blockIdx.y, row = pair / a.k;
    const int H = a.H, Ie = a.Ie, nb = H >> 5;
    const int e = moe_expert_of(a, pair);
    const uint8_t *W = reinterpret_cast<const uint8_t *>(a.gate_up) + static_cast<size_t>(e) * 2 * Ie * (H >> 1);
    const uint8_t *S = a.gate_up_scale + static_cast<size_t>(e) * 2 * Ie * nb;
    const int n_base = blockIdx.x * kMoeGemvCols + group * CPG;
    int blk[XB];
    half8_t xr[XB][4];
    const half_t *xg = a.x + static_cast<size_t>(row) * H;
#pragma unroll
    for (int j = 0; j < XB; ++j) {
        const int b = part * 64 + lane + 64 * KW * j;
        blk[j] = min(b, nb - 1);   // past the row end: a clamped load meets zero activations
#pragma unroll
        for (int i = 0; i < 4; ++i)
            xr[j][i] = b < nb ? *reinterpret_cast<const half8_t *>(xg + 32 * static_cast<size_t>(b) + 8 * i) : half8_t{0, 0, 0, 0, 0, 0, 0, 0};
    }
    uint4_t wb[2 * RP][XB];
    unsigned sb[2 * RP][XB];
    auto load_rows = [&](int it) {
#pragma unroll
        for (int r = 0; r < 2 * RP; ++r) {   // r = 2 c + {0: gate, 1: up} of column n_base + it * RP + c
            const size_t n = static_cast<size_t>(n_base + it * RP + (r >> 1) + (r & 1) * Ie);
#pragma unroll
            for (int j = 0; j < XB; ++j) {
                wb[r][j] = load_nt(reinterpret_cast<const uint4_t *>(W + n * (H >> 1) + 16 * static_cast<size_t>(blk[j])));
                sb[r][j] = S[n * nb + blk[j]];
            }
        }
    };
    load_rows(0);
#pragma unroll 1
    for (int it = 0; it < ITERS; ++it) {
        float acc[2 * RP];
#pragma unroll
        for (int r = 0; r < 2 * RP; ++r) {
            acc[r] = 0.f;
#pragma unroll
            for (int j = 0; j < XB; ++j) {
                float p = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) p = dot8(mx4_expand(wb[r][j][i]), xr[j][i], p);
                acc[r] += p * mx4_scale(sb[r][j]);
            }
        }
        if (it + 1 < ITERS) load_rows(it + 1);   // in flight across the reduction
        float v[2 * RP];
#pragma unroll
        for (int r = 0; r < 2 * RP; ++r) v[r] = wave_sum(acc[r]);
        if constexpr (KW > 1) {   // the parts' sums meet in LDS and are added in part order
            float (*slot)[2 * RP] = red[it & 1];
            if (lane == 0) {
#pragma unroll
                for (int r = 0; r < 2 * RP; ++r) slot[wave][r] = v[r];
            }
            __syncthreads();
            if (part == 0) {
#pragma unroll
                for (int r = 0; r < 2 * RP; ++r) {
                    v[r] = slot[wave][r];
#pragma unroll
                    for (int p = 1; p < KW; ++p) v[r] += slot[wave + p][r];
                }
            }
        }
        if (part == 0 && lane == 0) {
#pragma unroll
            for (int c = 0; c < RP; ++c) {
                const int n = n_base + it * RP + c;
                a.act[static_cast<size_t>(pair) * Ie + n] = from_f32<half_t>(moe_act_ex(a, e, n, v[2 * c], v[2 * c + 1]));
            }
        }
    }
}

// down + combine: grid (blocks of 16 H columns, row); a wave group walks the row's k experts in rank order over its own columns, four
// per step; the lane that reduces a column owns its sum through the whole walk (rank order, no race)
template <int XB, int KW>
__global__ __launch_bounds__(256) void moe_mx4_gemv_down_kernel(const MoeFfnArgs a) {
    constexpr int GROUPS = 4 / KW, CPG = kMoeGemvCols / GROUPS, RPW = 4, ITERS = CPG / RPW;
    __shared__ float red[2][4][RPW];
    __shared__ float ysum[kMoeGemvCols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, group = wave / KW, part = wave % KW;
    const int row = blockIdx.y;
    const int H = a.H, Ie = a.Ie, nb = Ie >> 5;
    const int n_base = blockIdx.x * kMoeGemvCols + group * CPG;
    const int steps = a.k * ITERS;   // step s: expert rank s / ITERS, columns n_base + (s % ITERS) * RPW ..
    const uint8_t *Wd = reinterpret_cast<const uint8_t *>(a.down);
    int blk[XB];
    bool live[XB];
#pragma unroll
    for (int j = 0; j < XB; ++j) {
        const int b = part * 64 + lane + 64 * KW * j;
        blk[j] = min(b, nb - 1), live[j] = b < nb;
    }
    uint4_t wb[RPW][XB];
    unsigned sb[RPW][XB];
    half8_t ar[XB][4], ar_next[XB][4];
    auto load_rows = [&](int s) {
        const int pair = row * a.k + s / ITERS, it = s % ITERS;
        const size_t wrow = static_cast<size_t>(moe_expert_of(a, pair)) * H + n_base + it * RPW;
#pragma unroll
        for (int r = 0; r < RPW; ++r)
#pragma unroll
            for (int j = 0; j < XB; ++j) {
                wb[r][j] = load_nt(reinterpret_cast<const uint4_t *>(Wd + (wrow + r) * (Ie >> 1) + 16 * static_cast<size_t>(blk[j])));
                sb[r][j] = a.down_scale[(wrow + r) * nb + blk[j]];
            }
        if (it == 0) {
            const half_t *ag = a.act + static_cast<size_t>(pair) * Ie;
#pragma unroll
            for (int j = 0; j < XB; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    ar_next[j][i] = live[j] ? *reinterpret_cast<const half8_t *>(ag + 32 * static_cast<size_t>(blk[j]) + 8 * i) : half8_t{0, 0, 0, 0, 0, 0, 0, 0};
        }
    };
    const bool owner = part == 0 && lane == 0;
    if (owner) {
#pragma unroll
        for (int c = 0; c < CPG; ++c) ysum[group * CPG + c] = 0.f;
    }
    load_rows(0);
#pragma unroll 1
    for (int s = 0; s < steps; ++s) {
        const int it = s % ITERS;
        if (it == 0) {
#pragma unroll
            for (int j = 0; j < XB; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) ar[j][i] = ar_next[j][i];
        }
        float acc[RPW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) {
            acc[r] = 0.f;
#pragma unroll
            for (int j = 0; j < XB; ++j) {
                float p = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) p = dot8(mx4_expand(wb[r][j][i]), ar[j][i], p);
                acc[r] += p * mx4_scale(sb[r][j]);
            }
        }
        if (s + 1 < steps) load_rows(s + 1);
        float v[RPW];
#pragma unroll
        for (int r = 0; r < RPW; ++r) v[r] = wave_sum(acc[r]);
        if constexpr (KW > 1) {
            float (*slot)[RPW] = red[s & 1];
            if (lane == 0) {
#pragma unroll
                for (int r = 0; r < RPW; ++r) slot[wave][r] = v[r];
            }
            __syncthreads();
            if (part == 0) {
#pragma unroll
                for (int r = 0; r < RPW; ++r) {
                    v[r] = slot[wave][r];
#pragma unroll
                    for (int p = 1; p < KW; ++p) v[r] += slot[wave + p][r];
                }
            }
        }
        if (owner) {
            const int pair = row * a.k + s / ITERS;
            const float wj = a.weight[pair];
#pragma unroll
            for (int r = 0; r < RPW; ++r) {
                const int c = group * CPG + it * RPW + r;
                float dj = v[r];
                if (a.down_bias) dj += to_f32(a.down_bias[static_cast<size_t>(moe_expert_of(a, pair)) * H + blockIdx.x * kMoeGemvCols + c]);
                ysum[c] = ysum[c] + wj * dj;
            }
        }
    }
    if (owner) {
#pragma unroll
        for (int c = 0; c < CPG; ++c) {
            const size_t at = static_cast<size_t>(row) * H + n_base + c;
            const float r = a.resid ? to_f32(a.resid[at]) : 0.f;
            a.y[at] = from_f32<half_t>(ysum[group * CPG + c] + r);
        }
    }
}

// grouped route, the operand order of mxfp4_mfma_kernel: A = the gathered rows of the tile's pairs (lane (c, g): pair slot c, k = 8 g ..
// 8 g + 7 of the block), B = the expanded codes (weight row n0 + c, the same k), so lane (c, g) of the C/D tile holds D[pair slot
// 4 g + j][column n0 + c]: one weight row and one scale per lane.  One MFMA per block of 32 into a zeroed tile; the tile times the
// block's 2^e (exact) is added to the accumulator.  No fp16 weight below the normal range reaches the MFMA.
template <int RT, bool SWIGLU>
__global__ __launch_bounds__(256) void moe_mx4_grouped_kernel(const MoeFfnArgs a) {
    constexpr int NA = SWIGLU ? 2 : 1;
    const int ti = blockIdx.x;
    if (ti >= a.hdr[0]) return;   // surplus tile (the whole workgroup)
    const int e = a.tile_expert[ti];
    if (e < 0 || e >= a.E) return;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    const int H = a.H, Ie = a.Ie;
    const int K = SWIGLU ? H : Ie, nb = K >> 5;
    const int n0 = blockIdx.y * kMoeGroupCols + wave * 16;
    const size_t row0 = SWIGLU ? static_cast<size_t>(e) * 2 * Ie : static_cast<size_t>(e) * H;   // the expert's first weight row
    const uint8_t *Wc = reinterpret_cast<const uint8_t *>(SWIGLU ? a.gate_up : a.down);
    const uint8_t *Sc = SWIGLU ? a.gate_up_scale : a.down_scale;
    const uint8_t *wp[NA], *sp[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const size_t n = row0 + static_cast<size_t>(i) * Ie + n0 + c;
        wp[i] = Wc + n * (K >> 1) + 4 * g, sp[i] = Sc + n * nb;
    }
    const int32_t *tp = a.tile_pairs + static_cast<size_t>(ti) * 16 * RT;
    const int first = tp[0];
    if (first < 0 || first >= a.pairs) return;   // (a tile in use has a first pair)
    const half_t *arow[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        int pa = tp[t * 16 + c];
        if (pa < 0 || pa >= a.pairs) pa = first;   // padding: any pair of the tile, the result is not stored
        arow[t] = (SWIGLU ? a.x + static_cast<size_t>(pa / a.k) * H : a.act + static_cast<size_t>(pa) * Ie) + 8 * g;
    }
    floatx4 acc[RT][NA];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int i = 0; i < NA; ++i) acc[t][i] = floatx4{0.f, 0.f, 0.f, 0.f};
    // K % 64 == 0: two blocks per body, all loads requested before the first MFMA
#pragma unroll 2
    for (int b = 0; b < nb; b += 2) {
        unsigned c0[NA], c1[NA], s0[NA], s1[NA];
        half8_t a0[RT], a1[RT];
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            c0[i] = load_nt(reinterpret_cast<const unsigned *>(wp[i] + 16 * static_cast<size_t>(b)));
            c1[i] = load_nt(reinterpret_cast<const unsigned *>(wp[i] + 16 * static_cast<size_t>(b + 1)));
            s0[i] = sp[i][b], s1[i] = sp[i][b + 1];
        }
#pragma unroll
        for (int t = 0; t < RT; ++t)
            a0[t] = *reinterpret_cast<const half8_t *>(arow[t] + 32 * static_cast<size_t>(b)), a1[t] = *reinterpret_cast<const half8_t *>(arow[t] + 32 * static_cast<size_t>(b + 1));
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const half8_t bw = mx4_expand(c0[i]);
            const float s = mx4_scale(s0[i]);
#pragma unroll
            for (int t = 0; t < RT; ++t) acc[t][i] += __builtin_amdgcn_mfma_f32_16x16x32_f16(a0[t], bw, floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0) * s;
        }
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const half8_t bw = mx4_expand(c1[i]);
            const float s = mx4_scale(s1[i]);
#pragma unroll
            for (int t = 0; t < RT; ++t) acc[t][i] += __builtin_amdgcn_mfma_f32_16x16x32_f16(a1[t], bw, floatx4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0) * s;
        }
    }
    // D: row (pair slot of the tile) = 4 g + j, column (output column) = n0 + c
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pq = tp[t * 16 + 4 * g + j];
            if (pq < 0 || pq >= a.pairs) continue;
            if constexpr (SWIGLU) a.act[static_cast<size_t>(pq) * Ie + n0 + c] = from_f32<half_t>(moe_act_ex(a, e, n0 + c, acc[t][0][j], acc[t][1][j]));
            else a.d[static_cast<size_t>(pq) * H + n0 + c] = acc[t][0][j];
        }
}

// what MoePrepared::args holds: the argument structs of the kernels above, filled once per call
struct MoeLaunchArgs {
    MoeRouteArgs r;
    MoeFfnArgs a;
};
static_assert(sizeof(MoeLaunchArgs) <= sizeof(MoePrepared::args) && alignof(MoeLaunchArgs) <= 16, "MoePrepared::args holds a MoeLaunchArgs");

void moe_route_launch(const MoeRouteArgs &r, hipStream_t st) { moe_route_kernel<<<(r.rows + 3) / 4, 256, 0, st>>>(r); }

// ---- a plan's fields -> the instantiation: f gets the template arguments as integral constants, so a launch is written once ----
template <int V> using MoeInt = std::integral_constant<int, V>;
// (the instantiations go into the code object in the order in which these alternatives and the launcher name them; both keep the order
// of the launch code they replaced, so the code object is that one's byte for byte -- where a kernel lies showed in the grouped
// route's time)
template <class F> void moe_ex_dispatch(bool ex, F f) { !ex ? f(std::false_type{}) : f(std::true_type{}); }   // (EX)
template <class F> void moe_rt_dispatch(int rt, F f) { rt == 4 ? f(MoeInt<4>{}) : f(MoeInt<1>{}); }           // (RT)
template <class F> void moe_gemv_dispatch(int xc, bool ex, F f) {   // fp16 GEMV pair: (XC, EX)
    const auto g = [&](auto x) { moe_ex_dispatch(ex, [&](auto e) { f(x, e); }); };
    xc == 1 ? g(MoeInt<1>{}) : (xc == 2 ? g(MoeInt<2>{}) : (xc == 4 ? g(MoeInt<4>{}) : g(MoeInt<8>{})));
}
template <class F> void moe_mx4_gemv_dispatch(int cfg, F f) {   // MXFP4 GEMV pair: (XB, KW) of moe_mx4_cfg's index
    using One = MoeInt<1>; using Two = MoeInt<2>;
    cfg == 0 ? f(One{}, One{}) : (cfg == 1 ? f(Two{}, One{}) : (cfg == 2 ? f(Two{}, Two{}) : f(Two{}, MoeInt<4>{})));
}

thread_local char g_moe_plan_text[256];

int moe_plan_line(const char *who, const MoeCall &c) {
    MoePlan p;
    if (int rc = moe_call_check(who, c, &p)) return rc;
    snprintf(g_moe_plan_text, sizeof(g_moe_plan_text), "route=%s rt=%d tiles=%d route_grid=%d plan_grid=%d gate_up_grid=%dx%d down_grid=%dx%d combine_grid=%dx%d ws=%zu",
             p.route == MOE_GEMV ? "gemv" : "grouped", p.rt, p.tiles, p.route_grid, p.route == MOE_GROUPED ? 1 : 0, p.gate_up_grid[0], p.gate_up_grid[1],
             p.down_grid[0], p.down_grid[1], p.combine_grid[0], p.combine_grid[1], p.ws.bytes);
    return LLMIE_OK;
}

// an expert descriptor on its own: format, the pointers every call needs, scales against the format, the act's constants
int moe_experts_check(const char *who, const llmie_moe_experts *ex) {
    LLMIE_REQUIRE(ex, "%s: NULL expert descriptor", who);
    if (ex->format != LLMIE_W_F16 && ex->format != LLMIE_W_MXFP4)
        LLMIE_UNSUPPORTED("%s: expert format %d is neither LLMIE_W_F16 nor LLMIE_W_MXFP4", who, static_cast<int>(ex->format));
    LLMIE_REQUIRE(ex->router && ex->gate_up && ex->down, "%s: NULL pointer", who);
    const bool mx = ex->format == LLMIE_W_MXFP4;
    LLMIE_REQUIRE(!mx || (ex->gate_up_scale && ex->down_scale), "%s: MXFP4 experts with a NULL scale", who);
    LLMIE_REQUIRE(mx || (!ex->gate_up_scale && !ex->down_scale), "%s: fp16 experts with a scale", who);
    LLMIE_REQUIRE(ex->act == LLMIE_MOE_ACT_SWIGLU || ex->act == LLMIE_MOE_ACT_SWIGLU_CLAMPED, "%s: unknown act %d", who, static_cast<int>(ex->act));
    if (ex->act == LLMIE_MOE_ACT_SWIGLU_CLAMPED)
        LLMIE_REQUIRE(ex->limit > 0.f && ex->limit <= 3.4028235e38f && ex->alpha >= -3.4028235e38f && ex->alpha <= 3.4028235e38f,
                      "%s: clamped SwiGLU needs a finite limit > 0 and a finite alpha (limit=%g alpha=%g)", who, ex->limit, ex->alpha);
    return LLMIE_OK;
}
int moe_experts_aligned(const char *who, const llmie_moe_experts *ex) {
    if (mis16(ex->router) || mis16(ex->gate_up) || mis16(ex->down)) LLMIE_UNSUPPORTED("%s: x / router / gate_up / down / resid / y not 16-byte aligned", who);
    if (reinterpret_cast<uintptr_t>(ex->router_bias) % 2 || reinterpret_cast<uintptr_t>(ex->gate_up_bias) % 2 || reinterpret_cast<uintptr_t>(ex->down_bias) % 2)
        LLMIE_UNSUPPORTED("%s: a bias is not 2-byte aligned", who);
    return LLMIE_OK;
}

// llmie_moe_route / _route_ex behind their NULL checks: the entry's name and the router bias (null: llmie_moe_route) are what they differ in
int moe_route_entry(const char *who, const MoeRouteArgs &r, unsigned flags, llmie_dtype dtype, llmie_stream stream) {
    if (int rc = moe_shape_check(who, MoeCall{r.rows, r.H, 64, r.E, r.k})) return rc;
    if (dtype != LLMIE_F16) LLMIE_UNSUPPORTED("%s: fp16 activations only", who);
    if (mis16(r.x) || mis16(r.router)) LLMIE_UNSUPPORTED("%s: x / router not 16-byte aligned", who);
    if (reinterpret_cast<uintptr_t>(r.bias) % 2) LLMIE_UNSUPPORTED("%s: router_bias not 2-byte aligned", who);
    LLMIE_REQUIRE(!(flags & ~kMoeFlags), "%s: unknown flags 0x%x", who, flags);
    moe_route_launch(r, as_stream(stream));
    return launch_status(who);
}

}  // namespace
}  // namespace llmie

using namespace llmie;

extern "C" size_t llmie_moe_workspace_bytes(int max_rows, int hidden, int inter, int experts, int top_k) {
    const MoeCall c{max_rows, hidden, inter, experts, top_k, 0, LLMIE_W_F16, false};
    return moe_shape_check("moe_workspace_bytes", c) ? 0 : moe_cover_carve(c).bytes;
}

extern "C" const char *llmie_moe_ffn_plan(int rows, int hidden, int inter, int experts, int top_k, unsigned flags) {
    return moe_plan_line("moe_ffn_plan", MoeCall{rows, hidden, inter, experts, top_k, flags, LLMIE_W_F16, false}) ? nullptr : g_moe_plan_text;
}

extern "C" const char *llmie_moe_ffn_plan_ex(int rows, int hidden, int inter, int experts, int top_k, unsigned flags, llmie_weight_format format,
                                             llmie_moe_act act) {
    if (format != LLMIE_W_F16 && format != LLMIE_W_MXFP4) {
        set_error("moe_ffn_plan_ex: expert format %d is neither LLMIE_W_F16 nor LLMIE_W_MXFP4", static_cast<int>(format));
        return nullptr;
    }
    if (act != LLMIE_MOE_ACT_SWIGLU && act != LLMIE_MOE_ACT_SWIGLU_CLAMPED) {
        set_error("moe_ffn_plan_ex: unknown act %d", static_cast<int>(act));
        return nullptr;
    }
    if (moe_plan_line("moe_ffn_plan_ex", MoeCall{rows, hidden, inter, experts, top_k, flags, format, act != LLMIE_MOE_ACT_SWIGLU})) return nullptr;
    const size_t n = strlen(g_moe_plan_text);
    snprintf(g_moe_plan_text + n, sizeof(g_moe_plan_text) - n, " format=%s act=%s", format == LLMIE_W_MXFP4 ? "mxfp4" : "f16",
             act == LLMIE_MOE_ACT_SWIGLU_CLAMPED ? "swiglu_clamped" : "swiglu");
    return g_moe_plan_text;
}

extern "C" int llmie_moe_route(const void *x, const void *router, int rows, int hidden, int experts, int top_k, unsigned flags, int32_t *expert_out,
                               float *weight_out, llmie_dtype dtype, llmie_stream stream) {
    LLMIE_REQUIRE(x && router && expert_out && weight_out, "moe_route: NULL pointer");
    return moe_route_entry("moe_route", MoeRouteArgs{static_cast<const half_t *>(x), static_cast<const half_t *>(router), rows, hidden, experts, top_k,
                                                     (flags & LLMIE_MOE_SOFTMAX_ALL) ? 1 : 0, expert_out, weight_out, nullptr}, flags, dtype, stream);
}

// llmie_moe_route with the descriptor's router and router bias; the expert matrices are not looked at
extern "C" int llmie_moe_route_ex(const void *x, const llmie_moe_experts *ex, int rows, int hidden, int experts, int top_k, unsigned flags,
                                  int32_t *expert_out, float *weight_out, llmie_dtype dtype, llmie_stream stream) {
    LLMIE_REQUIRE(x && ex && ex->router && expert_out && weight_out, "moe_route_ex: NULL pointer");
    return moe_route_entry("moe_route_ex", MoeRouteArgs{static_cast<const half_t *>(x), static_cast<const half_t *>(ex->router), rows, hidden, experts, top_k,
                                                        (flags & LLMIE_MOE_SOFTMAX_ALL) ? 1 : 0, expert_out, weight_out,
                                                        static_cast<const half_t *>(ex->router_bias)}, flags, dtype, stream);
}

int llmie::moe_call_check(const char *who, const MoeCall &c, MoePlan *plan) {
    MoePlan own;
    if (int rc = moe_shape_check(who, c)) return rc;
    return plan_moe(who, c, plan ? plan : &own);
}
// would the entries take this descriptor (llmie_decoder_moe_attach_ex checks every sparse layer's)?
int llmie::moe_experts_ok(const char *who, const llmie_moe_experts *ex) {
    if (int rc = moe_experts_check(who, ex)) return rc;
    return moe_experts_aligned(who, ex);
}

// llmie_moe_ffn / _ex = prepare + every stage
static int moe_ffn_entry(const char *who, const MoeCall &shape, const MoeOperands &o, llmie_stream stream) {
    MoePrepared m;
    if (int rc = moe_prepare(who, shape, o, nullptr, &m)) return rc;
    return moe_launch(m, MOE_STAGE_ALL, as_stream(stream));
}

extern "C" int llmie_moe_ffn(const void *x, const void *router, const void *gate_up, const void *down, const void *resid, void *y, int rows,
                             int hidden, int inter, int experts, int top_k, unsigned flags, void *workspace, size_t workspace_bytes,
                             llmie_dtype dtype, llmie_stream stream) {
    llmie_moe_experts ex{};   // fp16, no biases, plain SwiGLU
    ex.format = LLMIE_W_F16, ex.router = router, ex.gate_up = gate_up, ex.down = down, ex.act = LLMIE_MOE_ACT_SWIGLU;
    return moe_ffn_entry("moe_ffn", MoeCall{rows, hidden, inter, experts, top_k, flags}, MoeOperands{x, resid, y, &ex, workspace, workspace_bytes, dtype},
                         stream);
}

extern "C" int llmie_moe_ffn_ex(const void *x, const llmie_moe_experts *ex, const void *resid, void *y, int rows, int hidden, int inter, int experts,
                                int top_k, unsigned flags, void *workspace, size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream) {
    return moe_ffn_entry("moe_ffn_ex", MoeCall{rows, hidden, inter, experts, top_k, flags}, MoeOperands{x, resid, y, ex, workspace, workspace_bytes, dtype},
                         stream);
}

int llmie::moe_prepare(const char *who, const MoeCall &shape, const MoeOperands &o, const MoePlan *planned, MoePrepared *out) {
    const llmie_moe_experts *ex = o.experts;
    LLMIE_REQUIRE(o.x && o.y, "%s: NULL pointer", who);
    if (int rc = moe_experts_check(who, ex)) return rc;
    if (int rc = moe_shape_check(who, shape)) return rc;
    if (o.dtype != LLMIE_F16) LLMIE_UNSUPPORTED("%s: fp16 activations only", who);
    if (mis16(o.x) || mis16(o.resid) || mis16(o.y)) LLMIE_UNSUPPORTED("%s: x / router / gate_up / down / resid / y not 16-byte aligned", who);
    if (int rc = moe_experts_aligned(who, ex)) return rc;
    MoeCall c = shape;
    c.format = ex->format, c.ex = moe_epilogue_live(*ex);
    MoePlan &p = out->plan;
    if (planned && planned->call.format == c.format && planned->ex == c.ex) p = *planned;   // (a layer whose epilogue differs is planned here)
    else if (int rc = plan_moe(who, c, &p)) return rc;
    if (!o.workspace || o.workspace_bytes < p.ws.bytes || reinterpret_cast<uintptr_t>(o.workspace) % 256) {
        set_error("%s: workspace missing, too small or not 256-byte aligned (%zu < %zu)", who, o.workspace ? o.workspace_bytes : size_t(0), p.ws.bytes);
        return LLMIE_ERR_WORKSPACE;
    }
    char *base = static_cast<char *>(o.workspace);
    MoeLaunchArgs *la = new (out->args) MoeLaunchArgs{};
    MoeFfnArgs &a = la->a;
    a.x = static_cast<const half_t *>(o.x), a.gate_up = static_cast<const half_t *>(ex->gate_up), a.down = static_cast<const half_t *>(ex->down);
    a.resid = static_cast<const half_t *>(o.resid), a.y = static_cast<half_t *>(o.y), a.act = reinterpret_cast<half_t *>(base + p.ws.act);
    a.expert = reinterpret_cast<const int32_t *>(base + p.ws.expert), a.weight = reinterpret_cast<const float *>(base + p.ws.weight);
    a.rows = c.rows, a.H = c.H, a.Ie = c.Ie, a.E = c.E, a.k = c.k, a.pairs = p.pairs;
    a.hdr = reinterpret_cast<const int32_t *>(base), a.tile_expert = reinterpret_cast<const int32_t *>(base + p.ws.tile_expert);
    a.tile_pairs = reinterpret_cast<const int32_t *>(base + p.ws.tile_pairs), a.d = reinterpret_cast<float *>(base + p.ws.d);
    a.gate_up_scale = static_cast<const uint8_t *>(ex->gate_up_scale), a.down_scale = static_cast<const uint8_t *>(ex->down_scale);
    a.gate_up_bias = static_cast<const half_t *>(ex->gate_up_bias), a.down_bias = static_cast<const half_t *>(ex->down_bias);
    a.act_kind = static_cast<int>(ex->act), a.alpha = ex->alpha, a.limit = ex->limit;
    la->r = MoeRouteArgs{a.x, static_cast<const half_t *>(ex->router), c.rows, c.H, c.E, c.k, (c.flags & LLMIE_MOE_SOFTMAX_ALL) ? 1 : 0,
                         reinterpret_cast<int32_t *>(base + p.ws.expert), reinterpret_cast<float *>(base + p.ws.weight),
                         static_cast<const half_t *>(ex->router_bias)};
    return LLMIE_OK;
}

// the stages of a prepared call (the engine accounts them under three op kinds).  fp16 experts without a bias under plain SwiGLU
// (plan.ex false) launch the instantiations llmie_moe_ffn always launched
int llmie::moe_launch(const MoePrepared &m, unsigned stages, hipStream_t st) {
    const MoePlan &p = m.plan;
    const MoeLaunchArgs &la = *reinterpret_cast<const MoeLaunchArgs *>(m.args);
    const MoeFfnArgs &a = la.a;
    const bool mx4 = p.call.format == LLMIE_W_MXFP4, gemv = p.route == MOE_GEMV;
    const dim3 g1(p.gate_up_grid[0], p.gate_up_grid[1]), g2(p.down_grid[0], p.down_grid[1]), g3(p.combine_grid[0], p.combine_grid[1]);
    if (stages & MOE_STAGE_ROUTE) {
        moe_route_launch(la.r, st);
        if (int rc = launch_status("moe_ffn(route)")) return rc;
    }
    if (gemv) {
        if (stages & MOE_STAGE_GATE_UP) {
            if (mx4) moe_mx4_gemv_dispatch(p.gate_up_cfg, [&](auto xb, auto kw) { moe_mx4_gemv_gate_up_kernel<xb(), kw()><<<g1, 256, 0, st>>>(a); });
            else moe_gemv_dispatch(p.gate_up_cfg, p.ex, [&](auto xc, auto ex) { moe_gemv_gate_up_kernel<xc(), ex()><<<g1, 256, 0, st>>>(a); });
            if (int rc = launch_status("moe_ffn(gate_up gemv)")) return rc;
        }
        if (stages & MOE_STAGE_DOWN) {
            if (mx4) moe_mx4_gemv_dispatch(p.down_cfg, [&](auto xb, auto kw) { moe_mx4_gemv_down_kernel<xb(), kw()><<<g2, 256, 0, st>>>(a); });
            else moe_gemv_dispatch(p.down_cfg, p.ex, [&](auto xc, auto ex) { moe_gemv_down_kernel<xc(), ex()><<<g2, 256, 0, st>>>(a); });
            return launch_status("moe_ffn(down gemv)");
        }
        return LLMIE_OK;
    }
    if (stages & MOE_STAGE_GATE_UP) {
        moe_plan_kernel<<<1, 256, 0, st>>>(a.expert, p.pairs, a.E, p.rt, const_cast<int32_t *>(a.hdr), const_cast<int32_t *>(a.tile_expert),
                                           const_cast<int32_t *>(a.tile_pairs), p.tiles);
        if (int rc = launch_status("moe_ffn(plan)")) return rc;
        if (mx4) moe_rt_dispatch(p.rt, [&](auto rt) { moe_mx4_grouped_kernel<rt(), true><<<g1, 256, 0, st>>>(a); });
        else moe_ex_dispatch(p.ex, [&](auto ex) { moe_rt_dispatch(p.rt, [&](auto rt) { moe_grouped_kernel<rt(), true, ex()><<<g1, 256, 0, st>>>(a); }); });
        if (int rc = launch_status("moe_ffn(gate_up grouped)")) return rc;
    }
    if (stages & MOE_STAGE_DOWN) {
        if (mx4) moe_rt_dispatch(p.rt, [&](auto rt) { moe_mx4_grouped_kernel<rt(), false><<<g2, 256, 0, st>>>(a); });
        else moe_rt_dispatch(p.rt, [&](auto rt) { moe_grouped_kernel<rt(), false, false><<<g2, 256, 0, st>>>(a); });
        if (int rc = launch_status("moe_ffn(down grouped)")) return rc;
        moe_combine_kernel<<<g3, kMoeCombineThreads, 0, st>>>(a);
        return launch_status("moe_ffn(combine)");
    }
    return LLMIE_OK;
}
