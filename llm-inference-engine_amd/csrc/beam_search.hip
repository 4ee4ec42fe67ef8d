// llmie_beam_step and llmie_kv_pages_fork: several hypotheses per request on the paged KV cache (no reference launcher: the
// reference carries a beamwidth dimension and never fills it).
//
// beam step, two launches:
//   1. beam_row_kernel, one workgroup per live row r = g * width + w: the row is cut into chunks of 16 bytes by ELEMENT INDEX
//      (chunk c = elements [c N, c N + N)), thread t takes chunks t, t + 256, ... -- one 16-byte load where the row's address
//      allows it, N scalar loads otherwise, the same elements in the same order either way, so the bits of a row do not depend
//      on where it lies.  Per thread an online (max, sum) of the non-NaN logits and a sorted list of its `width` best
//      (value desc, id asc: llmie_topk's order); then the block maximum, the block sum in a fixed order (DPP inside a wave,
//      waves 0..3 in turn) and `width` rounds of block arg-max.  Writes lse and the `width` best (id, logit) of the row.
//      Dead and finished rows leave at once: they contribute without their logits.
//   2. beam_merge_kernel, one wave per group: candidate c = w * width + k (beam, rank in its row) -- the index IS the tie order
//      -- `width` rounds of wave arg-max on (key desc, c asc), then lane j writes slot j.  The group's state is copied to LDS
//      before anything is written.
//
// fork, two launches: gather (tails and the new table rows / lengths into the workspace, every read of the old state happens
// here) and scatter (workspace -> pools, table, lengths).  Inside a page [kvh, 128, hs] the first r token rows of one
// (layer, head) are r * row_bytes CONTIGUOUS bytes: one workgroup copies one such run, 16 bytes per lane where both addresses
// allow it and plain bytes otherwise.
#include "device_utils.cuh"

#include <climits>

namespace llmie {
namespace {

__device__ __forceinline__ bool beam_better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

template <int KMAX> struct BeamList {
    float v[KMAX];
    int id[KMAX];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int i = 0; i < KMAX; ++i) {
            v[i] = -INFINITY;
            id[i] = INT_MAX;
        }
    }
    // keeps (value desc, id asc); a NaN is never better than anything and never enters
    __device__ __forceinline__ void insert(float x, int xi) {
        if (!beam_better(x, xi, v[KMAX - 1], id[KMAX - 1])) return;
        v[KMAX - 1] = x;
        id[KMAX - 1] = xi;
#pragma unroll
        for (int j = KMAX - 1; j > 0; --j) {
            if (beam_better(v[j], id[j], v[j - 1], id[j - 1])) {
                const float tv = v[j]; v[j] = v[j - 1]; v[j - 1] = tv;
                const int ti = id[j]; id[j] = id[j - 1]; id[j - 1] = ti;
            }
        }
    }
    __device__ __forceinline__ void pop() {
#pragma unroll
        for (int j = 0; j < KMAX - 1; ++j) {
            v[j] = v[j + 1];
            id[j] = id[j + 1];
        }
        v[KMAX - 1] = -INFINITY;
        id[KMAX - 1] = INT_MAX;
    }
};

__device__ __forceinline__ bool beam_dead(float cum) { return !(cum > -INFINITY); }   // -inf or NaN

// workspace: lse [rows] floats, ids [rows, width] int32, vals [rows, width] floats
template <typename T, int KMAX>
__global__ __launch_bounds__(256) void beam_row_kernel(const T *__restrict__ logits, const float *__restrict__ cum,
                                                       const uint8_t *__restrict__ finished, int vocab, int width,
                                                       float *__restrict__ ws_lse, int32_t *__restrict__ ws_id,
                                                       float *__restrict__ ws_val) {
    __shared__ float s_f[4];
    __shared__ float s_v[4];
    __shared__ int s_i[4];
    const int row = blockIdx.x;
    if (beam_dead(cum[row]) || finished[row]) return;   // (uniform over the workgroup)
    constexpr int N = Vec16<T>::n;
    using V = typename Vec16<T>::type;
    const T *p = logits + static_cast<size_t>(row) * vocab;
    const bool vec_ok = reinterpret_cast<uintptr_t>(p) % 16 == 0;
    const int chunks = (vocab + N - 1) / N;
    BeamList<KMAX> tl;
    tl.init();
    float m = -INFINITY, s = 0.f;
    for (int c = threadIdx.x; c < chunks; c += 256) {
        float x[N];
        const int e0 = c * N;
        if (vec_ok && e0 + N <= vocab) {
            const V xv = reinterpret_cast<const V *>(p)[c];
#pragma unroll
            for (int e = 0; e < N; ++e) x[e] = to_f32(xv[e]);
        } else {
#pragma unroll
            for (int e = 0; e < N; ++e) x[e] = e0 + e < vocab ? to_f32(p[e0 + e]) : __builtin_nanf("");   // past the row: a NaN, skipped below
        }
        float cm = -INFINITY;
#pragma unroll
        for (int e = 0; e < N; ++e)
            if (x[e] == x[e]) cm = fmaxf(cm, x[e]);
        if (cm > m) {   // (cm > -inf here, so m - cm is -inf or finite, never NaN)
            s *= expf(m - cm);
            m = cm;
        }
        if (m > -INFINITY) {
#pragma unroll
            for (int e = 0; e < N; ++e)
                if (x[e] == x[e]) s += expf(x[e] - m);
        }
#pragma unroll
        for (int e = 0; e < N; ++e) tl.insert(x[e], e0 + e);
    }
    const float bm = block_max<4>(m, s_f);
    const float bs = block_sum<4>(m > -INFINITY ? s * expf(m - bm) : 0.f, s_f);
    if (threadIdx.x == 0) ws_lse[row] = bm + logf(bs);
    // `width` rounds of block arg-max over the heads of the per-thread lists
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int k = 0; k < width; ++k) {
        float bv = tl.v[0];
        int bi = tl.id[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = lane_xor_o(bv, o);
            const int oi = lane_xor_o(bi, o);
            if (beam_better(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
        __syncthreads();
        if (lane == 0) {
            s_v[wave] = bv;
            s_i[wave] = bi;
        }
        __syncthreads();
        bv = s_v[0];
        bi = s_i[0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (beam_better(s_v[w], s_i[w], bv, bi)) {
                bv = s_v[w];
                bi = s_i[w];
            }
        if (bi != INT_MAX && tl.id[0] == bi) tl.pop();   // ids are unique: exactly one owner
        if (threadIdx.x == 0) {
            ws_id[static_cast<size_t>(row) * width + k] = bi == INT_MAX ? -1 : bi;
            ws_val[static_cast<size_t>(row) * width + k] = bv;
        }
    }
}

struct BeamCand {
    float key, score;
    int token, len, fin;
    bool valid;
};

// candidate c = w * width + k of a group, from the group's old state (LDS) and the row pass's lists
__device__ __forceinline__ BeamCand beam_cand(int c, int n_cand, int width, int row0, const float *s_cum, const int *s_len,
                                              const uint8_t *s_fin, const float *__restrict__ ws_lse,
                                              const int32_t *__restrict__ ws_id, const float *__restrict__ ws_val, int end_id,
                                              float length_penalty) {
    BeamCand r;
    r.key = -INFINITY; r.score = -INFINITY; r.token = end_id; r.len = 0; r.fin = 1; r.valid = false;
    if (c >= n_cand) return r;
    const int w = c / width, k = c - w * width;
    const float cum = s_cum[w];
    if (beam_dead(cum)) return r;
    if (s_fin[w]) {
        if (k != 0) return r;
        r.score = cum; r.len = s_len[w]; r.valid = true;
    } else {
        const size_t at = static_cast<size_t>(row0 + w) * width + k;
        const int id = ws_id[at];
        if (id < 0) return r;
        const float lp = ws_val[at] - ws_lse[row0 + w];   // one subtract, one add, as the header states
        r.score = cum + lp;
        if (r.score != r.score) return r;   // a +inf logit (or an all -inf row) has no log-probability: no candidate
        r.token = id; r.len = s_len[w] + 1; r.fin = id == end_id; r.valid = true;
    }
    r.key = length_penalty == 0.f ? r.score : r.score / powf(static_cast<float>(r.len), length_penalty);
    if (r.key != r.key) r.key = -INFINITY;   // (0 / 0 at len 0: ranked last, never lost)
    return r;
}

__global__ __launch_bounds__(64) void beam_merge_kernel(int width, float *__restrict__ cum, int32_t *__restrict__ gen_len,
                                                        uint8_t *__restrict__ finished, int32_t *__restrict__ out_parent,
                                                        int32_t *__restrict__ out_token, const float *__restrict__ ws_lse,
                                                        const int32_t *__restrict__ ws_id, const float *__restrict__ ws_val,
                                                        int end_id, float length_penalty) {
    __shared__ float s_cum[LLMIE_BEAM_MAX_WIDTH];
    __shared__ int s_len[LLMIE_BEAM_MAX_WIDTH];
    __shared__ uint8_t s_fin[LLMIE_BEAM_MAX_WIDTH];
    const int lane = threadIdx.x, row0 = blockIdx.x * width;
    if (lane < width) {
        s_cum[lane] = cum[row0 + lane];
        s_len[lane] = gen_len[row0 + lane];
        s_fin[lane] = finished[row0 + lane];
    }
    __syncthreads();   // every read of the group's state lies in front of this barrier, every write behind it
    const int n_cand = width * width;   // <= 256: four per lane
    float key[4];
    int idx[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        const BeamCand cd = beam_cand(c, n_cand, width, row0, s_cum, s_len, s_fin, ws_lse, ws_id, ws_val, end_id, length_penalty);
        key[i] = cd.valid ? cd.key : -INFINITY;
        idx[i] = cd.valid ? c : INT_MAX;
    }
    int mine = INT_MAX;   // lane j: the candidate of slot j
    for (int j = 0; j < width; ++j) {
        float bv = key[0];
        int bi = idx[0];
#pragma unroll
        for (int i = 1; i < 4; ++i)
            if (beam_better(key[i], idx[i], bv, bi)) {
                bv = key[i];
                bi = idx[i];
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = lane_xor_o(bv, o);
            const int oi = lane_xor_o(bi, o);
            if (beam_better(ov, oi, bv, bi)) {
                bv = ov;
                bi = oi;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (idx[i] == bi && bi != INT_MAX) {   // its owner retires it
                key[i] = -INFINITY;
                idx[i] = INT_MAX;
            }
        if (lane == j) mine = bi;
    }
    if (lane < width) {
        const int r = row0 + lane;
        const BeamCand cd = beam_cand(mine == INT_MAX ? n_cand : mine, n_cand, width, row0, s_cum, s_len, s_fin, ws_lse, ws_id, ws_val,
                                      end_id, length_penalty);
        // no candidate left: a dead slot whose parent is the slot itself (the fork leaves it alone)
        out_parent[r] = cd.valid ? row0 + mine / width : r;
        out_token[r] = cd.token;
        cum[r] = cd.score;
        gen_len[r] = cd.len;
        finished[r] = static_cast<uint8_t>(cd.valid ? (s_fin[mine / width] || cd.fin) : 1);
    }
}

template <typename T>
int beam_rows(const void *logits, int rows, int vocab, int width, const float *cum, const uint8_t *finished, float *ws_lse,
              int32_t *ws_id, float *ws_val, hipStream_t st) {
    const T *p = static_cast<const T *>(logits);
    if (width <= 4) beam_row_kernel<T, 4><<<rows, 256, 0, st>>>(p, cum, finished, vocab, width, ws_lse, ws_id, ws_val);
    else if (width <= 8) beam_row_kernel<T, 8><<<rows, 256, 0, st>>>(p, cum, finished, vocab, width, ws_lse, ws_id, ws_val);
    else beam_row_kernel<T, 16><<<rows, 256, 0, st>>>(p, cum, finished, vocab, width, ws_lse, ws_id, ws_val);
    return launch_status("beam_step(rows)");
}

// ---------------------------------------------------------------- fork of paged KV rows
constexpr int kPage = LLMIE_KV_PAGE_TOKENS;

__host__ __device__ inline size_t fork_slot_bytes(size_t row_bytes) { return ((kPage - 1) * row_bytes + 15) / 16 * 16; }

// staged ints behind the tails: per row {act, n, dst page, pad} then the new table rows [rows, max_pages]
struct ForkPlan {
    int act, n, src, dst;
};

// what row j does, from the OLD state (gather kernel only)
__device__ __forceinline__ ForkPlan fork_plan(int j, const int32_t *__restrict__ block_table, const int32_t *__restrict__ own_table,
                                              const int32_t *__restrict__ parent, const int32_t *__restrict__ cached_len, int rows,
                                              int max_pages, int num_pages) {
    ForkPlan p = {0, 0, -1, -1};
    const int q = parent[j];
    if (q == j || q < 0 || q >= rows) return p;
    const int n = cached_len[q];
    if (n < 0 || n > kPage * max_pages) return p;
    const int pc = n / kPage, r = n % kPage;
    if (r > 0) {   // (then pc < max_pages)
        p.src = block_table[static_cast<size_t>(q) * max_pages + pc];
        p.dst = own_table[static_cast<size_t>(j) * max_pages + pc];
        if (p.src < 0 || p.src >= num_pages || p.dst < 0 || p.dst >= num_pages) return p;
    }
    p.act = 1;
    p.n = n;
    return p;
}

// `bytes` contiguous bytes; 16 per lane where both ends allow it
__device__ __forceinline__ void fork_copy_run(unsigned char *dst, const unsigned char *src, size_t bytes) {
    if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) % 16 == 0) {
        const size_t nv = bytes / 16;
        for (size_t i = threadIdx.x; i < nv; i += 256) reinterpret_cast<uint4_t *>(dst)[i] = reinterpret_cast<const uint4_t *>(src)[i];
        for (size_t i = nv * 16 + threadIdx.x; i < bytes; i += 256) dst[i] = src[i];
    } else {
        for (size_t i = threadIdx.x; i < bytes; i += 256) dst[i] = src[i];
    }
}

// grid (kv head, layer, 2 * row + pool)
__global__ __launch_bounds__(256) void kv_fork_gather_kernel(const unsigned char *__restrict__ k_pool, const unsigned char *__restrict__ v_pool,
                                                             const int32_t *__restrict__ block_table, const int32_t *__restrict__ own_table,
                                                             const int32_t *__restrict__ parent, const int32_t *__restrict__ cached_len,
                                                             int rows, int kvh, int max_pages, int num_pages, size_t row_bytes,
                                                             unsigned char *__restrict__ tails, int32_t *__restrict__ staged) {
    const int g = blockIdx.x, layer = blockIdx.y, j = blockIdx.z >> 1, pool = blockIdx.z & 1, layers = gridDim.y;
    const ForkPlan p = fork_plan(j, block_table, own_table, parent, cached_len, rows, max_pages, num_pages);
    if (g == 0 && layer == 0 && pool == 0) {   // one workgroup per row stages the plan and the new table row
        if (threadIdx.x == 0) {
            staged[4 * j + 0] = p.act;
            staged[4 * j + 1] = p.n;
            staged[4 * j + 2] = p.dst;
            staged[4 * j + 3] = 0;
        }
        if (p.act) {
            const int q = parent[j], pc = p.n / kPage;
            int32_t *row = staged + 4 * static_cast<size_t>(rows) + static_cast<size_t>(j) * max_pages;
            for (int i = threadIdx.x; i < max_pages; i += 256)
                row[i] = i < pc ? block_table[static_cast<size_t>(q) * max_pages + i] : own_table[static_cast<size_t>(j) * max_pages + i];
        }
    }
    const int r = p.n % kPage;
    if (!p.act || r == 0) return;
    const unsigned char *src = (pool ? v_pool : k_pool) + ((static_cast<size_t>(layer) * num_pages + p.src) * kvh + g) * kPage * row_bytes;
    unsigned char *dst = tails + (((static_cast<size_t>(j) * 2 + pool) * layers + layer) * kvh + g) * fork_slot_bytes(row_bytes);
    fork_copy_run(dst, src, r * row_bytes);
}

// reads the workspace (and nothing of the old state), writes pools, table and lengths
__global__ __launch_bounds__(256) void kv_fork_scatter_kernel(unsigned char *__restrict__ k_pool, unsigned char *__restrict__ v_pool,
                                                              int32_t *__restrict__ block_table, int32_t *__restrict__ cached_len,
                                                              int rows, int kvh, int max_pages, int num_pages, size_t row_bytes,
                                                              const unsigned char *__restrict__ tails, const int32_t *__restrict__ staged) {
    const int g = blockIdx.x, layer = blockIdx.y, j = blockIdx.z >> 1, pool = blockIdx.z & 1, layers = gridDim.y;
    if (!staged[4 * j]) return;
    const int n = staged[4 * j + 1], page = staged[4 * j + 2];
    if (g == 0 && layer == 0 && pool == 0) {
        if (threadIdx.x == 0) cached_len[j] = n;
        const int32_t *row = staged + 4 * static_cast<size_t>(rows) + static_cast<size_t>(j) * max_pages;
        for (int i = threadIdx.x; i < max_pages; i += 256) block_table[static_cast<size_t>(j) * max_pages + i] = row[i];
    }
    const int r = n % kPage;
    if (r == 0) return;
    unsigned char *dst = (pool ? v_pool : k_pool) + ((static_cast<size_t>(layer) * num_pages + page) * kvh + g) * kPage * row_bytes;
    const unsigned char *src = tails + (((static_cast<size_t>(j) * 2 + pool) * layers + layer) * kvh + g) * fork_slot_bytes(row_bytes);
    fork_copy_run(dst, src, r * row_bytes);
}

size_t fork_tail_bytes(int rows, int layers, int kvh, size_t row_bytes) {
    return static_cast<size_t>(rows) * 2 * layers * kvh * fork_slot_bytes(row_bytes);
}

}  // namespace
}  // namespace llmie

using namespace llmie;

extern "C" size_t llmie_beam_step_workspace_bytes(int groups, int width, int vocab) {
    if (groups < 1 || width < 1 || vocab < 1 || width > LLMIE_BEAM_MAX_WIDTH) return 0;
    return (static_cast<size_t>(groups) * width * (1 + 2 * static_cast<size_t>(width)) * 4 + 15) / 16 * 16;
}

extern "C" int llmie_beam_step(const void *logits, int groups, int width, int vocab, float *cum_logprob, int32_t *gen_len,
                               uint8_t *finished, int32_t *out_parent, int32_t *out_token, int end_id, float length_penalty,
                               void *workspace, size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream) {
    LLMIE_REQUIRE(logits && cum_logprob && gen_len && finished && out_parent && out_token, "beam_step: NULL pointer");
    LLMIE_REQUIRE(groups > 0 && width > 0 && vocab > 0, "beam_step: bad shape groups=%d width=%d vocab=%d", groups, width, vocab);
    LLMIE_REQUIRE(length_penalty == length_penalty, "beam_step: length_penalty is NaN");
    if (width > LLMIE_BEAM_MAX_WIDTH) LLMIE_UNSUPPORTED("beam_step: width %d above LLMIE_BEAM_MAX_WIDTH (%d)", width, LLMIE_BEAM_MAX_WIDTH);
    LLMIE_REQUIRE(static_cast<long long>(groups) * width <= INT_MAX / 2, "beam_step: groups * width = %lld rows", static_cast<long long>(groups) * width);
    const size_t need = llmie_beam_step_workspace_bytes(groups, width, vocab);
    if (!workspace || workspace_bytes < need || reinterpret_cast<uintptr_t>(workspace) % 4) {
        set_error("beam_step: workspace of %zu bytes at %p, %zu bytes at a 4-byte aligned address needed (llmie_beam_step_workspace_bytes)",
                  workspace ? workspace_bytes : size_t{0}, workspace, need);
        return LLMIE_ERR_WORKSPACE;
    }
    if (dtype != LLMIE_F16 && dtype != LLMIE_F32) LLMIE_UNSUPPORTED("beam_step: dtype %d", (int)dtype);
    LLMIE_REQUIRE(reinterpret_cast<uintptr_t>(logits) % (dtype == LLMIE_F16 ? 2 : 4) == 0, "beam_step: logits are not aligned to their element");
    const int rows = groups * width;
    float *ws_lse = static_cast<float *>(workspace);
    int32_t *ws_id = reinterpret_cast<int32_t *>(ws_lse + rows);
    float *ws_val = reinterpret_cast<float *>(ws_id + static_cast<size_t>(rows) * width);
    hipStream_t st = as_stream(stream);
    const int rc = dtype == LLMIE_F16 ? beam_rows<half_t>(logits, rows, vocab, width, cum_logprob, finished, ws_lse, ws_id, ws_val, st)
                                      : beam_rows<float>(logits, rows, vocab, width, cum_logprob, finished, ws_lse, ws_id, ws_val, st);
    if (rc != LLMIE_OK) return rc;
    beam_merge_kernel<<<groups, 64, 0, st>>>(width, cum_logprob, gen_len, finished, out_parent, out_token, ws_lse, ws_id, ws_val, end_id,
                                             length_penalty);
    return launch_status("beam_step(merge)");
}

extern "C" size_t llmie_kv_pages_fork_workspace_bytes(int rows, int layers, int kv_head_num, int head_size, int elem_bytes, int max_pages) {
    if (rows < 1 || layers < 1 || kv_head_num < 1 || head_size < 1 || elem_bytes < 1 || max_pages < 1) return 0;
    const size_t ints = static_cast<size_t>(rows) * (4 + static_cast<size_t>(max_pages)) * 4;
    return fork_tail_bytes(rows, layers, kv_head_num, static_cast<size_t>(head_size) * elem_bytes) + (ints + 15) / 16 * 16;
}

extern "C" int llmie_kv_pages_fork(void *k_pool, void *v_pool, int32_t *block_table, const int32_t *own_table, const int32_t *parent,
                                   int32_t *cached_len, int rows, int layers, int kv_head_num, int head_size, int max_pages, int num_pages,
                                   int elem_bytes, void *workspace, size_t workspace_bytes, llmie_stream stream) {
    LLMIE_REQUIRE(k_pool && v_pool && block_table && own_table && parent && cached_len, "kv_pages_fork: NULL pointer");
    LLMIE_REQUIRE(rows > 0 && layers > 0 && kv_head_num > 0 && head_size > 0 && max_pages > 0 && num_pages > 0 && elem_bytes > 0,
                  "kv_pages_fork: bad shape");
    LLMIE_REQUIRE(static_cast<long long>(max_pages) * LLMIE_KV_PAGE_TOKENS <= INT_MAX, "kv_pages_fork: max_pages %d too large", max_pages);
    if (kv_head_num > 65535 || layers > 65535 || rows > 32767)
        LLMIE_UNSUPPORTED("kv_pages_fork: grid too large (kv_head_num %d, layers %d above 65535 or rows %d above 32767)", kv_head_num, layers, rows);
    const size_t need = llmie_kv_pages_fork_workspace_bytes(rows, layers, kv_head_num, head_size, elem_bytes, max_pages);
    if (!workspace || workspace_bytes < need || reinterpret_cast<uintptr_t>(workspace) % 16) {
        set_error("kv_pages_fork: workspace of %zu bytes at %p, %zu bytes at a 16-byte aligned address needed "
                  "(llmie_kv_pages_fork_workspace_bytes)", workspace ? workspace_bytes : size_t{0}, workspace, need);
        return LLMIE_ERR_WORKSPACE;
    }
    const size_t row_bytes = static_cast<size_t>(head_size) * elem_bytes;
    unsigned char *tails = static_cast<unsigned char *>(workspace);
    int32_t *staged = reinterpret_cast<int32_t *>(tails + fork_tail_bytes(rows, layers, kv_head_num, row_bytes));
    hipStream_t st = as_stream(stream);
    const dim3 grid(kv_head_num, layers, 2 * rows);
    kv_fork_gather_kernel<<<grid, 256, 0, st>>>(static_cast<const unsigned char *>(k_pool), static_cast<const unsigned char *>(v_pool),
                                                block_table, own_table, parent, cached_len, rows, kv_head_num, max_pages, num_pages,
                                                row_bytes, tails, staged);
    const int rc = launch_status("kv_pages_fork(gather)");
    if (rc != LLMIE_OK) return rc;
    kv_fork_scatter_kernel<<<grid, 256, 0, st>>>(static_cast<unsigned char *>(k_pool), static_cast<unsigned char *>(v_pool), block_table,
                                                 cached_len, rows, kv_head_num, max_pages, num_pages, row_bytes, tails, staged);
    return launch_status("kv_pages_fork(scatter)");
}
