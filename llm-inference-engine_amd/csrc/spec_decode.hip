// Speculative decoding behind the logits: llmie_spec_verify (how many draft tokens survive, under the full per-request sampling
// semantics) and llmie_ngram_draft (a drafter that needs no second model).  No reference launcher.
//
// llmie_spec_verify, two launches:
//   rows    one 1024-thread workgroup per (sequence b, position i), r = b * (k + 1) + i: sp_sample_row -- the sampler's own body
//           (sampling_body.cuh) -- at Philox step s_b + i, on a history VIEW that splices draft_ids[b, 0..i) behind the stored
//           history.  Position i only matters when the picks 0..i-1 equalled the drafts 0..i-1, and then that view IS the history
//           i sequential sampler calls would have left; so the k + 1 positions of a sequence run side by side.  The pick, its raw
//           log-probability and its finish flag go to the workspace; no state is written.
//   accept  one thread per sequence walks its picks (<= 16), writes the outputs and moves the state exactly as `count` sampler
//           calls would have.
// The sampler is deterministic (Philox keyed by (step, seed), fixed-point masses), so position i has ONE pick plain decoding would
// have made from these logits, and draft i is accepted iff it equals it: the emitted tokens are bit for bit those of `count`
// llmie_sample_logits_ext calls.
//
// llmie_spec_verify_sampled, two launches of the same shape, for a drafter that SAMPLED its drafts: the rows kernel prepares the
// target row and the draft row (sp_prepare_row: the kept set and its fixed-point masses instead of a pick) in two key rows of the
// workspace and decides by the rejection rule min(1, p / q) -- cross-multiplied, one exact comparison of 128-bit integers -- and,
// behind a rejection, draws from the residual max(0, P_v S_Q - Q_v S_P) by a scan in ascending id order; the accept kernel walks
// the records.  include/llmie.h has the rule.
//
// llmie_ngram_draft, one launch, one 256-thread workgroup per sequence: ONE sweep over the row finds, for every n at once, the
// last place the sequence's final n tokens occurred before.  A thread that sees the final token at q extends the comparison
// backwards (<= 7 more loads, rare); the sweep itself reads 16 bytes per thread where the row is aligned.  "The last place" is an
// integer maximum in LDS: deterministic.
//
// Draft TREES (llmie_spec_tree_prepare, llmie_spec_verify_tree, llmie_ngram_draft_tree; include/llmie.h has the rules): up to 64 node
// slots per sequence, parent < child.  prepare: one launch, depth and a 64-bit ancestor mask per node ("live" = bit 0).  verify_tree:
// the rows launch of llmie_spec_verify with the history view of a node's PATH (its tokens gathered into LDS first) at Philox step
// s_b + depth, then one thread per sequence walks the tree in LDS -- the lowest live child that carries the pick.  ngram_draft_tree:
// the drafter's sweep, then the continuations of several suffix lengths merged into a trie by one thread.
//
// The verify entries are shells over ONE host function, spec_verify_impl (checks, workspace carve, rows launch, accept launch;
// SpecDraft::sampled / ::tree pick the kernels); the two rows kernels share spec_row_view and the sampler's epilogue helpers.  The accept
// kernels keep their own walk + state commit: one function around a per-position callable cost spec_accept_kernel a register.
#include "sampling_body.cuh"

namespace llmie {
namespace {

// the penalty history of position i: the stored history of sequence b, then -- as far as the appends of i sampler calls would
// have reached -- the drafts in front of i
struct SpSplicedHistory {
    const int32_t *row, *draft;   // history[b], draft_ids[b]
    int stored, len;
    __device__ __forceinline__ int length() const { return len; }
    __device__ __forceinline__ int at(int j) const { return j < stored ? row[j] : draft[j - stored]; }
};

// A rows kernel's view of workgroup r = b * (k + 1) + i: the sequence, the position, its Philox step and its penalty history
struct SpecRowView {
    int b, i, step;
    SpSplicedHistory hist;
};
__device__ __forceinline__ SpecRowView spec_row_view(int r, int k, const int32_t *__restrict__ history, int hstride,
                                                     const int32_t *__restrict__ history_len, int happend, const int32_t *__restrict__ draft_ids,
                                                     const int32_t *__restrict__ step_rows, int step_arg, const int32_t *step_dev) {
    const int b = r / (k + 1), i = r - b * (k + 1);
    const int step = (step_rows ? step_rows[b] : (step_dev ? *step_dev : step_arg)) + i;
    SpSplicedHistory hist{nullptr, draft_ids + static_cast<size_t>(b) * k, 0, 0};
    if (hstride > 0) {
        const int len0 = history_len[b];
        hist.row = history + static_cast<size_t>(b) * hstride;
        hist.stored = min(max(len0, 0), hstride);
        // (a negative length is never appended to: llmie_sample_logits appends while 0 <= history_len < history_stride)
        hist.len = (happend && len0 >= 0) ? min(hist.stored + i, hstride) : hist.stored;
    }
    return SpecRowView{b, i, step, hist};
}

struct SpecPick {   // workspace record of a row
    int32_t token;
    float logprob;
    int32_t fin, pad;
};

template <typename T, bool EXT>
__global__ __launch_bounds__(kSpThreads) void spec_verify_rows_kernel(
    const T *__restrict__ logits, int V, int k, const llmie_sampling_params *__restrict__ params, const int32_t *__restrict__ history,
    int hstride, const int32_t *__restrict__ history_len, int happend, const int32_t *__restrict__ draft_ids,
    const int32_t *__restrict__ step_rows, int step_arg, const int32_t *__restrict__ step_dev, int end_id, uint32_t *ws, size_t ws_row,
    SpecPick *__restrict__ picks, const llmie_sampling_ext ext) {
    __shared__ alignas(16) SpShared s;
    const int r = blockIdx.x;
    const SpecRowView v = spec_row_view(r, k, history, hstride, history_len, happend, draft_ids, step_rows, step_arg, step_dev);
    const T *lg = logits + static_cast<size_t>(r) * V;
    const SpPick pick = sp_sample_row<T, EXT>(lg, V, params[v.b], v.hist, v.step, end_id, ws + static_cast<size_t>(r) * ws_row, EXT ? &ext : nullptr,
                                              v.b, r, s);
    if (threadIdx.x == 0) {
        SpecPick out;
        out.token = pick.chosen;
        out.logprob = sp_logprob(lg, V, pick, pick.lse_m + logf(pick.lse_s), pick.chosen);
        out.fin = sp_finishes<EXT>(pick, pick.chosen, end_id) ? 1 : 0;
        out.pad = 0;
        picks[r] = out;
    }
}

// one workgroup (one working thread) per sequence
__global__ __launch_bounds__(64) void spec_accept_kernel(const SpecPick *__restrict__ picks, int k, const int32_t *__restrict__ draft_ids,
                                                         const int32_t *__restrict__ draft_len, int32_t *history, int hstride,
                                                         int32_t *history_len, int happend, int32_t *seq_len, uint8_t *finished,
                                                         int32_t *__restrict__ out_tokens, int32_t *__restrict__ out_count,
                                                         float *__restrict__ out_logprob, int32_t *last_token, int32_t *cached_len,
                                                         int32_t *step_rows) {
    if (threadIdx.x != 0) return;
    const int b = blockIdx.x, n = k + 1;
    int32_t *tok = out_tokens + static_cast<size_t>(b) * n;
    float *lp = out_logprob ? out_logprob + static_cast<size_t>(b) * n : nullptr;
    int count = 0;
    if (!finished[b]) {
        const int dl = draft_len ? min(max(draft_len[b], 0), k) : k;
        const SpecPick *p = picks + static_cast<size_t>(b) * n;
        const int32_t *draft = draft_ids + static_cast<size_t>(b) * k;
        int hl = (happend && hstride > 0) ? history_len[b] : -1;
        int fin = 0;
        for (int i = 0; i < n; ++i) {
            const SpecPick c = p[i];
            tok[i] = c.token;
            if (lp) lp[i] = c.logprob;
            ++count;
            if (hl >= 0 && hl < hstride) history[static_cast<size_t>(b) * hstride + hl++] = c.token;
            fin = c.fin;
            if (i == dl || fin || c.token != draft[i]) break;
        }
        seq_len[b] += count;
        finished[b] = static_cast<uint8_t>(fin);
        if (happend && hstride > 0 && hl >= 0) history_len[b] = hl;
        if (last_token) last_token[b] = tok[count - 1];
        if (cached_len) cached_len[b] += count;
        if (step_rows) step_rows[b] += count;
    }
    for (int i = count; i < n; ++i) {
        tok[i] = -1;
        if (lp) lp[i] = -INFINITY;
    }
    out_count[b] = count;
}

// ---------------------------------------------------------------------------------------------- llmie_spec_verify_tree
// A draft TREE per sequence: n node slots, node 0 = the last emitted token, parent < child.  llmie_spec_tree_prepare turns the
// parent array into a depth and an ancestor mask per node (bit j of anc[i]: node j lies on the path root -> i, i included); "live"
// is "bit 0 of anc is set" for every consumer.
constexpr int kTreeMax = LLMIE_SPEC_TREE_MAX_NODES;
static_assert(kTreeMax == 64, "an ancestor mask is one 64-bit word");

// one workgroup per sequence; the nodes depend on their parents, so one thread walks them in index order (<= 63 steps in LDS)
__global__ __launch_bounds__(64) void spec_tree_prepare_kernel(const int32_t *__restrict__ parent, const int32_t *__restrict__ node_count, int n,
                                                               int32_t *__restrict__ depth_out, u64 *__restrict__ anc_out) {
    __shared__ int32_t par[kTreeMax], dep[kTreeMax];
    __shared__ u64 anc[kTreeMax];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < n) par[tid] = parent[static_cast<size_t>(b) * n + tid];
    __syncthreads();
    if (tid == 0) {
        const int cnt = node_count ? min(max(node_count[b], 1), n) : n;
        dep[0] = 0;
        anc[0] = 1ull;
        for (int i = 1; i < n; ++i) {
            const int p = par[i];
            const bool live = i < cnt && p >= 0 && p < i && (anc[p] & 1ull);
            dep[i] = live ? dep[p] + 1 : 0;
            anc[i] = live ? (anc[p] | (1ull << i)) : (1ull << i);
        }
    }
    __syncthreads();
    if (tid < n) {
        depth_out[static_cast<size_t>(b) * n + tid] = dep[tid];
        anc_out[static_cast<size_t>(b) * n + tid] = anc[tid];
    }
}

// the penalty history of node i: the stored history of sequence b, then -- as far as the appends of depth_i sampler calls would have
// reached -- the tokens of the nodes on the path root -> i (root excluded, i included), gathered into LDS in depth order
struct SpTreeHistory {
    const int32_t *row, *path;   // history[b], LDS path[d - 1] = token of the ancestor at depth d
    int stored, len;
    __device__ __forceinline__ int length() const { return len; }
    __device__ __forceinline__ int at(int j) const { return j < stored ? row[j] : path[j - stored]; }
};

// One 1024-thread workgroup per (sequence b, node i), r = b * n + i: sp_sample_row at Philox step s_b + depth_i on the history view
// of the node's path.  A dead node (bit 0 of anc clear) samples at depth 0 on the stored history: the walk never reaches it, its
// top-N outputs are a property of the raw logits.  No state is written.
template <typename T, bool EXT>
__global__ __launch_bounds__(kSpThreads) void spec_tree_rows_kernel(
    const T *__restrict__ logits, int V, int n, const llmie_sampling_params *__restrict__ params, const int32_t *__restrict__ history,
    int hstride, const int32_t *__restrict__ history_len, int happend, const int32_t *__restrict__ node_ids,
    const int32_t *__restrict__ depth, const u64 *__restrict__ anc, const int32_t *__restrict__ step_rows, int step_arg,
    const int32_t *__restrict__ step_dev, int end_id, uint32_t *ws, size_t ws_row, SpecPick *__restrict__ picks, const llmie_sampling_ext ext) {
    __shared__ alignas(16) SpShared s;
    __shared__ int32_t path[kTreeMax];
    const int r = blockIdx.x;
    const int b = r / n, i = r - b * n;
    const size_t base = static_cast<size_t>(b) * n;
    const u64 mine = anc[base + i] & ((2ull << i) - 1ull);   // (2ull << 63 == 0: every bit)
    const bool live = (mine & 1ull) != 0;
    const int di = live ? min(max(depth[base + i], 0), i) : 0;
    if (threadIdx.x < kTreeMax) path[threadIdx.x] = -1;
    __syncthreads();
    if (live && threadIdx.x >= 1 && threadIdx.x <= static_cast<unsigned>(i) && ((mine >> threadIdx.x) & 1ull)) {
        const int dj = depth[base + threadIdx.x];
        if (dj >= 1 && dj <= di) path[dj - 1] = node_ids[base + threadIdx.x];
    }
    __syncthreads();
    const int step = (step_rows ? step_rows[b] : (step_dev ? *step_dev : step_arg)) + di;
    SpTreeHistory hist{nullptr, path, 0, 0};
    if (hstride > 0) {
        const int len0 = history_len[b];
        hist.row = history + static_cast<size_t>(b) * hstride;
        hist.stored = min(max(len0, 0), hstride);
        hist.len = (happend && len0 >= 0) ? min(hist.stored + di, hstride) : hist.stored;
    }
    const T *lg = logits + static_cast<size_t>(r) * V;
    const SpPick pick = sp_sample_row<T, EXT>(lg, V, params[b], hist, step, end_id, ws + static_cast<size_t>(r) * ws_row, EXT ? &ext : nullptr, b, r, s);
    if (threadIdx.x == 0) {
        SpecPick out;
        out.token = pick.chosen;
        out.logprob = sp_logprob(lg, V, pick, pick.lse_m + logf(pick.lse_s), pick.chosen);
        out.fin = sp_finishes<EXT>(pick, pick.chosen, end_id) ? 1 : 0;
        out.pad = 0;
        picks[r] = out;
    }
}

// one workgroup per sequence: the tree goes to LDS, one thread walks it -- emit the pick of `cur`, move to the lowest live child
// that carries that token -- and moves the state exactly as spec_accept_kernel does
__global__ __launch_bounds__(64) void spec_tree_accept_kernel(const SpecPick *__restrict__ picks, int n, const int32_t *__restrict__ node_ids,
                                                              const int32_t *__restrict__ parent, const u64 *__restrict__ anc, int32_t *history,
                                                              int hstride, int32_t *history_len, int happend, int32_t *seq_len,
                                                              uint8_t *finished, int32_t *__restrict__ out_tokens,
                                                              int32_t *__restrict__ out_count, float *__restrict__ out_logprob,
                                                              int32_t *__restrict__ out_path, int32_t *last_token, int32_t *cached_len,
                                                              int32_t *step_rows) {
    __shared__ int32_t par[kTreeMax], ids[kTreeMax];
    const int b = blockIdx.x, tid = threadIdx.x;
    const size_t base = static_cast<size_t>(b) * n;
    if (tid < n) {
        const bool live = tid >= 1 && (anc[base + tid] & 1ull);
        par[tid] = live ? parent[base + tid] : -1;   // (a dead node is nobody's child)
        ids[tid] = node_ids[base + tid];
    }
    __syncthreads();
    if (tid != 0) return;
    int32_t *tok = out_tokens + base;
    float *lp = out_logprob ? out_logprob + base : nullptr;
    int32_t *pth = out_path ? out_path + base : nullptr;
    int count = 0;
    if (!finished[b]) {
        const SpecPick *p = picks + base;
        int hl = (happend && hstride > 0) ? history_len[b] : -1;
        int fin = 0, cur = 0;
        while (count < n) {
            const SpecPick c = p[cur];
            tok[count] = c.token;
            if (lp) lp[count] = c.logprob;
            if (pth) pth[count] = cur;
            ++count;
            if (hl >= 0 && hl < hstride) history[static_cast<size_t>(b) * hstride + hl++] = c.token;
            fin = c.fin;
            if (fin) break;
            int next = -1;
            for (int j = cur + 1; j < n; ++j)
                if (par[j] == cur && ids[j] == c.token) {
                    next = j;
                    break;
                }
            if (next < 0) break;
            cur = next;
        }
        seq_len[b] += count;
        finished[b] = static_cast<uint8_t>(fin);
        if (happend && hstride > 0 && hl >= 0) history_len[b] = hl;
        if (last_token) last_token[b] = tok[count - 1];
        if (cached_len) cached_len[b] += count;
        if (step_rows) step_rows[b] += count;
    }
    for (int i = count; i < n; ++i) {
        tok[i] = -1;
        if (lp) lp[i] = -INFINITY;
        if (pth) pth[i] = -1;
    }
    out_count[b] = count;
}

// ---------------------------------------------------------------------------------------------- llmie_spec_verify_sampled
typedef unsigned __int128 u128;

struct SpecSampledRec {   // workspace record of a row
    int32_t token;        // the sampler's own pick of the row (lane 0), its raw log-probability and finish flag
    float logprob;
    int32_t fin;
    int32_t accept;       // bit 0: the draft is accepted; bit 1: the draft finishes the sequence
    float draft_logprob;
    int32_t res_token;    // what a rejection emits: the residual draw (the pick when SR == 0)
    float res_logprob;
    int32_t res_fin;
};

__device__ __forceinline__ u128 sp_shfl_up128(u128 v, int o) {
    const u64 lo = __shfl_up(static_cast<u64>(v), o), hi = __shfl_up(static_cast<u64>(v >> 64), o);
    return (static_cast<u128>(hi) << 64) | lo;
}
// exclusive prefix of a 128-bit integer over the block (thread order) and the block's total; the wave totals go through
// SpShared::hist
__device__ __forceinline__ u128 sp_excl_scan128(u128 v, u128 *total, SpShared &s) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    u128 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u128 y = sp_shfl_up128(inc, o);
        if (lane >= o) inc += y;
    }
    __syncthreads();
    if (lane == 63) {
        s.hist[2 * w] = static_cast<u64>(inc);
        s.hist[2 * w + 1] = static_cast<u64>(inc >> 64);
    }
    __syncthreads();
    u128 before = 0, all = 0;
    for (int i = 0; i < kSpWaves; ++i) {
        const u128 t = (static_cast<u128>(s.hist[2 * i + 1]) << 64) | s.hist[2 * i];
        if (i < w) before += t;
        all += t;
    }
    *total = all;
    return before + inc - v;
}

// the mass of token t under a prepared row (its keys, its kept set): 0 for a token not kept; the point mass is 1 on the pick
__device__ __forceinline__ u64 sp_mass_at(const uint32_t *keys, const SpRow &row, int t) {
    if (row.kept.point) return (row.pick.valid > 0 && t == row.pick.chosen) ? 1ull : 0ull;
    const uint32_t key = keys[t];
    return (key && row.kept.kept(t, key)) ? row.kept.mass(key) : 0ull;
}

// One 1024-thread workgroup per (sequence b, position i), r = b * (k + 1) + i.  The target row is prepared in key row 2r of the
// workspace (the sampler's first half: kept set P and its mass S_P) and its plain pick drawn (lane 0); for i < draft_len the
// draft row is prepared in key row 2r + 1 on the same history view (Q, S_Q), and the joint passes follow: the accept comparison
// on (P_d, Q_d, S_P, S_Q) and, behind a rejection, the residual R_v = max(0, P_v S_Q - Q_v S_P) -- every thread sums a contiguous
// chunk of ids, a block scan orders the chunks, and the one thread whose chunk holds thr walks it: the first id, ascending, at
// which the running sum exceeds thr.  All sums are 128-bit integers: exact in any order.  No state is written.
template <typename T, bool EXT>
__global__ __launch_bounds__(kSpThreads) void spec_sampled_rows_kernel(
    const T *__restrict__ logits, const T *__restrict__ draft_logits, int V, int k, const llmie_sampling_params *__restrict__ params,
    const llmie_sampling_params *__restrict__ draft_params, const int32_t *__restrict__ history, int hstride,
    const int32_t *__restrict__ history_len, int happend, const int32_t *__restrict__ draft_ids, const int32_t *__restrict__ draft_len,
    const int32_t *__restrict__ step_rows, int step_arg, const int32_t *step_dev, int end_id, uint32_t *ws, size_t ws_row,
    SpecSampledRec *__restrict__ recs, const llmie_sampling_ext ext) {
    __shared__ alignas(16) SpShared s;
    const int r = blockIdx.x;
    const auto [b, i, step, hist] = spec_row_view(r, k, history, hstride, history_len, happend, draft_ids, step_rows, step_arg, step_dev);
    const T *lg = logits + static_cast<size_t>(r) * V;
    uint32_t *keys_p = ws + static_cast<size_t>(2 * r) * ws_row, *keys_q = keys_p + ws_row;
    const llmie_sampling_params p = params[b];
    const SpRow P = sp_prepare_row<T, EXT>(lg, V, p, hist, step, end_id, keys_p, EXT ? &ext : nullptr, b, r, s);
    int plain = P.pick.chosen;
    if (!P.kept.point) {
        const int id = sp_draw_row(keys_p, V, P.kept, uniform_philox(static_cast<uint32_t>(step), p.seed), s);
        if (id >= 0) plain = id;
    }
    const float lse = P.pick.lse_m + logf(P.pick.lse_s);
    auto logprob = [&](int t) { return sp_logprob(lg, V, P.pick, lse, t); };
    auto finishes = [&](int t) { return sp_finishes<EXT>(P.pick, t, end_id) ? 1 : 0; };

    const int m = draft_len ? min(max(draft_len[b], 0), k) : k;
    bool accept = false;
    int d = -1, res = plain;
    if (i < m) {   // (uniform over the workgroup)
        __syncthreads();   // the draw is done with SpShared
        const T *dlg = draft_logits + (static_cast<size_t>(b) * k + i) * V;
        const SpRow Q = sp_prepare_row<T, false>(dlg, V, draft_params[b], hist, step, end_id, keys_q, nullptr, b, r, s);
        __syncthreads();   // both key rows are complete
        const u64 sp = P.kept.point ? (P.pick.valid > 0 ? 1ull : 0ull) : P.kept.total;
        const u64 sq = Q.kept.point ? (Q.pick.valid > 0 ? 1ull : 0ull) : Q.kept.total;
        d = draft_ids[static_cast<size_t>(b) * k + i];
        if (d >= 0 && d < V) {
            const u64 pd = sp_mass_at(keys_p, P, d), qd = sp_mass_at(keys_q, Q, d);
            const u64 u1 = philox_u24(static_cast<uint32_t>(step), p.seed, 1u) - 1u;
            // (U1 - 1) Q_d S_P < 2^24 P_d S_Q: below 2^24 * 2^32 * 2^51 on either side (vocab <= 2^19)
            accept = static_cast<u128>(u1 * qd) * sp < ((static_cast<u128>(pd) * sq) << 24);
        }
        if (!accept && sp != 0 && sq != 0) {
            const int chunk = (V + kSpThreads - 1) / kSpThreads;
            const int t0 = min(V, static_cast<int>(threadIdx.x) * chunk), t1 = min(V, t0 + chunk);
            auto residual = [&](int t) -> u128 {
                const u64 pv = sp_mass_at(keys_p, P, t);
                if (pv == 0) return 0;
                const u128 a = static_cast<u128>(pv) * sq, c = static_cast<u128>(sp_mass_at(keys_q, Q, t)) * sp;
                return a > c ? a - c : static_cast<u128>(0);
            };
            u128 mine = 0, sr;
            for (int t = t0; t < t1; ++t) mine += residual(t);
            if (threadIdx.x == 0) s.b_id = -1;
            const u128 ex = sp_excl_scan128(mine, &sr, s);   // (its barriers order the store above)
            if (sr != 0) {
                const u128 thr = (static_cast<u128>(philox_u24(static_cast<uint32_t>(step), p.seed, 2u) - 1u) * sr) >> 24;
                if (thr >= ex && thr < ex + mine) {
                    u128 run = ex;
                    for (int t = t0; t < t1; ++t) {
                        run += residual(t);
                        if (run > thr) {
                            s.b_id = t;
                            break;
                        }
                    }
                }
            }
            __syncthreads();
            if (s.b_id >= 0) res = s.b_id;
        }
    }
    if (threadIdx.x == 0) {
        SpecSampledRec out;
        out.token = plain;
        out.logprob = logprob(plain);
        out.fin = finishes(plain);
        out.accept = accept ? (1 | (finishes(d) << 1)) : 0;
        out.draft_logprob = accept ? logprob(d) : -INFINITY;
        out.res_token = res;
        out.res_logprob = logprob(res);
        out.res_fin = finishes(res);
        recs[r] = out;
    }
}

// one workgroup (one working thread) per sequence
__global__ __launch_bounds__(64) void spec_sampled_accept_kernel(const SpecSampledRec *__restrict__ recs, int k, const int32_t *__restrict__ draft_ids,
                                                                 const int32_t *__restrict__ draft_len, int32_t *history, int hstride,
                                                                 int32_t *history_len, int happend, int32_t *seq_len, uint8_t *finished,
                                                                 int32_t *__restrict__ out_tokens, int32_t *__restrict__ out_count,
                                                                 float *__restrict__ out_logprob, int32_t *__restrict__ out_accepted,
                                                                 int32_t *last_token, int32_t *cached_len, int32_t *step_rows) {
    if (threadIdx.x != 0) return;
    const int b = blockIdx.x, n = k + 1;
    int32_t *tok = out_tokens + static_cast<size_t>(b) * n;
    float *lp = out_logprob ? out_logprob + static_cast<size_t>(b) * n : nullptr;
    int count = 0, accepted = 0;
    if (!finished[b]) {
        const int dl = draft_len ? min(max(draft_len[b], 0), k) : k;
        const SpecSampledRec *p = recs + static_cast<size_t>(b) * n;
        const int32_t *draft = draft_ids + static_cast<size_t>(b) * k;
        int hl = (happend && hstride > 0) ? history_len[b] : -1;
        int fin = 0;
        for (int i = 0; i < n; ++i) {
            const SpecSampledRec c = p[i];
            const bool acc = i < dl && (c.accept & 1);
            const int32_t t = acc ? draft[i] : (i < dl ? c.res_token : c.token);
            tok[i] = t;
            if (lp) lp[i] = acc ? c.draft_logprob : (i < dl ? c.res_logprob : c.logprob);
            fin = acc ? (c.accept >> 1) : (i < dl ? c.res_fin : c.fin);
            ++count;
            accepted += acc ? 1 : 0;
            if (hl >= 0 && hl < hstride) history[static_cast<size_t>(b) * hstride + hl++] = t;
            if (!acc || fin) break;
        }
        seq_len[b] += count;
        finished[b] = static_cast<uint8_t>(fin);
        if (happend && hstride > 0 && hl >= 0) history_len[b] = hl;
        if (last_token) last_token[b] = tok[count - 1];
        if (cached_len) cached_len[b] += count;
        if (step_rows) step_rows[b] += count;
    }
    for (int i = count; i < n; ++i) {
        tok[i] = -1;
        if (lp) lp[i] = -INFINITY;
    }
    out_count[b] = count;
    if (out_accepted) out_accepted[b] = accepted;
}

constexpr int kSpecSampledMaxVocab = 1 << 19;   // S_P, S_Q < 2^51: the rule's products stay inside 128 bits

constexpr int kNgThreads = 256;
constexpr int kNgMaxN = 8;

__global__ __launch_bounds__(kNgThreads) void ngram_draft_kernel(const int32_t *__restrict__ tokens, int stride, const int32_t *__restrict__ len,
                                                                 const uint8_t *__restrict__ finished, int k, int max_n, int min_n, int pad_id,
                                                                 int32_t *__restrict__ out_ids, int32_t *__restrict__ out_draft_ids,
                                                                 int32_t *__restrict__ out_draft_len) {
    __shared__ int32_t suffix[kNgMaxN];                 // suffix[j] = tokens[L - 1 - j]
    __shared__ int best_any[kNgMaxN], best_full[kNgMaxN];   // per n - 1: the largest END p + n of a match / of one with k tokens behind it
    const int b = blockIdx.x, tid = threadIdx.x;
    const int32_t *row = tokens + static_cast<size_t>(b) * stride;
    const int L = min(max(len[b], 0), stride);
    const bool active = !(finished && finished[b]) && L >= min_n + 1;
    if (tid < kNgMaxN) {
        best_any[tid] = -1;
        best_full[tid] = -1;
        if (tid < L) suffix[tid] = row[L - 1 - tid];
    }
    __syncthreads();
    int m = 0, from = 0;   // the drafts are row[from .. from + m)
    if (active) {          // (uniform over the workgroup)
        const int nmax = min(max_n, L - 1);
        // (this sweep has a second copy, ngram_sweep below, for llmie_ngram_draft_tree: a change to the rule goes into both.  The copy
        // exists because calling the function from here moved this kernel's registers and instructions)
        int any[kNgMaxN], full[kNgMaxN];
#pragma unroll
        for (int j = 0; j < kNgMaxN; ++j) any[j] = full[j] = -1;
        const int32_t last = suffix[0];
        // q: where a candidate's final token sits, 0 <= q <= L - 2 (its continuation starts at e = q + 1 <= L - 1)
        auto visit = [&](int q, int32_t t) {
            if (t != last) return;
            int c = 1;   // tokens[q - c + 1 .. q] == the final c tokens
            while (c < nmax && q - c >= 0 && row[q - c] == suffix[c]) ++c;
            const int e = q + 1;
#pragma unroll
            for (int j = 0; j < kNgMaxN; ++j)
                if (c > j) {
                    any[j] = max(any[j], e);
                    if (e + k <= L) full[j] = max(full[j], e);
                }
        };
        const int quads = (reinterpret_cast<uintptr_t>(row) % 16 == 0) ? (L - 1) >> 2 : 0;
        for (int g = tid; g < quads; g += kNgThreads) {
            const int4 v = reinterpret_cast<const int4 *>(row)[g];
            visit(4 * g, v.x);
            visit(4 * g + 1, v.y);
            visit(4 * g + 2, v.z);
            visit(4 * g + 3, v.w);
        }
        for (int q = 4 * quads + tid; q < L - 1; q += kNgThreads) visit(q, row[q]);
#pragma unroll
        for (int j = 0; j < kNgMaxN; ++j) {
            if (any[j] >= 0) atomicMax(&best_any[j], any[j]);
            if (full[j] >= 0) atomicMax(&best_full[j], full[j]);
        }
        __syncthreads();
        for (int n = nmax; n >= min_n; --n)
            if (best_any[n - 1] >= 0) {   // the longest n with a match wins
                from = best_full[n - 1] >= 0 ? best_full[n - 1] : best_any[n - 1];
                m = min(k, L - from);
                break;
            }
    }
    if (tid <= k) out_ids[static_cast<size_t>(b) * (k + 1) + tid] = tid == 0 ? (L > 0 ? row[L - 1] : pad_id) : (tid - 1 < m ? row[from + tid - 1] : pad_id);
    if (tid < k) out_draft_ids[static_cast<size_t>(b) * k + tid] = tid < m ? row[from + tid] : pad_id;
    if (tid == 0) out_draft_len[b] = m;
}

static_assert(LLMIE_SPEC_MAX_DRAFT + 1 <= kNgThreads, "one thread per slot of the chunk");

// ngram_draft_kernel's sweep as a function, for the tree drafter (the kernel above keeps its own copy: its code stays as it was), by
// every thread of the workgroup: for every n <= nmax at once, the largest END of a match of the row's
// final n tokens (best_any[n - 1]) and of one with k tokens behind it (best_full[n - 1]); -1: none.  suffix[j] = row[L - 1 - j].
__device__ __forceinline__ void ngram_sweep(const int32_t *__restrict__ row, int L, int k, int nmax, const int32_t *suffix, int *best_any,
                                            int *best_full, int tid) {
    int any[kNgMaxN], full[kNgMaxN];
#pragma unroll
    for (int j = 0; j < kNgMaxN; ++j) any[j] = full[j] = -1;
    const int32_t last = suffix[0];
    // q: where a candidate's final token sits, 0 <= q <= L - 2 (its continuation starts at e = q + 1 <= L - 1)
    auto visit = [&](int q, int32_t t) {
        if (t != last) return;
        int c = 1;   // tokens[q - c + 1 .. q] == the final c tokens
        while (c < nmax && q - c >= 0 && row[q - c] == suffix[c]) ++c;
        const int e = q + 1;
#pragma unroll
        for (int j = 0; j < kNgMaxN; ++j)
            if (c > j) {
                any[j] = max(any[j], e);
                if (e + k <= L) full[j] = max(full[j], e);
            }
    };
    const int quads = (reinterpret_cast<uintptr_t>(row) % 16 == 0) ? (L - 1) >> 2 : 0;
    for (int g = tid; g < quads; g += kNgThreads) {
        const int4 v = reinterpret_cast<const int4 *>(row)[g];
        visit(4 * g, v.x);
        visit(4 * g + 1, v.y);
        visit(4 * g + 2, v.z);
        visit(4 * g + 3, v.w);
    }
    for (int q = 4 * quads + tid; q < L - 1; q += kNgThreads) visit(q, row[q]);
#pragma unroll
    for (int j = 0; j < kNgMaxN; ++j) {
        if (any[j] >= 0) atomicMax(&best_any[j], any[j]);
        if (full[j] >= 0) atomicMax(&best_full[j], full[j]);
    }
    __syncthreads();
}

// llmie_ngram_draft_tree: the same sweep; then every n' from nmax down to min_n that has a match contributes the continuation
// llmie_ngram_draft would choose with max_n = n' -- the first `branches` distinct starts -- and one thread merges them into a trie in
// that order (node order = creation order, so parent < child)
constexpr int kNgMaxBranches = 8;
__global__ __launch_bounds__(kNgThreads) void ngram_draft_tree_kernel(const int32_t *__restrict__ tokens, int stride, const int32_t *__restrict__ len,
                                                                      const uint8_t *__restrict__ finished, int n, int k, int branches, int max_n,
                                                                      int min_n, int pad_id, int32_t *__restrict__ out_ids,
                                                                      int32_t *__restrict__ out_parent, int32_t *__restrict__ out_node_count) {
    __shared__ int32_t suffix[kNgMaxN];
    __shared__ int best_any[kNgMaxN], best_full[kNgMaxN];
    __shared__ int32_t ids[kTreeMax], par[kTreeMax];
    __shared__ int cnt_s;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int32_t *row = tokens + static_cast<size_t>(b) * stride;
    const int L = min(max(len[b], 0), stride);
    const bool active = !(finished && finished[b]) && L >= min_n + 1;
    if (tid < kNgMaxN) {
        best_any[tid] = -1;
        best_full[tid] = -1;
        if (tid < L) suffix[tid] = row[L - 1 - tid];
    }
    __syncthreads();
    const int nmax = min(max_n, L - 1);
    if (active) ngram_sweep(row, L, k, nmax, suffix, best_any, best_full, tid);   // (uniform over the workgroup)
    if (tid == 0) {
        int cnt = 1;
        ids[0] = L > 0 ? row[L - 1] : pad_id;
        par[0] = -1;
        if (active) {
            int starts[kNgMaxBranches], ns = 0;
            for (int m = nmax; m >= min_n && ns < branches; --m) {
                if (best_any[m - 1] < 0) continue;
                const int from = best_full[m - 1] >= 0 ? best_full[m - 1] : best_any[m - 1];
                bool seen = false;
                for (int j = 0; j < ns; ++j) seen |= starts[j] == from;
                if (seen) continue;
                starts[ns++] = from;
                int cur = 0;
                for (int t = 0, e = min(k, L - from); t < e; ++t) {
                    const int32_t tok = row[from + t];
                    int child = -1;
                    for (int c = cur + 1; c < cnt; ++c)
                        if (par[c] == cur && ids[c] == tok) {
                            child = c;
                            break;
                        }
                    if (child < 0) {
                        if (cnt >= n) break;   // the budget ends: the candidate is cut here
                        ids[cnt] = tok, par[cnt] = cur, child = cnt++;
                    }
                    cur = child;
                }
            }
        }
        cnt_s = cnt;
    }
    __syncthreads();
    if (tid < n) {
        out_ids[static_cast<size_t>(b) * n + tid] = tid < cnt_s ? ids[tid] : pad_id;
        out_parent[static_cast<size_t>(b) * n + tid] = tid < cnt_s ? par[tid] : -1;
    }
    if (tid == 0) out_node_count[b] = cnt_s;
}


// the draft of a verify call: draft_ids [batch, k], draft_len [batch] or null (= k); sampled: the drafter SAMPLED them from
// draft_logits [batch, k, vocab] under draft_params (llmie_spec_verify_sampled), else both are unused
// a tree (llmie_spec_verify_tree): draft_ids is node_ids [batch, k + 1], draft_len unused, and tree_parent / tree_depth / tree_anc
// [batch, k + 1] are what llmie_spec_tree_prepare left; k + 1 = n node slots, so k may be 0
struct SpecDraft {
    bool sampled;
    const int32_t *draft_ids, *draft_len;
    int k;
    const void *draft_logits;
    const llmie_sampling_params *draft_params;
    bool tree = false;
    const int32_t *tree_parent = nullptr, *tree_depth = nullptr;
    const u64 *tree_anc = nullptr;
};
struct SpecOut {
    int32_t *out_tokens, *out_count, *out_accepted;
    float *out_logprob;
    int32_t *last_token, *cached_len;
    int32_t *out_path = nullptr;   // tree: [batch, n], the node of every emitted token (nullable)
};

// the workspace: 1 (2: sampled) key rows per position, then one record per position
size_t spec_records_offset(bool sampled, int rows, int vocab) { return (sampled ? 2 : 1) * static_cast<size_t>(rows) * sample_logits_ws_row(vocab) * sizeof(uint32_t); }
size_t spec_workspace_bytes(bool sampled, int batch, int k, int vocab) {
    if (batch <= 0 || k <= 0 || vocab <= 0 || k > LLMIE_SPEC_MAX_DRAFT || (sampled && vocab > kSpecSampledMaxVocab)) return 0;
    const int rows = batch * (k + 1);
    return spec_records_offset(sampled, rows, vocab) + static_cast<size_t>(rows) * (sampled ? sizeof(SpecSampledRec) : sizeof(SpecPick));
}
size_t spec_tree_workspace_bytes(int batch, int n, int vocab) {   // one key row and one SpecPick per node slot
    if (batch <= 0 || n <= 0 || vocab <= 0 || n > kTreeMax) return 0;
    const int rows = batch * n;
    return spec_records_offset(false, rows, vocab) + static_cast<size_t>(rows) * sizeof(SpecPick);
}

// step_rows: the per-sequence steps (wins over pos) or null
int spec_verify_impl(const SampleRows &r, const SpecDraft &d, const SampleState &s, const SamplePos &pos, int32_t *step_rows, const SpecOut &o,
                     SampleWs ws, const llmie_sampling_ext *ext, hipStream_t st) {
    const char *name = d.tree ? "spec_verify_tree" : (d.sampled ? "spec_verify_sampled" : "spec_verify");
    const int k = d.k;
    // the sampler's own checks, under this entry's name
    int rc = sample_logits_check(name, r, s, o.out_tokens);
    if (rc != LLMIE_OK) return rc;
    bool active;
    if ((rc = sample_ext_check(r.batch, r.vocab, ext, &active, name)) != LLMIE_OK) return rc;
    if (d.tree) {
        LLMIE_REQUIRE(k + 1 >= 1, "%s: n %d < 1", name, k + 1);
        LLMIE_REQUIRE(d.draft_ids && o.out_tokens && o.out_count, "%s: NULL node_ids / out_tokens / out_count", name);
        LLMIE_REQUIRE(d.tree_parent && d.tree_depth && d.tree_anc, "%s: NULL parent / depth / anc", name);
        if (k + 1 > kTreeMax) LLMIE_UNSUPPORTED("%s: n %d above LLMIE_SPEC_TREE_MAX_NODES (%d)", name, k + 1, kTreeMax);
    } else {
        LLMIE_REQUIRE(k >= 1, "%s: k %d < 1", name, k);
        LLMIE_REQUIRE(d.draft_ids && o.out_tokens && o.out_count, "%s: NULL draft_ids / out_tokens / out_count", name);
        if (d.sampled) LLMIE_REQUIRE(d.draft_logits && d.draft_params, "%s: NULL draft_logits / draft_params_dev", name);
        if (k > LLMIE_SPEC_MAX_DRAFT) LLMIE_UNSUPPORTED("%s: k %d above LLMIE_SPEC_MAX_DRAFT (%d)", name, k, LLMIE_SPEC_MAX_DRAFT);
    }
    if (d.sampled && r.vocab > kSpecSampledMaxVocab) LLMIE_UNSUPPORTED("%s: vocab %d above %d", name, r.vocab, kSpecSampledMaxVocab);
    const long long positions = static_cast<long long>(r.batch) * (k + 1);   // (sampled: two key rows each)
    LLMIE_REQUIRE(positions <= INT_MAX / (d.sampled ? 2 : 1), "%s: batch * (k + 1) = %lld rows", name, positions);
    rc = sample_workspace_check(name, ws, d.tree ? spec_tree_workspace_bytes(r.batch, k + 1, r.vocab) : spec_workspace_bytes(d.sampled, r.batch, k, r.vocab),
                                d.tree ? "llmie_spec_verify_tree_workspace_bytes"
                                       : (d.sampled ? "llmie_spec_verify_sampled_workspace_bytes" : "llmie_spec_verify_workspace_bytes"));
    if (rc != LLMIE_OK) return rc;
    const int rows = static_cast<int>(positions);
    uint32_t *keys = static_cast<uint32_t *>(ws.p);
    void *records = static_cast<unsigned char *>(ws.p) + spec_records_offset(d.sampled, rows, r.vocab);
    const size_t ws_row = sample_logits_ws_row(r.vocab);
    const llmie_sampling_ext none = {};
    const llmie_sampling_ext &e = active ? *ext : none;
    sample_dispatch(r.dtype, active, [&](auto type, auto with_ext) {
        using T = typename decltype(type)::type;
        constexpr bool EXT = decltype(with_ext)::value;
        const T *lg = static_cast<const T *>(r.logits);
        if (d.tree)
            spec_tree_rows_kernel<T, EXT><<<rows, kSpThreads, 0, st>>>(lg, r.vocab, k + 1, r.params, s.history, s.history_stride, s.history_len,
                                                                      s.history_append, d.draft_ids, d.tree_depth, d.tree_anc, step_rows, pos.step,
                                                                      pos.step_dev, r.end_id, keys, ws_row, static_cast<SpecPick *>(records), e);
        else if (d.sampled)
            spec_sampled_rows_kernel<T, EXT><<<rows, kSpThreads, 0, st>>>(
                lg, static_cast<const T *>(d.draft_logits), r.vocab, k, r.params, d.draft_params, s.history, s.history_stride, s.history_len,
                s.history_append, d.draft_ids, d.draft_len, step_rows, pos.step, pos.step_dev, r.end_id, keys, ws_row,
                static_cast<SpecSampledRec *>(records), e);
        else
            spec_verify_rows_kernel<T, EXT><<<rows, kSpThreads, 0, st>>>(lg, r.vocab, k, r.params, s.history, s.history_stride, s.history_len,
                                                                        s.history_append, d.draft_ids, step_rows, pos.step, pos.step_dev, r.end_id,
                                                                        keys, ws_row, static_cast<SpecPick *>(records), e);
    });
    if ((rc = launch_status(d.tree ? "spec_verify_tree(rows)" : (d.sampled ? "spec_verify_sampled(rows)" : "spec_verify(rows)"))) != LLMIE_OK) return rc;
    if (d.tree) {
        spec_tree_accept_kernel<<<r.batch, 64, 0, st>>>(static_cast<const SpecPick *>(records), k + 1, d.draft_ids, d.tree_parent, d.tree_anc, s.history,
                                                        s.history_stride, s.history_len, s.history_append, s.seq_len, s.finished, o.out_tokens,
                                                        o.out_count, o.out_logprob, o.out_path, o.last_token, o.cached_len, step_rows);
        return launch_status("spec_verify_tree(accept)");
    }
    if (d.sampled)
        spec_sampled_accept_kernel<<<r.batch, 64, 0, st>>>(static_cast<const SpecSampledRec *>(records), k, d.draft_ids, d.draft_len, s.history,
                                                           s.history_stride, s.history_len, s.history_append, s.seq_len, s.finished, o.out_tokens,
                                                           o.out_count, o.out_logprob, o.out_accepted, o.last_token, o.cached_len, step_rows);
    else
        spec_accept_kernel<<<r.batch, 64, 0, st>>>(static_cast<const SpecPick *>(records), k, d.draft_ids, d.draft_len, s.history, s.history_stride,
                                                   s.history_len, s.history_append, s.seq_len, s.finished, o.out_tokens, o.out_count, o.out_logprob,
                                                   o.last_token, o.cached_len, step_rows);
    return launch_status(d.sampled ? "spec_verify_sampled(accept)" : "spec_verify(accept)");
}

}  // namespace
}  // namespace llmie

using namespace llmie;

extern "C" size_t llmie_spec_verify_workspace_bytes(int batch, int k, int vocab) { return spec_workspace_bytes(false, batch, k, vocab); }
extern "C" size_t llmie_spec_verify_sampled_workspace_bytes(int batch, int k, int vocab) { return spec_workspace_bytes(true, batch, k, vocab); }

extern "C" int llmie_spec_verify(const void *logits, int batch, int k, int vocab, const int32_t *draft_ids, const int32_t *draft_len,
                                 const llmie_sampling_params *params_dev, int32_t *history, int history_stride, int32_t *history_len,
                                 int history_append, int32_t *seq_len, uint8_t *finished, int32_t *out_tokens, int32_t *out_count,
                                 float *out_logprob, int32_t *last_token, int32_t *cached_len, int32_t *step_rows, int step,
                                 const int32_t *step_dev, int end_id, void *workspace, size_t workspace_bytes, llmie_dtype dtype,
                                 llmie_stream stream, const llmie_sampling_ext *ext) {
    return spec_verify_impl(SampleRows{logits, batch, vocab, dtype, params_dev, end_id}, SpecDraft{false, draft_ids, draft_len, k, nullptr, nullptr},
                            SampleState{history, history_stride, history_len, history_append, seq_len, finished}, SamplePos{step, step_dev},
                            step_rows, SpecOut{out_tokens, out_count, nullptr, out_logprob, last_token, cached_len},
                            SampleWs{workspace, workspace_bytes}, ext, as_stream(stream));
}

extern "C" int llmie_spec_verify_sampled(const void *logits, const void *draft_logits, int batch, int k, int vocab, const int32_t *draft_ids,
                                         const int32_t *draft_len, const llmie_sampling_params *params_dev,
                                         const llmie_sampling_params *draft_params_dev, int32_t *history, int history_stride,
                                         int32_t *history_len, int history_append, int32_t *seq_len, uint8_t *finished, int32_t *out_tokens,
                                         int32_t *out_count, int32_t *out_accepted, float *out_logprob, int32_t *last_token, int32_t *cached_len,
                                         int32_t *step_rows, int step, const int32_t *step_dev, int end_id, void *workspace,
                                         size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream, const llmie_sampling_ext *ext) {
    return spec_verify_impl(SampleRows{logits, batch, vocab, dtype, params_dev, end_id},
                            SpecDraft{true, draft_ids, draft_len, k, draft_logits, draft_params_dev},
                            SampleState{history, history_stride, history_len, history_append, seq_len, finished}, SamplePos{step, step_dev},
                            step_rows, SpecOut{out_tokens, out_count, out_accepted, out_logprob, last_token, cached_len},
                            SampleWs{workspace, workspace_bytes}, ext, as_stream(stream));
}

extern "C" int llmie_ngram_draft(const int32_t *tokens, int stride, const int32_t *len, const uint8_t *finished, int batch, int k, int max_n,
                                 int min_n, int pad_id, int32_t *out_ids, int32_t *out_draft_ids, int32_t *out_draft_len,
                                 llmie_stream stream) {
    LLMIE_REQUIRE(tokens && len && out_ids && out_draft_ids && out_draft_len, "ngram_draft: NULL pointer");
    LLMIE_REQUIRE(batch > 0 && stride > 0, "ngram_draft: batch %d / stride %d must be positive", batch, stride);
    LLMIE_REQUIRE(k >= 1, "ngram_draft: k %d < 1", k);
    LLMIE_REQUIRE(min_n >= 1 && min_n <= max_n, "ngram_draft: need 1 <= min_n %d <= max_n %d", min_n, max_n);
    if (k > LLMIE_SPEC_MAX_DRAFT) LLMIE_UNSUPPORTED("ngram_draft: k %d above LLMIE_SPEC_MAX_DRAFT (%d)", k, LLMIE_SPEC_MAX_DRAFT);
    if (max_n > kNgMaxN) LLMIE_UNSUPPORTED("ngram_draft: max_n %d above %d", max_n, kNgMaxN);
    ngram_draft_kernel<<<batch, kNgThreads, 0, as_stream(stream)>>>(tokens, stride, len, finished, k, max_n, min_n, pad_id, out_ids, out_draft_ids,
                                                                    out_draft_len);
    return launch_status("ngram_draft");
}

extern "C" int llmie_spec_tree_prepare(const int32_t *parent, const int32_t *node_count, int batch, int n, int32_t *depth_out, uint64_t *anc_out,
                                       llmie_stream stream) {
    LLMIE_REQUIRE(parent && depth_out && anc_out, "spec_tree_prepare: NULL parent / depth_out / anc_out");
    LLMIE_REQUIRE(batch > 0, "spec_tree_prepare: batch %d must be positive", batch);
    LLMIE_REQUIRE(n >= 1, "spec_tree_prepare: n %d < 1", n);
    if (n > kTreeMax) LLMIE_UNSUPPORTED("spec_tree_prepare: n %d above LLMIE_SPEC_TREE_MAX_NODES (%d)", n, kTreeMax);
    spec_tree_prepare_kernel<<<batch, 64, 0, as_stream(stream)>>>(parent, node_count, n, depth_out, reinterpret_cast<u64 *>(anc_out));
    return launch_status("spec_tree_prepare");
}

extern "C" size_t llmie_spec_verify_tree_workspace_bytes(int batch, int n, int vocab) { return spec_tree_workspace_bytes(batch, n, vocab); }

extern "C" int llmie_spec_verify_tree(const void *logits, int batch, int n, int vocab, const int32_t *node_ids, const int32_t *parent,
                                      const int32_t *depth, const uint64_t *anc, const llmie_sampling_params *params_dev, int32_t *history,
                                      int history_stride, int32_t *history_len, int history_append, int32_t *seq_len, uint8_t *finished,
                                      int32_t *out_tokens, int32_t *out_count, int32_t *out_path, float *out_logprob, int32_t *last_token,
                                      int32_t *cached_len, int32_t *step_rows, int step, const int32_t *step_dev, int end_id, void *workspace,
                                      size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream, const llmie_sampling_ext *ext) {
    SpecDraft d{false, node_ids, nullptr, n - 1, nullptr, nullptr};
    d.tree = true, d.tree_parent = parent, d.tree_depth = depth, d.tree_anc = reinterpret_cast<const u64 *>(anc);
    SpecOut o{out_tokens, out_count, nullptr, out_logprob, last_token, cached_len};
    o.out_path = out_path;
    return spec_verify_impl(SampleRows{logits, batch, vocab, dtype, params_dev, end_id}, d,
                            SampleState{history, history_stride, history_len, history_append, seq_len, finished}, SamplePos{step, step_dev},
                            step_rows, o, SampleWs{workspace, workspace_bytes}, ext, as_stream(stream));
}

extern "C" int llmie_ngram_draft_tree(const int32_t *tokens, int stride, const int32_t *len, const uint8_t *finished, int batch, int n, int k,
                                      int branches, int max_n, int min_n, int pad_id, int32_t *out_ids, int32_t *out_parent,
                                      int32_t *out_node_count, llmie_stream stream) {
    LLMIE_REQUIRE(tokens && len && out_ids && out_parent && out_node_count, "ngram_draft_tree: NULL pointer");
    LLMIE_REQUIRE(batch > 0 && stride > 0, "ngram_draft_tree: batch %d / stride %d must be positive", batch, stride);
    LLMIE_REQUIRE(n >= 1, "ngram_draft_tree: n %d < 1", n);
    LLMIE_REQUIRE(k >= 1, "ngram_draft_tree: k %d < 1", k);
    LLMIE_REQUIRE(branches >= 1, "ngram_draft_tree: branches %d < 1", branches);
    LLMIE_REQUIRE(min_n >= 1 && min_n <= max_n, "ngram_draft_tree: need 1 <= min_n %d <= max_n %d", min_n, max_n);
    if (n > kTreeMax) LLMIE_UNSUPPORTED("ngram_draft_tree: n %d above LLMIE_SPEC_TREE_MAX_NODES (%d)", n, kTreeMax);
    if (k > LLMIE_SPEC_MAX_DRAFT) LLMIE_UNSUPPORTED("ngram_draft_tree: k %d above LLMIE_SPEC_MAX_DRAFT (%d)", k, LLMIE_SPEC_MAX_DRAFT);
    if (branches > kNgMaxBranches) LLMIE_UNSUPPORTED("ngram_draft_tree: branches %d above %d", branches, kNgMaxBranches);
    if (max_n > kNgMaxN) LLMIE_UNSUPPORTED("ngram_draft_tree: max_n %d above %d", max_n, kNgMaxN);
    ngram_draft_tree_kernel<<<batch, kNgThreads, 0, as_stream(stream)>>>(tokens, stride, len, finished, n, k, branches, max_n, min_n, pad_id, out_ids,
                                                                         out_parent, out_node_count);
    return launch_status("ngram_draft_tree");
}
