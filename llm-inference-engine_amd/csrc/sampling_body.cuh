// The device code of the per-request sampler (llmie_sample_logits and its _ext form): one 1024-thread workgroup samples one row.
// sampling_params.hip wraps it into the sampler's kernels, spec_decode.hip into the verify kernel of speculative decoding; the
// file comment of sampling_params.hip describes the passes.
#pragma once
#include "device_utils.cuh"
#include "llmie_internal.h"
#include "philox.cuh"

#include <cfloat>
#include <climits>

namespace llmie {

constexpr int kSpThreads = 1024;
constexpr int kSpMaxHistory = LLMIE_SAMPLE_MAX_HISTORY;
constexpr int kSpWaves = kSpThreads / 64;
typedef unsigned long long u64;

__device__ __forceinline__ uint32_t sp_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sp_val(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

struct SpShared {
    u64 hist[256];
    u64 red64[kSpWaves];
    float redm[kSpWaves], reds[kSpWaves];
    int redi[kSpWaves];
    u64 b_above;
    uint32_t b_prefix;
    int b_id;
    int sorted[kSpMaxHistory];
};

// block-wide reductions (fixed mapping and order: deterministic)
__device__ __forceinline__ u64 sp_sum64(u64 v, SpShared &s) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if (lane == 0) s.red64[w] = v;
    __syncthreads();
    u64 t = 0;
#pragma unroll
    for (int i = 0; i < kSpWaves; ++i) t += s.red64[i];
    return t;
}
__device__ __forceinline__ u64 sp_max64(u64 v, SpShared &s) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 y = __shfl_xor(v, o);
        v = y > v ? y : v;
    }
    __syncthreads();
    if (lane == 0) s.red64[w] = v;
    __syncthreads();
    u64 t = 0;
#pragma unroll
    for (int i = 0; i < kSpWaves; ++i) t = s.red64[i] > t ? s.red64[i] : t;
    return t;
}
// exclusive prefix of an int over the block (thread order)
__device__ __forceinline__ int sp_excl_scan(int v, SpShared &s) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(inc, o);
        if (lane >= o) inc += y;
    }
    __syncthreads();
    if (lane == 63) s.redi[w] = inc;
    __syncthreads();
    int before = 0;
    for (int i = 0; i < w; ++i) before += s.redi[i];
    return before + inc - v;
}
// f(t, key) over this thread's tokens (stride kSpThreads), kSpUnroll loads in flight: one CU streams the whole row, so the
// passes are bound by load latency unless the loads of several tokens overlap.  Keys past V read as 0 (excluded).
constexpr int kSpUnroll = 8;
// RAW: `keys` still holds pass 1's fp32 copy of the raw row; its keys are formed on the fly (NaN -> 0, -0 -> +0: llmie_topk's ties)
template <bool RAW> __device__ __forceinline__ uint32_t sp_load_key(const uint32_t *keys, int t) {
    if constexpr (RAW) {
        const float x = __uint_as_float(keys[t]);
        return x == x ? sp_key(x + 0.f) : 0u;
    } else {
        return keys[t];
    }
}
template <bool RAW = false, class F> __device__ __forceinline__ void sp_for_keys(const uint32_t *keys, int V, F f) {
    for (int t0 = threadIdx.x; t0 < V; t0 += kSpUnroll * kSpThreads) {
        uint32_t k[kSpUnroll];
#pragma unroll
        for (int u = 0; u < kSpUnroll; ++u) {
            const int t = t0 + u * kSpThreads;
            k[u] = t < V ? sp_load_key<RAW>(keys, t) : 0u;
        }
#pragma unroll
        for (int u = 0; u < kSpUnroll; ++u) f(t0 + u * kSpThreads, k[u]);
    }
}
// (max, sum of exp(x - max)) pairs
__device__ __forceinline__ void sp_lse_combine(float &m, float &sum, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    if (mn == -INFINITY) return;
    sum = (m == -INFINITY ? 0.f : sum * expf(m - mn)) + (m2 == -INFINITY ? 0.f : s2 * expf(m2 - mn));
    m = mn;
}

// In (value desc, id asc) order over the tokens t with in(t, key) (key != 0), the first token at which the running weight
// w(key) exceeds thr.  The caller guarantees that the total weight exceeds thr.  Returns its key; *above = the weight of the
// set strictly above that key.  4 passes over the keys, one 8-bit digit each, highest first.
template <bool RAW = false, class In, class W>
__device__ uint32_t radix_select(const uint32_t *keys, int V, In in, W w, u64 thr, u64 *above_out, SpShared &s) {
    const int tid = threadIdx.x;
    uint32_t prefix = 0;
    u64 above = 0;
    for (int d = 3; d >= 0; --d) {
        const int shift = 8 * d;
        const uint32_t hmask = d == 3 ? 0u : (0xffffffffu << (shift + 8));
        if (tid < 256) s.hist[tid] = 0;
        __syncthreads();
        sp_for_keys<RAW>(keys, V, [&](int t, uint32_t k) {
            if (k == 0 || (k & hmask) != prefix || !in(t, k)) return;
            const u64 wt = w(k);
            if (wt) atomicAdd(&s.hist[(k >> shift) & 255u], wt);
        });
        __syncthreads();
        if (tid < 64) {
            // lane l holds bins 255-4l .. 252-4l (descending value)
            const int base = 255 - 4 * tid;
            const u64 h0 = s.hist[base], h1 = s.hist[base - 1], h2 = s.hist[base - 2], h3 = s.hist[base - 3];
            const u64 sum = h0 + h1 + h2 + h3;
            u64 inc = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u64 y = __shfl_up(inc, o);
                if (tid >= o) inc += y;
            }
            const u64 hit = __ballot(above + inc > thr);
            const int first = hit ? __ffsll(static_cast<long long>(hit)) - 1 : 63;
            if (tid == first) {
                u64 c = above + inc - sum;
                int bin = base - 3;
                if (c + h0 > thr) bin = base;
                else if ((c += h0) + h1 > thr) bin = base - 1;
                else if ((c += h1) + h2 > thr) bin = base - 2;
                else c += h2;
                s.b_above = c;
                s.b_prefix = prefix | (static_cast<uint32_t>(bin) << shift);
            }
        }
        __syncthreads();
        prefix = s.b_prefix;
        above = s.b_above;
    }
    *above_out = above;
    return prefix;
}

// the j-th (0-based) id, ascending, among the tokens with keys[t] == key and in(t, key); -1 if there are not that many
template <bool RAW = false, class In>
__device__ int id_select(const uint32_t *keys, int V, uint32_t key, In in, u64 j, SpShared &s) {
    const int chunk = (V + kSpThreads - 1) / kSpThreads;
    const int t0 = min(V, threadIdx.x * chunk), t1 = min(V, t0 + chunk);
    int c = 0;
    for (int t = t0; t < t1; ++t) c += (sp_load_key<RAW>(keys, t) == key && in(t, key)) ? 1 : 0;
    if (threadIdx.x == 0) s.b_id = -1;
    const int ex = sp_excl_scan(c, s);   // (its barriers order the store above)
    if (j >= static_cast<u64>(ex) && j < static_cast<u64>(ex + c)) {
        int r = static_cast<int>(j - ex);
        for (int t = t0; t < t1; ++t)
            if (sp_load_key<RAW>(keys, t) == key && in(t, key) && r-- == 0) {
                s.b_id = t;
                break;
            }
    }
    __syncthreads();
    return s.b_id;
}

static_assert(LLMIE_SAMPLE_MAX_BIAS <= kSpThreads, "one thread per bias entry");
static_assert(LLMIE_SAMPLE_MAX_TOP_N <= 256, "the top-N candidates live in SpShared::hist");
static_assert(offsetof(SpShared, sorted) % 16 == 0, "the mask row is staged in `sorted` with 16-byte stores");

// EXT: the top_n largest raw logits of the row (value desc, id asc) and their raw log-softmax.  `keys` holds pass 1's fp32 copy,
// untouched so far; valid = its count of non-NaN values; lse = the raw log-sum-exp.
__device__ __forceinline__ void sp_top_n(const uint32_t *keys, int V, int valid, float lse, int top_n, int32_t *out_ids, float *out_lp, SpShared &s) {
    const int tid = threadIdx.x;
    const int n = min(top_n, valid);
    uint32_t kk = 0;   // the n-th token (kk, kid); kk == 0: every valid token is in
    int kid = INT_MAX;
    if (valid > top_n) {
        auto all = [](int, uint32_t) { return true; };
        u64 above;
        kk = radix_select<true>(keys, V, all, [](uint32_t) { return 1ull; }, static_cast<u64>(top_n - 1), &above, s);
        kid = id_select<true>(keys, V, kk, all, static_cast<u64>(top_n - 1) - above, s);
    }
    __syncthreads();   // every thread has read id_select's b_id
    if (tid == 0) s.b_id = 0;
    __syncthreads();
    sp_for_keys<true>(keys, V, [&](int t, uint32_t k) {
        if (k == 0 || !(k > kk || (k == kk && t <= kid))) return;
        const int slot = atomicAdd(&s.b_id, 1);   // (any order: the candidates rank themselves below)
        if (slot < LLMIE_SAMPLE_MAX_TOP_N) s.hist[slot] = (static_cast<u64>(k) << 32) | (0xffffffffu - static_cast<uint32_t>(t));
    });
    __syncthreads();
    if (tid < n) {
        const u64 mine = s.hist[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += s.hist[j] > mine ? 1 : 0;   // ids differ, so do the candidates
        out_ids[rank] = static_cast<int32_t>(0xffffffffu - static_cast<uint32_t>(mine & 0xffffffffu));
        out_lp[rank] = sp_val(static_cast<uint32_t>(mine >> 32)) - lse;
    } else if (tid < top_n) {
        out_ids[tid] = -1;
        out_lp[tid] = -INFINITY;
    }
    __syncthreads();   // hist / b_id are free again, and the copy may be patched
}

// Where a row's penalty history comes from.  SpStoredHistory: history[b, 0..history_len[b]) as it stands (the sampler's entries).
// length() is called once, behind pass 1; at(i) for i < length().
struct SpStoredHistory {
    const int32_t *history, *history_len;
    int b, hstride;
    __device__ __forceinline__ int length() const { return hstride > 0 ? min(max(history_len[b], 0), hstride) : 0; }
    __device__ __forceinline__ int at(int i) const { return history[static_cast<size_t>(b) * hstride + i]; }
};

// What sp_sample_row leaves for its caller's epilogue (the caller is a kernel: every field is per thread, block-uniform)
struct SpPick {
    int chosen, valid;
    float lse_m, lse_s;       // the raw row's log-sum-exp = lse_m + logf(lse_s)
    int slen;                 // (EXT) the row's stop list
    const int32_t *stops;
};

// A row's epilogue, shared by every kernel that emits a token of it.  Does `token` finish the sequence: end_id, or (EXT) a stop
template <bool EXT> __device__ __forceinline__ bool sp_finishes(const SpPick &pick, int token, int end_id) {
    bool fin = token == end_id;
    if constexpr (EXT)
        for (int i = 0; i < pick.slen; ++i) fin = fin || pick.stops[i] == token;
    return fin;
}
// and its raw log-probability.  lse = pick.lse_m + logf(pick.lse_s), computed by the caller: ONCE where it asks for several tokens
template <typename T> __device__ __forceinline__ float sp_logprob(const T *__restrict__ lg, int V, const SpPick &pick, float lse, int token) {
    return (token >= 0 && token < V && pick.valid > 0) ? to_f32(lg[token]) - lse : -INFINITY;
}

// The distribution a row is drawn from, over the row's keys: which tokens are kept and their fixed-point mass.  point: a greedy
// row or one with at most one valid token -- the point mass on the row's pick, no cuts, total unused.
struct SpKept {
    bool point;
    uint32_t kk, pk;   // the top-k cut is the token (kk, kid); the top-p cut keeps every key >= pk
    int kid;
    float min_p, vmax;
    u64 total;         // the mass of the kept set
    __device__ __forceinline__ u64 mass(uint32_t k) const {
        const float d = sp_val(k) - vmax;
        if (!(d > -23.f)) return 0ull;
        return static_cast<u64>(expf(d) * 4294967296.0f);
    }
    __device__ __forceinline__ bool in_k(int t, uint32_t k) const { return k > kk || (k == kk && t <= kid); }
    __device__ __forceinline__ bool kept(int t, uint32_t k) const {
        return in_k(t, k) && k >= pk && (min_p == 0.f || expf(sp_val(k) - vmax) >= min_p);
    }
};

// What sp_prepare_row leaves: SpPick with `chosen` the (key, id) maximum of the row (end_id without a valid token) -- the pick of
// a point-mass row -- and the kept set.
struct SpRow {
    SpPick pick;
    SpKept kept;
};

// The first half of the sampler's body for ONE row, run by the whole 1024-thread workgroup: steps 0a .. 6 of include/llmie.h on
// the logits `lg` -- everything up to the kept set and its mass -- with `keys` the row's workspace, which holds the row's keys
// afterwards.  b indexes the per-request operands (bias, stops, min_step, the mask row without a mask_index); r indexes
// mask_index and the top-N outputs (the sampler's entries: r == b).  ep: the extension (EXT) or null.
template <typename T, bool EXT, class History>
__device__ __forceinline__ SpRow sp_prepare_row(const T *__restrict__ lg, int V, const llmie_sampling_params p, const History hist, int step,
                                                int end_id, uint32_t *keys, const llmie_sampling_ext *ep, int b, int r, SpShared &s) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *rowf = reinterpret_cast<float *>(keys);

    // parameters, clamped (they live in device memory: the host cannot check them)
    float temp = p.temperature;
    if (!(temp >= 0.f)) temp = 0.f;
    int top_k = p.top_k < 0 ? 0 : (p.top_k > V ? V : p.top_k);
    float top_p = p.top_p;
    if (!(top_p > 0.f)) {   // <= 0 (or NaN): one token
        top_k = 1;
        top_p = 1.f;
    }
    top_p = fminf(top_p, 1.f);
    float min_p = p.min_p;
    min_p = (min_p >= 0.f) ? fminf(min_p, 1.f) : 0.f;
    float rep = p.repetition_penalty;
    if (!(rep > 0.f)) rep = 1.f;
    const float presence = p.presence_penalty, frequency = p.frequency_penalty;

    // pass 1: fp32 copy + raw log-sum-exp (per-thread online pairs, then a fixed tree)
    float m = -INFINITY, sum = 0.f;
    int nraw = 0;   // (EXT) non-NaN raw logits of this thread
    for (int t = tid; t < V; t += kSpThreads) {
        const float x = to_f32(lg[t]);
        rowf[t] = x;
        if (x == x) sp_lse_combine(m, sum, x, 1.f);
        if constexpr (EXT) nraw += x == x ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sp_lse_combine(m, sum, __shfl_xor(m, o), __shfl_xor(sum, o));
    if (lane == 0) {
        s.redm[wave] = m;
        s.reds[wave] = sum;
    }

    // (EXT) the stop list; the top-N of the raw row; then bias and min_step patch the copy in front of the penalties
    int slen = 0;
    const int32_t *stops = nullptr;
    if constexpr (EXT) {
        const llmie_sampling_ext &e = *ep;
        if (e.stop_ids) {
            slen = min(max(e.stop_len[b], 0), e.stop_stride);
            stops = e.stop_ids + static_cast<size_t>(b) * e.stop_stride;
        }
        if (e.top_n > 0) {
            const int rawvalid = static_cast<int>(sp_sum64(static_cast<u64>(nraw), s));   // (its barriers complete pass 1)
            float rm = s.redm[0], rs = s.reds[0];
            for (int i = 1; i < kSpWaves; ++i) sp_lse_combine(rm, rs, s.redm[i], s.reds[i]);
            sp_top_n(keys, V, rawvalid, rm + logf(rs), e.top_n, e.out_top_ids + static_cast<size_t>(r) * e.top_n,
                     e.out_top_logprobs + static_cast<size_t>(r) * e.top_n, s);
        } else {
            __syncthreads();   // pass 1's copy of the row is complete
        }
        const int blen = e.bias_ids ? min(max(e.bias_len[b], 0), e.bias_stride) : 0;
        if (blen > 0) {
            // entry tid of the list; -1: ignored.  It patches the row unless a later entry names the same id (last wins).
            int id = -1;
            float val = 0.f;
            if (tid < blen) {
                id = e.bias_ids[static_cast<size_t>(b) * e.bias_stride + tid];
                val = e.bias_vals[static_cast<size_t>(b) * e.bias_stride + tid];
                if (id < 0 || id >= V || val != val || val == INFINITY) id = -1;
            }
            s.sorted[tid] = id;
            __syncthreads();
            if (id >= 0) {
                bool last = true;
#pragma unroll 8
                for (int j = tid + 1; j < blen; ++j) last = last && s.sorted[j] != id;
                if (last) rowf[id] = val == -INFINITY ? __uint_as_float(0x7fc00000u) : rowf[id] + val;
            }
            __syncthreads();   // `sorted` is free for the history; the bias is in the row
        }
        if (e.min_step && step < e.min_step[b]) {
            // (the same NaN from several threads where ids repeat)
            if (tid < slen) {
                const int t = stops[tid];
                if (t >= 0 && t < V) rowf[t] = __uint_as_float(0x7fc00000u);
            }
            if (tid == LLMIE_SAMPLE_MAX_STOPS && end_id >= 0 && end_id < V) rowf[end_id] = __uint_as_float(0x7fc00000u);
        }
    }

    // penalties over the distinct ids of the history
    const int hlen = hist.length();
    const bool penal = hlen > 0 && (rep != 1.f || presence != 0.f || frequency != 0.f);
    if (penal) {
        int n = 1;
        while (n < hlen) n <<= 1;
        for (int i = tid; i < n; i += kSpThreads) {
            const int t = i < hlen ? hist.at(i) : -1;
            s.sorted[i] = (t >= 0 && t < V) ? t : INT_MAX;
        }
        __syncthreads();
        for (int k = 2; k <= n; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < n; i += kSpThreads) {
                    const int l = i ^ j;
                    if (l > i) {
                        const int a = s.sorted[i], c = s.sorted[l];
                        if ((a > c) == ((i & k) == 0)) {
                            s.sorted[i] = c;
                            s.sorted[l] = a;
                        }
                    }
                }
                __syncthreads();
            }
        __syncthreads();   // pass 1's copy of the row is complete
        for (int i = tid; i < n; i += kSpThreads) {
            const int t = s.sorted[i];
            if (t == INT_MAX || (i > 0 && s.sorted[i - 1] == t)) continue;
            int lo = i + 1, hi = n;   // first index past the run
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s.sorted[mid] == t) lo = mid + 1;
                else hi = mid;
            }
            const float c = static_cast<float>(lo - i);
            float x = rowf[t];
            x = x > 0.f ? x / rep : x * rep;
            x = x - presence;
            x = x - c * frequency;
            rowf[t] = x;
        }
    }
    __syncthreads();
    float lse_m = s.redm[0], lse_s = s.reds[0];
    for (int i = 1; i < kSpWaves; ++i) sp_lse_combine(lse_m, lse_s, s.redm[i], s.reds[i]);

    // (EXT) the row's allowed-token mask: its first kSpMaxHistory words (262144 tokens) go to `sorted`, which the penalties no
    // longer need; a longer row reads the rest from memory
    const uint32_t *mrow = nullptr;
    const uint32_t *mlds = reinterpret_cast<const uint32_t *>(s.sorted);
    if constexpr (EXT) {
        const llmie_sampling_ext &e = *ep;
        if (e.allowed_mask) {
            const int mi = e.mask_index ? e.mask_index[r] : b;
            if (mi >= 0 && mi < e.mask_rows) mrow = e.allowed_mask + static_cast<size_t>(mi) * e.mask_stride;
        }
        if (mrow) {
            const int lw = min((V + 31) >> 5, kSpMaxHistory);
            uint32_t *dst = reinterpret_cast<uint32_t *>(s.sorted);
            const int n4 = (reinterpret_cast<uintptr_t>(mrow) % 16 == 0) ? lw >> 2 : 0;
            for (int i = tid; i < n4; i += kSpThreads) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(mrow)[i];
            for (int i = 4 * n4 + tid; i < lw; i += kSpThreads) dst[i] = mrow[i];
            __syncthreads();
        }
    }

    // pass 2: keys (value desc, id asc -> the larger (key, ~id)), the maximum and the valid count
    const bool greedy = temp == 0.f;
    const float inv_t = greedy ? 1.f : temp;
    u64 best = 0;
    int nvalid = 0;
    for (int t0 = tid; t0 < V; t0 += kSpUnroll * kSpThreads) {
        float xs[kSpUnroll];
#pragma unroll
        for (int u = 0; u < kSpUnroll; ++u) {
            const int t = t0 + u * kSpThreads;
            xs[u] = t < V ? rowf[t] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kSpUnroll; ++u) {
            const int t = t0 + u * kSpThreads;
            if (t >= V) break;
            float x = xs[u];
            uint32_t k = 0;
            bool in = true;
            if constexpr (EXT) {
                if (mrow) {
                    const int w = t >> 5;
                    const uint32_t word = w < kSpMaxHistory ? mlds[w] : mrow[w];
                    in = (word >> (t & 31)) & 1u;
                }
            }
            if (x == x && in) {
                if (!greedy) x = fminf(fmaxf(x / inv_t, -FLT_MAX), FLT_MAX);
                k = sp_key(x);
                ++nvalid;
                const u64 c = (static_cast<u64>(k) << 32) | (0xffffffffu - static_cast<uint32_t>(t));
                best = c > best ? c : best;
            }
            keys[t] = k;
        }
    }
    best = sp_max64(best, s);
    const int valid = static_cast<int>(sp_sum64(static_cast<u64>(nvalid), s));
    int chosen = end_id;
    if (valid > 0) chosen = static_cast<int>(0xffffffffu - static_cast<uint32_t>(best & 0xffffffffu));

    SpKept kp{true, 0u, 0u, INT_MAX, min_p, 0.f, 0ull};
    if (!greedy && valid > 1) {
        kp.point = false;
        kp.vmax = sp_val(static_cast<uint32_t>(best >> 32));
        // top-k: the top_k-th token (kk, kid); the set {key > kk} + {key == kk, id <= kid}
        if (top_k > 0 && top_k < valid) {
            u64 above;
            auto all = [](int, uint32_t) { return true; };
            kp.kk = radix_select(keys, V, all, [](uint32_t) { return 1ull; }, static_cast<u64>(top_k - 1), &above, s);
            kp.kid = id_select(keys, V, kp.kk, all, static_cast<u64>(top_k - 1) - above, s);
        }
        const SpKept topk = kp;   // (pk == 0: the top-k set alone)
        auto in_k = [topk](int t, uint32_t k) { return topk.in_k(t, k); };
        auto mass = [topk](uint32_t k) { return topk.mass(k); };
        // top-p: keep every value >= that of the first token at which the mass reaches top_p * the top-k mass
        if (top_p < 1.f) {
            u64 ms = 0;
            sp_for_keys(keys, V, [&](int t, uint32_t k) {
                if (k && in_k(t, k)) ms += mass(k);
            });
            ms = sp_sum64(ms, s);
            u64 thr = static_cast<u64>(ceil(static_cast<double>(top_p) * static_cast<double>(ms)));
            thr = thr == 0 ? 0 : thr - 1;
            if (thr >= ms) thr = ms - 1;
            u64 above;
            kp.pk = radix_select(keys, V, in_k, mass, thr, &above, s);
        }
        const SpKept cut = kp;
        u64 mk = 0;
        sp_for_keys(keys, V, [&](int t, uint32_t k) {
            if (k && cut.kept(t, k)) mk += cut.mass(k);
        });
        kp.total = sp_sum64(mk, s);
    }
    return SpRow{SpPick{chosen, valid, lse_m, lse_s, slen, stops}, kp};
}

// The second half, for a row that is no point mass: the first kept token, in (value desc, id asc) order, at which the running
// mass exceeds u * kept mass (u == 1: the last kept token); -1 if there is none.
__device__ __forceinline__ int sp_draw_row(const uint32_t *keys, int V, const SpKept kp, float u, SpShared &s) {
    auto kept = [kp](int t, uint32_t k) { return kp.kept(t, k); };
    auto mass = [kp](uint32_t k) { return kp.mass(k); };
    const u64 mk = kp.total;
    u64 thr = static_cast<u64>(floor(static_cast<double>(u) * static_cast<double>(mk)));
    if (thr >= mk) thr = mk - 1;
    u64 above;
    const uint32_t dk = radix_select(keys, V, kept, mass, thr, &above, s);
    return id_select(keys, V, dk, kept, (thr - above) / mass(dk), s);
}

// The sampler's body for ONE row: the two halves in sequence (steps 0a .. 7 of include/llmie.h).
template <typename T, bool EXT, class History>
__device__ __forceinline__ SpPick sp_sample_row(const T *__restrict__ lg, int V, const llmie_sampling_params p, const History hist, int step,
                                                int end_id, uint32_t *keys, const llmie_sampling_ext *ep, int b, int r, SpShared &s) {
    const SpRow row = sp_prepare_row<T, EXT>(lg, V, p, hist, step, end_id, keys, ep, b, r, s);
    SpPick pick = row.pick;
    if (!row.kept.point) {
        const int id = sp_draw_row(keys, V, row.kept, uniform_philox(static_cast<uint32_t>(step), p.seed), s);
        if (id >= 0) pick.chosen = id;
    }
    return pick;
}

}  // namespace llmie
