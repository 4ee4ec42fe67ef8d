// Fused decode attention for gfx950: llmie_decoder_mha
// (replaces launchDecoderMaskedMultiHeadAttention, decoder_self_attention.cu:56-270).
//
// Math (reference fp32 kernel, with the batch-stride / step<=head_size / GQA-race defects of
// SURVEY 9-K4 fixed):   q,k,v (+bias)  ->  cache[layer,b,g,step-1,:] = k,v  ->
//   logit[t] = (q . K[t]) / sqrt(hs), t < step  ->  p = exp(l - max) / (sum + 1e-6)  ->  out = sum p V.
//
// Design: flash-decoding.  The KV range [0, step) of one (batch, kv-head) is split into chunks of
// CHUNK tokens; one 256-thread workgroup per chunk streams its K and V rows with 16-byte loads
// straight to VGPRs (a wave instruction covers 64/LPT whole rows = 1 KiB contiguous; every load
// of the chunk is issued before the first use), keeps all REP query heads of the kv head in
// registers (GQA reads each K/V byte once), does the softmax with wave64 shuffles, and writes an
// (m, l, o[hs]) partial.  A second tiny kernel merges the partials.  bs*kvh*splits workgroups
// fill the 256 CUs even at batch 1 (7B, S=2048: 32*16 = 512 workgroups).
// HBM-bound: algorithmic bytes = 2 * step * kvh * hs * sizeof(T) per sequence.
#include "llmie_internal.h"
#include "qk_norm.cuh"

#include <climits>
#include <cstdlib>
#include <type_traits>

namespace llmie {

// KV cache element formats: T itself (fp32 / fp16) or e4m3 bytes (stored = e4m3(x / scale), one static scale per cache)
struct fp8kv_t {
    uint8_t b;
};
template <typename KT> struct CacheVec {
    using type = typename Vec16<KT>::type;
    static constexpr int n = Vec16<KT>::n;
};
template <> struct CacheVec<fp8kv_t> {
    using type = uint4_t;
    static constexpr int n = 16;
};
// the N elements of one 16-byte cache vector as fp32 (fp8: unscaled; the scale is folded into q / the output)
template <typename KT, int N> __device__ __forceinline__ void kv_to_f32(const typename CacheVec<KT>::type &v, float (&o)[N]) {
    if constexpr (std::is_same<KT, fp8kv_t>::value) {
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(v[w]), false);
            const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8(static_cast<int>(v[w]), true);
            o[4 * w] = lo[0];
            o[4 * w + 1] = lo[1];
            o[4 * w + 2] = hi[0];
            o[4 * w + 3] = hi[1];
        }
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e) o[e] = to_f32(v[e]);
    }
}
// N values of the activation type -> one 16-byte cache vector (fp8: x * inv_scale, saturating e4m3)
template <typename KT, typename T, int N> __device__ __forceinline__ typename CacheVec<KT>::type kv_pack(const T (&x)[N], float inv_scale) {
    typename CacheVec<KT>::type v;
    if constexpr (std::is_same<KT, fp8kv_t>::value) {
#pragma unroll
        for (int w = 0; w < 4; ++w)
            v[w] = pack4_e4m3(to_f32(x[4 * w]) * inv_scale, to_f32(x[4 * w + 1]) * inv_scale, to_f32(x[4 * w + 2]) * inv_scale,
                              to_f32(x[4 * w + 3]) * inv_scale);
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e) v[e] = x[e];
    }
    return v;
}
// N consecutive activation elements (N * sizeof(T) bytes = one or two 16-byte loads)
template <typename T, int N> __device__ __forceinline__ void load_elems(const T *p, T (&dst)[N]) {
    constexpr int PER = Vec16<T>::n;
    static_assert(N % PER == 0, "whole 16-byte loads");
#pragma unroll
    for (int c = 0; c < N / PER; ++c) {
        const typename Vec16<T>::type v = reinterpret_cast<const typename Vec16<T>::type *>(p)[c];
#pragma unroll
        for (int e = 0; e < PER; ++e) dst[c * PER + e] = v[e];
    }
}

// geometry of the split kernel: NWV waves per workgroup, GL K (and V) 16-byte loads in flight per lane
template <typename KT, int HS, int NWV = 4, int GL = 8> struct AttnGeom {
    static constexpr int N = CacheVec<KT>::n;        // cache elements per 16-byte load = head dims per lane
    static constexpr int LPT = HS / N;               // lanes per token row
    static constexpr int TPW = 64 / LPT;             // token rows per wave instruction
    static constexpr int CHUNK = NWV * GL * TPW;     // tokens per workgroup
};

__host__ __device__ inline int attn_min_chunk() { return 32; }

// Sliding window with sink tokens (include/llmie.h): the query at step - 1 sees key j iff j < step and (j >= step - window or
// j < sinks); window <= 0 is full attention.  Chunks of `chunk` tokens stay aligned to token 0; the LIVE chunks of a sequence --
// those that hold a visible key -- are the sink chunks [0, ceil(min(sinks, step) / chunk)), then the chunks from
// floor(max(0, step - window) / chunk) to the last; a chunk of both lists counts once.  The split kernel's grid x, its partial
// slots, the merge (kernel or ticket) and the host planner all index the live chunks compactly through this one mapping, so the
// slot count, `nsplits` and the ticket count agree by construction.  A window that covers the context gives the unwindowed walk.
struct AttnLive {
    int sink_chunks;   // live chunks in front of `first` (0 when the two lists meet or overlap)
    int first;         // first chunk of the window's list
    int total;         // live chunks
};
__host__ __device__ inline AttnLive attn_live_chunks(int step, int window, int sinks, int chunk) {
    const int n = (step + chunk - 1) / chunk;
    if (window <= 0 || window >= step) return AttnLive{0, 0, n};
    const int first = (step - window) / chunk;
    const int s = sinks < step ? (sinks > 0 ? sinks : 0) : step;
    const int ns = (s + chunk - 1) / chunk;
    if (ns >= first) return AttnLive{0, 0, n};   // the lists meet or overlap: one run from chunk 0
    return AttnLive{ns, first, ns + n - first};
}
// chunk of live index i (< total); its first token is this times the chunk length
__host__ __device__ inline int attn_live_chunk(const AttnLive &lv, int i) { return i < lv.sink_chunks ? i : lv.first + (i - lv.sink_chunks); }
// grid x of a call whose position the host does not know: no context has more live chunks than this
__host__ __device__ inline int attn_live_bound(int max_seq_len, int window, int sinks, int chunk) {
    const int n = (max_seq_len + chunk - 1) / chunk;
    if (window <= 0) return n;
    const long long s = sinks > 0 ? sinks : 0, w = window;
    const long long b = (s + chunk - 1) / chunk + (w + chunk - 1) / chunk + 1;
    return b < n ? static_cast<int>(b) : n;
}

// q/k/v source when the QKV projection's split-K finalize is fused into the attention: fp32 slabs [KS][batch][qkv_dim]
struct QkvSlabs {
    const float *slab;
    int KS;
    size_t stride;          // floats between slabs (= batch * qkv_dim)
    SlabScale sc;           // scales of the projection's weight format (int8: per channel; fp8: channel x token)
};

// Paged KV cache: pool [L][num_pages][kvh][KV_PAGE tokens][hs]; block_table[b * max_pages + p] = pool page of
// the p-th page of sequence b.  table == null: the reference's dense [L][batch][kvh][max_seq][hs] slab.
constexpr int KV_PAGE = 128;
struct PagedKv {
    const int32_t *table;
    int max_pages;
    // (two more launch-wide layout facts ride along with the cache layout)
    int step_stride;   // 0: one position for the whole batch (step / *step_dev); 1: ragged batch, step_dev[b] = context length
                       // of sequence b INCLUDING this step's token
    int out_x32;       // the output rows go to the x32 activation image of the packed projections (<= 32 sequences)
};
// position of sequence b (a value outside [1, max_seq_len] makes every workgroup of that sequence return without touching
// the caches or the output: a corrupt device-resident position must not become an out-of-bounds append)
__device__ __forceinline__ int seq_step(const int32_t *step_dev, int step_arg, int stride, int b, int max_seq_len) {
    const int s = step_dev ? step_dev[static_cast<size_t>(b) * stride] : step_arg;
    return (s >= 1 && s <= max_seq_len) ? s : 0;
}
// element index of (sequence b, feature k) in the attention output: row-major [batch][width] or the x32 image
__device__ __forceinline__ size_t attn_out_index(int x32, int b, int k, int width) {
    if (!x32) return static_cast<size_t>(b) * width + k;
    return (static_cast<size_t>(k >> 5) * 2 + (b >> 4)) * 512 + ((k & 31) >> 3) * 128 + (b & 15) * 8 + (k & 7);
}

// Merge of the per-split (m, l, o[d]) partials of one (batch, head) for output dim d: 16 splits per round,
// every load of a round issued before the first use.  Shared by the stand-alone merge kernel and by the
// in-kernel merge of the last-arriving workgroup, so both give bit-identical results.
// one round of the merge: the 16 (m, l, o[d]) triples of splits s0 .. s0 + 15 (those >= nsplits are ignored) enter (M, L, o)
__device__ __forceinline__ void merge_round(const float (&ms)[16], const float (&ls)[16], const float (&os)[16], int s0, int nsplits,
                                            float &M, float &L, float &o) {
    float Mc = M;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (s0 + i < nsplits) Mc = fmaxf(Mc, ms[i]);
    const float rescale = (M == -INFINITY) ? 0.f : __expf(M - Mc);
    L *= rescale;
    o *= rescale;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (s0 + i < nsplits) {
            const float f = __expf(ms[i] - Mc);
            L = fmaf(f, ls[i], L);
            o = fmaf(f, os[i], o);
        }
    M = Mc;
}
// loads of one round; slots are clamped to `last` (nsplits - 1, or the last slot of the buffer when the loads are issued before
// the number of splits is known: what a clamped-away slot holds is never used)
__device__ __forceinline__ void merge_load(const float *__restrict__ p, int s0, int last, size_t stride, int d, float (&ms)[16],
                                           float (&ls)[16], float (&os)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int s = min(s0 + i, last);
        ms[i] = p[s * stride];
        ls[i] = p[s * stride + 1];
        os[i] = p[s * stride + 2 + d];
    }
}
__device__ __forceinline__ float merge_splits(const float *__restrict__ p, int nsplits, size_t stride, int d) {
    float M = -INFINITY, L = 0.f, o = 0.f;
    for (int s0 = 0; s0 < nsplits; s0 += 16) {
        float ms[16], ls[16], os[16];
        merge_load(p, s0, nsplits - 1, stride, d, ms, ls, os);
        merge_round(ms, ls, os, s0, nsplits, M, L, o);
    }
    return o / (L + 1e-6f);
}
// Learned per-head sink logit (include/llmie.h): one more partial (m = s, l = 1, o = 0) merged LAST into the merged state (M, L, o) of
// a (sequence, head), at every place that normalises -- so it enters once per row whatever the number of splits or waves.  s = -inf:
// the maximum stays M, exp(M - M) = 1 and fma(0, 1, L) = L, i.e. the bits of o / (L + 1e-6) without a sink.
__device__ __forceinline__ float sink_finish(float M, float L, float o, float s) {
    const float Mc = fmaxf(M, s);
    const float rescale = (M == -INFINITY) ? 0.f : __expf(M - Mc);
    L *= rescale;
    o *= rescale;
    const float f = (s == -INFINITY) ? 0.f : __expf(s - Mc);
    L = fmaf(f, 1.f, L);
    return o / (L + 1e-6f);
}
// merge_splits, then the sink: the same rounds in the same order, so the ticket merge and the combine kernel agree bit for bit
__device__ __forceinline__ float merge_splits_sink(const float *__restrict__ p, int nsplits, size_t stride, int d, float s) {
    float M = -INFINITY, L = 0.f, o = 0.f;
    for (int s0 = 0; s0 < nsplits; s0 += 16) {
        float ms[16], ls[16], os[16];
        merge_load(p, s0, nsplits - 1, stride, d, ms, ls, os);
        merge_round(ms, ls, os, s0, nsplits, M, L, o);
    }
    return sink_finish(M, L, o, s);
}

// WIN (compile time) selects the sliding-window form: the workgroup's chunk comes from the live-chunk mapping, a row is masked from
// below as well as from above, and no load goes through the block-table entry of a page without a live row.  Its two launch
// arguments (window, sinks) are the pack WinArgs = (int, int); WIN = false has an empty pack: the arguments and the code the kernel
// had before there was a window.  SINK (compile time) adds the per-head sink logit: one more argument at the end of the pack, the
// device array head_sink[head_num] (fp32), read where an output row is normalised (sink_finish); the streaming loop does not know it.
// QKN (compile time) adds the per-head q/k RMSNorm in front of the rotation (include/llmie.h, llmie_qk_norm; qk_norm.cuh): three more
// arguments at the end of the pack, (const T *q_gamma, const T *k_gamma, float eps); every line of it sits behind if constexpr (QKN).
template <typename T, int HS, int REP, int kAttnWaves = 4, int kAttnG = 8, typename KT = T, bool WIN = false, bool SINK = false, bool QKN = false,
          typename... WinArgs>
__global__ __launch_bounds__(kAttnWaves * 64) void decode_attn_split_kernel(
    const T *__restrict__ qkv, const T *__restrict__ qkv_bias, KT *k_cache, KT *v_cache,
    float *__restrict__ part, T *__restrict__ out, int head_num, int kv_head_num, int max_seq_len,
    int step_arg, const int32_t *__restrict__ step_dev, int max_splits,
    const float2 *__restrict__ rope /* [max_pos][HS/2] (cos,sin) or null */, int rotary_dim,
    int32_t *tickets /* [batch, kv_head_num] zero-initialised arrival counters, or null = separate merge kernel */,
    const QkvSlabs qs /* qs.slab != null: q/k/v come from the split-K partial slabs of the QKV projection (qkv unused) */,
    const float k_scale, const float v_scale /* fp8 cache: stored = e4m3(x / scale); 1 otherwise */,
    const PagedKv pg /* pg.table != null: k_cache / v_cache are this layer's page pools */,
    const int cpw /* chunks of CHUNK tokens one workgroup walks through (online softmax across them): large batches amortise
                     the per-workgroup prologue / merge (~550 of ~1000 VALU instructions per wave at one chunk) */,
    const WinArgs... win /* WIN: window, sinks -- the query sees key j iff j >= step - window or j < sinks (and j < step);
                            SINK: then const float *head_sink; QKN: then const T *q_gamma, const T *k_gamma, float eps */) {
    static_assert(sizeof...(WinArgs) == (WIN ? 2 : 0) + (SINK ? 1 : 0) + (QKN ? 3 : 0), "window, sinks, head_sink, q_gamma, k_gamma, eps");
    using G = AttnGeom<KT, HS, kAttnWaves, kAttnG>;
    using V = typename CacheVec<KT>::type;  // one 16-byte vector of cache elements
    constexpr int N = G::N, LPT = G::LPT, TPW = G::TPW, CHUNK = G::CHUNK;
    constexpr int NT = kAttnWaves * 64;
    constexpr bool FP8KV = std::is_same<KT, fp8kv_t>::value;
    static_assert(HS % N == 0 && LPT >= 1 && LPT <= 64 && (LPT & (LPT - 1)) == 0, "head size");

    const int split = blockIdx.x, g = blockIdx.y, b = blockIdx.z;
    const int step = seq_step(step_dev, step_arg, pg.step_stride, b, max_seq_len);
    const int span = cpw * CHUNK;   // tokens of one workgroup
    // WIN: blockIdx.x counts the sequence's LIVE spans; t_lo = first token of the window, s_eff = its sink tokens
    int t0w = split * span, nsw = 0, t_lo = 0, s_eff = 0;
    if constexpr (WIN) {
        const int window = pack_arg<0>(win...), sinks = pack_arg<1>(win...);
        const AttnLive lv = attn_live_chunks(step, window, sinks, span);
        if (split >= lv.total) return;   // (also: invalid position, total = 0)
        t0w = attn_live_chunk(lv, split) * span;
        nsw = lv.total;
        t_lo = (window > 0 && window < step) ? step - window : 0;
        s_eff = max(0, min(sinks, step));
    }
    const int t0 = t0w;
    if (t0 >= step) return;  // whole workgroup exits together (also: invalid position)
    int tc0 = t0;                             // first token of the chunk being processed
    if constexpr (WIN) {
        if (t0 >= s_eff) tc0 = max(t0, t_lo / CHUNK * CHUNK);   // cpw > 1: the span's first live chunk
    }
    int t_end = min(step, tc0 + CHUNK);       // end of that chunk
    const int nsplits = WIN ? nsw : (step + span - 1) / span;
    // WIN: is row t of the current chunk visible / does the chunk at tc (< step) hold a visible row
    auto row_live = [&](int t) { return t < t_end && (!WIN || t >= t_lo || t < s_eff); };
    auto chunk_live = [&](int tc) { return tc < s_eff || tc + CHUNK > t_lo; };
    const int batch = gridDim.z;
    const float *head_sink = nullptr;
    if constexpr (SINK) head_sink = pack_arg<WIN ? 2 : 0>(win...);
    (void)head_sink;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LPT, dl = lane % LPT;
    const int qkv_heads = head_num + 2 * kv_head_num;
    const float scale = rsqrtf(static_cast<float>(HS));

    const T *row = qkv + static_cast<size_t>(b) * qkv_heads * HS;
    // q for the REP heads of this kv head, pre-scaled, fp32
    // Cache rows of this workgroup's chunk: one base pointer per 128-token page the chunk touches (1 or 2).  Dense layout: the
    // page-aligned pieces of the head's contiguous [max_seq][HS] slab; paged: looked up ONCE here in the block table (uniform
    // scalar loads), so the K/V loads below never depend on a table load.
    constexpr int NPG = CHUNK > KV_PAGE ? CHUNK / KV_PAGE : 1;
    static_assert(CHUNK % KV_PAGE == 0 || KV_PAGE % CHUNK == 0, "chunk vs page size");
    int pg0 = 0;
    KT *kbase[NPG], *vbase[NPG];
    auto set_pages = [&]() {   // of the chunk at tc0
        pg0 = tc0 / KV_PAGE;
        // WIN, chunks of several pages: a page without a visible row (before the window and past the sinks, or past the context)
        // may be unmapped, so its slot takes the base of the chunk's first page that has one and no load goes through its entry
        auto page_live = [&](int j) {
            const int a = (pg0 + j) * KV_PAGE;
            return a < t_end && (a < s_eff || min(a + KV_PAGE, t_end) > t_lo);
        };
        int jl = 0;
        if constexpr (WIN && NPG > 1) {
#pragma unroll
            for (int j = NPG - 1; j >= 0; --j)
                if (page_live(j)) jl = j;
        }
#pragma unroll
        for (int j0 = 0; j0 < NPG; ++j0) {
            int j = j0;
            if constexpr (WIN && NPG > 1) j = page_live(j0) ? j0 : jl;
            size_t off;
            if (pg.table) {
                const int page = pg.table[static_cast<size_t>(b) * pg.max_pages + min(pg0 + j, pg.max_pages - 1)];
                off = (static_cast<size_t>(page) * kv_head_num + g) * KV_PAGE * HS;
            } else {
                off = (static_cast<size_t>(b) * kv_head_num + g) * max_seq_len * HS + static_cast<size_t>(pg0 + j) * KV_PAGE * HS;
            }
            kbase[j0] = k_cache + off;
            vbase[j0] = v_cache + off;
        }
    };
    set_pages();
    auto krow = [&](int t) { return kbase[NPG == 1 ? 0 : (t / KV_PAGE - pg0)] + static_cast<size_t>(t % KV_PAGE) * HS; };
    auto vrow = [&](int t) { return vbase[NPG == 1 ? 0 : (t / KV_PAGE - pg0)] + static_cast<size_t>(t % KV_PAGE) * HS; };
    KT *kc = kbase[0];  // a readable address of this head (dummy source of the unconditional loads below)
    const int t_new = step - 1;
    // small L2-resident operands first (q rows, RoPE row), then the K/V stream; q is processed after the K/V
    // loads have been issued, so its latency hides under theirs (vmcnt retires in order: q is older)
    // Slab mode (q/k/v still in the QKV projection's split-K slabs): the rows this workgroup needs -- REP q heads, plus
    // the new k and v rows when its chunk holds this step's token -- are reduced ONCE per workgroup into LDS by the
    // first threads (one float4 column each, all slab loads in flight together, summed in the finalize kernel's
    // order, scaled and rounded like it) instead of by every lane (16 lanes x 4 waves hold the same q slice).
    T qraw[REP][N];
    constexpr int ITEMS_PER_HEAD = HS / 4;
    constexpr int LROUNDS = ((REP + 2) * ITEMS_PER_HEAD + NT - 1) / NT;
    __shared__ __attribute__((aligned(16))) T qkvlds[(REP + 2) * HS];
    const bool wg_has_new = t_new >= t0 && t_new < t0 + span;  // workgroup-uniform
    floatx4 spart[LROUNDS][4];
    half4_t sscale[LROUNDS];
    floatx4 sscalef[LROUNDS];
    const float xs_b = (qs.slab && qs.sc.wf) ? qs.sc.xs[b] : 1.f;
    size_t scol[LROUNDS];
    bool sact[LROUNDS];
    if (qs.slab) {
#pragma unroll
        for (int lr = 0; lr < LROUNDS; ++lr) {
            const int item = lr * NT + threadIdx.x;
            const int hsel = item / ITEMS_PER_HEAD, d4 = item - hsel * ITEMS_PER_HEAD;
            sact[lr] = hsel < REP || (wg_has_new && hsel < REP + 2);
            const int hh = hsel < REP ? g * REP + hsel : (hsel == REP ? head_num + g : head_num + kv_head_num + g);
            scol[lr] = static_cast<size_t>(hh) * HS + d4 * 4;
            if (sact[lr]) {
                const float *p = qs.slab + static_cast<size_t>(b) * qkv_heads * HS + scol[lr];
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    spart[lr][kk] = *reinterpret_cast<const floatx4 *>(p + static_cast<size_t>(min(kk, qs.KS - 1)) * qs.stride);
                if (qs.sc.wh) sscale[lr] = *reinterpret_cast<const half4_t *>(qs.sc.wh + scol[lr]);
                if (qs.sc.wf) sscalef[lr] = *reinterpret_cast<const floatx4 *>(qs.sc.wf + scol[lr]);
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < REP; ++r) load_elems<T, N>(row + static_cast<size_t>(g * REP + r) * HS + dl * N, qraw[r]);
    }
    // this step's k/v rows and the bias slices: loaded by every workgroup, unconditionally (a load under a divergent
    // or data-dependent branch makes the compiler drain vmcnt at the join -- measured: the K/V stream below used to
    // stall after its second load).  Without a bias / outside slab mode the address is a dummy valid one (the head's
    // first cache row) and the value is dropped by a select.
    const int hk = head_num + g, hv = head_num + kv_head_num + g;
    const T *dummy = reinterpret_cast<const T *>(kc);  // N * sizeof(T) <= 32 readable bytes at the head's first cache rows
    T knraw[N], vnraw[N], qbias[REP][N], kbias[N], vbias[N];
    load_elems<T, N>(qs.slab ? dummy : row + static_cast<size_t>(hk) * HS + dl * N, knraw);
    load_elems<T, N>(qs.slab ? dummy : row + static_cast<size_t>(hv) * HS + dl * N, vnraw);
#pragma unroll
    for (int r = 0; r < REP; ++r)
        load_elems<T, N>(qkv_bias ? qkv_bias + static_cast<size_t>(g * REP + r) * HS + dl * N : dummy, qbias[r]);
    load_elems<T, N>(qkv_bias ? qkv_bias + static_cast<size_t>(hk) * HS + dl * N : dummy, kbias);
    load_elems<T, N>(qkv_bias ? qkv_bias + static_cast<size_t>(hv) * HS + dl * N : dummy, vbias);
    // QKN: this lane's slices of the two gammas (its head dims dl * N .. + N), with the other small operands
    T qgam[QKN ? N : 1], kgam[QKN ? N : 1];
    float qkn_eps = 0.f;
    if constexpr (QKN) {
        constexpr int Q0 = (WIN ? 2 : 0) + (SINK ? 1 : 0);
        load_elems<T, N>(pack_arg<Q0>(win...) + dl * N, qgam);
        load_elems<T, N>(pack_arg<Q0 + 1>(win...) + dl * N, kgam);
        qkn_eps = pack_arg<Q0 + 2>(win...);
    }
    (void)qgam, (void)kgam, (void)qkn_eps;
    float2 csraw[N];
    if (rope) {
        const float2 *cs = rope + static_cast<size_t>(t_new) * (HS / 2) + (dl % (LPT / 2)) * N;
#pragma unroll
        for (int e = 0; e < N; ++e) csraw[e] = cs[e];
    }
    // ---- issue every K and V load of this wave's token range ----
    V kv[kAttnG], vv[kAttnG];
    int tok[kAttnG];
    auto issue_loads = [&]() {   // of the chunk at tc0 (pages set)
        // WIN: a masked row -- past the chunk end, or between the sinks and the window -- re-reads one visible row of the chunk (the
        // window's first row there, else the chunk's first row, a sink), so the clamp holds from below as from above
        const int t_fb = (tc0 + CHUNK > t_lo) ? max(tc0, t_lo) : tc0;
#pragma unroll
        for (int i = 0; i < kAttnG; ++i) {
            const int t = tc0 + (wave * kAttnG + i) * TPW + sub;
            tok[i] = t;
            // unwindowed: rows past the chunk end re-read its last row (masked below); WIN: every masked row, those past the chunk
            // end included, re-reads t_fb.  The slot of this step's token is read as it is (stale, replaced below): every load is
            // unconditional so all 2*G of them are in flight together
            if constexpr (WIN) kv[i] = load_nt(reinterpret_cast<const V *>(krow(row_live(t) ? t : t_fb)) + dl);
            else kv[i] = load_nt(reinterpret_cast<const V *>(krow(min(t, t_end - 1))) + dl);
        }
#pragma unroll
        for (int i = 0; i < kAttnG; ++i) {
            if constexpr (WIN) vv[i] = load_nt(reinterpret_cast<const V *>(vrow(row_live(tok[i]) ? tok[i] : t_fb)) + dl);
            else vv[i] = load_nt(reinterpret_cast<const V *>(vrow(min(tok[i], t_end - 1))) + dl);
        }
    };
    issue_loads();
    if (qs.slab) {
#pragma unroll
        for (int lr = 0; lr < LROUNDS; ++lr) {
            if (sact[lr]) {
                const float *p = qs.slab + static_cast<size_t>(b) * qkv_heads * HS + scol[lr];
                floatx4 f = spart[lr][0];
#pragma unroll
                for (int kk = 1; kk < 4; ++kk)
                    if (kk < qs.KS) f += spart[lr][kk];
                for (int k = 4; k < qs.KS; ++k) f += *reinterpret_cast<const floatx4 *>(p + static_cast<size_t>(k) * qs.stride);
                const int item = lr * NT + threadIdx.x;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v = f[e];
                    if (qs.sc.wh) v *= to_f32(sscale[lr][e]);          // the arithmetic of SlabScale::apply
                    if (qs.sc.wf) v *= sscalef[lr][e] * xs_b;
                    qkvlds[item * 4 + e] = from_f32<T>(v);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < REP; ++r) load_elems<T, N>(&qkvlds[r * HS + dl * N], qraw[r]);
    }
    // RoPE (fused form of launchRope, rope.cu:4-43): rotate-half pairs (d, d+HS/2) live LPT/2 lanes apart
    const bool rope_first = dl < LPT / 2;
    float rc[N], rs[N];
    if (rope) {
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const bool rot = ((dl % (LPT / 2)) * N + e) < (rotary_dim >> 1);
            const float2 v = rot ? csraw[e] : float2{1.f, 0.f};
            rc[e] = v.x;
            rs[e] = rope_first ? -v.y : v.y;
        }
    }
    auto rotate = [&](float (&x)[N]) {
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const float partner = (LPT / 2 < 16) ? lane_xor_lt16<(LPT / 2 < 16 ? LPT / 2 : 8)>(x[e]) : __shfl_xor(x[e], LPT / 2, 64);
            x[e] = x[e] * rc[e] + partner * rs[e];
        }
    };
    // e4m3 cache: the scale operand of v_cvt_scalef32_pk_f16_fp8 is E8M0 (only the exponent bits of the float are used), so the
    // conversion gets the power-of-two part of k_scale and q carries the mantissa remainder (in [1, 2)) in fp32
    const float k_p2 = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, k_scale) & 0x7f800000u);
    const float k_q = FP8KV ? k_scale / k_p2 : k_scale;
    (void)k_p2;
    // QKN: the head row this lane holds a slice of (fp16 values, as the projection stored them) -> normalised, rounded to T: the
    // sum of squares in qk_norm.cuh's order (N = 16: the two groups of a lane differ in the group index's lowest bit, added first)
    auto qk_normalise = [&](float (&x)[N], const T (&gam)[QKN ? N : 1]) {
        if constexpr (QKN) {
            float ss = qkn_group_ss(x);
            if constexpr (N == 16) ss = ss + qkn_group_ss(x + 8);
            const float inv = qkn_inv(qkn_lane_butterfly<LPT>(ss), HS, qkn_eps);
#pragma unroll
            for (int e = 0; e < N; ++e) x[e] = to_f32(qkn_apply<T>(x[e], inv, to_f32(gam[e])));
        }
    };
    float qf[REP][N];
#pragma unroll
    for (int r = 0; r < REP; ++r) {
        float f[N];
#pragma unroll
        for (int e = 0; e < N; ++e) f[e] = to_f32(qraw[r][e]);
        qk_normalise(f, qgam);   // QKN: one sum per head
        if (rope) {
            rotate(f);
#pragma unroll
            for (int e = 0; e < N; ++e) f[e] = to_f32(from_f32<T>(f[e]));  // as stored by the unfused RoPE kernel
        }
#pragma unroll
        for (int e = 0; e < N; ++e) {
            f[e] += qkv_bias ? to_f32(qbias[r][e]) : 0.f;
            qf[r][e] = f[e] * (scale * k_q);  // the cache holds k / k_scale (fp8: the conversion applies the power-of-two part)
        }
    }
    // e4m3 cache: K.q on packed fp16 -- v_cvt_scalef32_pk_f16_fp8 turns two cache bytes into (k0, k1) * k_scale in one instruction
    // and v_dot2_f32_f16 adds both products to the fp32 logit: 16 instructions per 16-byte vector instead of 8 conversions + 16
    // fp32 FMAs.  q (already scaled by 1/sqrt(hs), O(0.1)) is rounded to fp16 for this: 2^-11 relative, far below the cache's
    // own e4m3 step (2^-4).
    half2_t qh[FP8KV ? REP : 1][FP8KV ? N / 2 : 1];
    if constexpr (FP8KV) {
#pragma unroll
        for (int r = 0; r < REP; ++r)
#pragma unroll
            for (int j = 0; j < N / 2; ++j) qh[r][j] = half2_t{from_f32<half_t>(qf[r][2 * j]), from_f32<half_t>(qf[r][2 * j + 1])};
    }

    // the token of this step comes from the qkv buffer / slabs (RoPE, then +bias, as the reference's rope.cu then
    // decoder_self_attention.cu:111-118) and is appended to the cache; computed by every lane, kept by the token's lanes
    V knv, vnv;   // in the cache's element format: what is stored is what this step attends to
    {
        T kn[N], vn[N];
#pragma unroll
        for (int e = 0; e < N; ++e) {
            kn[e] = knraw[e];
            vn[e] = vnraw[e];
        }
        if (qs.slab) {
            load_elems<T, N>(&qkvlds[REP * HS + dl * N], kn);
            load_elems<T, N>(&qkvlds[(REP + 1) * HS + dl * N], vn);
        }
        if constexpr (QKN) {   // k (never v): normalised by every lane, like the rotation below
            float f[N];
#pragma unroll
            for (int e = 0; e < N; ++e) f[e] = to_f32(kn[e]);
            qk_normalise(f, kgam);
#pragma unroll
            for (int e = 0; e < N; ++e) kn[e] = from_f32<T>(f[e]);
        }
        if (rope) {
            float f[N];
#pragma unroll
            for (int e = 0; e < N; ++e) f[e] = to_f32(kn[e]);
            rotate(f);
#pragma unroll
            for (int e = 0; e < N; ++e) kn[e] = from_f32<T>(f[e]);
        }
#pragma unroll
        for (int e = 0; e < N; ++e) {
            kn[e] = qkv_bias ? from_f32<T>(to_f32(kn[e]) + to_f32(kbias[e])) : kn[e];
            vn[e] = qkv_bias ? from_f32<T>(to_f32(vn[e]) + to_f32(vbias[e])) : vn[e];
        }
        knv = kv_pack<KT, T, N>(kn, 1.0f / k_scale);
        vnv = kv_pack<KT, T, N>(vn, 1.0f / v_scale);
    }
    auto inject = [&]() {   // chunk at tc0, its loads issued
        bool mine = false;
        if (t_new >= tc0 && t_new < tc0 + CHUNK) {   // workgroup-uniform: every other chunk skips 8 selects per loaded vector
#pragma unroll
        for (int i = 0; i < kAttnG; ++i) {
            const bool is_new = tok[i] == t_new;
            mine |= is_new;
            uint4_t kw = __builtin_bit_cast(uint4_t, kv[i]), vw = __builtin_bit_cast(uint4_t, vv[i]);
            const uint4_t knw = __builtin_bit_cast(uint4_t, knv), vnw = __builtin_bit_cast(uint4_t, vnv);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                kw[w] = is_new ? knw[w] : kw[w];
                vw[w] = is_new ? vnw[w] : vw[w];
            }
            kv[i] = __builtin_bit_cast(V, kw);
            vv[i] = __builtin_bit_cast(V, vw);
        }
        }
        if (mine) {
            reinterpret_cast<V *>(krow(t_new))[dl] = knv;
            reinterpret_cast<V *>(vrow(t_new))[dl] = vnv;
        }
    };
    inject();

    // running softmax state of this wave over the chunks of the workgroup: maximum (wave-uniform), and per lane the sum of
    // numerators and the weighted value sums of ITS token slots (reduced across the lanes once, after the last chunk)
    float mx[REP], acc[REP][N], ls[REP];
#pragma unroll
    for (int r = 0; r < REP; ++r) {
        mx[r] = -INFINITY;
        ls[r] = 0.f;
#pragma unroll
        for (int e = 0; e < N; ++e) acc[r][e] = 0.f;
    }
    auto accumulate = [&](const bool first) {   // chunk at tc0, its vectors landed and patched
    // ---- logits ----
    float lg[REP][kAttnG];
    float cm[REP];
#pragma unroll
    for (int r = 0; r < REP; ++r) cm[r] = -INFINITY;
#pragma unroll
    for (int i = 0; i < kAttnG; ++i) {
        const bool valid = row_live(tok[i]);
        float kf[FP8KV ? 1 : N];
        half2_t kh[FP8KV ? N / 2 : 1];
        if constexpr (FP8KV) {
            const uint4_t kw = __builtin_bit_cast(uint4_t, kv[i]);
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                kh[2 * w] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(static_cast<int>(kw[w]), k_p2, false);
                kh[2 * w + 1] = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(static_cast<int>(kw[w]), k_p2, true);
            }
        } else {
            kv_to_f32<KT, N>(kv[i], kf);
        }
#pragma unroll
        for (int r = 0; r < REP; ++r) {
            float d = 0.f;
            if (valid) {
                if constexpr (FP8KV) {
#pragma unroll
                    for (int j = 0; j < N / 2; ++j) d = __builtin_amdgcn_fdot2(kh[j], qh[r][j], d, false);
                } else {
#pragma unroll
                    for (int e = 0; e < N; ++e) d = fmaf(qf[r][e], kf[e], d);
                }
            }
            d = group_sum<LPT>(d);
            lg[r][i] = valid ? d : -INFINITY;
            cm[r] = fmaxf(cm[r], lg[r][i]);
        }
    }
    // wave max over the TPW token slots (lanes differing in sub), then the running maximum; what was accumulated under the old
    // maximum is rescaled (nothing to rescale in a workgroup's first chunk)
#pragma unroll
    for (int r = 0; r < REP; ++r) {
#pragma unroll
        for (int o = LPT; o < 64; o <<= 1) cm[r] = lane_xor_max_o(cm[r], o);
        const float mnew = fmaxf(mx[r], cm[r]);
        if (!first) {
            const float f = (mx[r] == -INFINITY) ? 0.f : __expf(mx[r] - mnew);
            ls[r] *= f;
#pragma unroll
            for (int e = 0; e < N; ++e) acc[r][e] *= f;
        }
        mx[r] = mnew;
    }
    // ---- softmax numerators and P.V ----
#pragma unroll
    for (int i = 0; i < kAttnG; ++i) {
        const bool valid = row_live(tok[i]);
        if (valid) {
            float vf[N];
            kv_to_f32<KT, N>(vv[i], vf);
#pragma unroll
            for (int r = 0; r < REP; ++r) {
                const float p = __expf(lg[r][i] - mx[r]);
                ls[r] += p;
#pragma unroll
                for (int e = 0; e < N; ++e) acc[r][e] = fmaf(p, vf[e], acc[r][e]);
            }
        }
    }
    };
    accumulate(true);
    // the workgroup's further chunks: same loads, same arithmetic, the prologue above paid once.  e4m3 cache only: there the
    // fixed work is ~550 of ~1000 VALU instructions per wave and batch 32 x ctx 2048 went from 130 to 98 us per layer (4.1 ->
    // 5.5 TB/s); the fp16 cache streams at 6.2-6.3 TB/s with one chunk per workgroup and the loop's longer register live ranges
    // (146 -> 177 VGPRs, two workgroups per CU instead of three) cost 2.5 us per launch at ctx 128, so it is compiled out there.
    if constexpr (FP8KV) {
        for (int c = 1; c < cpw; ++c) {
            tc0 += CHUNK;
            if (tc0 >= step) break;   // workgroup-uniform
            if constexpr (WIN) {      // (the span's first live chunk may lie past its start; a chunk between sinks and window is skipped)
                if (tc0 >= t0 + span) break;
                if (!chunk_live(tc0)) continue;
            }
            t_end = min(step, tc0 + CHUNK);
            set_pages();
            issue_loads();
            inject();
            accumulate(false);
        }
    }
#pragma unroll
    for (int r = 0; r < REP; ++r) {
#pragma unroll
        for (int o = LPT; o < 64; o <<= 1) {
            // (v + v[lane ^ o] through the row swaps / DPP: no LDS round trips; bit-identical to the __shfl_xor butterfly)
            ls[r] = lane_xor_sum_o(ls[r], o);
#pragma unroll
            for (int e = 0; e < N; ++e) acc[r][e] = lane_xor_sum_o(acc[r][e], o);
        }
    }
    // ---- merge the 4 waves through LDS ----
    __shared__ float s_m[REP][kAttnWaves], s_l[REP][kAttnWaves];
    __shared__ float s_o[REP][kAttnWaves][HS];
    if (sub == 0) {
#pragma unroll
        for (int r = 0; r < REP; ++r) {
#pragma unroll
            for (int e = 0; e < N; ++e) s_o[r][wave][dl * N + e] = acc[r][e] * v_scale;  // the cache holds v / v_scale
            if (dl == 0) {
                s_m[r][wave] = mx[r];
                s_l[r][wave] = ls[r];
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < REP * HS; i += NT) {
        const int r = i / HS, d = i - r * HS;
        float M = s_m[r][0];
#pragma unroll
        for (int w = 1; w < kAttnWaves; ++w) M = fmaxf(M, s_m[r][w]);
        float L = 0.f, o = 0.f;
#pragma unroll
        for (int w = 0; w < kAttnWaves; ++w) {
            const float f = (s_m[r][w] == -INFINITY) ? 0.f : __expf(s_m[r][w] - M);
            L += f * s_l[r][w];
            o += f * s_o[r][w][d];
        }
        const int h = g * REP + r;
        if (nsplits == 1) {
            if constexpr (SINK) out[attn_out_index(pg.out_x32, b, h * HS + d, head_num * HS)] = from_f32<T>(sink_finish(M, L, o, head_sink[h]));
            else out[attn_out_index(pg.out_x32, b, h * HS + d, head_num * HS)] = from_f32<T>(o / (L + 1e-6f));
        } else {
            float *p = part + ((static_cast<size_t>(b) * head_num + h) * max_splits + split) * (HS + 2);
            p[2 + d] = o;
            if (d == 0) {
                p[0] = M;
                p[1] = L;
            }
        }
    }
    (void)batch;
    // ---- in-launch merge by the last-arriving workgroup of this (batch, kv head) ----
    // Placement-independent hand-off (cdna_hip_programming.md Guideline 16, counter form): plain partial stores ->
    // every storing wave drains vmcnt -> workgroup barrier -> lane 0: agent-scope release, drained, then ONE relaxed
    // agent-scope ticket -> the workgroup that draws nsplits-1 acquires (agent scope), barrier, reads all partials.
    if (tickets && nsplits > 1) {
        __shared__ int s_ticket;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        int32_t *cnt = tickets + static_cast<size_t>(b) * kv_head_num + g;
        if (threadIdx.x == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            s_ticket = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (s_ticket == nsplits - 1) {  // workgroup-uniform
            if (threadIdx.x == 0) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm for the next launch
            }
            __syncthreads();
            const size_t stride = static_cast<size_t>(HS) + 2;
            for (int i = threadIdx.x; i < REP * HS; i += NT) {
                const int r = i / HS, d = i - r * HS;
                const int h = g * REP + r;
                const float *p = part + (static_cast<size_t>(b) * head_num + h) * max_splits * stride;
                float v;
                if constexpr (SINK) v = merge_splits_sink(p, nsplits, stride, d, head_sink[h]);
                else v = merge_splits(p, nsplits, stride, d);
                out[attn_out_index(pg.out_x32, b, h * HS + d, head_num * HS)] = from_f32<T>(v);
            }
        }
    }
}

// merge the per-split partials: grid (head_num, batch), one thread per output dim.  Every thread reads the
// (m, l) pairs itself (broadcast loads) and its own o values, 16 splits per round with all loads issued before
// the first use, so the kernel is about one L2 round trip per 16 splits -- no LDS, no barrier.
// WIN: the partial slots are the live chunks of the window (attn_live_chunks), as the split kernel filled them.  SINK: the head-sink
// array ends the pack; the sink of head h enters after the last round (sink_finish).
template <typename T, bool WIN = false, bool SINK = false, typename... WinArgs>
__global__ __launch_bounds__(256) void decode_attn_combine_kernel(const float *__restrict__ part,
                                                                  T *__restrict__ out, int head_num,
                                                                  int head_size, int chunk, int step_arg,
                                                                  const int32_t *__restrict__ step_dev,
                                                                  int max_splits, int step_stride, int max_seq_len, int out_x32,
                                                                  const WinArgs... win /* WIN: window, sinks; SINK: head_sink */) {
    static_assert(sizeof...(WinArgs) == (WIN ? 2 : 0) + (SINK ? 1 : 0), "window, sinks, head_sink");
    const int h = blockIdx.x, b = blockIdx.y;
    float sink = -INFINITY;
    if constexpr (SINK) sink = pack_arg<WIN ? 2 : 0>(win...)[h];   // beside the first round's loads
    (void)sink;
    const size_t stride = static_cast<size_t>(head_size) + 2;
    const float *p = part + (static_cast<size_t>(b) * head_num + h) * max_splits * stride;
    // The first round's loads do not wait for the device-resident position: they go out beside its load, clamped to the buffer
    // (a slot past the live splits holds an older step's values, which merge_round never looks at) -- one L2 round trip less in
    // a kernel that is three dependent round trips and a launch.  Same arithmetic as merge_splits: bit-identical.
    int d = threadIdx.x;
    float ms[16], ls[16], os[16];
    merge_load(p, 0, max_splits - 1, stride, min(d, head_size - 1), ms, ls, os);
    const int step = seq_step(step_dev, step_arg, step_stride, b, max_seq_len);
    int nsplits = (step + chunk - 1) / chunk;
    if constexpr (WIN) {
        nsplits = attn_live_chunks(step, pack_arg<0>(win...), pack_arg<1>(win...), chunk).total;
    }
    if (nsplits <= 1) return;  // the split kernel already wrote the final output (or: invalid position)
    if (d < head_size) {
        float M = -INFINITY, L = 0.f, o = 0.f;
        merge_round(ms, ls, os, 0, nsplits, M, L, o);
        for (int s0 = 16; s0 < nsplits; s0 += 16) {
            merge_load(p, s0, nsplits - 1, stride, d, ms, ls, os);
            merge_round(ms, ls, os, s0, nsplits, M, L, o);
        }
        if constexpr (SINK) out[attn_out_index(out_x32, b, h * head_size + d, head_num * head_size)] = from_f32<T>(sink_finish(M, L, o, sink));
        else out[attn_out_index(out_x32, b, h * head_size + d, head_num * head_size)] = from_f32<T>(o / (L + 1e-6f));
    }
    for (d += blockDim.x; d < head_size; d += blockDim.x) {   // head sizes above the block size
        if constexpr (SINK) out[attn_out_index(out_x32, b, h * head_size + d, head_num * head_size)] = from_f32<T>(merge_splits_sink(p, nsplits, stride, d, sink));
        else out[attn_out_index(out_x32, b, h * head_size + d, head_num * head_size)] = from_f32<T>(merge_splits(p, nsplits, stride, d));
    }
}

// Any head size / GQA ratio (e.g. the reference unit test's hs=4): one workgroup per (b, q-head),
// scalar loads, logits in LDS.  step*4 bytes of dynamic LDS.
template <typename T>
__global__ __launch_bounds__(256) void decode_attn_generic_kernel(
    const T *__restrict__ qkv, const T *__restrict__ qkv_bias, T *k_cache, T *v_cache, T *__restrict__ out,
    int head_num, int kv_head_num, int head_size, int max_seq_len, int step_arg,
    const int32_t *__restrict__ step_dev) {
    extern __shared__ float logits[];  // [step]
    __shared__ float red[4];
    const int h = blockIdx.x, b = blockIdx.y;
    const int step = seq_step(step_dev, step_arg, 0, b, max_seq_len);
    if (step == 0) return;   // invalid device-resident position
    const int rep = head_num / kv_head_num, g = h / rep;
    const int qkv_heads = head_num + 2 * kv_head_num;
    const T *row = qkv + static_cast<size_t>(b) * qkv_heads * head_size;
    const int hk = head_num + g, hv = head_num + kv_head_num + g;
    const size_t head_off = (static_cast<size_t>(b) * kv_head_num + g) * max_seq_len * head_size;
    T *kc = k_cache + head_off, *vc = v_cache + head_off;
    const int t_new = step - 1;
    const float scale = rsqrtf(static_cast<float>(head_size));
    auto qv = [&](int d) { return to_f32(row[static_cast<size_t>(h) * head_size + d]) + (qkv_bias ? to_f32(qkv_bias[static_cast<size_t>(h) * head_size + d]) : 0.f); };
    auto knew = [&](int d) { return from_f32<T>(to_f32(row[static_cast<size_t>(hk) * head_size + d]) + (qkv_bias ? to_f32(qkv_bias[static_cast<size_t>(hk) * head_size + d]) : 0.f)); };
    auto vnew = [&](int d) { return from_f32<T>(to_f32(row[static_cast<size_t>(hv) * head_size + d]) + (qkv_bias ? to_f32(qkv_bias[static_cast<size_t>(hv) * head_size + d]) : 0.f)); };
    if (h % rep == 0) {  // one q-head per kv group appends; the others read k/v_new from qkv
        for (int d = threadIdx.x; d < head_size; d += 256) {
            kc[static_cast<size_t>(t_new) * head_size + d] = knew(d);
            vc[static_cast<size_t>(t_new) * head_size + d] = vnew(d);
        }
    }
    float mx = -INFINITY;
    for (int t = threadIdx.x; t < step; t += 256) {
        float acc = 0.f;
        for (int d = 0; d < head_size; ++d) {
            const float kvl = (t == t_new) ? to_f32(knew(d)) : to_f32(kc[static_cast<size_t>(t) * head_size + d]);
            acc = fmaf(qv(d), kvl, acc);
        }
        acc *= scale;
        logits[t] = acc;
        mx = fmaxf(mx, acc);
    }
    mx = block_max<4>(mx, red);
    float sum = 0.f;
    for (int t = threadIdx.x; t < step; t += 256) {
        const float p = expf(logits[t] - mx);
        logits[t] = p;
        sum += p;
    }
    sum = block_sum<4>(sum, red) + 1e-6f;
    __syncthreads();
    for (int d = threadIdx.x; d < head_size; d += 256) {
        float o = 0.f;
        for (int t = 0; t < step; ++t) {
            const float vvl = (t == t_new) ? to_f32(vnew(d)) : to_f32(vc[static_cast<size_t>(t) * head_size + d]);
            o = fmaf(logits[t], vvl, o);
        }
        out[(static_cast<size_t>(b) * head_num + h) * head_size + d] = from_f32<T>(o / sum);
    }
}

struct KvScale {
    float k, v;
};

// ---- the launch plan: pure host code (no pointer read, no environment, no HIP call, no error text) ----
// tokens per chunk of the split kernel's geometry (4 waves, 8 K + 8 V loads in flight per lane; 8 waves x 8 and 4 x 4 measured
// slower, round 1) for a supported head size
template <typename KT> static int attn_chunk(int hs) {
    switch (hs) {
        case 32: return AttnGeom<KT, 32>::CHUNK;
        case 64: return AttnGeom<KT, 64>::CHUNK;
        case 128: return AttnGeom<KT, 128>::CHUNK;
        default: return AttnGeom<KT, 256>::CHUNK;
    }
}
static bool attn_fused_geometry(const DecodeAttnCall &c) {
    const int rep = c.head_num / c.kv_head_num;
    return (c.head_size == 32 || c.head_size == 64 || c.head_size == 128 || c.head_size == 256) && (rep == 1 || rep == 2 || rep == 4 || rep == 8);
}
static DecodeAttnPlan attn_refusal(int refusal, size_t need = 0) {
    DecodeAttnPlan p{};
    p.kind = DA_REFUSED, p.refusal = refusal, p.workspace_bytes = need;
    return p;
}
static DecodeAttnPlan plan_attn_split(const DecodeAttnCall &c, size_t need) {
    DecodeAttnPlan p{};
    const int bound = c.step_dev ? c.max_seq_len : c.step;
    p.kind = DA_SPLIT, p.hs = c.head_size, p.rep = c.head_num / c.kv_head_num, p.e4m3 = c.kv_e4m3;
    // chunks per workgroup: a function of the batch geometry ONLY (not of the step: the host-step and the device-step form of
    // one call must chunk alike), 1 while the grid needs every chunk as its own workgroup, up to 8 for large batches (batch 32 x 32
    // heads at ctx 2048: one workgroup per (sequence, head), no partials and no merge launch at all); e4m3 cache only, see the kernel
    p.cpw = 1;
    if (c.kv_e4m3)
        while (p.cpw < 8 && c.batch * c.kv_head_num >= 128 * p.cpw) p.cpw *= 2;   // >= 256 workgroups per chunk row are kept
    const int base = c.kv_e4m3 ? attn_chunk<fp8kv_t>(p.hs) : (c.dtype == LLMIE_F32 ? attn_chunk<float>(p.hs) : attn_chunk<half_t>(p.hs));
    p.chunk = p.cpw * base;
    p.grid[0] = (bound + p.chunk - 1) / p.chunk, p.grid[1] = c.kv_head_num, p.grid[2] = c.batch;
    if (c.window > 0) {   // grid x = live spans: known from a host step, bounded by the window (not by max_seq_len) otherwise
        p.window = c.window, p.sinks = c.sinks;
        p.grid[0] = c.step_dev ? attn_live_bound(c.max_seq_len, c.window, c.sinks, p.chunk) : attn_live_chunks(c.step, c.window, c.sinks, p.chunk).total;
    }
    p.head_sink = c.head_sink;
    p.qk_norm = c.qk_norm;
    p.max_splits_ws = (c.max_seq_len + attn_min_chunk() - 1) / attn_min_chunk();
    p.merge = p.grid[0] > 1 && !c.tickets;
    p.merge_grid[0] = c.head_num, p.merge_grid[1] = c.batch;
    p.merge_block = p.hs < 64 ? 64 : p.hs;
    p.workspace_bytes = need;
    return p;
}

DecodeAttnPlan plan_decode_attn(const DecodeAttnCall &c) {
    if (c.ragged && !c.step_dev) return attn_refusal(DAREF_RAGGED_LENGTHS);
    if (c.out_x32 && (c.batch > 32 || c.dtype != LLMIE_F16)) return attn_refusal(DAREF_X32);
    if (c.paged && (c.max_pages <= 0 || c.num_pages <= 0 || static_cast<long long>(c.max_pages) * KV_PAGE < c.max_seq_len))
        return attn_refusal(DAREF_PAGES);
    if (c.slabs && (c.mis_wh8 || c.mis_wf || c.mis_slab || c.slab_stride_mod4)) return attn_refusal(DAREF_SLAB_ALIGNMENT);
    const int rep = c.head_num / c.kv_head_num;
    const bool aligned = !(c.mis_qkv | c.mis_k | c.mis_v | c.mis_bias);
    const size_t need = llmie_decoder_mha_workspace_bytes(c.batch, c.head_num, c.head_size, c.max_seq_len);
    const bool ws_ok = c.workspace && c.workspace_bytes >= need;
    // a window runs on the split kernel's windowed instantiations only: fp16 activations, head size 64 / 128 (ratios as below)
    if (c.window > 0 && (c.dtype != LLMIE_F16 || (c.head_size != 64 && c.head_size != 128))) return attn_refusal(DAREF_WINDOW);
    // ... and so does a head sink: the SINK instantiations exist where the windowed ones do
    if (c.head_sink && (c.dtype != LLMIE_F16 || (c.head_size != 64 && c.head_size != 128))) return attn_refusal(DAREF_HEAD_SINK);
    // QK-norm: the QKN instantiations exist for the same activations and head sizes, without a window or a head sink; the norm runs in
    // front of RoPE and a QKV bias is added behind it here (in front of it in the prefill kernel), so the two together are refused
    if (c.qk_norm && (c.dtype != LLMIE_F16 || (c.head_size != 64 && c.head_size != 128) || c.bias || c.window > 0 || c.head_sink))
        return attn_refusal(DAREF_QK_NORM);
    if (c.kv_e4m3) {
        // fp16 activations over e4m3 cache bytes: 16 cache elements per 16-byte load (8 lanes per token row at head size 128,
        // 256-token chunks); head ratio 8 does not fit registers (16 dims per lane x 8 heads); no generic form, and one refusal
        // for everything -- a short workspace included, which the native cache answers with LLMIE_ERR_WORKSPACE
        if (c.dtype != LLMIE_F16 || c.tickets) return attn_refusal(DAREF_E4M3_FORM);
        if (!aligned || !ws_ok || c.batch > 65535 || !c.scales_positive || (rep != 1 && rep != 2 && rep != 4) ||
            (c.head_size != 128 && c.head_size != 64))
            return attn_refusal(DAREF_E4M3, need);
        return plan_attn_split(c, need);
    }
    // an unaligned call or one past the grid's y / z range has no split form: it runs on the generic kernel unless it asked for
    // something only the split kernel does
    const bool geometry = attn_fused_geometry(c);
    if (aligned && c.batch <= 65535 && c.kv_head_num <= 65535 && geometry)
        return ws_ok ? plan_attn_split(c, need) : attn_refusal(DAREF_WORKSPACE, need);
    if (c.window > 0) return attn_refusal(DAREF_WINDOW);   // the generic kernel attends to everything
    if (c.head_sink) return attn_refusal(DAREF_HEAD_SINK);   // ... and normalises over the real keys only
    if (c.qk_norm) return attn_refusal(DAREF_QK_NORM);       // ... and reads q and k as the projection left them
    if (c.paged) return attn_refusal(DAREF_PAGED_GEOMETRY);
    if (c.slabs) return attn_refusal(DAREF_SLABS_GEOMETRY);
    // (tickets on a supported geometry that fell through -- unaligned -- are ignored: the generic kernel has no partials)
    if (c.rope || (c.tickets && !geometry)) return attn_refusal(DAREF_ROPE_GEOMETRY);
    if (c.ragged || c.out_x32) return attn_refusal(DAREF_RAGGED_GEOMETRY);
    DecodeAttnPlan p{};
    p.lds_bytes = sizeof(float) * static_cast<size_t>(c.step_dev ? c.max_seq_len : c.step);   // the logits of one (sequence, head)
    if (p.lds_bytes > 60 * 1024) return attn_refusal(DAREF_GENERIC_SPAN);
    p.kind = DA_GENERIC, p.grid[0] = c.head_num, p.grid[1] = c.batch, p.grid[2] = 1;
    return p;
}

int decode_attn_refuse(const DecodeAttnCall &c, const DecodeAttnPlan &p) {
    const char *fused = "head_size in {32,64,128,256} and head_num/kv_head_num in {1,2,4,8}";
    switch (p.refusal) {
        case DAREF_RAGGED_LENGTHS: set_error("decoder_mha: a ragged batch needs the device array of context lengths"); return LLMIE_ERR_INVALID_ARG;
        case DAREF_X32: set_error("decoder_mha: the x32 output image holds at most 32 fp16 rows"); break;
        case DAREF_PAGES: set_error("decoder_mha: paged KV cache needs max_pages * %d >= max_seq_len and num_pages > 0", KV_PAGE); break;
        case DAREF_SLAB_ALIGNMENT: set_error("decoder_mha: q/k/v from split-K slabs needs 16-byte aligned slabs and aligned scale vectors"); break;
        case DAREF_E4M3_FORM: set_error("decoder_mha(fp8 KV): fp16 activations, separate merge kernel only"); break;
        case DAREF_E4M3:
            set_error("decoder_mha(fp8 KV): needs head_size 64/128, head ratio 1/2/4, 16-byte aligned buffers, positive scales and "
                      "the llmie_decoder_mha workspace");
            break;
        case DAREF_WORKSPACE:
            set_error("decoder_mha: workspace too small (%zu < %zu bytes)", c.workspace_bytes, p.workspace_bytes);
            return LLMIE_ERR_WORKSPACE;
        case DAREF_PAGED_GEOMETRY: set_error("decoder_mha: the paged KV cache needs %s", fused); break;
        case DAREF_SLABS_GEOMETRY: set_error("decoder_mha: q/k/v from split-K slabs needs %s", fused); break;
        case DAREF_ROPE_GEOMETRY: set_error("decoder_mha: fused RoPE / in-launch merge need %s", fused); break;
        case DAREF_RAGGED_GEOMETRY: set_error("decoder_mha: ragged batches / x32 output need %s", fused); break;
        case DAREF_WINDOW:
            set_error("decoder_mha: a sliding window needs fp16 activations, head_size 64/128, head_num/kv_head_num in {1,2,4,8} (e4m3 cache: "
                      "{1,2,4}) and 16-byte aligned buffers (head_size=%d, rep=%d)", c.head_size, c.head_num / c.kv_head_num);
            break;
        case DAREF_HEAD_SINK:
            set_error("decoder_mha: a head sink needs fp16 activations, head_size 64/128, head_num/kv_head_num in {1,2,4,8} (e4m3 cache: "
                      "{1,2,4}) and 16-byte aligned buffers (head_size=%d, rep=%d)", c.head_size, c.head_num / c.kv_head_num);
            break;
        case DAREF_QK_NORM:
            set_error("decoder_mha: QK-norm needs fp16 activations, head_size 64/128, head_num/kv_head_num in {1,2,4,8} (e4m3 cache: {1,2,4}), "
                      "16-byte aligned buffers, and no QKV bias, window or head sink (head_size=%d, rep=%d)", c.head_size, c.head_num / c.kv_head_num);
            break;
        case DAREF_GENERIC_SPAN:
            set_error("decoder_mha: generic path supports at most 15360 tokens (head_size=%d, rep=%d)", c.head_size, c.head_num / c.kv_head_num);
            break;
        default: set_error("decoder_mha: refused"); break;
    }
    return LLMIE_ERR_UNSUPPORTED;
}

// ---- the launcher: what the kernels read, built once per call ----
struct DecodeAttnArgs {
    const void *qkv, *bias;
    void *kc, *vc, *out;   // kc / vc: this layer's cache (or page pool)
    float *part;
    int head_num, kv_head_num, head_size, max_seq_len, step;
    const int32_t *step_dev;
    const float2 *rope;
    int rot_dim;
    int32_t *tickets;
    QkvSlabs qs;
    KvScale ks;
    PagedKv pg;
    const float *head_sink;   // [head_num] fp32 of this layer, or null
    const void *q_gamma, *k_gamma;   // QK-norm: [head_size] each in the activation type, of this layer, or both null
    float qk_eps;
};

template <typename T, int HS, int REP, typename KT> static void launch_split(const DecodeAttnPlan &p, const DecodeAttnArgs &a, hipStream_t st) {
    // the windowed instantiations: fp16 activations, head size 64 / 128 (what plan_decode_attn plans with a window)
    if constexpr (std::is_same<T, half_t>::value && (HS == 64 || HS == 128)) {
        if (p.qk_norm) {   // the QKN instantiations (no window, no head sink: plan_decode_attn); the merge launch is the plain one
            decode_attn_split_kernel<T, HS, REP, 4, 8, KT, false, false, true, const T *, const T *, float>
                <<<dim3(p.grid[0], p.grid[1], p.grid[2]), 4 * 64, 0, st>>>(
                    static_cast<const T *>(a.qkv), static_cast<const T *>(a.bias), static_cast<KT *>(a.kc), static_cast<KT *>(a.vc), a.part,
                    static_cast<T *>(a.out), a.head_num, a.kv_head_num, a.max_seq_len, a.step, a.step_dev, p.max_splits_ws, a.rope, a.rot_dim,
                    a.tickets, a.qs, a.ks.k, a.ks.v, a.pg, p.cpw, static_cast<const T *>(a.q_gamma), static_cast<const T *>(a.k_gamma), a.qk_eps);
            if (p.merge)
                decode_attn_combine_kernel<T><<<dim3(p.merge_grid[0], p.merge_grid[1]), p.merge_block, 0, st>>>(
                    a.part, static_cast<T *>(a.out), a.head_num, HS, p.chunk, a.step, a.step_dev, p.max_splits_ws, a.pg.step_stride,
                    a.max_seq_len, a.pg.out_x32);
            return;
        }
        if (p.head_sink) {   // the SINK instantiations, windowed or not: the same launches with the head-sink array as last argument
            auto run = [&](auto win_c, auto... ex) {
                constexpr bool W = decltype(win_c)::value;
                decode_attn_split_kernel<T, HS, REP, 4, 8, KT, W, true, false, decltype(ex)...><<<dim3(p.grid[0], p.grid[1], p.grid[2]), 4 * 64, 0, st>>>(
                    static_cast<const T *>(a.qkv), static_cast<const T *>(a.bias), static_cast<KT *>(a.kc), static_cast<KT *>(a.vc), a.part,
                    static_cast<T *>(a.out), a.head_num, a.kv_head_num, a.max_seq_len, a.step, a.step_dev, p.max_splits_ws, a.rope, a.rot_dim,
                    a.tickets, a.qs, a.ks.k, a.ks.v, a.pg, p.cpw, ex...);
                if (p.merge)
                    decode_attn_combine_kernel<T, W, true, decltype(ex)...><<<dim3(p.merge_grid[0], p.merge_grid[1]), p.merge_block, 0, st>>>(
                        a.part, static_cast<T *>(a.out), a.head_num, HS, p.chunk, a.step, a.step_dev, p.max_splits_ws, a.pg.step_stride,
                        a.max_seq_len, a.pg.out_x32, ex...);
            };
            if (p.window > 0) run(std::true_type{}, p.window, p.sinks, a.head_sink);
            else run(std::false_type{}, a.head_sink);
            return;
        }
        if (p.window > 0) {
            decode_attn_split_kernel<T, HS, REP, 4, 8, KT, true, false, false, int, int><<<dim3(p.grid[0], p.grid[1], p.grid[2]), 4 * 64, 0, st>>>(
                static_cast<const T *>(a.qkv), static_cast<const T *>(a.bias), static_cast<KT *>(a.kc), static_cast<KT *>(a.vc), a.part,
                static_cast<T *>(a.out), a.head_num, a.kv_head_num, a.max_seq_len, a.step, a.step_dev, p.max_splits_ws, a.rope, a.rot_dim,
                a.tickets, a.qs, a.ks.k, a.ks.v, a.pg, p.cpw, p.window, p.sinks);
            if (p.merge)
                decode_attn_combine_kernel<T, true, false, int, int><<<dim3(p.merge_grid[0], p.merge_grid[1]), p.merge_block, 0, st>>>(
                    a.part, static_cast<T *>(a.out), a.head_num, HS, p.chunk, a.step, a.step_dev, p.max_splits_ws, a.pg.step_stride,
                    a.max_seq_len, a.pg.out_x32, p.window, p.sinks);
            return;
        }
    }
    decode_attn_split_kernel<T, HS, REP, 4, 8, KT><<<dim3(p.grid[0], p.grid[1], p.grid[2]), 4 * 64, 0, st>>>(
        static_cast<const T *>(a.qkv), static_cast<const T *>(a.bias), static_cast<KT *>(a.kc), static_cast<KT *>(a.vc), a.part,
        static_cast<T *>(a.out), a.head_num, a.kv_head_num, a.max_seq_len, a.step, a.step_dev, p.max_splits_ws, a.rope, a.rot_dim, a.tickets,
        a.qs, a.ks.k, a.ks.v, a.pg, p.cpw);
    if (p.merge)
        decode_attn_combine_kernel<T><<<dim3(p.merge_grid[0], p.merge_grid[1]), p.merge_block, 0, st>>>(
            a.part, static_cast<T *>(a.out), a.head_num, HS, p.chunk, a.step, a.step_dev, p.max_splits_ws, a.pg.step_stride, a.max_seq_len,
            a.pg.out_x32);
}
template <typename T> static void launch_generic(const DecodeAttnPlan &p, const DecodeAttnArgs &a, hipStream_t st) {
    decode_attn_generic_kernel<T><<<dim3(p.grid[0], p.grid[1]), 256, p.lds_bytes, st>>>(
        static_cast<const T *>(a.qkv), static_cast<const T *>(a.bias), static_cast<T *>(a.kc), static_cast<T *>(a.vc), static_cast<T *>(a.out),
        a.head_num, a.kv_head_num, a.head_size, a.max_seq_len, a.step, a.step_dev);
}
// every instantiation of the split kernel: head sizes 32 / 64 / 128 / 256 x head ratios 1 / 2 / 4 / 8 over the native cache, head
// sizes 64 / 128 x ratios 1 / 2 / 4 over e4m3 bytes (the planner plans nothing else)
template <typename T, int HS, typename KT> static void launch_split_rep(const DecodeAttnPlan &p, const DecodeAttnArgs &a, hipStream_t st) {
    switch (p.rep) {
        case 1: return launch_split<T, HS, 1, KT>(p, a, st);
        case 2: return launch_split<T, HS, 2, KT>(p, a, st);
        case 4: return launch_split<T, HS, 4, KT>(p, a, st);
        case 8:
            if constexpr (std::is_same<KT, T>::value) return launch_split<T, HS, 8, KT>(p, a, st);
    }
}
template <typename T, typename KT> static void launch_split_hs(const DecodeAttnPlan &p, const DecodeAttnArgs &a, hipStream_t st) {
    switch (p.hs) {
        case 128: return launch_split_rep<T, 128, KT>(p, a, st);
        case 64: return launch_split_rep<T, 64, KT>(p, a, st);
        case 32:
            if constexpr (std::is_same<KT, T>::value) return launch_split_rep<T, 32, KT>(p, a, st);
            break;
        case 256:
            if constexpr (std::is_same<KT, T>::value) return launch_split_rep<T, 256, KT>(p, a, st);
            break;
    }
}
static int launch_decode_attn(const DecodeAttnCall &c, const DecodeAttnPlan &p, const DecodeAttnArgs &a, hipStream_t st) {
    const bool split = p.kind == DA_SPLIT;
    if (p.e4m3) launch_split_hs<half_t, fp8kv_t>(p, a, st);
    else if (c.dtype == LLMIE_F32) split ? launch_split_hs<float, float>(p, a, st) : launch_generic<float>(p, a, st);
    else split ? launch_split_hs<half_t, half_t>(p, a, st) : launch_generic<half_t>(p, a, st);
    return launch_status(p.e4m3 ? "decoder_mha(fp8 KV)" : "decoder_mha");
}

// elements in front of `layer` in a dense cache or a page pool
static size_t kv_layer_offset(const DecodeAttnShape &g, const KvView &kv, int layer) {
    return kv.block_table ? static_cast<size_t>(layer) * kv.num_pages * g.kv_head_num * KV_PAGE * g.head_size
                          : static_cast<size_t>(layer) * g.batch * g.kv_head_num * g.max_seq_len * g.head_size;
}
static DecodeAttnArgs decode_attn_args(const DecodeAttnShape &g, const DecodeAttnIo &io, const KvView &kv, const DecodePos &pos, int layer) {
    const size_t elem = kv.fp8 ? 1 : (g.dtype == LLMIE_F32 ? sizeof(float) : sizeof(half_t));
    const size_t layer_bytes = kv_layer_offset(g, kv, layer) * elem;
    QkvSlabs qs{nullptr, 0, 0, SlabScale{nullptr, nullptr, nullptr}};
    if (io.qkv_slabs)
        qs = QkvSlabs{io.qkv_slabs->slab, io.qkv_slabs->KS, static_cast<size_t>(io.qkv_slabs->M) * io.qkv_slabs->N,
                      io.qkv_scale ? *io.qkv_scale : SlabScale{nullptr, nullptr, nullptr}};
    return DecodeAttnArgs{io.qkv, io.qkv_bias, static_cast<char *>(kv.k) + layer_bytes, static_cast<char *>(kv.v) + layer_bytes, io.out,
                          static_cast<float *>(io.workspace), g.head_num, g.kv_head_num, g.head_size, g.max_seq_len, pos.step, pos.step_dev,
                          io.rope, io.rot_dim, io.tickets, qs, KvScale{kv.k_scale, kv.v_scale},
                          PagedKv{kv.block_table, kv.max_pages, pos.ragged ? 1 : 0, io.out_x32 ? 1 : 0}, io.head_sink, io.q_gamma, io.k_gamma,
                          io.qk_eps};
}
static DecodeAttnCall decode_attn_call(const DecodeAttnShape &g, const DecodeAttnIo &io, const KvView &kv, const DecodePos &pos,
                                       const DecodeAttnArgs &a) {
    DecodeAttnCall c{};
    c.dtype = g.dtype, c.kv_e4m3 = kv.fp8 != 0, c.scales_positive = kv.k_scale > 0.f && kv.v_scale > 0.f;
    c.head_size = g.head_size, c.head_num = g.head_num, c.kv_head_num = g.kv_head_num, c.batch = g.batch, c.max_seq_len = g.max_seq_len;
    c.step = pos.step, c.step_dev = pos.step_dev != nullptr, c.ragged = pos.ragged != 0;
    c.bias = io.qkv_bias != nullptr, c.rope = io.rope != nullptr, c.tickets = io.tickets != nullptr, c.slabs = io.qkv_slabs != nullptr;
    c.paged = kv.block_table != nullptr, c.out_x32 = io.out_x32 != 0, c.max_pages = kv.max_pages, c.num_pages = kv.num_pages;
    c.mis_qkv = mis16(a.qkv), c.mis_bias = mis16(a.bias), c.mis_k = mis16(a.kc), c.mis_v = mis16(a.vc);
    if (c.slabs) {
        c.mis_slab = mis16(a.qs.slab), c.mis_wf = mis16(a.qs.sc.wf), c.mis_wh8 = mis16(a.qs.sc.wh) % 8;
        c.slab_stride_mod4 = static_cast<unsigned>(a.qs.stride % 4);
    }
    c.workspace = io.workspace != nullptr, c.workspace_bytes = io.workspace_bytes;
    c.window = io.window > 0 ? io.window : 0, c.sinks = io.window > 0 ? io.sinks : 0;
    c.head_sink = io.head_sink != nullptr;
    c.qk_norm = io.q_gamma != nullptr;
    return c;
}

int decoder_mha_rope(const DecodeAttnShape &g, const DecodeAttnIo &io, const KvView &kv, const DecodePos &pos, int layer, hipStream_t st) {
    const DecodeAttnArgs a = decode_attn_args(g, io, kv, pos, layer);
    const DecodeAttnCall c = decode_attn_call(g, io, kv, pos, a);
    const DecodeAttnPlan p = plan_decode_attn(c);
    if (p.kind == DA_REFUSED) return decode_attn_refuse(c, p);
    return launch_decode_attn(c, p, a, st);
}

// the argument checks of every entry, in front of the plan
static int decode_attn_validate(const char *who, const DecodeAttnShape &g, const DecodePos &pos, bool pointers, int layer, bool rope, int rot_dim) {
    LLMIE_REQUIRE(pointers && (!pos.ragged || pos.step_dev), "%s: NULL pointer", who);
    LLMIE_REQUIRE(layer >= 0 && g.batch > 0 && g.head_num > 0 && g.kv_head_num > 0 && g.head_size > 0 && g.max_seq_len > 0, "%s: bad shape", who);
    LLMIE_REQUIRE(g.head_num % g.kv_head_num == 0, "%s: kv_head_num must divide head_num", who);
    LLMIE_REQUIRE(pos.step_dev || (pos.step >= 1 && pos.step <= g.max_seq_len), "%s: step %d outside [1, max_seq_len=%d]", who, pos.step,
                  g.max_seq_len);
    LLMIE_REQUIRE(!rope || (rot_dim > 0 && rot_dim % 2 == 0), "%s: bad rotary_dim", who);
    if (g.dtype != LLMIE_F32 && g.dtype != LLMIE_F16) LLMIE_UNSUPPORTED("%s: dtype %d", who, (int)g.dtype);
    return LLMIE_OK;
}
// the window of a call: window >= 0 (0 = full attention: the sinks are then ignored), sinks >= 0
static int decode_attn_validate_window(const char *who, int window, int sinks) {
    LLMIE_REQUIRE(window >= 0 && sinks >= 0, "%s: window %d / sinks %d must not be negative", who, window, sinks);
    return LLMIE_OK;
}
// a public entry: validate, then as the engine's calls
static int decode_attn_entry(const char *who, const DecodeAttnShape &g, const DecodeAttnIo &io, const KvView &kv, const DecodePos &pos, int layer,
                             llmie_stream stream) {
    const int rc = decode_attn_validate(who, g, pos, io.qkv && kv.k && kv.v && io.out, layer, io.rope != nullptr, io.rot_dim);
    return rc != LLMIE_OK ? rc : decoder_mha_rope(g, io, kv, pos, layer, as_stream(stream));
}

// "split f16 hs128 rep4 kv=e4m3 cpw2 chunk512 grid 4x8x16 merge 32x16/128" (merge: grid / block, "in-launch" by tickets, "none"
// for one split) or "generic f16 grid 32x2 lds 1028"; a window adds " window 4096 sinks 4 live <=34"
static void decode_attn_plan_text(const DecodeAttnCall &c, const DecodeAttnPlan &p, char *text, size_t n) {
    const char *dt = c.dtype == LLMIE_F32 ? "f32" : "f16";
    if (p.kind == DA_GENERIC) {
        snprintf(text, n, "generic %s grid %dx%d lds %zu", dt, p.grid[0], p.grid[1], p.lds_bytes);
        return;
    }
    const int k = snprintf(text, n, "split %s hs%d rep%d kv=%s cpw%d chunk%d grid %dx%dx%d merge ", dt, p.hs, p.rep, p.e4m3 ? "e4m3" : dt, p.cpw,
                           p.chunk, p.grid[0], p.grid[1], p.grid[2]);
    int m;
    if (p.merge) m = snprintf(text + k, n - k, "%dx%d/%d", p.merge_grid[0], p.merge_grid[1], p.merge_block);
    else m = snprintf(text + k, n - k, "%s", p.grid[0] > 1 ? "in-launch" : "none");
    // a windowed call (no window: the line above, unchanged): the mask and what grid x counts -- the live spans of the host step, or
    // their bound for any position
    int w = 0;
    if (p.window > 0) w = snprintf(text + k + m, n - k - m, " window %d sinks %d live %s%d", p.window, p.sinks, c.step_dev ? "<=" : "", p.grid[0]);
    int s = 0;
    if (p.head_sink) s = snprintf(text + k + m + w, n - k - m - w, " head_sink");   // the SINK instantiation of the same launches
    if (p.qk_norm) snprintf(text + k + m + w + s, n - k - m - w - s, " qk_norm");   // the QKN instantiation of the split kernel
}

// The page ring of a windowed sequence (llmie_kv_window_advance): one thread per sequence.  The logical pages the positions
// [cached, cached + n) need and that are unmapped (-1) take the pool pages of the lowest mapped logical pages that lie wholly at or
// above the sink pages and wholly below cached + 1 - window (dead for this and every later query); all of them or none.
__global__ __launch_bounds__(64) void kv_window_advance_kernel(int32_t *__restrict__ table, int max_pages, const int32_t *__restrict__ cached_len,
                                                               const int32_t *__restrict__ new_tokens, int batch, int window, int sinks,
                                                               int32_t *__restrict__ status) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    int32_t *row = table + static_cast<size_t>(b) * max_pages;
    const int cached = cached_len[b], n = new_tokens ? new_tokens[b] : 1;
    if (n <= 0) {
        status[b] = 0;
        return;
    }
    if (cached < 0 || static_cast<long long>(cached) + n > static_cast<long long>(max_pages) * KV_PAGE) {
        status[b] = 2;   // the positions do not fit the table row
        return;
    }
    const int p0 = cached / KV_PAGE, p1 = (cached + n - 1) / KV_PAGE;
    const int lo = min((sinks + KV_PAGE - 1) / KV_PAGE, max_pages);                  // first page without a sink token
    const long long dead_end = static_cast<long long>(cached) + 1 - window;         // tokens below are dead
    const int hi = dead_end > 0 ? static_cast<int>(min(static_cast<long long>(p0), dead_end / KV_PAGE)) : 0;   // pages [lo, hi) are dead
    int need = 0, have = 0;
    for (int p = p0; p <= p1; ++p) need += row[p] < 0;
    for (int p = lo; p < hi; ++p) have += row[p] >= 0;
    if (have < need) {
        status[b] = 1;   // the caller must supply a page; the row is as it was
        return;
    }
    int d = lo;
    for (int p = p0; p <= p1; ++p) {
        if (row[p] >= 0) continue;
        while (row[d] < 0) ++d;   // (have >= need: stops below hi)
        row[p] = row[d];
        row[d] = -1;
        ++d;
    }
    status[b] = 0;
}

}  // namespace llmie

using namespace llmie;

extern "C" size_t llmie_decoder_mha_workspace_bytes(int batch, int head_num, int head_size, int max_seq_len) {
    if (batch <= 0 || head_num <= 0 || head_size <= 0 || max_seq_len <= 0) return 0;
    const size_t splits = (static_cast<size_t>(max_seq_len) + attn_min_chunk() - 1) / attn_min_chunk();
    return static_cast<size_t>(batch) * head_num * splits * (head_size + 2) * sizeof(float);
}

extern "C" int llmie_decoder_mha(const void *qkv, const void *qkv_bias, void *k_cache, void *v_cache, void *out,
                                 int layer, int batch, int head_num, int kv_head_num, int head_size,
                                 int max_seq_len, int step, const int32_t *step_dev, void *workspace,
                                 size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream) {
    return decode_attn_entry("decoder_mha", DecodeAttnShape{batch, head_num, kv_head_num, head_size, max_seq_len, dtype},
                             DecodeAttnIo{qkv, qkv_bias, out, workspace, workspace_bytes, nullptr, 0, nullptr, nullptr, nullptr, 0},
                             kv_dense(k_cache, v_cache), DecodePos{step, step_dev, 0}, layer, stream);
}

extern "C" int llmie_decoder_mha_rope(const void *qkv, const void *qkv_bias, void *k_cache, void *v_cache, void *out,
                                      int layer, int batch, int head_num, int kv_head_num, int head_size,
                                      int max_seq_len, int step, const int32_t *step_dev, void *workspace,
                                      size_t workspace_bytes, const void *rope_table, int rotary_dim, int32_t *tickets,
                                      llmie_dtype dtype, llmie_stream stream) {
    return decode_attn_entry("decoder_mha_rope", DecodeAttnShape{batch, head_num, kv_head_num, head_size, max_seq_len, dtype},
                             DecodeAttnIo{qkv, qkv_bias, out, workspace, workspace_bytes, static_cast<const float2 *>(rope_table), rotary_dim,
                                          tickets, nullptr, nullptr, 0},
                             kv_dense(k_cache, v_cache), DecodePos{step, step_dev, 0}, layer, stream);
}

// Ragged batch: RoPE position, append slot and attention span per sequence (ctx_len_dev[b] includes this step's token);
// block_table != NULL: paged cache pools.  Same kernels as llmie_decoder_mha_rope.
extern "C" int llmie_decoder_mha_ragged(const void *qkv, const void *qkv_bias, void *k_cache, void *v_cache, void *out, int layer,
                                        int batch, int head_num, int kv_head_num, int head_size, int max_seq_len,
                                        const int32_t *ctx_len_dev, void *workspace, size_t workspace_bytes, const void *rope_table,
                                        int rotary_dim, const int32_t *block_table, int max_pages, int num_pages,
                                        llmie_dtype dtype, llmie_stream stream) {
    return decode_attn_entry("decoder_mha_ragged", DecodeAttnShape{batch, head_num, kv_head_num, head_size, max_seq_len, dtype},
                             DecodeAttnIo{qkv, qkv_bias, out, workspace, workspace_bytes, static_cast<const float2 *>(rope_table), rotary_dim,
                                          nullptr, nullptr, nullptr, 0},
                             KvView{k_cache, v_cache, block_table, max_pages, num_pages, 0, 1.f, 1.f}, DecodePos{-1, ctx_len_dev, 1}, layer,
                             stream);
}

static const char *decode_attn_plan_query(const char *who, llmie_dtype dtype, int kv_e4m3, int batch, int head_num, int kv_head_num, int head_size,
                                          int max_seq_len, int step, unsigned forms, int max_pages, int num_pages,
                                          unsigned long long residues, long long workspace_bytes, int window, int sinks, int *status) {
    static thread_local char text[160];
    static const int32_t some_position = 0;   // stands for the device position: never read
    auto res = [&](int i) { return static_cast<unsigned>((residues >> (4 * i)) & 15u); };
    const DecodeAttnShape g{batch, head_num, kv_head_num, head_size, max_seq_len, dtype};
    const DecodePos pos{step, (forms & LLMIE_ATTN_STEP_DEV) ? &some_position : nullptr, (forms & LLMIE_ATTN_RAGGED) != 0};
    int rc = decode_attn_validate(who, g, pos, true, 0, (forms & LLMIE_ATTN_ROPE) != 0, 2);
    if (rc == LLMIE_OK) rc = decode_attn_validate_window(who, window, sinks);
    if (rc == LLMIE_OK) {
        DecodeAttnCall c{};
        c.dtype = dtype, c.kv_e4m3 = kv_e4m3 != 0, c.scales_positive = !(forms & LLMIE_ATTN_BAD_SCALES);
        c.head_size = head_size, c.head_num = head_num, c.kv_head_num = kv_head_num, c.batch = batch, c.max_seq_len = max_seq_len;
        c.step = step, c.step_dev = pos.step_dev != nullptr, c.ragged = pos.ragged != 0;
        c.bias = (forms & LLMIE_ATTN_BIAS) != 0, c.rope = (forms & LLMIE_ATTN_ROPE) != 0, c.tickets = (forms & LLMIE_ATTN_TICKETS) != 0;
        c.slabs = (forms & LLMIE_ATTN_SLABS) != 0, c.paged = (forms & LLMIE_ATTN_PAGED) != 0, c.out_x32 = (forms & LLMIE_ATTN_X32) != 0;
        c.max_pages = max_pages, c.num_pages = num_pages;
        c.mis_qkv = res(0), c.mis_bias = c.bias ? res(1) : 0, c.mis_k = res(2), c.mis_v = res(3);
        if (c.slabs) c.mis_slab = res(4), c.mis_wf = res(5), c.mis_wh8 = res(6) % 8, c.slab_stride_mod4 = res(7) % 4;
        c.workspace = workspace_bytes >= 0, c.workspace_bytes = c.workspace ? static_cast<size_t>(workspace_bytes) : 0;
        c.window = window, c.sinks = window > 0 ? sinks : 0;
        c.head_sink = (forms & LLMIE_ATTN_HEAD_SINK) != 0;
        c.qk_norm = (forms & LLMIE_ATTN_QK_NORM) != 0;
        const DecodeAttnPlan p = plan_decode_attn(c);
        if (p.kind == DA_REFUSED) rc = decode_attn_refuse(c, p);
        else decode_attn_plan_text(c, p, text, sizeof(text));
    }
    if (status) *status = rc;
    return rc == LLMIE_OK ? text : nullptr;
}

extern "C" const char *llmie_decoder_mha_plan(llmie_dtype dtype, int kv_e4m3, int batch, int head_num, int kv_head_num, int head_size,
                                              int max_seq_len, int step, unsigned forms, int max_pages, int num_pages,
                                              unsigned long long residues, long long workspace_bytes, int *status) {
    return decode_attn_plan_query("decoder_mha_plan", dtype, kv_e4m3, batch, head_num, kv_head_num, head_size, max_seq_len, step,
                                  forms & ~(LLMIE_ATTN_HEAD_SINK | LLMIE_ATTN_QK_NORM),
                                  max_pages, num_pages, residues, workspace_bytes, 0, 0, status);
}

extern "C" const char *llmie_decoder_mha_window_plan(llmie_dtype dtype, int kv_e4m3, int batch, int head_num, int kv_head_num, int head_size,
                                                     int max_seq_len, int step, unsigned forms, int max_pages, int num_pages,
                                                     unsigned long long residues, long long workspace_bytes, int window, int sinks,
                                                     int *status) {
    return decode_attn_plan_query("decoder_mha_window_plan", dtype, kv_e4m3, batch, head_num, kv_head_num, head_size, max_seq_len, step,
                                  forms & ~(LLMIE_ATTN_HEAD_SINK | LLMIE_ATTN_QK_NORM), max_pages, num_pages, residues, workspace_bytes, window,
                                  sinks, status);
}

// Sliding-window decode attention on the operands of llmie_decoder_mha_ragged (+ tickets and the e4m3 cache, which the engine's calls
// use): the windowed split kernel without an engine around it.  window = 0: full attention, the call llmie_decoder_mha_ragged makes.
extern "C" int llmie_decoder_mha_window(const void *qkv, const void *qkv_bias, void *k_cache, void *v_cache, void *out, int layer,
                                        int batch, int head_num, int kv_head_num, int head_size, int max_seq_len,
                                        const int32_t *ctx_len_dev, void *workspace, size_t workspace_bytes, const void *rope_table,
                                        int rotary_dim, const int32_t *block_table, int max_pages, int num_pages, int window, int sinks,
                                        int32_t *tickets, int kv_e4m3, float k_scale, float v_scale, llmie_dtype dtype,
                                        llmie_stream stream) {
    const int rc = decode_attn_validate_window("decoder_mha_window", window, sinks);
    if (rc != LLMIE_OK) return rc;
    return decode_attn_entry("decoder_mha_window", DecodeAttnShape{batch, head_num, kv_head_num, head_size, max_seq_len, dtype},
                             DecodeAttnIo{qkv, qkv_bias, out, workspace, workspace_bytes, static_cast<const float2 *>(rope_table), rotary_dim,
                                          tickets, nullptr, nullptr, 0, window, sinks},
                             KvView{k_cache, v_cache, block_table, max_pages, num_pages, kv_e4m3 ? 1 : 0, kv_e4m3 ? k_scale : 1.f,
                                    kv_e4m3 ? v_scale : 1.f},
                             DecodePos{-1, ctx_len_dev, 1}, layer, stream);
}

// llmie_decoder_mha_window plus the learned per-head sink logit (head_sink: device fp32 [head_num], nullable = that entry's call)
extern "C" int llmie_decoder_mha_sink(const void *qkv, const void *qkv_bias, void *k_cache, void *v_cache, void *out, int layer, int batch,
                                      int head_num, int kv_head_num, int head_size, int max_seq_len, const int32_t *ctx_len_dev,
                                      void *workspace, size_t workspace_bytes, const void *rope_table, int rotary_dim,
                                      const int32_t *block_table, int max_pages, int num_pages, int window, int sinks, int32_t *tickets,
                                      int kv_e4m3, float k_scale, float v_scale, const float *head_sink, llmie_dtype dtype,
                                      llmie_stream stream) {
    const int rc = decode_attn_validate_window("decoder_mha_sink", window, sinks);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(reinterpret_cast<uintptr_t>(head_sink) % sizeof(float) == 0, "decoder_mha_sink: head_sink must be 4-byte aligned");
    return decode_attn_entry("decoder_mha_sink", DecodeAttnShape{batch, head_num, kv_head_num, head_size, max_seq_len, dtype},
                             DecodeAttnIo{qkv, qkv_bias, out, workspace, workspace_bytes, static_cast<const float2 *>(rope_table), rotary_dim,
                                          tickets, nullptr, nullptr, 0, window, sinks, head_sink},
                             KvView{k_cache, v_cache, block_table, max_pages, num_pages, kv_e4m3 ? 1 : 0, kv_e4m3 ? k_scale : 1.f,
                                    kv_e4m3 ? v_scale : 1.f},
                             DecodePos{-1, ctx_len_dev, 1}, layer, stream);
}

extern "C" const char *llmie_decoder_mha_sink_plan(llmie_dtype dtype, int kv_e4m3, int batch, int head_num, int kv_head_num, int head_size,
                                                   int max_seq_len, int step, unsigned forms, int max_pages, int num_pages,
                                                   unsigned long long residues, long long workspace_bytes, int window, int sinks,
                                                   int *status) {
    return decode_attn_plan_query("decoder_mha_sink_plan", dtype, kv_e4m3, batch, head_num, kv_head_num, head_size, max_seq_len, step,
                                  forms & ~LLMIE_ATTN_QK_NORM, max_pages, num_pages, residues, workspace_bytes, window, sinks, status);
}

// llmie_decoder_mha_sink plus the per-head q/k RMSNorm in front of RoPE (q_gamma / k_gamma: device [head_size] in the activation type,
// both NULL = that entry's call)
extern "C" int llmie_decoder_mha_qknorm(const void *qkv, const void *qkv_bias, void *k_cache, void *v_cache, void *out, int layer, int batch,
                                        int head_num, int kv_head_num, int head_size, int max_seq_len, const int32_t *ctx_len_dev,
                                        void *workspace, size_t workspace_bytes, const void *rope_table, int rotary_dim,
                                        const int32_t *block_table, int max_pages, int num_pages, int window, int sinks, int32_t *tickets,
                                        int kv_e4m3, float k_scale, float v_scale, const float *head_sink, const void *q_gamma,
                                        const void *k_gamma, float qk_eps, llmie_dtype dtype, llmie_stream stream) {
    const int rc = decode_attn_validate_window("decoder_mha_qknorm", window, sinks);
    if (rc != LLMIE_OK) return rc;
    LLMIE_REQUIRE(reinterpret_cast<uintptr_t>(head_sink) % sizeof(float) == 0, "decoder_mha_qknorm: head_sink must be 4-byte aligned");
    LLMIE_REQUIRE((q_gamma != nullptr) == (k_gamma != nullptr), "decoder_mha_qknorm: q_gamma and k_gamma go together (one is NULL)");
    if (q_gamma) {
        LLMIE_REQUIRE((reinterpret_cast<uintptr_t>(q_gamma) | reinterpret_cast<uintptr_t>(k_gamma)) % 16 == 0,
                      "decoder_mha_qknorm: the gammas must be 16-byte aligned");
        LLMIE_REQUIRE(qk_eps >= 0.f, "decoder_mha_qknorm: qk_eps must be a number >= 0");
    }
    return decode_attn_entry("decoder_mha_qknorm", DecodeAttnShape{batch, head_num, kv_head_num, head_size, max_seq_len, dtype},
                             DecodeAttnIo{qkv, qkv_bias, out, workspace, workspace_bytes, static_cast<const float2 *>(rope_table), rotary_dim,
                                          tickets, nullptr, nullptr, 0, window, sinks, head_sink, q_gamma, k_gamma, q_gamma ? qk_eps : 0.f},
                             KvView{k_cache, v_cache, block_table, max_pages, num_pages, kv_e4m3 ? 1 : 0, kv_e4m3 ? k_scale : 1.f,
                                    kv_e4m3 ? v_scale : 1.f},
                             DecodePos{-1, ctx_len_dev, 1}, layer, stream);
}

extern "C" const char *llmie_decoder_mha_qknorm_plan(llmie_dtype dtype, int kv_e4m3, int batch, int head_num, int kv_head_num, int head_size,
                                                     int max_seq_len, int step, unsigned forms, int max_pages, int num_pages,
                                                     unsigned long long residues, long long workspace_bytes, int window, int sinks,
                                                     int *status) {
    return decode_attn_plan_query("decoder_mha_qknorm_plan", dtype, kv_e4m3, batch, head_num, kv_head_num, head_size, max_seq_len, step,
                                  forms, max_pages, num_pages, residues, workspace_bytes, window, sinks, status);
}

extern "C" int llmie_kv_window_advance(int32_t *block_table, int max_pages, const int32_t *cached_len, const int32_t *new_tokens, int batch,
                                       int window, int sinks, int32_t *status, llmie_stream stream) {
    LLMIE_REQUIRE(block_table && cached_len && status, "kv_window_advance: NULL pointer");
    LLMIE_REQUIRE(batch > 0 && max_pages > 0, "kv_window_advance: bad shape");
    LLMIE_REQUIRE(static_cast<long long>(max_pages) * KV_PAGE <= INT_MAX, "kv_window_advance: max_pages %d too large", max_pages);
    LLMIE_REQUIRE(window >= 1 && sinks >= 0, "kv_window_advance: needs window >= 1 and sinks >= 0 (window %d, sinks %d)", window, sinks);
    kv_window_advance_kernel<<<(batch + 63) / 64, 64, 0, as_stream(stream)>>>(block_table, max_pages, cached_len, new_tokens, batch, window,
                                                                              sinks, status);
    return launch_status("kv_window_advance");
}
