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
// llmie_ngram_draft, one launch, one 256-thread workgroup per sequence: ONE sweep over the row finds, for every n at once, the
// last place the sequence's final n tokens occurred before.  A thread that sees the final token at q extends the comparison
// backwards (<= 7 more loads, rare); the sweep itself reads 16 bytes per thread where the row is aligned.  "The last place" is an
// integer maximum in LDS: deterministic.
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
    const int r = blockIdx.x, b = r / (k + 1), i = r - b * (k + 1);
    const int step = (step_rows ? step_rows[b] : (step_dev ? *step_dev : step_arg)) + i;
    SpSplicedHistory hist{nullptr, draft_ids + static_cast<size_t>(b) * k, 0, 0};
    if (hstride > 0) {
        const int len0 = history_len[b];
        hist.row = history + static_cast<size_t>(b) * hstride;
        hist.stored = min(max(len0, 0), hstride);
        // (a negative length is never appended to: llmie_sample_logits appends while 0 <= history_len < history_stride)
        hist.len = (happend && len0 >= 0) ? min(hist.stored + i, hstride) : hist.stored;
    }
    const T *lg = logits + static_cast<size_t>(r) * V;
    const SpPick pick = sp_sample_row<T, EXT>(lg, V, params[b], hist, step, end_id, ws + static_cast<size_t>(r) * ws_row, EXT ? &ext : nullptr, b,
                                              r, s);
    if (threadIdx.x == 0) {
        const int chosen = pick.chosen;
        bool fin = chosen == end_id;
        if constexpr (EXT)
            for (int j = 0; j < pick.slen; ++j) fin = fin || pick.stops[j] == chosen;
        SpecPick out;
        out.token = chosen;
        out.logprob = (chosen >= 0 && chosen < V && pick.valid > 0) ? to_f32(lg[chosen]) - (pick.lse_m + logf(pick.lse_s)) : -INFINITY;
        out.fin = fin ? 1 : 0;
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

size_t spec_picks_offset(int rows, int vocab) { return static_cast<size_t>(rows) * sample_logits_ws_row(vocab) * sizeof(uint32_t); }

template <typename T>
void spec_rows_launch(bool ext_active, const void *logits, int rows, int vocab, int k, const llmie_sampling_params *params, const int32_t *history,
                      int hstride, const int32_t *history_len, int happend, const int32_t *draft_ids, const int32_t *step_rows, int step,
                      const int32_t *step_dev, int end_id, uint32_t *ws, SpecPick *picks, const llmie_sampling_ext &ext, hipStream_t st) {
    const size_t ws_row = sample_logits_ws_row(vocab);
    if (ext_active)
        spec_verify_rows_kernel<T, true><<<rows, kSpThreads, 0, st>>>(static_cast<const T *>(logits), vocab, k, params, history, hstride, history_len,
                                                                      happend, draft_ids, step_rows, step, step_dev, end_id, ws, ws_row, picks, ext);
    else
        spec_verify_rows_kernel<T, false><<<rows, kSpThreads, 0, st>>>(static_cast<const T *>(logits), vocab, k, params, history, hstride, history_len,
                                                                       happend, draft_ids, step_rows, step, step_dev, end_id, ws, ws_row, picks, ext);
}

}  // namespace
}  // namespace llmie

using namespace llmie;

extern "C" size_t llmie_spec_verify_workspace_bytes(int batch, int k, int vocab) {
    if (batch <= 0 || k <= 0 || vocab <= 0 || k > LLMIE_SPEC_MAX_DRAFT) return 0;
    const int rows = batch * (k + 1);
    return spec_picks_offset(rows, vocab) + static_cast<size_t>(rows) * sizeof(SpecPick);
}

extern "C" int llmie_spec_verify(const void *logits, int batch, int k, int vocab, const int32_t *draft_ids, const int32_t *draft_len,
                                 const llmie_sampling_params *params_dev, int32_t *history, int history_stride, int32_t *history_len,
                                 int history_append, int32_t *seq_len, uint8_t *finished, int32_t *out_tokens, int32_t *out_count,
                                 float *out_logprob, int32_t *last_token, int32_t *cached_len, int32_t *step_rows, int step,
                                 const int32_t *step_dev, int end_id, void *workspace, size_t workspace_bytes, llmie_dtype dtype,
                                 llmie_stream stream, const llmie_sampling_ext *ext) {
    // the sampler's own checks, under this entry's name (the workspace is this entry's: checked below)
    int rc = sample_logits_check(logits, batch, vocab, params_dev, history, history_stride, history_len, seq_len, finished, out_tokens, nullptr, 0,
                                 dtype, "spec_verify", false);
    if (rc != LLMIE_OK) return rc;
    bool active;
    if ((rc = sample_ext_check(batch, vocab, ext, &active, "spec_verify")) != LLMIE_OK) return rc;
    LLMIE_REQUIRE(k >= 1, "spec_verify: k %d < 1", k);
    LLMIE_REQUIRE(draft_ids && out_tokens && out_count, "spec_verify: NULL draft_ids / out_tokens / out_count");
    if (k > LLMIE_SPEC_MAX_DRAFT) LLMIE_UNSUPPORTED("spec_verify: k %d above LLMIE_SPEC_MAX_DRAFT (%d)", k, LLMIE_SPEC_MAX_DRAFT);
    LLMIE_REQUIRE(static_cast<long long>(batch) * (k + 1) <= INT_MAX, "spec_verify: batch * (k + 1) = %lld rows",
                  static_cast<long long>(batch) * (k + 1));
    const size_t need = llmie_spec_verify_workspace_bytes(batch, k, vocab);
    if (!workspace || workspace_bytes < need || reinterpret_cast<uintptr_t>(workspace) % 16 != 0) {
        set_error("spec_verify: workspace %zu bytes (need %zu, 16-byte aligned: llmie_spec_verify_workspace_bytes)",
                  workspace ? workspace_bytes : (size_t)0, need);
        return LLMIE_ERR_WORKSPACE;
    }
    const int rows = batch * (k + 1);
    uint32_t *ws = static_cast<uint32_t *>(workspace);
    SpecPick *picks = reinterpret_cast<SpecPick *>(static_cast<unsigned char *>(workspace) + spec_picks_offset(rows, vocab));
    const llmie_sampling_ext none = {};
    const llmie_sampling_ext &e = active ? *ext : none;
    hipStream_t st = as_stream(stream);
    if (dtype == LLMIE_F16)
        spec_rows_launch<half_t>(active, logits, rows, vocab, k, params_dev, history, history_stride, history_len, history_append, draft_ids,
                                 step_rows, step, step_dev, end_id, ws, picks, e, st);
    else
        spec_rows_launch<float>(active, logits, rows, vocab, k, params_dev, history, history_stride, history_len, history_append, draft_ids,
                                step_rows, step, step_dev, end_id, ws, picks, e, st);
    if ((rc = launch_status("spec_verify(rows)")) != LLMIE_OK) return rc;
    spec_accept_kernel<<<batch, 64, 0, st>>>(picks, k, draft_ids, draft_len, history, history_stride, history_len, history_append, seq_len,
                                             finished, out_tokens, out_count, out_logprob, last_token, cached_len, step_rows);
    return launch_status("spec_verify(accept)");
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
