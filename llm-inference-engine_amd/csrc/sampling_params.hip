// llmie_sample_logits / llmie_lm_head_sample_params: per-request sampling controls over the whole vocabulary (no reference
// launcher: the reference samples from the top-K only).
//
// ONE launch per step: one 1024-thread workgroup per row; everything below runs inside it.
//   pass 1   raw logits (fp16 / fp32) -> fp32 copy of the row in the workspace + the raw log-sum-exp (for out_logprob)
//   penalty  the history (<= kSpMaxHistory ids) is bitonic-sorted in LDS; every distinct id patches its entry of the copy
//   pass 2   temperature + clamp -> order-preserving 32-bit keys in place (0 = NaN, excluded) + the (key, id) maximum and
//            the number of valid tokens.  Greedy rows (T == 0) stop here.
//   then up to three runs of ONE operation, radix_select: in (value desc, id asc) order, the first token at which a running
//   integer weight exceeds a threshold -- 4 digit passes of a 256-bin histogram in LDS over the keys (narrowing the prefix
//   after each digit), then, for exact-value ties, id_select: the j-th id of the tie group by a block-wide scan.
//     top-k: weight 1, threshold top_k - 1;  top-p: mass, ceil(top_p * kept mass) - 1;  draw: mass, floor(u * kept mass).
//   The kept set is always a prefix of that order (top-k, top-p and min-p each cut it), so the three runs compose.
//
// Masses are fixed point: mass(t) = floor(exp(v_t - v_max) * 2^32) as uint64 (a token below 2^-32 of the maximum weighs 0 and is
// never drawn).  Every sum is an integer sum, so LDS atomics in any order give the same bits; the float reductions (max,
// log-sum-exp) use a fixed thread mapping and a fixed tree.  A row's result does not depend on the batch it runs in.
//
// llmie_sample_logits_ext / llmie_lm_head_sample_ext launch the EXT instantiation of the same body (sample_params_ext_kernel);
// the entries without the extension keep sample_params_kernel, whose code the extension does not touch.  EXT adds, in order:
//   top-N    behind pass 1, on the raw fp32 copy: radix_select (weight 1) + id_select find the top_n-th raw token, one more sweep
//            collects the <= 32 tokens at or above it into LDS, and each ranks itself among them
//   bias     one thread per list entry (<= 1024 = the block): an entry patches the copy unless a later entry names its id
//   min_step the stop ids and end_id become NaN in the copy while step < min_step
//   penalty  (as before)
//   mask     the row's bit mask is staged in LDS (16-byte loads) behind the penalties, which are done with `sorted` by then;
//            pass 2 turns a token whose bit is clear into key 0, what a NaN gets -- everything downstream ignores key 0
//   stops    finished also if the pick is in the row's stop list
//
// The device code of all this lives in sampling_body.cuh, which spec_decode.hip shares; this file keeps the kernel's shell, its one
// launch and the host checks.  On the host a call is the structs of llmie_internal.h (rows, state, position, ...) from entry to launch.
#include "sampling_body.cuh"

namespace llmie {

// Ext is empty (the kernel of the entries without the extension: their parameter list and their code are what they were before the
// extension existed) or one llmie_sampling_ext by value (EXT)
__device__ __forceinline__ const llmie_sampling_ext &sp_ext(const llmie_sampling_ext &e) { return e; }
template <typename T, typename... Ext>
__global__ __launch_bounds__(kSpThreads) void sample_params_kernel(
    const T *__restrict__ logits, int V, const llmie_sampling_params *__restrict__ params, int32_t *history, int hstride,
    int32_t *history_len, int happend, int32_t *__restrict__ seq_len, uint8_t *__restrict__ finished, int32_t *__restrict__ out_id,
    float *__restrict__ out_logprob, int step_arg, const int32_t *step_dev, int end_id, uint32_t *ws, size_t ws_row,
    const T *__restrict__ embed, T *__restrict__ next_hidden, int hidden, int advance, unsigned *ticket, int rows, Ext... ext) {
    constexpr bool EXT = sizeof...(Ext) == 1;
    __shared__ alignas(EXT ? 16 : alignof(SpShared)) SpShared s;   // (EXT stages the mask row with 16-byte stores)
    const int b = blockIdx.x, tid = threadIdx.x;
    const int step = step_dev ? *step_dev : step_arg;
    const llmie_sampling_ext *ep = nullptr;
    if constexpr (EXT) ep = &sp_ext(ext...);
    const SpPick pick = sp_sample_row<T, EXT>(logits + static_cast<size_t>(b) * V, V, params[b], SpStoredHistory{history, history_len, b, hstride},
                                              step, end_id, ws + static_cast<size_t>(b) * ws_row, ep, b, b, s);
    const int chosen = pick.chosen;

    if (tid == 0) {
        out_id[b] = chosen;
        if (!finished[b]) ++seq_len[b];
        finished[b] = static_cast<uint8_t>(sp_finishes<EXT>(pick, chosen, end_id));
        if (out_logprob) out_logprob[b] = sp_logprob(logits + static_cast<size_t>(b) * V, V, pick, pick.lse_m + logf(pick.lse_s), chosen);
        if (happend && hstride > 0) {
            const int len = history_len[b];
            if (len >= 0 && len < hstride) {
                history[static_cast<size_t>(b) * hstride + len] = chosen;
                history_len[b] = len + 1;
            }
        }
    }
    if (next_hidden && chosen >= 0 && chosen < V) {
        // llmie_input_embedding's rule: ids outside the table are skipped
        const T *src = embed + static_cast<size_t>(chosen) * hidden;
        T *dst = next_hidden + static_cast<size_t>(b) * hidden;
        for (int i = tid; i < hidden; i += kSpThreads) dst[i] = src[i];
    }
    if (advance && step_dev && tid == 0) {
        // every thread of the row has read the step (the barriers above): the last row moves the counter, re-zeroes the ticket
        if (atomicAdd(ticket, 1u) == static_cast<unsigned>(rows) - 1u) {
            *const_cast<int32_t *>(step_dev) = step + 1;
            atomicExch(ticket, 0u);
        }
    }
}

size_t sample_logits_ws_row(int vocab) { return (static_cast<size_t>(vocab) + 63) & ~static_cast<size_t>(63); }

int sample_logits_launch(const SampleRows &rows, const SampleState &state, const SamplePos &pos, const SampleOut &out, const SampleTail &tail,
                         SampleWs ws, const llmie_sampling_ext *ext, hipStream_t st) {
    sample_dispatch(rows.dtype, ext != nullptr, [&](auto type, auto with_ext) {
        using T = typename decltype(type)::type;
        auto launch = [&](auto... e) {   // e: nothing, or one llmie_sampling_ext -- which is what chooses the kernel
            sample_params_kernel<T, decltype(e)...><<<rows.batch, kSpThreads, 0, st>>>(
                static_cast<const T *>(rows.logits), rows.vocab, rows.params, state.history, state.history_stride, state.history_len,
                state.history_append, state.seq_len, state.finished, out.out_id, out.out_logprob, pos.step, pos.step_dev, rows.end_id,
                static_cast<uint32_t *>(ws.p), sample_logits_ws_row(rows.vocab), static_cast<const T *>(tail.embed),
                static_cast<T *>(tail.next_hidden), tail.hidden, tail.advance, tail.ticket, rows.batch, e...);
        };
        if constexpr (decltype(with_ext)::value) launch(*ext);
        else launch();
    });
    return launch_status("sample_logits");
}

// llmie_sampling_ext as the host can judge it (the arrays live in device memory).  *active: some control is on -- the EXT kernel
// is needed; otherwise the call is the entry without the extension.
int sample_ext_check(int batch, int vocab, const llmie_sampling_ext *e, bool *active, const char *entry) {
    *active = false;
    if (!e) return LLMIE_OK;
    LLMIE_REQUIRE(e->mask_stride >= 0 && e->mask_rows >= 0 && e->bias_stride >= 0 && e->stop_stride >= 0 && e->top_n >= 0,
                  "%s: negative mask_stride %d / mask_rows %d / bias_stride %d / stop_stride %d / top_n %d", entry, e->mask_stride,
                  e->mask_rows, e->bias_stride, e->stop_stride, e->top_n);
    const bool bias_any = e->bias_ids || e->bias_vals || e->bias_len;
    LLMIE_REQUIRE(!bias_any || (e->bias_ids && e->bias_vals && e->bias_len),
                  "%s: bias needs bias_ids, bias_vals and bias_len together", entry);
    LLMIE_REQUIRE(!e->stop_ids == !e->stop_len, "%s: stop_ids and stop_len go together", entry);
    LLMIE_REQUIRE(e->allowed_mask || !e->mask_index, "%s: mask_index without allowed_mask", entry);
    if (e->allowed_mask) {
        LLMIE_REQUIRE(e->mask_stride >= (vocab + 31) / 32, "%s: mask_stride %d words below ceil(vocab %d / 32)", entry,
                      e->mask_stride, vocab);
        LLMIE_REQUIRE(e->mask_rows >= 1, "%s: mask_rows %d < 1", entry, e->mask_rows);
        LLMIE_REQUIRE(e->mask_index || e->mask_rows >= batch, "%s: mask_rows %d below batch %d without a mask_index", entry,
                      e->mask_rows, batch);
    }
    LLMIE_REQUIRE(e->top_n == 0 || (e->out_top_ids && e->out_top_logprobs), "%s: top_n %d without out_top_ids / out_top_logprobs", entry,
                  e->top_n);
    if (e->bias_stride > LLMIE_SAMPLE_MAX_BIAS)
        LLMIE_UNSUPPORTED("%s: bias_stride %d above %d", entry, e->bias_stride, LLMIE_SAMPLE_MAX_BIAS);
    if (e->stop_stride > LLMIE_SAMPLE_MAX_STOPS)
        LLMIE_UNSUPPORTED("%s: stop_stride %d above %d", entry, e->stop_stride, LLMIE_SAMPLE_MAX_STOPS);
    if (e->top_n > LLMIE_SAMPLE_MAX_TOP_N) LLMIE_UNSUPPORTED("%s: top_n %d above %d", entry, e->top_n, LLMIE_SAMPLE_MAX_TOP_N);
    *active = e->allowed_mask || bias_any || e->stop_ids || e->min_step || e->top_n > 0;
    return LLMIE_OK;
}

int sample_logits_check(const char *entry, const SampleRows &r, const SampleState &s, const void *out) {
    LLMIE_REQUIRE(r.logits && r.params && s.seq_len && s.finished && out, "%s: NULL pointer", entry);
    LLMIE_REQUIRE(r.batch > 0 && r.vocab > 0, "%s: batch %d / vocab %d must be positive", entry, r.batch, r.vocab);
    LLMIE_REQUIRE(s.history_stride >= 0, "%s: history_stride %d < 0", entry, s.history_stride);
    LLMIE_REQUIRE(s.history_stride == 0 || (s.history && s.history_len), "%s: history_stride %d > 0 without history / history_len", entry,
                  s.history_stride);
    if (s.history_stride > kSpMaxHistory) LLMIE_UNSUPPORTED("%s: history_stride %d above %d", entry, s.history_stride, kSpMaxHistory);
    if (r.dtype != LLMIE_F16 && r.dtype != LLMIE_F32) LLMIE_UNSUPPORTED("%s: dtype %d", entry, (int)r.dtype);
    return LLMIE_OK;
}

int sample_workspace_check(const char *entry, SampleWs ws, size_t need, const char *query) {
    if (ws.p && ws.bytes >= need && reinterpret_cast<uintptr_t>(ws.p) % 16 == 0) return LLMIE_OK;
    set_error("%s: workspace %zu bytes (need %zu, 16-byte aligned%s%s)", entry, ws.p ? ws.bytes : (size_t)0, need, query ? ": " : "",
              query ? query : "");
    return LLMIE_ERR_WORKSPACE;
}

}  // namespace llmie

using namespace llmie;

extern "C" size_t llmie_sample_logits_workspace_bytes(int batch, int vocab) {
    if (batch <= 0 || vocab <= 0) return 0;
    return static_cast<size_t>(batch) * sample_logits_ws_row(vocab) * sizeof(uint32_t);
}

extern "C" int llmie_sample_logits_ext(const void *logits, int batch, int vocab, const llmie_sampling_params *params_dev, int32_t *history,
                                       int history_stride, int32_t *history_len, int history_append, int32_t *seq_len,
                                       uint8_t *finished, int32_t *out_id, float *out_logprob, int step, const int32_t *step_dev,
                                       int end_id, void *workspace, size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream,
                                       const llmie_sampling_ext *ext) {
    const SampleRows rows{logits, batch, vocab, dtype, params_dev, end_id};
    const SampleState state{history, history_stride, history_len, history_append, seq_len, finished};
    const SampleWs ws{workspace, workspace_bytes};
    int rc = sample_logits_check("sample_logits", rows, state, out_id);
    if (rc != LLMIE_OK) return rc;
    if ((rc = sample_workspace_check("sample_logits", ws, llmie_sample_logits_workspace_bytes(batch, vocab), nullptr)) != LLMIE_OK) return rc;
    bool active;
    if ((rc = sample_ext_check(batch, vocab, ext, &active)) != LLMIE_OK) return rc;
    return sample_logits_launch(rows, state, SamplePos{step, step_dev}, SampleOut{out_id, out_logprob}, SampleTail{}, ws,
                                active ? ext : nullptr, as_stream(stream));
}

// (no extension: nothing for sample_ext_check to refuse, and the kernel without it)
extern "C" int llmie_sample_logits(const void *logits, int batch, int vocab, const llmie_sampling_params *params_dev, int32_t *history,
                                   int history_stride, int32_t *history_len, int history_append, int32_t *seq_len, uint8_t *finished,
                                   int32_t *out_id, float *out_logprob, int step, const int32_t *step_dev, int end_id, void *workspace,
                                   size_t workspace_bytes, llmie_dtype dtype, llmie_stream stream) {
    return llmie_sample_logits_ext(logits, batch, vocab, params_dev, history, history_stride, history_len, history_append, seq_len, finished,
                                   out_id, out_logprob, step, step_dev, end_id, workspace, workspace_bytes, dtype, stream, nullptr);
}
