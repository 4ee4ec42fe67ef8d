// C++ API mirror, part 6: the 18 `launch*` templates of src/kernels/includes/*.cuh plus
// CublasWrapper (cublas_utils.cuh:17-75), as inline adaptors over the C ABI (include/llmie.h).
// Shapes are taken from the TensorWrappers exactly where the reference launchers take them;
// a failing C-ABI status becomes the reference's LLM_CHECK exception.
#pragma once
#include "params.hpp"
#include "tensor.hpp"
#include "weights.hpp"

typedef void *llmieBlasHandle_t;  // stands where the reference takes cublasHandle_t / cublasLtHandle_t (ignored)

// GEMM context: name and constructor shape of the reference's CublasWrapper; holds no vendor library.  Like the reference's
// (whose cuBLAS handle owns its workspace) it owns the scratch the GEMMs use: fp32 split-K slabs, allocated HERE, once -- the
// C ABI never allocates on the compute path.  A shape that needs more than the wrapper holds runs the non-split kernels.
class CublasWrapper {
private:
    llmie_dtype dtype_ = LLMIE_F32;
    void *ws_ = nullptr;
    size_t ws_bytes_ = 0;

public:
    explicit CublasWrapper(llmieBlasHandle_t = nullptr, llmieBlasHandle_t = nullptr, size_t workspace_bytes = size_t(128) << 20) {
        if (workspace_bytes && hipMalloc(&ws_, workspace_bytes) == hipSuccess) ws_bytes_ = workspace_bytes;
    }
    ~CublasWrapper() {
        if (ws_) (void)hipFree(ws_);
    }
    CublasWrapper(const CublasWrapper &) = delete;
    CublasWrapper &operator=(const CublasWrapper &) = delete;
    void setFP32GemmConfig() { dtype_ = LLMIE_F32; }
    void setFP16GemmConfig() { dtype_ = LLMIE_F16; }
    llmie_dtype dtype() const { return dtype_; }
    // the wrapper's scratch if it covers `need` bytes, else none
    void *workspace(size_t need) const { return need <= ws_bytes_ ? ws_ : nullptr; }
    size_t workspace_bytes(size_t need) const { return need <= ws_bytes_ ? ws_bytes_ : 0; }
};

namespace llmie_api {
inline hipStream_t st() { return launch_stream(); }

// grow-only device scratch for launchers whose C-ABI form takes a workspace (decode attention)
inline void *scratch(size_t bytes) {
    static thread_local void *buf = nullptr;
    static thread_local size_t cap = 0;
    if (bytes > cap) {
        if (buf) CHECK(hipFree(buf));
        CHECK(hipMalloc(&buf, bytes));
        cap = bytes;
    }
    return buf;
}
}  // namespace llmie_api

// input_embedding.cuh:8-12
template <typename T>
void launchInputEmbedding(TensorWrapper<int> *input_ids, TensorWrapper<T> *output, EmbeddingWeight<T> *embed_table) {
    const int num_tokens = output->shape[0], hidden = output->shape[1];
    LLM_CHECK_WITH_INFO(num_tokens == input_ids->shape[0], "Input ids 1st shape should equal to 1st shape of output");
    const int vocab = embed_table->shape.empty() ? (1 << 30) : embed_table->shape[0];
    LLMIE_CALL(llmie_input_embedding(input_ids->data, embed_table->data, output->data, num_tokens, hidden, vocab,
                                     llmie_api::dtype_of<T>(), llmie_api::st()));
}

// cal_padding_offset.cuh:16-20
inline void launchCalPaddingOffset(TensorWrapper<int> *padding_offset, TensorWrapper<int> *cum_seqlens,
                                   TensorWrapper<int> *input_lengths) {
    const int batch = padding_offset->shape[0], max_q_len = padding_offset->shape[1];
    LLM_CHECK_WITH_INFO(batch == input_lengths->shape[0],
                        "Input lengths numbers should equal to padding offset batch size dimension!");
    LLM_CHECK_WITH_INFO(batch == cum_seqlens->shape[0] - 1,
                        "Cumulative sequence length should equal to padding offset batch size dimension plus 1!");
    LLMIE_CALL(llmie_cal_padding_offset(padding_offset->data, cum_seqlens->data, input_lengths->data, batch, max_q_len,
                                        llmie_api::st()));
}

// build_causal_mask.cuh:10-14
template <typename T>
void launchBuildCausalMasks(TensorWrapper<T> *mask, TensorWrapper<int> *q_lens, TensorWrapper<int> *k_lens) {
    LLMIE_CALL(llmie_build_causal_mask(mask->data, q_lens->data, k_lens->data, mask->shape[0], mask->shape[1],
                                       mask->shape[2], llmie_api::dtype_of<T>(), llmie_api::st()));
}

// rmsnorm.cuh:10-15
template <typename T>
void launchRMSNorm(TensorWrapper<T> *decoder_out, TensorWrapper<T> *decoder_residual,
                   LayerNormWeight<T> *attention_norm_weight, float eps, bool is_last = false) {
    (void)is_last;
    LLMIE_CALL(llmie_rmsnorm(decoder_out->data, decoder_residual ? decoder_residual->data : nullptr,
                             attention_norm_weight->gamma, eps, decoder_out->shape[0], decoder_out->shape[1],
                             llmie_api::dtype_of<T>(), llmie_api::st()));
}

// add_residual_and_rmsnorm.cuh:12-18 (norm->bias is the bias; scale = gamma)
template <typename T>
void launchFusedAddBiasResidualAndRMSNorm(TensorWrapper<T> *residual, TensorWrapper<T> *decoder_out,
                                          BaseWeight<T> *norm, T *scale, float eps) {
    LLMIE_CALL(llmie_fused_add_bias_residual_rmsnorm(residual ? residual->data : nullptr, decoder_out->data,
                                                     norm ? norm->bias : nullptr, scale, eps, decoder_out->shape[0],
                                                     decoder_out->shape[1], llmie_api::dtype_of<T>(), llmie_api::st()));
}

// add_residual.cuh:10-14
template <typename T>
void launchAddResidual(TensorWrapper<T> *residual, TensorWrapper<T> *decoder_out, bool is_print = false) {
    (void)is_print;
    LLMIE_CALL(llmie_add_residual(residual->data, decoder_out->data, decoder_out->shape[0], decoder_out->shape[1],
                                  llmie_api::dtype_of<T>(), llmie_api::st()));
}

// linear.cuh:14-21.  3-D inputs/outputs are flattened on dims 1,2 (linear.cu:37-43); trans_b selects
// y = x.W^T (W [N,K]) vs y = x.W (W [K,N]) -- the intent of the reference.
template <typename T>
void launchLinearGemm(TensorWrapper<T> *input, BaseWeight<T> *weight, TensorWrapper<T> *output,
                      CublasWrapper *cublas_wrapper, bool trans_a = false, bool trans_b = false) {
    LLM_CHECK_WITH_INFO(!trans_a, "trans_a is not used by any caller of the reference and is not supported");
    const int Am = input->shape[0];
    const int An = input->shape.size() == 3 ? input->shape[1] * input->shape[2] : input->shape[1];
    const int Cm = output->shape[0];
    const int Cn = output->shape.size() == 3 ? output->shape[1] * output->shape[2] : output->shape[1];
    int opBm = weight->shape[0], opBn = weight->shape[1];
    if (trans_b) std::swap(opBm, opBn);
    LLM_CHECK_WITH_INFO(An == opBm, "2nd dim of weight MUST = 1st dim of input");
    LLM_CHECK_WITH_INFO(Am == Cm && opBn == Cn, "output shape should be equal to weight shape");
    const size_t need = (cublas_wrapper && trans_b && std::is_same<T, half>::value) ? llmie_linear_workspace_bytes(LLMIE_W_F16, Cm, An, Cn) : 0;
    LLMIE_CALL(llmie_linear(input->data, weight->data, output->data, Cm, An, Cn, trans_b ? 1 : 0, nullptr, nullptr,
                            llmie_api::dtype_of<T>(), need ? cublas_wrapper->workspace(need) : nullptr,
                            need ? cublas_wrapper->workspace_bytes(need) : 0, llmie_api::st()));
}

// linear.cuh:23-29: per (b,h): C = A.B or A.B^T
template <typename T>
void launchLinearStridedBatchGemm(TensorWrapper<T> *input1, TensorWrapper<T> *input2, TensorWrapper<T> *output,
                                  CublasWrapper *cublas_wrapper, bool trans_a = false, bool trans_b = false) {
    (void)cublas_wrapper;
    LLM_CHECK_WITH_INFO(!trans_a, "trans_a is not supported");
    const int Am = input1->shape[2], An = input1->shape[3];
    int opBm = input2->shape[2], opBn = input2->shape[3];
    if (trans_b) std::swap(opBm, opBn);
    const int Cm = output->shape[2], Cn = output->shape[3];
    LLM_CHECK_WITH_INFO(An == opBm, "2nd dim of weight MUST = 1st dim of input");
    LLM_CHECK_WITH_INFO(Am == Cm && opBn == Cn, "output shape should be equal to weight shape");
    const int batch = input1->shape[0] * input1->shape[1];
    LLM_CHECK_WITH_INFO(batch == input2->shape[0] * input2->shape[1], "dim 0 and dim 1 wrong!");
    LLMIE_CALL(llmie_batched_gemm(input1->data, input2->data, output->data, batch, Cm, Cn, An, trans_b ? 1 : 0,
                                  llmie_api::dtype_of<T>(), llmie_api::st()));
}

// qkv_bias_and_rope.cuh:13-23.  The reference never applies the bias (9-K10): neither do we here.
template <typename T>
void launchFusedQKVAddBiasAndTransposeAndRope(TensorWrapper<T> *q_buf, TensorWrapper<T> *k_buf, TensorWrapper<T> *v_buf,
                                              TensorWrapper<T> *QKV, BaseWeight<T> *qkv,
                                              TensorWrapper<int> *padding_offset, TensorWrapper<int> *history_length,
                                              TensorWrapper<int> *input_length,
                                              LlamaAttentionStaticParams *static_params) {
    (void)qkv;
    (void)input_length;
    const int token_num = QKV->shape[0], qkv_head_num = QKV->shape[1], head_size = QKV->shape[2];
    const int batch = q_buf->shape[0], head_num = q_buf->shape[1], seq_len = q_buf->shape[2];
    LLM_CHECK_WITH_INFO(k_buf->shape[1] == v_buf->shape[1], "k and v should have same head_num");
    LLM_CHECK_WITH_INFO(k_buf->shape[1] == (qkv_head_num - head_num) / 2, "k and v should have same head_num");
    LLM_CHECK_WITH_INFO(q_buf->shape[3] == head_size, "head_size does not match!");
    LLMIE_CALL(llmie_qkv_bias_transpose_rope(q_buf->data, k_buf->data, v_buf->data, QKV->data, nullptr,
                                             padding_offset->data, history_length->data, batch, seq_len, token_num,
                                             head_num, k_buf->shape[1], head_size, static_params->rotary_embedding_dim,
                                             static_params->rotary_embedding_base, llmie_api::dtype_of<T>(),
                                             llmie_api::st()));
}

// rope.cuh:13-17
template <typename T>
void launchRope(TensorWrapper<T> *qkv_buf, TensorWrapper<int> *step, LlamaAttentionStaticParams *static_params) {
    const int batch = qkv_buf->shape[0], qkv_head_num = qkv_buf->shape[1], head_size = qkv_buf->shape[2];
    const int head_num = static_params->head_num, kv_head_num = static_params->kv_head_num;
    LLM_CHECK_WITH_INFO(qkv_head_num == head_num + 2 * kv_head_num, "qkv_buf heads != head_num + 2*kv_head_num");
    LLMIE_CALL(llmie_rope_decode(qkv_buf->data, batch, head_num, kv_head_num, head_size, step->getVal(), nullptr,
                                 static_params->rotary_embedding_dim, static_params->rotary_embedding_base,
                                 llmie_api::dtype_of<T>(), llmie_api::st()));
}

// decoder_self_attention.cuh:12-22
template <typename T>
void launchDecoderMaskedMultiHeadAttention(TensorWrapper<T> *qkv_buf, BaseWeight<T> *qkv, TensorWrapper<int> *layer_id,
                                           TensorWrapper<T> *k_cache, TensorWrapper<T> *v_cache,
                                           TensorWrapper<bool> *finished, TensorWrapper<int> *step,
                                           TensorWrapper<T> *mha_output, LlamaAttentionStaticParams *static_params) {
    (void)finished;
    (void)static_params;
    const int batch = qkv_buf->shape[0], qkv_head_num = qkv_buf->shape[1], head_size = qkv_buf->shape[2];
    const int kv_head_num = k_cache->shape[2], max_seq_len = k_cache->shape[3];
    const int head_num = qkv_head_num - 2 * kv_head_num;
    const size_t ws = llmie_decoder_mha_workspace_bytes(batch, head_num, head_size, max_seq_len);
    LLMIE_CALL(llmie_decoder_mha(qkv_buf->data, qkv ? qkv->bias : nullptr, k_cache->data, v_cache->data,
                                 mha_output->data, layer_id->getVal(), batch, head_num, kv_head_num, head_size,
                                 max_seq_len, step->getVal(), nullptr, llmie_api::scratch(ws), ws,
                                 llmie_api::dtype_of<T>(), llmie_api::st()));
}

// concat_past_kv.cuh:10-18
template <typename T>
void launchConcatKVCache(TensorWrapper<T> *k_src, TensorWrapper<T> *v_src, TensorWrapper<int> *layer_id,
                         TensorWrapper<int> *cur_query_length, TensorWrapper<int> *history_length,
                         TensorWrapper<T> *k_dst, TensorWrapper<T> *v_dst) {
    const int batch = k_src->shape[0], kv_head_num = k_src->shape[1], max_q_len = k_src->shape[2];
    const int head_size = k_src->shape[3], max_seq_len = k_dst->shape[3], layer = layer_id->getVal();
    LLMIE_CALL(llmie_concat_kv(k_src->data, k_dst->data, cur_query_length->data, history_length->data, layer, batch,
                               kv_head_num, max_q_len, max_seq_len, head_size, llmie_api::dtype_of<T>(), llmie_api::st()));
    LLMIE_CALL(llmie_concat_kv(v_src->data, v_dst->data, cur_query_length->data, history_length->data, layer, batch,
                               kv_head_num, max_q_len, max_seq_len, head_size, llmie_api::dtype_of<T>(), llmie_api::st()));
}

// repeat_kv.cuh:10-17
template <typename T>
void launchRepeatKVCache(TensorWrapper<T> *k_cache_src, TensorWrapper<T> *v_cache_src,
                         TensorWrapper<int> *context_length, TensorWrapper<int> *layer_id,
                         TensorWrapper<T> *k_cache_dst, TensorWrapper<T> *v_cache_dst) {
    const int batch = context_length->shape[0], kv_head_num = k_cache_src->shape[2];
    const int max_seq_len = k_cache_src->shape[3], head_num = k_cache_dst->shape[1];
    const int max_k_len = k_cache_dst->shape[2], head_size = k_cache_dst->shape[3], layer = layer_id->getVal();
    LLMIE_CALL(llmie_repeat_kv(v_cache_src->data, v_cache_dst->data, context_length->data, layer, batch, head_num,
                               kv_head_num, max_k_len, max_seq_len, head_size, llmie_api::dtype_of<T>(), llmie_api::st()));
    LLMIE_CALL(llmie_repeat_kv(k_cache_src->data, k_cache_dst->data, context_length->data, layer, batch, head_num,
                               kv_head_num, max_k_len, max_seq_len, head_size, llmie_api::dtype_of<T>(), llmie_api::st()));
}

// scale_and_mask_and_softmax.cuh:11-16
template <typename T>
void launchFusedScaleMaskAndSoftmax(TensorWrapper<T> *qk, TensorWrapper<T> *mask, TensorWrapper<T> *attention_weights,
                                    float scale) {
    LLMIE_CALL(llmie_scale_mask_softmax(qk->data, mask->data, attention_weights->data, scale, qk->shape[0],
                                        qk->shape[1], qk->shape[2], qk->shape[3], llmie_api::dtype_of<T>(),
                                        llmie_api::st()));
}

// transpose_and_remove_padding.cuh:9-13
template <typename T>
void launchFusedTransposeAndRemovePadding(TensorWrapper<T> *padded_qkv_buf, TensorWrapper<int> *padding_offset,
                                          TensorWrapper<T> *lineared_qkv) {
    LLMIE_CALL(llmie_transpose_remove_padding(padded_qkv_buf->data, lineared_qkv->data, padding_offset->data,
                                              lineared_qkv->shape[0], padded_qkv_buf->shape[0], padded_qkv_buf->shape[2],
                                              padded_qkv_buf->shape[1], padded_qkv_buf->shape[3],
                                              llmie_api::dtype_of<T>(), llmie_api::st()));
}

// silu_and_mul.cuh:10-13
template <typename T> void launchSiluAndMul(TensorWrapper<T> *input, TensorWrapper<T> *output) {
    LLM_CHECK_WITH_INFO(input->shape.size() == 3 && input->shape[1] == 2, "SiluAndMul input must be [tokens, 2, inter]");
    LLMIE_CALL(llmie_silu_and_mul(input->data, output->data, input->shape[0], input->shape[2],
                                  llmie_api::dtype_of<T>(), llmie_api::st()));
}

// topk.cuh:45-51.  K = last dim of final_topk_ids (the reference hard-codes 5 and ignores the
// buffers' shapes); blocks per row = topk_ids->shape[2].
template <typename T>
void launchTopKForBeamSearch(TensorWrapper<T> *probs, TensorWrapper<int> *topk_ids, TensorWrapper<T> *topk_vals,
                             TensorWrapper<int> *final_topk_ids, TensorWrapper<T> *final_topk_vals) {
    const int rows = probs->shape[0], vocab = probs->shape[1];
    const int K = final_topk_ids->shape.back();
    const int bpr = topk_ids->shape.size() >= 4 ? topk_ids->shape[2] : 1;
    LLMIE_CALL(llmie_topk(probs->data, topk_ids->data, topk_vals->data, final_topk_ids->data, final_topk_vals->data,
                          rows, vocab, K, bpr, llmie_api::dtype_of<T>(), llmie_api::st()));
}

// sampling.cuh:12-19
template <typename T>
void launchSampling(TensorWrapper<int> *topk_id, TensorWrapper<T> *topk_val, TensorWrapper<int> *seqlen,
                    TensorWrapper<bool> *is_finished, TensorWrapper<int> *output_id, MapStringToInt *params) {
    static_assert(sizeof(bool) == 1, "finished flags are one byte each");
    LLMIE_CALL(llmie_sampling(topk_id->data, topk_val->data, seqlen->data,
                              reinterpret_cast<uint8_t *>(is_finished->data), output_id->data, topk_id->shape[0],
                              topk_id->shape[1], params->at("step"), nullptr, params->at("end_id"),
                              params->at("vocab_size"), llmie_api::dtype_of<T>(), llmie_api::st()));
}

// No reference launcher (the reference names a beamwidth and never fills it): one beam-search step on the logits
// [groups * width, vocab] of a decode step.  cum_logprob / gen_len / finished [groups, width] are updated in place; parent (ABSOLUTE
// rows, ready for launchForkKVPages) and token [groups, width] are written.
template <typename T>
void launchBeamSearchStep(TensorWrapper<T> *logits, TensorWrapper<float> *cum_logprob, TensorWrapper<int> *gen_len,
                          TensorWrapper<bool> *finished, TensorWrapper<int> *parent, TensorWrapper<int> *token, int end_id,
                          float length_penalty = 0.f) {
    static_assert(sizeof(bool) == 1, "finished flags are one byte each");
    const int groups = cum_logprob->shape[0], width = cum_logprob->shape[1], vocab = logits->shape[1];
    LLM_CHECK_WITH_INFO(logits->shape[0] == groups * width, "logits rows should equal groups * width of the beam state");
    const size_t ws = llmie_beam_step_workspace_bytes(groups, width, vocab);
    LLMIE_CALL(llmie_beam_step(logits->data, groups, width, vocab, cum_logprob->data, gen_len->data,
                               reinterpret_cast<uint8_t *>(finished->data), parent->data, token->data, end_id, length_penalty,
                               llmie_api::scratch(ws), ws, llmie_api::dtype_of<T>(), llmie_api::st()));
}

// No reference launcher: row j of the paged caches [layers, num_pages, kv_heads, 128, head_size] continues the sequence of row
// parent[j]; completed pages are shared through block_table [rows, max_pages], the partial tail page is copied into own_table's.
template <typename T>
void launchForkKVPages(TensorWrapper<T> *k_pool, TensorWrapper<T> *v_pool, TensorWrapper<int> *block_table,
                       TensorWrapper<int> *own_table, TensorWrapper<int> *parent, TensorWrapper<int> *cached_len) {
    const int layers = k_pool->shape[0], num_pages = k_pool->shape[1], kv_head_num = k_pool->shape[2], head_size = k_pool->shape[4];
    const int rows = block_table->shape[0], max_pages = block_table->shape[1];
    LLM_CHECK_WITH_INFO(k_pool->shape[3] == LLMIE_KV_PAGE_TOKENS, "pages hold 128 tokens");
    LLM_CHECK_WITH_INFO(own_table->shape[0] == rows && own_table->shape[1] == max_pages, "own_table should have block_table's shape");
    const size_t ws = llmie_kv_pages_fork_workspace_bytes(rows, layers, kv_head_num, head_size, static_cast<int>(sizeof(T)), max_pages);
    LLMIE_CALL(llmie_kv_pages_fork(k_pool->data, v_pool->data, block_table->data, own_table->data, parent->data, cached_len->data, rows,
                                   layers, kv_head_num, head_size, max_pages, num_pages, static_cast<int>(sizeof(T)),
                                   llmie_api::scratch(ws), ws, llmie_api::st()));
}

// No reference launcher: exact-match verification of k draft tokens per sequence on the logits [batch * (k + 1), vocab] of a
// chunk (row b * (k + 1) + i follows input i of sequence b; include/llmie.h has the semantics).  draft_ids [batch, k];
// out_tokens [batch, k + 1] and out_count [batch] are written; seq_len / finished and -- where given -- the history
// [batch, stride] + history_len, last_token, cached_len and step_rows [batch] move as `count` sampler calls would move them.
// draft_len, history (with history_len), last_token, cached_len, step_rows, out_logprob and ext may be null; without step_rows
// every sequence draws at `step`.
template <typename T>
void launchSpecVerify(TensorWrapper<T> *logits, TensorWrapper<int> *draft_ids, TensorWrapper<int> *draft_len,
                      const llmie_sampling_params *params_dev, TensorWrapper<int> *history, TensorWrapper<int> *history_len,
                      bool history_append, TensorWrapper<int> *seq_len, TensorWrapper<bool> *finished, TensorWrapper<int> *out_tokens,
                      TensorWrapper<int> *out_count, TensorWrapper<float> *out_logprob, TensorWrapper<int> *last_token,
                      TensorWrapper<int> *cached_len, TensorWrapper<int> *step_rows, int step, int end_id,
                      const llmie_sampling_ext *ext = nullptr) {
    static_assert(sizeof(bool) == 1, "finished flags are one byte each");
    const int batch = draft_ids->shape[0], k = draft_ids->shape[1], vocab = logits->shape[1];
    LLM_CHECK_WITH_INFO(logits->shape[0] == batch * (k + 1), "logits rows should equal batch * (k + 1)");
    const size_t ws = llmie_spec_verify_workspace_bytes(batch, k, vocab);
    LLMIE_CALL(llmie_spec_verify(logits->data, batch, k, vocab, draft_ids->data, draft_len ? draft_len->data : nullptr, params_dev,
                                 history ? history->data : nullptr, history ? history->shape[1] : 0,
                                 history_len ? history_len->data : nullptr, history_append ? 1 : 0, seq_len->data,
                                 reinterpret_cast<uint8_t *>(finished->data), out_tokens->data, out_count->data,
                                 out_logprob ? out_logprob->data : nullptr, last_token ? last_token->data : nullptr,
                                 cached_len ? cached_len->data : nullptr, step_rows ? step_rows->data : nullptr, step, nullptr, end_id,
                                 llmie_api::scratch(ws), ws, llmie_api::dtype_of<T>(), llmie_api::st(), ext));
}

// No reference launcher: rejection-sampling verification against a drafter that sampled its drafts (include/llmie.h has the rule).
// launchSpecVerify's operands, plus draft_logits [batch, k, vocab] -- the logits draft i of sequence b was sampled from --, the
// drafter's controls draft_params_dev [batch] and out_accepted [batch] (may be null: the drafts among the emitted tokens).
template <typename T>
void launchSpecVerifySampled(TensorWrapper<T> *logits, TensorWrapper<T> *draft_logits, TensorWrapper<int> *draft_ids,
                             TensorWrapper<int> *draft_len, const llmie_sampling_params *params_dev,
                             const llmie_sampling_params *draft_params_dev, TensorWrapper<int> *history, TensorWrapper<int> *history_len,
                             bool history_append, TensorWrapper<int> *seq_len, TensorWrapper<bool> *finished, TensorWrapper<int> *out_tokens,
                             TensorWrapper<int> *out_count, TensorWrapper<int> *out_accepted, TensorWrapper<float> *out_logprob,
                             TensorWrapper<int> *last_token, TensorWrapper<int> *cached_len, TensorWrapper<int> *step_rows, int step, int end_id,
                             const llmie_sampling_ext *ext = nullptr) {
    static_assert(sizeof(bool) == 1, "finished flags are one byte each");
    const int batch = draft_ids->shape[0], k = draft_ids->shape[1], vocab = logits->shape[1];
    LLM_CHECK_WITH_INFO(logits->shape[0] == batch * (k + 1), "logits rows should equal batch * (k + 1)");
    LLM_CHECK_WITH_INFO(draft_logits->shape.size() == 3 && draft_logits->shape[0] == batch && draft_logits->shape[1] == k &&
                            draft_logits->shape[2] == vocab,
                        "draft_logits should be [batch, k, vocab]");
    const size_t ws = llmie_spec_verify_sampled_workspace_bytes(batch, k, vocab);
    LLMIE_CALL(llmie_spec_verify_sampled(logits->data, draft_logits->data, batch, k, vocab, draft_ids->data, draft_len ? draft_len->data : nullptr,
                                         params_dev, draft_params_dev, history ? history->data : nullptr, history ? history->shape[1] : 0,
                                         history_len ? history_len->data : nullptr, history_append ? 1 : 0, seq_len->data,
                                         reinterpret_cast<uint8_t *>(finished->data), out_tokens->data, out_count->data,
                                         out_accepted ? out_accepted->data : nullptr, out_logprob ? out_logprob->data : nullptr,
                                         last_token ? last_token->data : nullptr, cached_len ? cached_len->data : nullptr,
                                         step_rows ? step_rows->data : nullptr, step, nullptr, end_id, llmie_api::scratch(ws), ws,
                                         llmie_api::dtype_of<T>(), llmie_api::st(), ext));
}

// No reference launcher: prompt-lookup drafts from each sequence's own tokens [batch, stride] (len [batch] of them): the last
// max_n .. min_n tokens are looked up earlier in the row and what followed them there becomes the draft.  out_ids [batch, k + 1]
// (the verify chunk's inputs: the last token, then the drafts), out_draft_ids [batch, k], out_draft_len [batch].
inline void launchNgramDraft(TensorWrapper<int> *tokens, TensorWrapper<int> *len, TensorWrapper<bool> *finished, int max_n, int min_n,
                             int pad_id, TensorWrapper<int> *out_ids, TensorWrapper<int> *out_draft_ids, TensorWrapper<int> *out_draft_len) {
    static_assert(sizeof(bool) == 1, "finished flags are one byte each");
    const int batch = tokens->shape[0], stride = tokens->shape[1], k = out_draft_ids->shape[1];
    LLM_CHECK_WITH_INFO(out_ids->shape[0] == batch && out_ids->shape[1] == k + 1, "out_ids should be [batch, k + 1]");
    LLMIE_CALL(llmie_ngram_draft(tokens->data, stride, len->data, finished ? reinterpret_cast<uint8_t *>(finished->data) : nullptr, batch, k,
                                 max_n, min_n, pad_id, out_ids->data, out_draft_ids->data, out_draft_len->data, llmie_api::st()));
}

// No reference launchers: draft TREES (include/llmie.h has the rules).  parent [batch, n] (node_count [batch] or null = n) ->
// depth [batch, n], anc [batch, n] (64-bit ancestor masks; live = bit 0).
inline void launchSpecTreePrepare(TensorWrapper<int> *parent, TensorWrapper<int> *node_count, TensorWrapper<int> *depth, uint64_t *anc) {
    const int batch = parent->shape[0], n = parent->shape[1];
    LLM_CHECK_WITH_INFO(depth->shape[0] == batch && depth->shape[1] == n, "depth should be [batch, n]");
    LLMIE_CALL(llmie_spec_tree_prepare(parent->data, node_count ? node_count->data : nullptr, batch, n, depth->data, anc, llmie_api::st()));
}

// launchSpecVerify's operands with the draft chain replaced by a tree: node_ids / parent / depth [batch, n] and anc as
// launchSpecTreePrepare left them; logits [batch * n, vocab]; out_tokens / out_path (may be null) / out_logprob (may be null) [batch, n].
template <typename T>
void launchSpecVerifyTree(TensorWrapper<T> *logits, TensorWrapper<int> *node_ids, TensorWrapper<int> *parent, TensorWrapper<int> *depth,
                          const uint64_t *anc, const llmie_sampling_params *params_dev, TensorWrapper<int> *history,
                          TensorWrapper<int> *history_len, bool history_append, TensorWrapper<int> *seq_len, TensorWrapper<bool> *finished,
                          TensorWrapper<int> *out_tokens, TensorWrapper<int> *out_count, TensorWrapper<int> *out_path,
                          TensorWrapper<float> *out_logprob, TensorWrapper<int> *last_token, TensorWrapper<int> *cached_len,
                          TensorWrapper<int> *step_rows, int step, int end_id, const llmie_sampling_ext *ext = nullptr) {
    static_assert(sizeof(bool) == 1, "finished flags are one byte each");
    const int batch = node_ids->shape[0], n = node_ids->shape[1], vocab = logits->shape[1];
    LLM_CHECK_WITH_INFO(logits->shape[0] == batch * n, "logits rows should equal batch * n");
    const size_t ws = llmie_spec_verify_tree_workspace_bytes(batch, n, vocab);
    LLMIE_CALL(llmie_spec_verify_tree(logits->data, batch, n, vocab, node_ids->data, parent->data, depth->data, anc, params_dev,
                                      history ? history->data : nullptr, history ? history->shape[1] : 0,
                                      history_len ? history_len->data : nullptr, history_append ? 1 : 0, seq_len->data,
                                      reinterpret_cast<uint8_t *>(finished->data), out_tokens->data, out_count->data,
                                      out_path ? out_path->data : nullptr, out_logprob ? out_logprob->data : nullptr,
                                      last_token ? last_token->data : nullptr, cached_len ? cached_len->data : nullptr,
                                      step_rows ? step_rows->data : nullptr, step, nullptr, end_id, llmie_api::scratch(ws), ws,
                                      llmie_api::dtype_of<T>(), llmie_api::st(), ext));
}

// Behind the verify: the K / V rows of the accepted path move from slot base_len + out_path[m] to base_len + m.  Caches
// [L, batch, kvh, max_seq_len, hs], or pools [L, num_pages, kvh, 128, hs] with block_table [batch, max_pages].  base_len: the
// history lengths THE FORWARD ran with (not the array the verify advanced).
template <typename T>
void launchKvTreeCommit(TensorWrapper<T> *k_cache, TensorWrapper<T> *v_cache, TensorWrapper<int> *block_table, TensorWrapper<int> *base_len,
                        TensorWrapper<int> *out_path, TensorWrapper<int> *out_count) {
    const int batch = out_path->shape[0], n = out_path->shape[1];
    const int layers = k_cache->shape[0], kvh = k_cache->shape[2], hs = k_cache->shape[4];
    LLMIE_CALL(llmie_kv_tree_commit(k_cache->data, v_cache->data, block_table ? block_table->data : nullptr, base_len->data, out_path->data,
                                    out_count->data, batch, n, layers, kvh, block_table ? 0 : k_cache->shape[3], hs,
                                    block_table ? block_table->shape[1] : 0, block_table ? k_cache->shape[1] : 0, static_cast<int>(sizeof(T)),
                                    llmie_api::st()));
}

// launchNgramDraft's tree form: up to `branches` continuations of up to k tokens merged into a trie of out_ids->shape[1] nodes
inline void launchNgramDraftTree(TensorWrapper<int> *tokens, TensorWrapper<int> *len, TensorWrapper<bool> *finished, int k, int branches,
                                 int max_n, int min_n, int pad_id, TensorWrapper<int> *out_ids, TensorWrapper<int> *out_parent,
                                 TensorWrapper<int> *out_node_count) {
    static_assert(sizeof(bool) == 1, "finished flags are one byte each");
    const int batch = tokens->shape[0], stride = tokens->shape[1], n = out_ids->shape[1];
    LLM_CHECK_WITH_INFO(out_ids->shape[0] == batch && out_parent->shape[0] == batch && out_parent->shape[1] == n, "out_ids / out_parent should be [batch, n]");
    LLMIE_CALL(llmie_ngram_draft_tree(tokens->data, stride, len->data, finished ? reinterpret_cast<uint8_t *>(finished->data) : nullptr, batch, n,
                                      k, branches, max_n, min_n, pad_id, out_ids->data, out_parent->data, out_node_count->data, llmie_api::st()));
}

// No reference launcher: decode attention of a ragged batch under a sliding window with sink tokens (include/llmie.h has the mask):
// qkv_buf [batch, head_num + 2 kv_head_num, head_size] (bias: the QKV bias or null), ctx_len [batch] = context length of every
// sequence with this step's token, caches [L, batch, kvh, max_seq_len, hs] -- or, with block_table [batch, max_pages], page pools
// [L, num_pages, kvh, 128, hs] and max_seq_len given --, rope_table: [max_pos][hs / 2] (cos, sin) pairs or null (q, k rotated
// already).  window = 0: full attention.  Appends k / v at ctx_len - 1 and attends; entries of dead pages are never followed.
template <typename T>
void launchDecoderWindowAttention(TensorWrapper<T> *qkv_buf, const T *qkv_bias, int layer, TensorWrapper<T> *k_cache, TensorWrapper<T> *v_cache,
                                  TensorWrapper<int> *ctx_len, const void *rope_table, int rotary_dim, TensorWrapper<int> *block_table,
                                  int max_seq_len, int window, int sinks, TensorWrapper<T> *mha_output) {
    const int batch = qkv_buf->shape[0], qkv_head_num = qkv_buf->shape[1], head_size = qkv_buf->shape[2];
    const int kv_head_num = k_cache->shape[2];
    const int head_num = qkv_head_num - 2 * kv_head_num;
    if (!block_table) max_seq_len = k_cache->shape[3];
    const size_t ws = llmie_decoder_mha_workspace_bytes(batch, head_num, head_size, max_seq_len);
    LLMIE_CALL(llmie_decoder_mha_window(qkv_buf->data, qkv_bias, k_cache->data, v_cache->data, mha_output->data, layer, batch, head_num,
                                        kv_head_num, head_size, max_seq_len, ctx_len->data, llmie_api::scratch(ws), ws, rope_table, rotary_dim,
                                        block_table ? block_table->data : nullptr, block_table ? block_table->shape[1] : 0,
                                        block_table ? k_cache->shape[1] : 0, window, sinks, nullptr, 0, 1.f, 1.f, llmie_api::dtype_of<T>(),
                                        llmie_api::st()));
}

// No reference launcher: launchDecoderWindowAttention with a learned sink logit per query head (include/llmie.h
// llmie_decoder_mha_sink): head_sink [head_num] fp32 on the device (-INFINITY: no sink for that head), or null = that launcher's call.
// The softmax of head h runs over the keys the mask exposes and one extra column with logit head_sink[h] and no value row.
template <typename T>
void launchDecoderSinkAttention(TensorWrapper<T> *qkv_buf, const T *qkv_bias, int layer, TensorWrapper<T> *k_cache, TensorWrapper<T> *v_cache,
                                TensorWrapper<int> *ctx_len, const void *rope_table, int rotary_dim, TensorWrapper<int> *block_table,
                                int max_seq_len, int window, int sinks, TensorWrapper<float> *head_sink, TensorWrapper<T> *mha_output) {
    const int batch = qkv_buf->shape[0], qkv_head_num = qkv_buf->shape[1], head_size = qkv_buf->shape[2];
    const int kv_head_num = k_cache->shape[2];
    const int head_num = qkv_head_num - 2 * kv_head_num;
    LLM_CHECK_WITH_INFO(!head_sink || head_sink->shape[0] == head_num, "head_sink should be [head_num]");
    if (!block_table) max_seq_len = k_cache->shape[3];
    const size_t ws = llmie_decoder_mha_workspace_bytes(batch, head_num, head_size, max_seq_len);
    LLMIE_CALL(llmie_decoder_mha_sink(qkv_buf->data, qkv_bias, k_cache->data, v_cache->data, mha_output->data, layer, batch, head_num,
                                      kv_head_num, head_size, max_seq_len, ctx_len->data, llmie_api::scratch(ws), ws, rope_table, rotary_dim,
                                      block_table ? block_table->data : nullptr, block_table ? block_table->shape[1] : 0,
                                      block_table ? k_cache->shape[1] : 0, window, sinks, nullptr, 0, 1.f, 1.f,
                                      head_sink ? head_sink->data : nullptr, llmie_api::dtype_of<T>(), llmie_api::st()));
}

// No reference launcher: per-head RMSNorm of the q and k heads of packed rows, in place (include/llmie.h llmie_qk_norm; Qwen3 q_norm /
// k_norm): qkv_buf [rows, head_num + 2 kv_head_num, head_size], q_gamma / k_gamma [head_size] on the device.  The v heads are not
// touched.  Runs between the QKV projection and launchFusedQKVAddBiasAndTransposeAndRope in a per-kernel loop.
template <typename T>
void launchQkNorm(TensorWrapper<T> *qkv_buf, int kv_head_num, TensorWrapper<T> *q_gamma, TensorWrapper<T> *k_gamma, float eps) {
    const int rows = qkv_buf->shape[0], head_num = qkv_buf->shape[1] - 2 * kv_head_num, head_size = qkv_buf->shape[2];
    LLM_CHECK_WITH_INFO(q_gamma->shape[0] == head_size && k_gamma->shape[0] == head_size, "q_gamma / k_gamma should be [head_size]");
    LLMIE_CALL(llmie_qk_norm(qkv_buf->data, rows, head_num, kv_head_num, head_size, q_gamma->data, k_gamma->data, eps, llmie_api::dtype_of<T>(),
                             llmie_api::st()));
}

// No reference launcher: launchDecoderSinkAttention with QK-norm fused in front of the rotation (include/llmie.h
// llmie_decoder_mha_qknorm): q_gamma / k_gamma [head_size] on the device, or both null = that launcher's call.  Bit-identical to
// launchQkNorm on qkv_buf followed by launchDecoderSinkAttention.
template <typename T>
void launchDecoderQkNormAttention(TensorWrapper<T> *qkv_buf, const T *qkv_bias, int layer, TensorWrapper<T> *k_cache, TensorWrapper<T> *v_cache,
                                  TensorWrapper<int> *ctx_len, const void *rope_table, int rotary_dim, TensorWrapper<int> *block_table,
                                  int max_seq_len, int window, int sinks, TensorWrapper<float> *head_sink, TensorWrapper<T> *q_gamma,
                                  TensorWrapper<T> *k_gamma, float qk_eps, TensorWrapper<T> *mha_output) {
    const int batch = qkv_buf->shape[0], qkv_head_num = qkv_buf->shape[1], head_size = qkv_buf->shape[2];
    const int kv_head_num = k_cache->shape[2];
    const int head_num = qkv_head_num - 2 * kv_head_num;
    LLM_CHECK_WITH_INFO(!head_sink || head_sink->shape[0] == head_num, "head_sink should be [head_num]");
    LLM_CHECK_WITH_INFO((!q_gamma || q_gamma->shape[0] == head_size) && (!k_gamma || k_gamma->shape[0] == head_size),
                        "q_gamma / k_gamma should be [head_size]");
    if (!block_table) max_seq_len = k_cache->shape[3];
    const size_t ws = llmie_decoder_mha_workspace_bytes(batch, head_num, head_size, max_seq_len);
    LLMIE_CALL(llmie_decoder_mha_qknorm(qkv_buf->data, qkv_bias, k_cache->data, v_cache->data, mha_output->data, layer, batch, head_num,
                                        kv_head_num, head_size, max_seq_len, ctx_len->data, llmie_api::scratch(ws), ws, rope_table, rotary_dim,
                                        block_table ? block_table->data : nullptr, block_table ? block_table->shape[1] : 0,
                                        block_table ? k_cache->shape[1] : 0, window, sinks, nullptr, 0, 1.f, 1.f,
                                        head_sink ? head_sink->data : nullptr, q_gamma ? q_gamma->data : nullptr,
                                        k_gamma ? k_gamma->data : nullptr, qk_eps, llmie_api::dtype_of<T>(), llmie_api::st()));
}

// No reference launcher: the page ring of windowed sequences (include/llmie.h llmie_kv_window_advance).  block_table [batch,
// max_pages] (in / out, -1 = unmapped), cached_len [batch], new_tokens [batch] or null (one each), status [batch] (0 mapped, 1 no
// dead page: the row is untouched, 2 past the table).  One launch, nothing read by the host.
inline void launchKvWindowAdvance(TensorWrapper<int> *block_table, TensorWrapper<int> *cached_len, TensorWrapper<int> *new_tokens, int window,
                                  int sinks, TensorWrapper<int> *status) {
    const int batch = block_table->shape[0];
    LLM_CHECK_WITH_INFO(cached_len->shape[0] == batch && status->shape[0] == batch, "cached_len and status should be [batch]");
    LLMIE_CALL(llmie_kv_window_advance(block_table->data, block_table->shape[1], cached_len->data, new_tokens ? new_tokens->data : nullptr, batch,
                                       window, sinks, status->data, llmie_api::st()));
}

// No reference launcher: per-row LoRA adapters on top of a projection (include/llmie.h has the semantics).  x [rows, K], y [rows, N]
// (updated in place), slot [rows] (-1: no adapter); table: the device slot table (llmie_lora_table_bytes / llmie_lora_slot_load) of
// `slots` slots and `layers` layers; block_widths: the column blocks of y (q / k / v, gate / up; one block otherwise).  Plans the
// rows (one launch), then shrink + expand.
template <typename T>
void launchLoraApply(TensorWrapper<T> *x, TensorWrapper<T> *y, TensorWrapper<int> *slot, const void *table, int slots, int layers, int layer,
                     int module, const std::vector<int> &block_widths) {
    const int rows = x->shape[0], K = x->shape[1], N = y->shape[1], blocks = static_cast<int>(block_widths.size());
    LLM_CHECK_WITH_INFO(y->shape[0] == rows && slot->shape[0] == rows, "x, y and slot should have the same rows");
    const size_t ws = llmie_lora_workspace_bytes(rows, slots, 64 * (blocks < 1 ? 1 : (blocks > 3 ? 3 : blocks)));
    void *scratch = llmie_api::scratch(ws);
    LLMIE_CALL(llmie_lora_plan(slot->data, nullptr, rows, rows, table, slots, scratch, ws, llmie_api::st()));
    LLMIE_CALL(llmie_lora_apply(x->data, y->data, rows, K, N, blocks, block_widths.data(), table, slots, layers, layer, module, scratch, ws,
                                llmie_api::dtype_of<T>(), llmie_api::st()));
}

// No reference launchers: the mixture-of-experts FFN (include/llmie.h states the arithmetic).  x [rows, H], router [E, H], gate_up
// [E, 2 Ie, H], down [E, H, Ie], resid [rows, H] or null, y [rows, H], all fp16; expert [rows, k] / weight [rows, k] receive the routing.
inline void launchMoeRoute(TensorWrapper<half> *x, TensorWrapper<half> *router, TensorWrapper<int> *expert, TensorWrapper<float> *weight,
                           unsigned flags = 0) {
    const int rows = x->shape[0], H = x->shape[1], E = router->shape[0], k = expert->shape[1];
    LLM_CHECK_WITH_INFO(router->shape[1] == H && expert->shape[0] == rows && weight->shape[0] == rows && weight->shape[1] == k,
                        "router should be [E, H], expert and weight [rows, k]");
    LLMIE_CALL(llmie_moe_route(x->data, router->data, rows, H, E, k, flags, expert->data, weight->data, LLMIE_F16, llmie_api::st()));
}
inline void launchMoeFfn(TensorWrapper<half> *x, TensorWrapper<half> *router, TensorWrapper<half> *gate_up, TensorWrapper<half> *down,
                         TensorWrapper<half> *resid, TensorWrapper<half> *y, int top_k, unsigned flags = 0) {
    const int rows = x->shape[0], H = x->shape[1], E = router->shape[0], Ie = down->shape[2];
    LLM_CHECK_WITH_INFO(router->shape[1] == H && gate_up->shape[0] == E && gate_up->shape[1] == 2 * Ie && gate_up->shape[2] == H &&
                            down->shape[0] == E && down->shape[1] == H && y->shape[0] == rows && y->shape[1] == H,
                        "router [E, H], gate_up [E, 2 Ie, H], down [E, H, Ie], y [rows, H]");
    const size_t ws = llmie_moe_workspace_bytes(rows, H, Ie, E, top_k);
    LLM_CHECK_WITH_INFO(ws > 0, std::string(llmie_last_error()));
    LLMIE_CALL(llmie_moe_ffn(x->data, router->data, gate_up->data, down->data, resid ? resid->data : nullptr, y->data, rows, H, Ie, E, top_k,
                             flags, llmie_api::scratch(ws), ws, LLMIE_F16, llmie_api::st()));
}
// The same under an expert descriptor (include/llmie.h llmie_moe_experts: fp16 or MXFP4 experts, router / gate-up / down biases, the
// clamped SwiGLU); the descriptor's DEVICE pointers are the caller's, inter and experts say their shapes
inline void launchMoeFfnEx(TensorWrapper<half> *x, const llmie_moe_experts &ex, TensorWrapper<half> *resid, TensorWrapper<half> *y, int inter,
                           int experts, int top_k, unsigned flags = 0) {
    const int rows = x->shape[0], H = x->shape[1];
    LLM_CHECK_WITH_INFO(y->shape[0] == rows && y->shape[1] == H && (!resid || (resid->shape[0] == rows && resid->shape[1] == H)),
                        "y and resid should be [rows, H]");
    const size_t ws = llmie_moe_workspace_bytes(rows, H, inter, experts, top_k);
    LLM_CHECK_WITH_INFO(ws > 0, std::string(llmie_last_error()));
    LLMIE_CALL(llmie_moe_ffn_ex(x->data, &ex, resid ? resid->data : nullptr, y->data, rows, H, inter, experts, top_k, flags, llmie_api::scratch(ws), ws,
                                LLMIE_F16, llmie_api::st()));
}

// No reference launchers: MXFP4 weights (include/llmie.h has the format).  w [N, K] fp16 <-> wq: device bytes [N, K/2] (e2m1 codes, low
// nibble = even k) + scale: device bytes [N, K/32] (e8m0); the linear is weight-only under fp16 activations, y [M, N] = x [M, K] . W^T
// (+ bias [N]) (+ residual [M, N], may be y).  From 192 rows the fp16 image of the matrix goes through the adaptors' scratch.
inline void launchQuantizeMxfp4(TensorWrapper<half> *w, uint8_t *wq, uint8_t *scale) {
    LLMIE_CALL(llmie_quantize_mxfp4(w->data, wq, scale, w->shape[0], w->shape[1], llmie_api::st()));
}
inline void launchDequantizeMxfp4(const uint8_t *wq, const uint8_t *scale, TensorWrapper<half> *w16) {
    LLMIE_CALL(llmie_dequantize_mxfp4(wq, scale, w16->data, w16->shape[0], w16->shape[1], llmie_api::st()));
}
inline void launchLinearMxfp4(TensorWrapper<half> *x, const uint8_t *wq, const uint8_t *scale, TensorWrapper<half> *y,
                              TensorWrapper<half> *bias = nullptr, TensorWrapper<half> *residual = nullptr) {
    const int M = x->shape[0], K = x->shape[1], N = y->shape[1];
    LLM_CHECK_WITH_INFO(y->shape[0] == M, "x and y should have the same rows");
    const size_t ws = llmie_linear_workspace_bytes(LLMIE_W_MXFP4, M, K, N);
    LLMIE_CALL(llmie_linear_mxfp4(x->data, wq, scale, y->data, M, K, N, bias ? bias->data : nullptr, residual ? residual->data : nullptr,
                                  ws ? llmie_api::scratch(ws) : nullptr, ws, llmie_api::st()));
}
