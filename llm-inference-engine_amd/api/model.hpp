// C++ API mirror, part 8: BaseModel (src/models/basemodel.h:14-61), LlamaModel<T>
// (src/models/llama/llama.h:14-214, llama.cpp) and llm::create*LLMModel (src/utils/model_utils.h:16-94),
// i.e. everything user_entry.cpp touches.  The reference's model layer never compiled;
// it is used as the specification of names and control flow: prefill once through the context decoder,
// then <= output_token_limit decode steps, LM head on the last token, top-k, sampling, callback.
#pragma once
#include <algorithm>
#include <functional>
#include <utility>
#include <vector>

#include "layers.hpp"
#include "tokenizer.hpp"

using CallBack = std::function<void(int, const char *)>;

class BaseModel {
public:
    std::string model_name;
    hipStream_t stream;
    CublasWrapper *cublas_wrapper;
    BaseAllocator *allocator;
    hipDeviceProp_t *device_prop;

    BaseModel(hipStream_t stream, CublasWrapper *cublas_wrapper, BaseAllocator *allocator,
              hipDeviceProp_t *device_prop = nullptr)
        : stream(stream), cublas_wrapper(cublas_wrapper), allocator(allocator), device_prop(device_prop) {}
    virtual ~BaseModel() = default;

    virtual void loadTokenizer(const std::string &file) = 0;
    virtual void loadWeights(const std::string &file) = 0;
    virtual void loadWeightsFromDummy() = 0;
    virtual std::vector<std::string> makeInput(const std::string &history, int round, const std::string &input) const = 0;
    virtual std::string makeHistory(const std::string &history, int round, const std::string &input,
                                    const std::string &output) const = 0;
    virtual std::string response(const std::vector<std::string> &input, CallBack printRes) = 0;

    // user_entry.cpp:25,39 spells these with capitals (basemodel.h:36-60 with lower case): both exist.
    std::vector<std::string> MakeInput(const std::string &h, int r, const std::string &i) const { return makeInput(h, r, i); }
    std::string MakeHistory(const std::string &h, int r, const std::string &i, const std::string &o) const {
        return makeHistory(h, r, i, o);
    }
    std::string Response(const std::vector<std::string> &input, CallBack printRes) { return response(input, printRes); }
};

template <typename T> class LlamaModel : public BaseModel {
private:
    int head_num, kv_head_num, head_size, inter_size, num_layers, vocab_size, vocab_size_padded;
    float rmsnorm_eps = 1e-5f;  // llama.h:23
    int hidden_units, max_seq_len;
    int pad_token_id = 0, bos_token_id = 1, eos_token_id = 2;
    int layer_id = 0, batch_size = 1, beamwidth = 1, blocks_per_beam = 8, K = 4;
    std::string prompt;
    Tokenizer tokenizer;
    LlamaAttentionStaticParams static_params;
    std::unique_ptr<CublasWrapper> owned_cublas;
    std::unique_ptr<BaseAllocator> owned_allocator;
    std::unique_ptr<LlamaWeight<T>> llama_weights;
    std::unique_ptr<LlamaContextDecoder<T>> context_decoder;
    std::unique_ptr<LlamaSelfDecoder<T>> self_decoder;
    std::vector<LlamaLayerWeight<T> *> layer_ptrs;
    MapStringToInt int_params_of_sample;
    int h_step = 0;

    template <typename U> struct DevBuf {
        U *p = nullptr;
        size_t n = 0;
        ~DevBuf() { if (p) (void)hipFree(p); }
        U *ensure(size_t count) {
            if (count > n) {
                if (p) CHECK(hipFree(p));
                CHECK(hipMalloc(reinterpret_cast<void **>(&p), sizeof(U) * count));
                n = count;
            }
            return p;
        }
    };
    DevBuf<T> d_ctx_in, d_ctx_out, d_dec_in, d_dec_out, d_kcache, d_vcache, d_probs, d_topk_val, d_final_val, d_unused;
    DevBuf<int> d_ids, d_in_len, d_hist_len, d_ctx_len, d_seq_len, d_token, d_topk_id, d_final_id;
    DevBuf<bool> d_finished;
    DevBuf<llmie_sampling_params> d_sparams;
    DevBuf<int> d_penalty_ids, d_penalty_len;
    DevBuf<unsigned char> d_sample_ws, d_score_ws;
    DevBuf<int> d_targets, d_spec;
    DevBuf<uint64_t> d_tree_anc;
    DevBuf<float> d_logprob;
    DevBuf<unsigned char> d_lora_table;   // the adapter slot table (loadAdapter)
    DevBuf<int> d_lora_slot;              // the slot of the one sequence this model runs
    std::vector<int> penalty_ids;   // prompt + generated ids: the penalty history of the SamplingConfig path
    // llmie_sampling_ext of the SamplingConfig path: mask, bias list, stop list, min_step, and the top-N of the last step
    DevBuf<uint32_t> d_mask;
    DevBuf<int> d_bias_ids, d_bias_len, d_stop_ids, d_stop_len, d_min_step, d_top_ids;
    DevBuf<float> d_bias_vals, d_top_logprobs, d_pick_logprob;
    std::vector<int> last_top_ids;
    std::vector<float> last_top_logprobs;
    float last_logprob = 0.f;
    int first_step = 0;   // h_step at the first generated token: min_tokens counts from it

    // SamplingConfig path: llmie_sample_logits(_ext) over the whole vocabulary, seeded by (h_step, sampling.seed)
    int sampleWithConfig(TensorWrapper<T> &probs, TensorWrapper<int> &seq, TensorWrapper<bool> &fin, TensorWrapper<int> &tok) {
        const llmie_sampling_params p{sampling.temperature, sampling.top_k, sampling.top_p, sampling.min_p,
                                      sampling.repetition_penalty, sampling.presence_penalty, sampling.frequency_penalty,
                                      sampling.seed};
        const int n = static_cast<int>(std::min<size_t>(penalty_ids.size(), LLMIE_SAMPLE_MAX_HISTORY));
        const int *recent = penalty_ids.data() + (penalty_ids.size() - n);   // the most recent ids when the context is longer
        int *hist = d_penalty_ids.ensure(std::max(n, 1));
        int *hlen = d_penalty_len.ensure(1);
        CHECK(hipMemcpyAsync(d_sparams.ensure(1), &p, sizeof(p), hipMemcpyHostToDevice, llmie_api::st()));
        if (n) CHECK(hipMemcpyAsync(hist, recent, sizeof(int) * n, hipMemcpyHostToDevice, llmie_api::st()));
        CHECK(hipMemcpyAsync(hlen, &n, sizeof(int), hipMemcpyHostToDevice, llmie_api::st()));
        // the controls of llmie_sampling_ext that are set (an empty struct is llmie_sample_logits itself)
        llmie_sampling_ext ext{};
        std::vector<int> bias_ids;
        std::vector<float> bias_vals;
        const int n_bias = static_cast<int>(sampling.logit_bias.size()), n_stop = static_cast<int>(sampling.stop_token_ids.size());
        const int min_step = first_step + sampling.min_tokens, top_n = sampling.top_logprobs;
        if (!sampling.allowed_tokens.empty()) {
            const size_t words = sampling.allowed_tokens.size();
            LLM_CHECK_WITH_INFO(words >= static_cast<size_t>(vocab_size + 31) / 32, "allowed_tokens holds fewer than vocab_size bits");
            CHECK(hipMemcpyAsync(d_mask.ensure(words), sampling.allowed_tokens.data(), sizeof(uint32_t) * words, hipMemcpyHostToDevice,
                                 llmie_api::st()));
            ext.allowed_mask = d_mask.p;
            ext.mask_stride = static_cast<int>(words);
            ext.mask_rows = 1;
        }
        if (n_bias) {
            for (const auto &e : sampling.logit_bias) {
                bias_ids.push_back(e.first);
                bias_vals.push_back(e.second);
            }
            CHECK(hipMemcpyAsync(d_bias_ids.ensure(n_bias), bias_ids.data(), sizeof(int) * n_bias, hipMemcpyHostToDevice, llmie_api::st()));
            CHECK(hipMemcpyAsync(d_bias_vals.ensure(n_bias), bias_vals.data(), sizeof(float) * n_bias, hipMemcpyHostToDevice, llmie_api::st()));
            CHECK(hipMemcpyAsync(d_bias_len.ensure(1), &n_bias, sizeof(int), hipMemcpyHostToDevice, llmie_api::st()));
            ext.bias_ids = d_bias_ids.p;
            ext.bias_vals = d_bias_vals.p;
            ext.bias_len = d_bias_len.p;
            ext.bias_stride = n_bias;   // above LLMIE_SAMPLE_MAX_BIAS: the call refuses it
        }
        if (n_stop) {
            CHECK(hipMemcpyAsync(d_stop_ids.ensure(n_stop), sampling.stop_token_ids.data(), sizeof(int) * n_stop, hipMemcpyHostToDevice,
                                 llmie_api::st()));
            CHECK(hipMemcpyAsync(d_stop_len.ensure(1), &n_stop, sizeof(int), hipMemcpyHostToDevice, llmie_api::st()));
            ext.stop_ids = d_stop_ids.p;
            ext.stop_len = d_stop_len.p;
            ext.stop_stride = n_stop;
        }
        if (sampling.min_tokens > 0) {
            CHECK(hipMemcpyAsync(d_min_step.ensure(1), &min_step, sizeof(int), hipMemcpyHostToDevice, llmie_api::st()));
            ext.min_step = d_min_step.p;
        }
        if (top_n > 0) {
            ext.top_n = top_n;
            ext.out_top_ids = d_top_ids.ensure(top_n);
            ext.out_top_logprobs = d_top_logprobs.ensure(top_n);
        }
        const size_t ws = llmie_sample_logits_workspace_bytes(batch_size, vocab_size);
        LLMIE_CALL(llmie_sample_logits_ext(probs.data, batch_size, vocab_size, d_sparams.p, hist, std::max(n, 1), hlen, 0, seq.data,
                                           reinterpret_cast<uint8_t *>(fin.data), tok.data, d_pick_logprob.ensure(1), h_step, nullptr,
                                           eos_token_id, d_sample_ws.ensure(ws), ws, llmie_api::dtype_of<T>(), llmie_api::st(), &ext));
        int h_tok = 0;
        last_top_ids.assign(std::max(top_n, 0), -1);
        last_top_logprobs.assign(std::max(top_n, 0), 0.f);
        CHECK(hipMemcpyAsync(&h_tok, tok.data, sizeof(int), hipMemcpyDeviceToHost, llmie_api::st()));
        CHECK(hipMemcpyAsync(&last_logprob, d_pick_logprob.p, sizeof(float), hipMemcpyDeviceToHost, llmie_api::st()));
        if (top_n > 0) {
            CHECK(hipMemcpyAsync(last_top_ids.data(), d_top_ids.p, sizeof(int) * top_n, hipMemcpyDeviceToHost, llmie_api::st()));
            CHECK(hipMemcpyAsync(last_top_logprobs.data(), d_top_logprobs.p, sizeof(float) * top_n, hipMemcpyDeviceToHost, llmie_api::st()));
        }
        CHECK(hipStreamSynchronize(llmie_api::st()));   // (also keeps p / n / the lists alive until the copies are done)
        return h_tok;
    }

    int lmHeadAndSample(T *hidden_row /*[1,H] device*/) {
        const DataType ty = getTensorType<T>(), ti = getTensorType<int>();
        TensorWrapper<T> x(Device::GPU, ty, {batch_size, hidden_units}, hidden_row);
        TensorWrapper<T> unused(Device::GPU, ty, {batch_size, hidden_units}, d_unused.ensure(hidden_units));
        launchRMSNorm(&x, &unused, &llama_weights->out_rmsnorm_weight, rmsnorm_eps, true);      // llama.cpp:247
        TensorWrapper<T> probs(Device::GPU, ty, {batch_size, vocab_size}, d_probs.ensure(vocab_size));
        launchLinearGemm(&x, &llama_weights->post_decoder_embedding_weight, &probs, cublas_wrapper, false, true);  // :282
        if (!sampling.isDefault()) {
            TensorWrapper<int> seq(Device::GPU, ti, {batch_size}, d_seq_len.ensure(1));
            TensorWrapper<bool> fin(Device::GPU, getTensorType<bool>(), {batch_size}, d_finished.ensure(1));
            TensorWrapper<int> tok(Device::GPU, ti, {batch_size}, d_token.ensure(1));
            return sampleWithConfig(probs, seq, fin, tok);
        }
        TensorWrapper<int> topk_id(Device::GPU, ti, {batch_size, beamwidth, blocks_per_beam, K}, d_topk_id.ensure(blocks_per_beam * K));
        TensorWrapper<T> topk_val(Device::GPU, ty, {batch_size, beamwidth, blocks_per_beam, K}, d_topk_val.ensure(blocks_per_beam * K));
        TensorWrapper<int> final_id(Device::GPU, ti, {batch_size * beamwidth, K}, d_final_id.ensure(K));
        TensorWrapper<T> final_val(Device::GPU, ty, {batch_size * beamwidth, K}, d_final_val.ensure(K));
        launchTopKForBeamSearch(&probs, &topk_id, &topk_val, &final_id, &final_val);                // :293
        int_params_of_sample["step"] = h_step;
        TensorWrapper<int> seq(Device::GPU, ti, {batch_size}, d_seq_len.ensure(1));
        TensorWrapper<bool> fin(Device::GPU, getTensorType<bool>(), {batch_size}, d_finished.ensure(1));
        TensorWrapper<int> tok(Device::GPU, ti, {batch_size}, d_token.ensure(1));
        launchSampling(&final_id, &final_val, &seq, &fin, &tok, &int_params_of_sample);            // :304
        int h_tok = 0;
        CHECK(hipMemcpyAsync(&h_tok, tok.data, sizeof(int), hipMemcpyDeviceToHost, llmie_api::st()));  // :314
        CHECK(hipStreamSynchronize(llmie_api::st()));
        return h_tok;
    }

public:
    int output_token_limit = 20;  // llama.h:26

    // Per-request sampling controls (llmie_sampling_params; include/llmie.h has the semantics).  The default keeps the
    // reference's tail bit for bit (top-4 at temperature 1: launchTopKForBeamSearch + launchSampling); any other value
    // samples with llmie_sample_logits over the whole vocabulary, with the prompt and the generated ids as the penalty
    // history and Philox(step, seed) as the draw.  logit_bias / stop_token_ids / min_tokens / top_logprobs / allowed_tokens are
    // the controls of llmie_sampling_ext (same header): the bias list (a value of -INFINITY bans a token), stop tokens that end
    // the reply like EOS, no EOS or stop token among the first min_tokens generated tokens (min_step = the step of the first
    // generated token + min_tokens), the top_logprobs most likely tokens of every step (lastTopIds / lastTopLogprobs), and a
    // host bit mask of the allowed tokens (bit v % 32 of word v / 32; uploaded at every step; empty: unconstrained).
    struct SamplingConfig {
        float temperature = 1.0f;   // 0: greedy
        int top_k = 0;              // 0: off
        float top_p = 1.0f;         // >= 1: off
        float min_p = 0.0f;         // 0: off
        float repetition_penalty = 1.0f;
        float presence_penalty = 0.0f;
        float frequency_penalty = 0.0f;
        uint32_t seed = 0;
        std::vector<std::pair<int, float>> logit_bias;
        std::vector<int> stop_token_ids;
        int min_tokens = 0;
        int top_logprobs = 0;                   // <= LLMIE_SAMPLE_MAX_TOP_N
        std::vector<uint32_t> allowed_tokens;   // >= ceil(vocab_size / 32) words
        bool isDefault() const {
            return temperature == 1.0f && top_k == 0 && top_p == 1.0f && min_p == 0.0f && repetition_penalty == 1.0f &&
                   presence_penalty == 0.0f && frequency_penalty == 0.0f && seed == 0 && logit_bias.empty() &&
                   stop_token_ids.empty() && min_tokens == 0 && top_logprobs == 0 && allowed_tokens.empty();
        }
    };
    SamplingConfig sampling;

    // Per-request LoRA adapters (include/llmie.h llmie_lora_* / llmie_decoder_lora_attach).  loadAdapter puts a host description
    // (rank, scale, per layer and module the DEVICE A / B matrices, which the caller keeps alive) into one of kAdapterSlots slots
    // of the model's device table (nullptr empties the slot); selectAdapter names the slot the NEXT request runs with (-1: the base
    // model).  Both decoders read the table and the slot on the device, so neither call rebuilds anything.  fp16 models only.
    static constexpr int kAdapterSlots = 8;
    void loadAdapter(int slot, const llmie_lora_adapter *desc) {
        // the adapter updates live in the fused engine's lora sequence; the per-kernel loops know none, and a model that runs them
        // must not take an adapter and then ignore it
        LLM_CHECK_WITH_INFO((std::is_same<T, half>::value) && head_size == 128 && EngineHolder<T>::usable(&layer_ptrs),
                            "loadAdapter: adapters need the fused engine (fp16, head_size 128, every layer matrix in HF layout)");
        if (!d_lora_table.p) {
            const size_t bytes = llmie_lora_table_bytes(kAdapterSlots, num_layers);
            CHECK(hipMemsetAsync(d_lora_table.ensure(bytes), 0, bytes, llmie_api::st()));
            const int none = -1;
            CHECK(hipMemcpyAsync(d_lora_slot.ensure(1), &none, sizeof(int), hipMemcpyHostToDevice, llmie_api::st()));
            CHECK(hipStreamSynchronize(llmie_api::st()));
            typename EngineHolder<T>::LoraBinding b;
            b.table = d_lora_table.p, b.slots = kAdapterSlots, b.seq_slot = d_lora_slot.p, b.max_tokens = max_seq_len;
            context_decoder->setLora(b);
            self_decoder->setLora(b);
        }
        LLMIE_CALL(llmie_lora_slot_load(d_lora_table.p, kAdapterSlots, num_layers, slot, desc, llmie_api::st()));
    }
    void selectAdapter(int slot) {
        LLM_CHECK_WITH_INFO(d_lora_table.p != nullptr, "selectAdapter: no adapter was loaded");
        CHECK(hipMemcpyAsync(d_lora_slot.p, &slot, sizeof(int), hipMemcpyHostToDevice, llmie_api::st()));
        CHECK(hipStreamSynchronize(llmie_api::st()));   // (`slot` lives on this frame)
    }
    // Mixture-of-experts layers (include/llmie.h llmie_decoder_moe_attach).  layers: one entry per layer with the DEVICE router
    // [experts, H], gate_up [experts, 2 inter, H] and down [experts, H, inter] (fp16, kept alive by the caller); router == nullptr keeps
    // the layer's dense FFN.  Takes effect from the next prefill / decode call of both decoders; detachExperts goes back.  The expert
    // kernels live in the fused engine, and a model that runs the per-kernel loops must not take experts and then ignore them.
    void attachExperts(const std::vector<llmie_moe_layer> &layers, int inter, int experts, int top_k, unsigned flags = 0) {
        LLM_CHECK_WITH_INFO(static_cast<int>(layers.size()) == num_layers, "attachExperts: one entry per layer");
        LLM_CHECK_WITH_INFO((std::is_same<T, half>::value) && head_size == 128 && EngineHolder<T>::usable(&layer_ptrs),
                            "attachExperts: experts need the fused engine (fp16, head_size 128, every layer matrix in HF layout)");
        LLM_CHECK_WITH_INFO(d_lora_table.p == nullptr, "attachExperts: adapters and experts cannot be used on one model");
        typename EngineHolder<T>::MoeBinding b;
        b.layers = layers, b.inter = inter, b.experts = experts, b.top_k = top_k, b.flags = flags, b.max_tokens = max_seq_len;
        context_decoder->setExperts(b);
        self_decoder->setExperts(b);
    }
    // The same with expert descriptors (include/llmie.h llmie_decoder_moe_attach_ex): MXFP4 or fp16 experts, biases, the clamped SwiGLU
    void attachExperts(const std::vector<llmie_moe_experts> &layers, int inter, int experts, int top_k, unsigned flags = 0) {
        LLM_CHECK_WITH_INFO(static_cast<int>(layers.size()) == num_layers, "attachExperts: one entry per layer");
        LLM_CHECK_WITH_INFO((std::is_same<T, half>::value) && head_size == 128 && EngineHolder<T>::usable(&layer_ptrs),
                            "attachExperts: experts need the fused engine (fp16, head_size 128, every layer matrix in HF layout)");
        LLM_CHECK_WITH_INFO(d_lora_table.p == nullptr, "attachExperts: adapters and experts cannot be used on one model");
        typename EngineHolder<T>::MoeBinding b;
        b.descriptors = layers, b.inter = inter, b.experts = experts, b.top_k = top_k, b.flags = flags, b.max_tokens = max_seq_len;
        context_decoder->setExperts(b);
        self_decoder->setExperts(b);
    }
    void detachExperts() {
        typename EngineHolder<T>::MoeBinding none;
        context_decoder->setExperts(none);
        self_decoder->setExperts(none);
    }
    // Sliding-window attention with sink tokens (include/llmie.h llmie_decoder_set_window): layer_window[l] tokens on layer l (0 keeps
    // that layer global), `sinks` sink tokens on the windowed layers; an empty vector goes back to full attention.  Takes effect from
    // the next prefill / decode call of both decoders.  The windowed kernels live in the fused engine, and a model that runs the
    // per-kernel loops must not take a window and then attend to everything.
    void setAttentionWindow(const std::vector<int> &layer_window, int sinks = 0) {
        LLM_CHECK_WITH_INFO(layer_window.empty() || static_cast<int>(layer_window.size()) == num_layers, "setAttentionWindow: one window per layer");
        LLM_CHECK_WITH_INFO(layer_window.empty() || ((std::is_same<T, half>::value) && head_size == 128 && EngineHolder<T>::usable(&layer_ptrs)),
                            "setAttentionWindow: a window needs the fused engine (fp16, head_size 128, every layer matrix in HF layout)");
        for (int w : layer_window) LLM_CHECK_WITH_INFO(w >= 0, "setAttentionWindow: negative window");
        LLM_CHECK_WITH_INFO(sinks >= 0, "setAttentionWindow: negative sinks");
        context_decoder->setWindow(layer_window, layer_window.empty() ? 0 : sinks);
        self_decoder->setWindow(layer_window, layer_window.empty() ? 0 : sinks);
    }
    // Learned per-head sink logits (gpt-oss `self_attn.sinks`; include/llmie.h llmie_decoder_set_head_sinks): head_sink_dev is a DEVICE
    // array [num_layers, head_num] of fp32 (a loader converts the stored bf16 values) that must stay alive while it is set; nullptr
    // clears.  Takes effect from the next prefill / decode call of both decoders; the per-kernel loops know no sink column.
    void setAttentionSinks(const float *head_sink_dev) {
        LLM_CHECK_WITH_INFO(!head_sink_dev || ((std::is_same<T, half>::value) && head_size == 128 && EngineHolder<T>::usable(&layer_ptrs)),
                            "setAttentionSinks: head sinks need the fused engine (fp16, head_size 128, every layer matrix in HF layout)");
        context_decoder->setHeadSinks(head_sink_dev);
        self_decoder->setHeadSinks(head_sink_dev);
    }
    // QK-norm (Qwen3 `self_attn.q_norm` / `k_norm`; include/llmie.h llmie_decoder_set_qk_norm): q / k are DEVICE arrays [num_layers,
    // head_size] of fp16, 16-byte aligned, that must stay alive while they are set; both nullptr clears.  eps: `rms_norm_eps`.  Takes
    // effect from the next prefill / decode call of both decoders; the per-kernel loops do not normalise q and k.
    void setQkNorm(const half *q, const half *k, float eps) {
        LLM_CHECK_WITH_INFO((q != nullptr) == (k != nullptr), "setQkNorm: q and k gammas go together");
        LLM_CHECK_WITH_INFO(!q || ((std::is_same<T, half>::value) && head_size == 128 && EngineHolder<T>::usable(&layer_ptrs)),
                            "setQkNorm: QK-norm needs the fused engine (fp16, head_size 128, every layer matrix in HF layout)");
        context_decoder->setQkNorm(q, k, eps);
        self_decoder->setQkNorm(q, k, eps);
    }
    // RoPE frequency scaling (`rope_scaling` of a config.json; include/llmie.h llmie_rope_scaling): both decoders' engines refill their
    // (cos, sin) table; kind LLMIE_ROPE_NONE goes back to the unscaled table.  One synchronous copy per engine, at its next call.
    void setRopeScaling(const llmie_rope_scaling &scaling) {
        LLM_CHECK_WITH_INFO(scaling.kind == LLMIE_ROPE_NONE || ((std::is_same<T, half>::value) && head_size == 128 && EngineHolder<T>::usable(&layer_ptrs)),
                            "setRopeScaling: a scaled table needs the fused engine (fp16, head_size 128, every layer matrix in HF layout)");
        std::vector<float> probe(static_cast<size_t>(head_size));   // the struct's own checks, before an engine meets it
        LLM_CHECK_WITH_INFO(llmie_rope_table_fill(probe.data(), 1, head_size, head_size, 10000.f, scaling.kind == LLMIE_ROPE_NONE ? nullptr : &scaling) == LLMIE_OK,
                            std::string(llmie_last_error()));
        context_decoder->setRopeScaling(scaling);
        self_decoder->setRopeScaling(scaling);
    }
    // the last step of the SamplingConfig path: the top_logprobs most likely tokens of the raw row (id -1 / -INFINITY past the
    // row's valid tokens) and the picked token's raw log-probability
    const std::vector<int> &lastTopIds() const { return last_top_ids; }
    const std::vector<float> &lastTopLogprobs() const { return last_top_logprobs; }
    float lastLogprob() const { return last_logprob; }
    // the [1, vocab_size] logits of the last step (device), as the sampler read them
    const T *lastLogits() const { return d_probs.p; }
    bool isStopToken(int id) const {
        return id == eos_token_id ||
               std::find(sampling.stop_token_ids.begin(), sampling.stop_token_ids.end(), id) != sampling.stop_token_ids.end();
    }

    LlamaModel(int head_num, int kv_head_num, int head_size, int inter_size, int num_layers, int vocab_size,
               const LlamaAttentionStaticParams &attention_static_params, int max_seq_len, hipStream_t stream,
               CublasWrapper *cublas_wrapper, BaseAllocator *allocator, hipDeviceProp_t *device_prop = nullptr)
        : BaseModel(stream, cublas_wrapper, allocator, device_prop), head_num(head_num), kv_head_num(kv_head_num),
          head_size(head_size), inter_size(inter_size), num_layers(num_layers), vocab_size(vocab_size),
          vocab_size_padded(vocab_size), hidden_units(head_num * head_size), max_seq_len(max_seq_len),
          static_params(attention_static_params) {
        model_name = "llama";
        int_params_of_sample["vocab_size"] = vocab_size;
        int_params_of_sample["end_id"] = eos_token_id;
        llama_weights = std::make_unique<LlamaWeight<T>>(head_num, kv_head_num, head_size, inter_size, vocab_size,
                                                         num_layers, false, getWeightType<T>());
        layer_ptrs = llama_weights->layerPointers();
        self_decoder = std::make_unique<LlamaSelfDecoder<T>>(head_num, kv_head_num, head_size, inter_size, num_layers,
                                                             static_params, rmsnorm_eps, stream, cublas_wrapper, allocator);
        context_decoder = std::make_unique<LlamaContextDecoder<T>>(head_num, kv_head_num, head_size, inter_size,
                                                                   num_layers, &static_params, rmsnorm_eps, stream,
                                                                   cublas_wrapper, allocator);
        const size_t kv = static_cast<size_t>(num_layers) * batch_size * kv_head_num * max_seq_len * head_size;
        CHECK(hipMemset(d_kcache.ensure(kv), 0, sizeof(T) * kv));
        CHECK(hipMemset(d_vcache.ensure(kv), 0, sizeof(T) * kv));
    }
    // model_utils.h creates the GEMM context and allocator on the stack and releases the model: keep them alive here
    void adopt(std::unique_ptr<CublasWrapper> c, std::unique_ptr<BaseAllocator> a) {
        owned_cublas = std::move(c);
        owned_allocator = std::move(a);
    }
    void loadTokenizer(const std::string &file) override { tokenizer.Initialize(file); }
    void loadWeights(const std::string &dir) override { llama_weights->loadWeightsFromFile(dir); }
    void loadWeightsFromDummy() override { llama_weights->loadWeightsFromDummy(); }
    LlamaWeight<T> *weights() { return llama_weights.get(); }

    // llama.cpp:128-150
    std::vector<std::string> makeInput(const std::string &history, int round, const std::string &input) const override {
        return {(round == 0 ? "" : history) + input, history, input};
    }
    std::string makeHistory(const std::string &history, int round, const std::string &input,
                            const std::string &output) const override {
        return (round == 0 ? prompt : history) + input + output;
    }

    // llama.cpp:165-217: prefill of `ids` on top of `history_len` cached tokens; returns the first new token
    int generateFirstToken(const std::vector<int> &ids, int history_len) {
        T *ctx_out = runContext(ids, history_len);
        first_step = h_step;
        return lmHeadAndSample(ctx_out + (ids.size() - 1) * hidden_units);  // last token only (:262-279)
    }

    // Log-probability of every prompt token after the first under the model: the prefill of generateFirstToken (no history), then
    // llmie_score_tokens on all n rows of the context decoder's output, row i scoring ids[i + 1] (the last row has no target).
    // Returns the n - 1 values log P(ids[i] | ids[0..i)), i = 1 .. n - 1.  fp16 models only (T = float throws: unsupported).  The
    // model is left as after a prefill of `ids`: continueWith can follow.
    std::vector<float> scoreTokens(const std::vector<int> &ids) {
        const int n = static_cast<int>(ids.size());
        const T *ctx_out = runContext(ids, 0);
        std::vector<int> targets(ids.begin() + 1, ids.end());
        targets.push_back(-1);
        CHECK(hipMemcpyAsync(d_targets.ensure(n), targets.data(), sizeof(int) * n, hipMemcpyHostToDevice, llmie_api::st()));
        const size_t ws = llmie_score_tokens_workspace_bytes(n, hidden_units, vocab_size);
        LLMIE_CALL(llmie_score_tokens(ctx_out, llama_weights->out_rmsnorm_weight.gamma, rmsnorm_eps,
                                      llama_weights->post_decoder_embedding_weight.data, nullptr, d_targets.p, d_logprob.ensure(n),
                                      nullptr, nullptr, nullptr, n, hidden_units, vocab_size, d_score_ws.ensure(std::max<size_t>(ws, 16)),
                                      ws, llmie_api::dtype_of<T>(), llmie_api::st()));
        std::vector<float> logprob(n);
        CHECK(hipMemcpyAsync(logprob.data(), d_logprob.p, sizeof(float) * n, hipMemcpyDeviceToHost, llmie_api::st()));
        CHECK(hipStreamSynchronize(llmie_api::st()));   // (also keeps `targets` alive until its copy is done)
        logprob.pop_back();
        return logprob;
    }
    // One speculative step.  `last` -- emitted, not yet in the cache -- and `drafts` (<= LLMIE_SPEC_MAX_DRAFT guesses of what follows it:
    // an n-gram lookup, a small model) run as ONE chunk of the context decoder on top of the cached tokens; llmie_spec_verify then
    // emits what plain decoding would have emitted from those logits: 1 .. drafts.size() + 1 tokens, the accepted drafts and one
    // more.  The rejected drafts' cache rows are scratch: the next call overwrites them.  The pick behind cache position c draws at
    // Philox step c + 1, as continueWith does.  Samples with the seven llmie_sampling_params of `sampling` over the whole vocabulary
    // (temperature 0: greedy; the reference's top-4 tail and the llmie_sampling_ext controls have no form here), the prompt and the
    // generated ids as the penalty history.  Stops behind EOS.  lastLogits() holds the chunk's [drafts.size() + 1, vocab_size] rows.
    std::vector<int> speculativeStep(int last, const std::vector<int> &drafts) {
        const int k = static_cast<int>(drafts.size()), cached = h_step;
        LLM_CHECK_WITH_INFO(k >= 1 && k <= LLMIE_SPEC_MAX_DRAFT, "1 .. LLMIE_SPEC_MAX_DRAFT drafts");
        std::vector<int> chunk{last};
        chunk.insert(chunk.end(), drafts.begin(), drafts.end());
        const size_t fed = penalty_ids.size();
        T *ctx_out = runContext(chunk, cached);   // (checks the fit; resets finished / seq_len; h_step = cached + k + 1)
        penalty_ids.resize(fed);
        penalty_ids.push_back(last);
        const DataType ty = getTensorType<T>();
        TensorWrapper<T> x(Device::GPU, ty, {k + 1, hidden_units}, ctx_out);
        TensorWrapper<T> unused(Device::GPU, ty, {k + 1, hidden_units}, d_unused.ensure(static_cast<size_t>(k + 1) * hidden_units));
        launchRMSNorm(&x, &unused, &llama_weights->out_rmsnorm_weight, rmsnorm_eps, true);
        TensorWrapper<T> probs(Device::GPU, ty, {k + 1, vocab_size}, d_probs.ensure(static_cast<size_t>(k + 1) * vocab_size));
        launchLinearGemm(&x, &llama_weights->post_decoder_embedding_weight, &probs, cublas_wrapper, false, true);
        const llmie_sampling_params p{sampling.temperature, sampling.top_k, sampling.top_p, sampling.min_p,
                                      sampling.repetition_penalty, sampling.presence_penalty, sampling.frequency_penalty,
                                      sampling.seed};
        // the penalty history: the most recent ids, with room for the k + 1 picks behind them
        const int room = LLMIE_SAMPLE_MAX_HISTORY - (k + 1);
        const int n = static_cast<int>(std::min<size_t>(penalty_ids.size(), room)), stride = n + k + 1;
        int *hist = d_penalty_ids.ensure(stride), *hlen = d_penalty_len.ensure(1);
        int *spec = d_spec.ensure(2 * (k + 1) + 1);   // drafts [k] | tokens [k + 1] | count
        CHECK(hipMemcpyAsync(d_sparams.ensure(1), &p, sizeof(p), hipMemcpyHostToDevice, llmie_api::st()));
        CHECK(hipMemcpyAsync(hist, penalty_ids.data() + (penalty_ids.size() - n), sizeof(int) * n, hipMemcpyHostToDevice, llmie_api::st()));
        CHECK(hipMemcpyAsync(hlen, &n, sizeof(int), hipMemcpyHostToDevice, llmie_api::st()));
        CHECK(hipMemcpyAsync(spec, drafts.data(), sizeof(int) * k, hipMemcpyHostToDevice, llmie_api::st()));
        const size_t ws = llmie_spec_verify_workspace_bytes(1, k, vocab_size);
        LLMIE_CALL(llmie_spec_verify(probs.data, 1, k, vocab_size, spec, nullptr, d_sparams.p, hist, stride, hlen, 1, d_seq_len.p,
                                     reinterpret_cast<uint8_t *>(d_finished.p), spec + k, spec + 2 * k + 1, nullptr, nullptr, nullptr,
                                     nullptr, cached + 1, nullptr, eos_token_id, d_sample_ws.ensure(ws), ws, llmie_api::dtype_of<T>(),
                                     llmie_api::st(), nullptr));
        std::vector<int> got(k + 2);
        CHECK(hipMemcpyAsync(got.data(), spec + k, sizeof(int) * (k + 2), hipMemcpyDeviceToHost, llmie_api::st()));
        CHECK(hipStreamSynchronize(llmie_api::st()));   // (also keeps p / n / drafts alive until the copies are done)
        const int count = got[k + 1];
        got.resize(count);
        penalty_ids.insert(penalty_ids.end(), got.begin(), got.end() - 1);   // the last pick joins when it is fed
        h_step = cached + count;   // `last` and the accepted drafts are cached; the last pick is not
        return got;
    }
    // speculativeStep with a draft TREE (include/llmie.h llmie_spec_verify_tree): node 0 is `last`, node i >= 1 carries draft_ids[i - 1]
    // and hangs on parent[i] (parent[0] is not read; parent < child), n = draft_ids.size() + 1 <= LLMIE_SPEC_TREE_MAX_NODES.  One
    // forward over the n nodes with the tree set on the context decoder (a node sees the history and its ancestors, and is rotated at
    // cached + depth), the LM head on every row, the walk, then llmie_kv_tree_commit moves the accepted nodes' K / V rows to the slots
    // cached + m.  Returns the emitted tokens (path: the node of each, if wanted); state moves as in speculativeStep.  Needs the
    // fused engine (fp16, head_size 128): the per-kernel loops know no tree.  lastLogits() holds the [n, vocab_size] rows.
    std::vector<int> speculativeTreeStep(int last, const std::vector<int> &draft_ids, const std::vector<int> &parent, std::vector<int> *path = nullptr) {
        const int n = static_cast<int>(draft_ids.size()) + 1, cached = h_step;
        LLM_CHECK_WITH_INFO(n >= 1 && n <= LLMIE_SPEC_TREE_MAX_NODES && static_cast<int>(parent.size()) == n, "1 .. LLMIE_SPEC_TREE_MAX_NODES nodes, one parent each");
        LLM_CHECK_WITH_INFO((std::is_same<T, half>::value) && head_size == 128 && EngineHolder<T>::usable(&layer_ptrs),
                            "speculativeTreeStep: tree attention needs the fused engine (fp16, head_size 128, every layer matrix in HF layout)");
        std::vector<int> chunk{last};
        chunk.insert(chunk.end(), draft_ids.begin(), draft_ids.end());
        // tree [n]: parent | depth | ids | tokens | path | count, then the 64-bit masks
        int *tree = d_spec.ensure(5 * n + 1);
        uint64_t *anc = d_tree_anc.ensure(n);
        int *d_parent = tree, *d_depth = tree + n, *d_node_ids = tree + 2 * n, *d_tokens = tree + 3 * n, *d_path = tree + 4 * n, *d_count = tree + 5 * n;
        CHECK(hipMemcpyAsync(d_parent, parent.data(), sizeof(int) * n, hipMemcpyHostToDevice, llmie_api::st()));
        CHECK(hipMemcpyAsync(d_node_ids, chunk.data(), sizeof(int) * n, hipMemcpyHostToDevice, llmie_api::st()));
        LLMIE_CALL(llmie_spec_tree_prepare(d_parent, nullptr, 1, n, d_depth, anc, llmie_api::st()));
        const size_t fed = penalty_ids.size();
        // the tree is set for this one prefill call only: the guard clears it on every way out, an exception of runContext (a chunk that
        // does not fit) included, so that no later prefill reads this step's buffers (takes effect at the next prefill call)
        struct TreeGuard {
            LlamaContextDecoder<T> *dec;
            ~TreeGuard() { dec->setTree(nullptr, nullptr, 0); }
        };
        T *ctx_out = nullptr;
        {
            TreeGuard guard{context_decoder.get()};
            context_decoder->setTree(d_depth, anc, n);
            ctx_out = runContext(chunk, cached);   // (checks the fit; resets finished / seq_len; leaves cached in d_hist_len)
        }
        penalty_ids.resize(fed);
        penalty_ids.push_back(last);
        const DataType ty = getTensorType<T>();
        TensorWrapper<T> x(Device::GPU, ty, {n, hidden_units}, ctx_out);
        TensorWrapper<T> unused(Device::GPU, ty, {n, hidden_units}, d_unused.ensure(static_cast<size_t>(n) * hidden_units));
        launchRMSNorm(&x, &unused, &llama_weights->out_rmsnorm_weight, rmsnorm_eps, true);
        TensorWrapper<T> probs(Device::GPU, ty, {n, vocab_size}, d_probs.ensure(static_cast<size_t>(n) * vocab_size));
        launchLinearGemm(&x, &llama_weights->post_decoder_embedding_weight, &probs, cublas_wrapper, false, true);
        const llmie_sampling_params p{sampling.temperature, sampling.top_k, sampling.top_p, sampling.min_p,
                                      sampling.repetition_penalty, sampling.presence_penalty, sampling.frequency_penalty,
                                      sampling.seed};
        const int room = LLMIE_SAMPLE_MAX_HISTORY - n;
        const int nh = static_cast<int>(std::min<size_t>(penalty_ids.size(), room)), stride = nh + n;
        int *hist = d_penalty_ids.ensure(stride), *hlen = d_penalty_len.ensure(1);
        CHECK(hipMemcpyAsync(d_sparams.ensure(1), &p, sizeof(p), hipMemcpyHostToDevice, llmie_api::st()));
        CHECK(hipMemcpyAsync(hist, penalty_ids.data() + (penalty_ids.size() - nh), sizeof(int) * nh, hipMemcpyHostToDevice, llmie_api::st()));
        CHECK(hipMemcpyAsync(hlen, &nh, sizeof(int), hipMemcpyHostToDevice, llmie_api::st()));
        const size_t ws = llmie_spec_verify_tree_workspace_bytes(1, n, vocab_size);
        LLMIE_CALL(llmie_spec_verify_tree(probs.data, 1, n, vocab_size, d_node_ids, d_parent, d_depth, anc, d_sparams.p, hist, stride, hlen, 1,
                                          d_seq_len.p, reinterpret_cast<uint8_t *>(d_finished.p), d_tokens, d_count, d_path, nullptr, nullptr,
                                          nullptr, nullptr, cached + 1, nullptr, eos_token_id, d_sample_ws.ensure(ws), ws,
                                          llmie_api::dtype_of<T>(), llmie_api::st(), nullptr));
        // base_len = the history length the forward ran with (d_hist_len, which nothing advanced)
        LLMIE_CALL(llmie_kv_tree_commit(d_kcache.p, d_vcache.p, nullptr, d_hist_len.p, d_path, d_count, 1, n, num_layers, kv_head_num, max_seq_len,
                                        head_size, 0, 0, static_cast<int>(sizeof(T)), llmie_api::st()));
        std::vector<int> got(2 * n + 1);
        CHECK(hipMemcpyAsync(got.data(), d_tokens, sizeof(int) * (2 * n + 1), hipMemcpyDeviceToHost, llmie_api::st()));
        CHECK(hipStreamSynchronize(llmie_api::st()));   // (also keeps p / nh / the tree alive until the copies are done)
        const int count = got[2 * n];
        if (path) path->assign(got.begin() + n, got.begin() + n + count);
        got.resize(count);
        penalty_ids.insert(penalty_ids.end(), got.begin(), got.end() - 1);   // the last pick joins when it is fed
        h_step = cached + count;   // `last` and the accepted nodes are cached, in place; the last pick is not
        return got;
    }
    // the context decoder's output [n, hidden_units] of the last prefill (generateFirstToken normalises its last row in place)
    const T *contextOutput() const { return d_ctx_out.p; }
    // the K cache [num_layers, 1, kv_head_num, max_seq_len, head_size] and the number of its rows that are valid (the cached tokens)
    const T *keyCache() const { return d_kcache.p; }
    int cachedLength() const { return h_step; }
    // the self decoder's output [1, hidden_units] of the last decode step, before the final norm
    const T *decodeOutput() const { return d_dec_out.p; }
    // the decode step response() runs after a prefill: token `id` joins the context, then generateNextToken
    int continueWith(int id) {
        LLM_CHECK_WITH_INFO(h_step + 1 < max_seq_len, "context does not fit max_seq_len");
        ++h_step;
        return generateNextToken(id);
    }

private:
    // embedding + context decoder over `ids` on top of `history_len` cached tokens -> its output [n, hidden_units] (device)
    T *runContext(const std::vector<int> &ids, int history_len) {
        const int n = static_cast<int>(ids.size());
        LLM_CHECK_WITH_INFO(n > 0 && history_len + n < max_seq_len, "prompt does not fit max_seq_len");
        const DataType ty = getTensorType<T>(), ti = getTensorType<int>();
        const int ctx = history_len + n;
        CHECK(hipMemcpy(d_ids.ensure(n), ids.data(), sizeof(int) * n, hipMemcpyHostToDevice));
        CHECK(hipMemcpy(d_in_len.ensure(1), &n, sizeof(int), hipMemcpyHostToDevice));
        CHECK(hipMemcpy(d_hist_len.ensure(1), &history_len, sizeof(int), hipMemcpyHostToDevice));
        CHECK(hipMemcpy(d_ctx_len.ensure(1), &ctx, sizeof(int), hipMemcpyHostToDevice));
        bool f = false;
        CHECK(hipMemcpy(d_finished.ensure(1), &f, sizeof(bool), hipMemcpyHostToDevice));
        CHECK(hipMemset(d_seq_len.ensure(1), 0, sizeof(int)));
        TensorWrapper<int> input_ids(Device::GPU, ti, {n}, d_ids.p);
        TensorWrapper<T> ctx_in(Device::GPU, ty, {n, hidden_units}, d_ctx_in.ensure(static_cast<size_t>(n) * hidden_units));
        TensorWrapper<T> ctx_out(Device::GPU, ty, {n, hidden_units}, d_ctx_out.ensure(static_cast<size_t>(n) * hidden_units));
        launchInputEmbedding<T>(&input_ids, &ctx_in, &llama_weights->pre_decoder_embedding_weight);
        TensorWrapper<int> in_len(Device::GPU, ti, {1}, d_in_len.p), hist(Device::GPU, ti, {1}, d_hist_len.p);
        TensorWrapper<int> ctx_len(Device::GPU, ti, {1}, d_ctx_len.p);
        TensorWrapper<int> layer(Device::CPU, ti, {1}, &layer_id);
        TensorWrapper<T> kc(Device::GPU, ty, {num_layers, batch_size, kv_head_num, max_seq_len, head_size}, d_kcache.p);
        TensorWrapper<T> vc(Device::GPU, ty, {num_layers, batch_size, kv_head_num, max_seq_len, head_size}, d_vcache.p);
        TensorMap decoder_inputs{{"decoder_input", &ctx_in}, {"history_length", &hist}, {"input_length", &in_len},
                                 {"context_length", &ctx_len}, {"layer_id", &layer}};
        TensorMap decoder_outputs{{"decoder_output", &ctx_out}, {"all_k_cache", &kc}, {"all_v_cache", &vc}};
        LlamaAttentionDynamicParams dyn{};
        dyn.batch_size = 1;
        dyn.num_tokens = n;
        dyn.max_q_len = n;
        dyn.max_k_len = ctx;
        dyn.num_layers = num_layers;
        context_decoder->forward(&decoder_inputs, &layer_ptrs, &decoder_outputs, &dyn);
        h_step = ctx;
        if (history_len == 0) penalty_ids.clear();
        penalty_ids.insert(penalty_ids.end(), ids.begin(), ids.end());
        return ctx_out.data;
    }

public:

    // llama.cpp:219-257: one decode step for token `id`; h_step = context length including it
    int generateNextToken(int id) {
        const DataType ty = getTensorType<T>(), ti = getTensorType<int>();
        CHECK(hipMemcpy(d_ids.ensure(1), &id, sizeof(int), hipMemcpyHostToDevice));
        TensorWrapper<int> input_ids(Device::GPU, ti, {1}, d_ids.p);
        TensorWrapper<T> dec_in(Device::GPU, ty, {1, hidden_units}, d_dec_in.ensure(hidden_units));
        TensorWrapper<T> dec_out(Device::GPU, ty, {1, hidden_units}, d_dec_out.ensure(hidden_units));
        launchInputEmbedding<T>(&input_ids, &dec_in, &llama_weights->pre_decoder_embedding_weight);
        TensorWrapper<int> step(Device::CPU, ti, {1}, &h_step);
        TensorWrapper<int> layer(Device::CPU, ti, {1}, &layer_id);
        TensorWrapper<bool> fin(Device::GPU, getTensorType<bool>(), {1}, d_finished.ensure(1));
        TensorWrapper<T> kc(Device::GPU, ty, {num_layers, batch_size, kv_head_num, max_seq_len, head_size}, d_kcache.p);
        TensorWrapper<T> vc(Device::GPU, ty, {num_layers, batch_size, kv_head_num, max_seq_len, head_size}, d_vcache.p);
        TensorMap decoder_inputs{{"decoder_input", &dec_in}, {"step", &step}, {"finished", &fin}, {"layer_id", &layer}};
        TensorMap decoder_outputs{{"decoder_output", &dec_out}, {"all_k_cache", &kc}, {"all_v_cache", &vc}};
        LlamaAttentionDynamicParams dyn{};
        dyn.batch_size = 1;
        dyn.num_layers = num_layers;
        self_decoder->forward(&decoder_inputs, &layer_ptrs, &decoder_outputs, &dyn);
        penalty_ids.push_back(id);
        return lmHeadAndSample(dec_out.data);
    }

    // llama.cpp:322-398.  Returns the generated text; printRes(index, piece), index -1 = end of reply.
    std::vector<int> last_token_ids;
    const Tokenizer &getTokenizer() const { return tokenizer; }
    std::string response(const std::vector<std::string> &input, CallBack printRes) override {
        const std::vector<int> history_ids = input.size() > 1 && !input[1].empty() ? tokenizer.Encode(input[1]) : std::vector<int>();
        const std::vector<int> cur_ids = tokenizer.Encode(input.empty() ? std::string() : input[0]);
        (void)history_ids;  // batch-1, single round: the whole context is re-prefilled, as the reference does
        last_token_ids.clear();
        std::string ret_string;
        int ret = 0;
        for (int index = 0; index < output_token_limit; ++index) {
            if (index == 0) {
                ret = generateFirstToken(cur_ids, 0);
            } else {
                if (h_step + 1 >= max_seq_len) break;
                ++h_step;  // the token generated last round becomes part of the context
                ret = generateNextToken(ret);
                if (isStopToken(ret)) break;
            }
            last_token_ids.push_back(ret);
            const std::string piece = tokenizer.Decode({ret});
            ret_string += piece;
            if (printRes) printRes(index, piece.c_str());
        }
        if (printRes) printRes(-1, ret_string.c_str());
        return ret_string;
    }
};

namespace llm {
// Replaces the JSON file read from a hard-coded home path (model_utils.h:22-40, llama_config.json):
// Llama-2-7B defaults, editable before the first create* call.
struct ModelConfig {
    int head_num = 32, kv_head_num = 32, head_size = 128, inter_size = 11008, num_layers = 32, max_seq_len = 2048;
    int vocab_size = 32000;
    int rotary_embedding_dim = 128, max_position_embeddings = 2048;
    float rotary_embedding_base = 10000.0f;
    bool use_dynamic_ntk = false, attn_bias = false;
};
inline ModelConfig &config() {
    static ModelConfig c;
    return c;
}

template <typename T> BaseModel *createModelWithName(const std::string &model_name) {
    LLM_CHECK_WITH_INFO(model_name == "llama", "Currently, only llama models are supported!");
    const ModelConfig &c = config();
    LlamaAttentionStaticParams sp{};
    sp.rotary_embedding_dim = c.rotary_embedding_dim;
    sp.rotary_embedding_base = c.rotary_embedding_base;
    sp.max_position_embeddings = c.max_position_embeddings;
    sp.use_dynamic_ntk = c.use_dynamic_ntk;
    auto cublas_wrapper = std::make_unique<CublasWrapper>(nullptr, nullptr);
    if (std::is_same<T, half>::value) cublas_wrapper->setFP16GemmConfig();
    else cublas_wrapper->setFP32GemmConfig();
    std::unique_ptr<BaseAllocator> allocator = std::make_unique<CudaAllocator>();
    static hipDeviceProp_t device_prop;
    CHECK(hipGetDeviceProperties(&device_prop, 0));
    auto model = std::make_unique<LlamaModel<T>>(c.head_num, c.kv_head_num, c.head_size, c.inter_size, c.num_layers,
                                                 c.vocab_size, sp, c.max_seq_len, nullptr, cublas_wrapper.get(),
                                                 allocator.get(), &device_prop);
    model->adopt(std::move(cublas_wrapper), std::move(allocator));
    return model.release();
}
template <typename T> BaseModel *createDummyLLMModel(const std::string &tokenizer_file) {
    auto model = std::unique_ptr<BaseModel>(createModelWithName<T>("llama"));
    model->loadTokenizer(tokenizer_file);
    model->loadWeightsFromDummy();
    return model.release();
}
template <typename T> BaseModel *createRealLLMModel(const std::string &model_dir, const std::string &tokenizer_file) {
    auto model = std::unique_ptr<BaseModel>(createModelWithName<T>("llama"));
    std::cout << "Start creating model..." << std::endl;
    model->loadTokenizer(tokenizer_file);
    model->loadWeights(model_dir);
    std::cout << "Finish creating model..." << std::endl;
    return model.release();
}
}  // namespace llm
