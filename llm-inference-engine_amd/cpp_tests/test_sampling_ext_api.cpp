// LlamaModel::SamplingConfig's logit_bias / stop_token_ids / min_tokens / top_logprobs / allowed_tokens on the dummy-weight model:
// a step equals llmie_sample_logits_ext called here on the step's logits with the same controls (what the Python binding calls),
// the mask / ban / min_tokens / stop rules hold over a reply, and a default config keeps the reference's tail.  Run on the GPU
// by tests/test_sampling_ext_cpp_gpu.py; exit code != 0 on any failure.
#include <cstdlib>
#include <memory>

#include "../src/utils/model_utils.h"
#include "test_common.hpp"

template <typename T> static void run(const char *name) {
    llm::ModelConfig &c = llm::config();
    c.head_num = 4; c.kv_head_num = 4; c.head_size = 32; c.inter_size = 344; c.num_layers = 2;
    c.max_seq_len = 64; c.vocab_size = 30000; c.rotary_embedding_dim = 32;
    const int V = c.vocab_size, EOS = 2;
    srand(42);
    std::unique_ptr<BaseModel> model(llm::createDummyLLMModel<T>("/nonexistent/tokenizer.bin"));
    LlamaModel<T> *lm = static_cast<LlamaModel<T> *>(model.get());
    const auto fail = [&](const char *what) { std::printf("FAIL %s: %s\n", name, what); ++g_failures; };
    const auto tokens = [&]() {
        (void)model->Response(model->MakeInput("", 0, "Hey, are you conscious? Can you talk to me?"), nullptr);
        return lm->last_token_ids;
    };
    const std::vector<int> untouched = tokens();

    // one step with every control, against the C entry on the same logits
    const std::vector<int> ids = {1, 17, 29999, 5, 5, 1234, 42, 7};
    typename LlamaModel<T>::SamplingConfig plain;
    plain.temperature = 0.0f;
    lm->sampling = plain;
    const int free_pick = lm->generateFirstToken(ids, 0);
    typename LlamaModel<T>::SamplingConfig cfg;
    cfg.temperature = 0.7f;
    cfg.top_p = 0.95f;
    cfg.seed = 5;
    cfg.top_logprobs = 6;
    cfg.min_tokens = 3;
    cfg.stop_token_ids = {free_pick, 11};
    cfg.logit_bias = {{100, 2.5f}, {200, -1.0f}, {100, -3.0f}, {V + 9, 4.0f}, {300, -INFINITY}, {EOS, 100.0f}};
    cfg.allowed_tokens.assign((V + 31) / 32, 0u);
    for (int v = 0; v < V; ++v)
        if (v % 3 != 1 || v == free_pick || v == EOS) cfg.allowed_tokens[v / 32] |= 1u << (v % 32);
    lm->sampling = cfg;
    const int tok = lm->generateFirstToken(ids, 0);
    const std::vector<int> top_ids = lm->lastTopIds();
    const std::vector<float> top_lp = lm->lastTopLogprobs();
    {
        const llmie_sampling_params p{cfg.temperature, cfg.top_k, cfg.top_p, cfg.min_p, cfg.repetition_penalty, cfg.presence_penalty,
                                      cfg.frequency_penalty, cfg.seed};
        DeviceArray<llmie_sampling_params> d_p(std::vector<llmie_sampling_params>{p});
        std::vector<int> bi;
        std::vector<float> bv;
        for (const auto &e : cfg.logit_bias) { bi.push_back(e.first); bv.push_back(e.second); }
        DeviceArray<uint32_t> d_mask(cfg.allowed_tokens);
        DeviceArray<int> d_bi(bi), d_bl(std::vector<int>{static_cast<int>(bi.size())}), d_si(cfg.stop_token_ids),
            d_sl(std::vector<int>{static_cast<int>(cfg.stop_token_ids.size())}),
            d_ms(std::vector<int>{static_cast<int>(ids.size()) + cfg.min_tokens}), d_seq(std::vector<int>{0}), d_out(1), d_tid(6);
        DeviceArray<float> d_bv(bv), d_tlp(6), d_lp(1);
        DeviceArray<uint8_t> d_fin(std::vector<uint8_t>{0});
        const size_t ws = llmie_sample_logits_workspace_bytes(1, V);
        DeviceArray<unsigned char> d_ws(ws);
        llmie_sampling_ext e{};
        e.allowed_mask = d_mask.d; e.mask_stride = static_cast<int>(cfg.allowed_tokens.size()); e.mask_rows = 1;
        e.bias_ids = d_bi.d; e.bias_vals = d_bv.d; e.bias_len = d_bl.d; e.bias_stride = static_cast<int>(bi.size());
        e.stop_ids = d_si.d; e.stop_len = d_sl.d; e.stop_stride = static_cast<int>(cfg.stop_token_ids.size());
        e.min_step = d_ms.d;
        e.top_n = 6; e.out_top_ids = d_tid.d; e.out_top_logprobs = d_tlp.d;
        LLMIE_CALL(llmie_sample_logits_ext(lm->lastLogits(), 1, V, d_p.d, nullptr, 0, nullptr, 0, d_seq.d, d_fin.d, d_out.d, d_lp.d,
                                           static_cast<int>(ids.size()), nullptr, EOS, d_ws.d, ws, llmie_api::dtype_of<T>(),
                                           llmie_api::st(), &e));
        CHECK(hipStreamSynchronize(llmie_api::st()));
        check_equal("SamplingConfig step == llmie_sample_logits_ext: token", std::vector<int>{tok}, d_out.download());
        check_equal("SamplingConfig step == llmie_sample_logits_ext: top ids", top_ids, d_tid.download());
        check_equal("SamplingConfig step == llmie_sample_logits_ext: top logprobs", top_lp, d_tlp.download());
        check_equal("SamplingConfig step == llmie_sample_logits_ext: logprob", std::vector<float>{lm->lastLogprob()}, d_lp.download());
    }
    if (top_ids.size() != 6 || top_ids[0] != free_pick) fail("the first alternative is not the unconstrained greedy pick");
    for (size_t i = 1; i < top_lp.size(); ++i)
        if (!(top_lp[i] <= top_lp[i - 1]) || !(top_lp[i] <= 0.f)) fail("top logprobs are not descending values <= 0");
    if (tok == EOS || tok == free_pick || tok == 300 || tok % 3 == 1) fail("the first token breaks min_tokens, the ban or the mask");

    // a reply: EOS carries +100, so it comes as soon as min_tokens allows it -- and not before
    const std::vector<int> reply = tokens();
    bool ok = static_cast<int>(reply.size()) == cfg.min_tokens;
    for (int t : reply) ok = ok && t != EOS && t != free_pick && t != 11 && t != 300 && t % 3 != 1;
    if (!ok) fail("the reply does not run min_tokens allowed tokens and then stop at EOS");
    else std::printf("%s: reply of %zu tokens under mask, ban and min_tokens passed\n", name, reply.size());

    // a stop token ends the reply like EOS: greedy, with the stop token pushed to the top from the third token on
    typename LlamaModel<T>::SamplingConfig stop;
    stop.temperature = 0.0f;
    stop.min_tokens = 2;
    stop.stop_token_ids = {777};
    stop.logit_bias = {{777, 100.0f}};
    lm->sampling = stop;
    const std::vector<int> r2 = tokens();
    bool ok2 = r2.size() == 2;
    for (int t : r2) ok2 = ok2 && t != 777 && t != EOS;
    if (!ok2) fail("the stop token did not end the reply right behind min_tokens");
    else std::printf("%s: stop token ends the reply passed\n", name);

    lm->sampling = typename LlamaModel<T>::SamplingConfig();
    if (!lm->sampling.isDefault() || cfg.isDefault() || stop.isDefault()) fail("isDefault ignores the new fields");
    const std::vector<int> back = tokens();
    if (back != untouched || back.empty()) fail("the default config changed the tokens");
    else std::printf("%s: default config keeps the reference's tail passed\n", name);
}

int main() {
    run<half>("fp16");
    run<float>("fp32");
    std::printf(g_failures ? "%d FAILED\n" : "all passed (%d failures)\n", g_failures);
    return g_failures ? 1 : 0;
}
