// LlamaModel::scoreTokens on the dummy-weight model: n - 1 finite log-probabilities <= 0, equal to llmie_score_tokens called here
// on the context decoder's output; a decode step can follow; the fp32 model refuses.  Run on the GPU by
// tests/test_score_cpp_gpu.py; exit code != 0 on any failure.
#include <cstdlib>
#include <memory>
#include <stdexcept>

#include "../src/utils/model_utils.h"
#include "test_common.hpp"

static void set_geometry() {
    llm::ModelConfig &c = llm::config();
    c.head_num = 4; c.kv_head_num = 4; c.head_size = 32; c.inter_size = 344; c.num_layers = 2;
    c.max_seq_len = 64; c.vocab_size = 30000; c.rotary_embedding_dim = 32;
}

static void run_half() {
    set_geometry();
    const llm::ModelConfig &c = llm::config();
    const int H = c.head_num * c.head_size, V = c.vocab_size;
    srand(42);
    std::unique_ptr<BaseModel> model(llm::createDummyLLMModel<half>("/nonexistent/tokenizer.bin"));
    LlamaModel<half> *lm = static_cast<LlamaModel<half> *>(model.get());
    const std::vector<int> ids = {1, 17, 29999, 5, 5, 1234, 42, 7, 20000, 3, 11};
    const int n = static_cast<int>(ids.size());
    const std::vector<float> got = lm->scoreTokens(ids);
    if (static_cast<int>(got.size()) != n - 1) { std::printf("FAIL scoreTokens: %zu values for %d ids\n", got.size(), n); ++g_failures; return; }
    bool sane = true;
    for (float v : got) sane = sane && std::isfinite(v) && v <= 0.f;
    if (!sane) { std::printf("FAIL scoreTokens: a value is not a finite log-probability\n"); ++g_failures; }
    else std::printf("scoreTokens: %d finite values <= 0 (first %g) passed\n", n - 1, got[0]);

    // the same through the C ABI on the context decoder's output (scoreTokens leaves it as the decoder wrote it)
    std::vector<int> targets(ids.begin() + 1, ids.end());
    targets.push_back(-1);
    DeviceArray<int> d_targets(targets);
    DeviceArray<float> d_logprob(n);
    const size_t ws = llmie_score_tokens_workspace_bytes(n, H, V);
    DeviceArray<unsigned char> d_ws(ws);
    LLMIE_CALL(llmie_score_tokens(lm->contextOutput(), lm->weights()->out_rmsnorm_weight.gamma, 1e-5f,
                                  lm->weights()->post_decoder_embedding_weight.data, nullptr, d_targets.d, d_logprob.d, nullptr, nullptr,
                                  nullptr, n, H, V, d_ws.d, ws, LLMIE_F16, llmie_api::st()));
    CHECK(hipStreamSynchronize(llmie_api::st()));
    std::vector<float> again = d_logprob.download();
    if (again.back() != 0.0f) { std::printf("FAIL llmie_score_tokens: the row without a target is %g, not 0\n", again.back()); ++g_failures; }
    again.pop_back();
    check_equal("scoreTokens == llmie_score_tokens on the context decoder's output", got, again);

    const int tok = lm->continueWith(ids.back());
    const int tok2 = lm->continueWith(tok);
    if (tok < 0 || tok >= V || tok2 < 0 || tok2 >= V) { std::printf("FAIL decode steps after scoreTokens: tokens %d %d\n", tok, tok2); ++g_failures; }
    else std::printf("decode steps after scoreTokens (tokens %d, %d) passed\n", tok, tok2);
}

static void run_float() {
    set_geometry();
    srand(42);
    std::unique_ptr<BaseModel> model(llm::createDummyLLMModel<float>("/nonexistent/tokenizer.bin"));
    LlamaModel<float> *lm = static_cast<LlamaModel<float> *>(model.get());
    bool threw = false;
    try {
        (void)lm->scoreTokens({1, 2, 3, 4});
    } catch (const std::exception &e) {
        threw = true;
        std::printf("fp32 scoreTokens refused (%s) passed\n", e.what());
    }
    if (!threw) { std::printf("FAIL fp32 scoreTokens did not throw\n"); ++g_failures; }
}

int main() {
    run_half();
    run_float();
    std::printf(g_failures ? "%d FAILED\n" : "all passed (%d failures)\n", g_failures);
    return g_failures ? 1 : 0;
}
