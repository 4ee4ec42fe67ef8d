// LlamaModel::SamplingConfig on the dummy-weight model (user_entry.cpp's flow): greedy == top-1, a seed reproduces its tokens,
// and the default config keeps the tokens of a model on which nothing was set.  Run on the GPU by
// tests/test_sampling_config_gpu.py; exit code != 0 on any failure.
#include <cstdlib>
#include <memory>

#include "../src/utils/model_utils.h"
#include "test_common.hpp"

template <typename T> static void run(const char *name) {
    llm::ModelConfig &c = llm::config();
    c.head_num = 4; c.kv_head_num = 4; c.head_size = 32; c.inter_size = 344; c.num_layers = 2;
    c.max_seq_len = 64; c.vocab_size = 30000; c.rotary_embedding_dim = 32;
    srand(42);
    std::unique_ptr<BaseModel> model(llm::createDummyLLMModel<T>("/nonexistent/tokenizer.bin"));
    LlamaModel<T> *lm = static_cast<LlamaModel<T> *>(model.get());
    const auto tokens = [&]() {
        (void)model->Response(model->MakeInput("", 0, "Hey, are you conscious? Can you talk to me?"), nullptr);
        return lm->last_token_ids;
    };
    const std::vector<int> untouched = tokens();
    typename LlamaModel<T>::SamplingConfig greedy;
    greedy.temperature = 0.0f;
    lm->sampling = greedy;
    const std::vector<int> g = tokens();
    typename LlamaModel<T>::SamplingConfig top1;
    top1.top_k = 1;
    top1.seed = 99;
    lm->sampling = top1;
    const std::vector<int> t1 = tokens();
    typename LlamaModel<T>::SamplingConfig mixed;
    mixed.temperature = 0.8f;
    mixed.top_p = 0.9f;
    mixed.min_p = 0.01f;
    mixed.repetition_penalty = 1.2f;
    mixed.frequency_penalty = 0.1f;
    mixed.seed = 7;
    lm->sampling = mixed;
    const std::vector<int> m1 = tokens();
    const std::vector<int> m2 = tokens();
    lm->sampling = typename LlamaModel<T>::SamplingConfig();
    const std::vector<int> back = tokens();
    std::printf("%s: %zu untouched, %zu greedy, %zu seeded tokens\n", name, untouched.size(), g.size(), m1.size());
    const bool ok = !g.empty() && !m1.empty() && !untouched.empty();
    if (!ok) { std::printf("FAIL %s: empty reply\n", name); ++g_failures; }
    if (g != t1) { std::printf("FAIL %s: temperature 0 and top_k 1 differ\n", name); ++g_failures; }
    if (m1 != m2) { std::printf("FAIL %s: the same seed gave different tokens\n", name); ++g_failures; }
    if (back != untouched) { std::printf("FAIL %s: the default config changed the tokens\n", name); ++g_failures; }
}

int main() {
    run<half>("fp16");
    run<float>("fp32");
    std::printf(g_failures ? "%d FAILED\n" : "all passed (%d failures)\n", g_failures);
    return g_failures ? 1 : 0;
}
