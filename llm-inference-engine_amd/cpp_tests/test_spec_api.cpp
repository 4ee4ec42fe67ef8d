// launchSpecVerify and launchNgramDraft (api/kernels.hpp) on a tiny case each, against plain loops here; then
// LlamaModel::speculativeStep on the dummy-weight model: a greedy speculative loop fed the plain loop's continuation as drafts
// (some corrupted) must emit, chunk by chunk, exactly the walk over the arg-maxima of its own logits rows, accept and reject.
// Run on the GPU by tests/test_speculative_gpu.py; exit code != 0 on any failure.
#include <algorithm>
#include <cstdlib>
#include <memory>

#include "../src/utils/model_utils.h"
#include "test_common.hpp"

static int argmax_row(const float *row, int V) {   // ties -> the lower id
    int best = 0;
    for (int v = 1; v < V; ++v)
        if (row[v] > row[best]) best = v;
    return best;
}

static void run_verify() {
    const int B = 3, K = 3, V = 11, END = 4;
    std::vector<float> logits(static_cast<size_t>(B) * (K + 1) * V);
    for (int r = 0; r < B * (K + 1); ++r)
        for (int v = 0; v < V; ++v) logits[r * V + v] = 0.25f * static_cast<float>((7 * v + 5 * r) % 13) - 1.f;
    std::vector<int> pick(B * (K + 1));
    for (int r = 0; r < B * (K + 1); ++r) pick[r] = argmax_row(&logits[r * V], V);
    // sequence 0: every draft right (count K + 1 unless END comes up); 1: the second draft wrong; 2: finished on entry
    std::vector<int> drafts(B * K);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < K; ++i) drafts[b * K + i] = pick[b * (K + 1) + i];
    drafts[1 * K + 1] = (drafts[1 * K + 1] + 1) % V;
    std::vector<int> seq = {10, 20, 30}, last = {-7, -7, -7}, cached = {100, 200, 300}, steps = {5, 6, 7};
    std::vector<uint8_t> fin = {0, 0, 1};
    std::vector<int> e_tok(B * (K + 1), -1), e_cnt(B, 0), e_seq = seq, e_last = last, e_cached = cached, e_steps = steps;
    std::vector<uint8_t> e_fin = fin;
    for (int b = 0; b < B; ++b) {
        if (fin[b]) continue;
        for (int i = 0; i <= K; ++i) {
            const int t = pick[b * (K + 1) + i];
            e_tok[b * (K + 1) + i] = t;
            ++e_cnt[b];
            e_fin[b] = t == END;
            if (i == K || t == END || t != drafts[b * K + i]) break;
        }
        e_seq[b] += e_cnt[b]; e_cached[b] += e_cnt[b]; e_steps[b] += e_cnt[b];
        e_last[b] = e_tok[b * (K + 1) + e_cnt[b] - 1];
    }
    std::vector<llmie_sampling_params> params(B, llmie_sampling_params{0.f, 0, 1.f, 0.f, 1.f, 0.f, 0.f, 0u});   // greedy
    DeviceArray<float> d_logits(logits);
    DeviceArray<int> d_drafts(drafts), d_seq(seq), d_last(last), d_cached(cached), d_steps(steps), d_tok(B * (K + 1)), d_cnt(B);
    DeviceArray<uint8_t> d_fin(fin);
    DeviceArray<llmie_sampling_params> d_params(params);
    const DataType ti = getTensorType<int>();
    TensorWrapper<float> t_logits(Device::GPU, getTensorType<float>(), {B * (K + 1), V}, d_logits.d);
    TensorWrapper<int> t_drafts(Device::GPU, ti, {B, K}, d_drafts.d), t_seq(Device::GPU, ti, {B}, d_seq.d), t_last(Device::GPU, ti, {B}, d_last.d),
        t_cached(Device::GPU, ti, {B}, d_cached.d), t_steps(Device::GPU, ti, {B}, d_steps.d), t_tok(Device::GPU, ti, {B, K + 1}, d_tok.d),
        t_cnt(Device::GPU, ti, {B}, d_cnt.d);
    TensorWrapper<bool> t_fin(Device::GPU, getTensorType<bool>(), {B}, reinterpret_cast<bool *>(d_fin.d));
    launchSpecVerify(&t_logits, &t_drafts, static_cast<TensorWrapper<int> *>(nullptr), d_params.d, static_cast<TensorWrapper<int> *>(nullptr),
                     static_cast<TensorWrapper<int> *>(nullptr), false, &t_seq, &t_fin, &t_tok, &t_cnt, static_cast<TensorWrapper<float> *>(nullptr),
                     &t_last, &t_cached, &t_steps, 0, END);
    CHECK(hipStreamSynchronize(llmie_api::st()));
    check_equal("SpecVerify tokens", d_tok.download(), e_tok);
    check_equal("SpecVerify counts", d_cnt.download(), e_cnt);
    check_equal("SpecVerify seq_len", d_seq.download(), e_seq);
    check_equal("SpecVerify finished", d_fin.download(), e_fin);
    check_equal("SpecVerify last_token", d_last.download(), e_last);
    check_equal("SpecVerify cached_len", d_cached.download(), e_cached);
    check_equal("SpecVerify step_rows", d_steps.download(), e_steps);
    if (e_cnt[1] != 2 || e_cnt[2] != 0 || e_cnt[0] < 2) { std::printf("FAIL SpecVerify: the case does not cover accept / reject / finished\n"); ++g_failures; }
}

static void run_ngram() {
    const int B = 4, STRIDE = 19, K = 4, MAXN = 3, MINN = 1, PAD = -5;
    std::vector<int> tokens(B * STRIDE, 99), len = {16, 11, 2, 12};
    const int r0[] = {1, 2, 3, 4, 5, 6, 7, 1, 2, 3, 9, 9, 8, 1, 2, 3};   // "1 2 3" twice before, both with 4 tokens behind them: the later one wins
    const int r1[] = {5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};             // no match
    const int r2[] = {3, 3};                                              // the one match has a single token behind it
    const int r3[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 2, 3, 4};                // finished below
    std::copy(r0, r0 + 16, tokens.begin());
    std::copy(r1, r1 + 11, tokens.begin() + STRIDE);
    std::copy(r2, r2 + 2, tokens.begin() + 2 * STRIDE);
    std::copy(r3, r3 + 12, tokens.begin() + 3 * STRIDE);
    std::vector<uint8_t> fin = {0, 0, 0, 1};
    std::vector<int> e_ids(B * (K + 1), PAD), e_drafts(B * K, PAD), e_len(B, 0);
    for (int b = 0; b < B; ++b) {
        const int *t = &tokens[b * STRIDE], L = std::min(std::max(len[b], 0), STRIDE);
        e_ids[b * (K + 1)] = L > 0 ? t[L - 1] : PAD;
        if (fin[b] || L < MINN + 1) continue;
        for (int n = std::min(MAXN, L - 1); n >= MINN; --n) {
            int full = -1, any = -1;
            for (int p = 0; p <= L - n - 1; ++p)
                if (std::equal(t + p, t + p + n, t + L - n)) {
                    any = p;
                    if (p + n + K <= L) full = p;
                }
            if (any < 0) continue;
            const int p = full >= 0 ? full : any, m = std::min(K, L - p - n);
            for (int i = 0; i < m; ++i) e_drafts[b * K + i] = e_ids[b * (K + 1) + 1 + i] = t[p + n + i];
            e_len[b] = m;
            break;
        }
    }
    DeviceArray<int> d_tokens(tokens), d_len(len), d_ids(B * (K + 1)), d_drafts(B * K), d_dlen(B);
    DeviceArray<uint8_t> d_fin(fin);
    const DataType ti = getTensorType<int>();
    TensorWrapper<int> t_tokens(Device::GPU, ti, {B, STRIDE}, d_tokens.d), t_len(Device::GPU, ti, {B}, d_len.d), t_ids(Device::GPU, ti, {B, K + 1}, d_ids.d),
        t_drafts(Device::GPU, ti, {B, K}, d_drafts.d), t_dlen(Device::GPU, ti, {B}, d_dlen.d);
    TensorWrapper<bool> t_fin(Device::GPU, getTensorType<bool>(), {B}, reinterpret_cast<bool *>(d_fin.d));
    launchNgramDraft(&t_tokens, &t_len, &t_fin, MAXN, MINN, PAD, &t_ids, &t_drafts, &t_dlen);
    CHECK(hipStreamSynchronize(llmie_api::st()));
    check_equal("NgramDraft input ids", d_ids.download(), e_ids);
    check_equal("NgramDraft draft ids", d_drafts.download(), e_drafts);
    check_equal("NgramDraft draft lengths", d_dlen.download(), e_len);
    if (e_len != std::vector<int>{4, 0, 1, 0}) { std::printf("FAIL NgramDraft: the case does not cover full / none / short / finished\n"); ++g_failures; }
}

static void run_model() {
    llm::ModelConfig &c = llm::config();
    c.head_num = 4; c.kv_head_num = 4; c.head_size = 32; c.inter_size = 344; c.num_layers = 2;
    c.max_seq_len = 64; c.vocab_size = 500; c.rotary_embedding_dim = 32;
    const int V = c.vocab_size, K = 3, N = 12;
    const std::vector<int> prompt = {1, 17, 499, 5, 5, 123, 42, 7, 200, 3, 11};
    // the plain greedy loop: the continuation the drafts are taken from
    srand(42);
    std::unique_ptr<BaseModel> plain_model(llm::createDummyLLMModel<half>("/nonexistent/tokenizer.bin"));
    LlamaModel<half> *plain = static_cast<LlamaModel<half> *>(plain_model.get());
    plain->sampling.temperature = 0.f;
    std::vector<int> cont = {plain->generateFirstToken(prompt, 0)};
    while (static_cast<int>(cont.size()) < N + K + 1) cont.push_back(plain->continueWith(cont.back()));
    plain_model.reset();

    srand(42);
    std::unique_ptr<BaseModel> model(llm::createDummyLLMModel<half>("/nonexistent/tokenizer.bin"));
    LlamaModel<half> *lm = static_cast<LlamaModel<half> *>(model.get());
    lm->sampling.temperature = 0.f;
    std::vector<int> out = {lm->generateFirstToken(prompt, 0)};
    bool walk_ok = out[0] == cont[0];
    int steps = 0, accepted = 0, rejected = 0;
    while (static_cast<int>(out.size()) < N && walk_ok) {
        const int at = static_cast<int>(out.size());   // out[at - 1] is the last emitted token
        std::vector<int> drafts(cont.begin() + at, cont.begin() + at + K);
        if (steps % 2 == 1) drafts[steps / 2 % K] = (drafts[steps / 2 % K] + 1) % V;   // every other chunk carries one wrong draft
        const std::vector<int> got = lm->speculativeStep(out.back(), drafts);
        std::vector<half> rows(static_cast<size_t>(K + 1) * V);
        CHECK(hipMemcpy(rows.data(), lm->lastLogits(), sizeof(half) * rows.size(), hipMemcpyDeviceToHost));
        const std::vector<float> f = to_float(rows);
        std::vector<int> expect;
        for (int i = 0; i <= K; ++i) {
            const int t = argmax_row(&f[static_cast<size_t>(i) * V], V);
            expect.push_back(t);
            if (i == K || t == 2 /* EOS */ || t != drafts[i]) break;
        }
        walk_ok = got == expect;
        accepted += static_cast<int>(got.size()) - 1;
        rejected += got.size() < static_cast<size_t>(K + 1) ? 1 : 0;
        out.insert(out.end(), got.begin(), got.end());
        std::printf("speculativeStep %d: %zu tokens\n", steps, got.size());
        ++steps;
        if (std::find(got.begin(), got.end(), 2) != got.end()) break;
    }
    if (!walk_ok) { std::printf("FAIL speculativeStep: a chunk's tokens are not the walk over its logits' arg-maxima\n"); ++g_failures; }
    else std::printf("speculativeStep emits the walk over its logits passed\n");
    if (accepted < 1 || rejected < 1) { std::printf("FAIL speculativeStep: %d drafts accepted, %d chunks cut short: the loop covers too little\n", accepted, rejected); ++g_failures; }
    else std::printf("speculativeStep accepted %d drafts in %d chunks, %d cut short passed\n", accepted, steps, rejected);
    // chunked and one-token forwards round differently, so agreement with the plain loop is reported, not required
    const size_t n = std::min(out.size(), cont.size());
    size_t same = 0;
    while (same < n && out[same] == cont[same]) ++same;
    std::printf("speculative loop agrees with the plain greedy loop on the first %zu of %zu tokens\n", same, n);
}

int main() {
    run_verify();
    run_ngram();
    run_model();
    std::printf(g_failures ? "%d FAILED\n" : "all passed (%d failures)\n", g_failures);
    return g_failures ? 1 : 0;
}
