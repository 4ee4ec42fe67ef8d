// Sliding-window attention with sink tokens through the C++ API mirror:
//   launchDecoderWindowAttention (api/kernels.hpp)  a ragged fp16 batch (head size 128, head ratio 2, contexts 300 / 5 / 140, W = 17,
//       S = 3, no RoPE) against a plain double loop over the keys the mask exposes; every cache row the mask hides is NaN, so a kernel
//       that read one would not produce a finite number; window = 0 on clean caches against the same loop without the mask;
//   launchKvWindowAdvance  table rows whose outcome is known by hand: a dead page recycled, no dead page (status 1, row untouched),
//       positions past the table (status 2), nothing to map;
//   LlamaModel::setAttentionWindow  a small fp16 model (both decoders on the fused engine): a window over the whole context gives the
//       bits of a model without one; under W = 5, S = 0 the first 5 prefill rows -- which see everything they saw before -- keep their
//       bits and later rows move; clearing the window restores the bits; a model on the per-kernel loops refuses the window.
// Run on the GPU by tests/test_window_cpp_gpu.py; exit code != 0 on any failure.
#include <limits>
#include <memory>
#include <stdexcept>

#include "../src/kernels/includes/linear.cuh"   // all launchers arrive through api/kernels.hpp
#include "../src/utils/model_utils.h"
#include "test_common.hpp"

namespace {
const std::vector<int> kPrompt = {1, 17, 499, 5, 5, 123, 42, 7, 200, 3, 11, 8, 90, 301, 44, 12, 6, 77};
struct ModelRun {
    std::vector<float> prefill, decode;
};
ModelRun run(LlamaModel<half> *lm, int H) {
    ModelRun r;
    lm->generateFirstToken(kPrompt, 0);
    std::vector<half> h(kPrompt.size() * H);
    CHECK(hipMemcpy(h.data(), lm->contextOutput(), sizeof(half) * h.size(), hipMemcpyDeviceToHost));
    h.resize((kPrompt.size() - 1) * H);   // (the last row was normalised in place for the LM head)
    r.prefill = to_float(h);
    lm->continueWith(33);
    std::vector<half> d(H);
    CHECK(hipMemcpy(d.data(), lm->decodeOutput(), sizeof(half) * H, hipMemcpyDeviceToHost));
    r.decode = to_float(d);
    return r;
}
std::unique_ptr<BaseModel> make_model(bool hf_layout) {
    srand(42);
    std::unique_ptr<BaseModel> model(llm::createDummyLLMModel<half>("/nonexistent/tokenizer.bin"));
    LlamaModel<half> *lm = static_cast<LlamaModel<half> *>(model.get());
    lm->sampling.temperature = 0.f;
    const llm::ModelConfig &c = llm::config();
    const int H = c.head_num * c.head_size, QKV = (c.head_num + 2 * c.kv_head_num) * c.head_size, I = c.inter_size;
    std::mt19937_64 rng(7);
    LlamaWeight<half> *w = lm->weights();
    llmie_api::upload(w->pre_decoder_embedding_weight.data, to_half(randn(rng, static_cast<size_t>(c.vocab_size) * H, 1.f)));
    for (auto &lw : w->llama_layer_weight) {
        llmie_api::upload(lw->self_attention_weight.qkv.data, to_half(randu(rng, static_cast<size_t>(QKV) * H, 2.f / std::sqrt(float(H)))));
        llmie_api::upload(lw->self_attention_weight.output.data, to_half(randu(rng, static_cast<size_t>(H) * H, 2.f / std::sqrt(float(H)))));
        llmie_api::upload(lw->ffn_weight.gate_and_up.data, to_half(randu(rng, static_cast<size_t>(2 * I) * H, 2.f / std::sqrt(float(H)))));
        llmie_api::upload(lw->ffn_weight.down.data, to_half(randu(rng, static_cast<size_t>(H) * I, 2.f / std::sqrt(float(I)))));
        lw->self_attention_weight.output.is_transposed = hf_layout;
    }
    return model;
}
double max_abs_diff(const std::vector<float> &a, const std::vector<float> &b, size_t from, size_t to) {
    double m = 0;
    for (size_t i = from; i < to; ++i) m = std::max(m, std::fabs(double(a[i]) - b[i]));
    return m;
}
void verdict(bool ok, const char *what) {
    if (ok) std::printf("%s passed\n", what);
    else { std::printf("FAIL %s\n", what); ++g_failures; }
}

void run_model() {
    llm::ModelConfig &c = llm::config();
    c.head_num = 4; c.kv_head_num = 4; c.head_size = 128; c.inter_size = 352; c.num_layers = 2;
    c.max_seq_len = 64; c.vocab_size = 500; c.rotary_embedding_dim = 128;
    const int H = 512, W = 5;
    std::unique_ptr<BaseModel> plain_model = make_model(true);
    const ModelRun base = run(static_cast<LlamaModel<half> *>(plain_model.get()), H);
    plain_model.reset();

    std::unique_ptr<BaseModel> model = make_model(true);
    LlamaModel<half> *lm = static_cast<LlamaModel<half> *>(model.get());
    lm->setAttentionWindow({64, 64}, 2);
    const ModelRun whole = run(lm, H);
    check_equal("LlamaModel window over the context, prefill", whole.prefill, base.prefill);
    check_equal("LlamaModel window over the context, decode", whole.decode, base.decode);
    lm->setAttentionWindow({W, W}, 0);
    const ModelRun local = run(lm, H);
    const std::vector<float> head_l(local.prefill.begin(), local.prefill.begin() + W * H), head_b(base.prefill.begin(), base.prefill.begin() + W * H);
    check_equal("LlamaModel rows inside the first window keep their bits", head_l, head_b);
    const double moved_p = max_abs_diff(local.prefill, base.prefill, static_cast<size_t>(W) * H, local.prefill.size());
    const double moved_d = max_abs_diff(local.decode, base.decode, 0, local.decode.size());
    std::printf("LlamaModel window %d: rows behind it move by up to %.4g (prefill) / %.4g (decode)\n", W, moved_p, moved_d);
    verdict(moved_p > 0.02 && moved_d > 0.02, "LlamaModel rows behind the window move");   // (fp16 noise on these rows: ~5e-3)
    lm->setAttentionWindow({W, 0}, 1);   // one local, one global layer: accepted, and not the all-local answer
    const ModelRun mixed = run(lm, H);
    verdict(max_abs_diff(mixed.decode, local.decode, 0, mixed.decode.size()) > 0.02 && max_abs_diff(mixed.decode, base.decode, 0, mixed.decode.size()) > 0.02,
            "LlamaModel local + global layers differ from all-local and all-global");
    lm->setAttentionWindow({});
    const ModelRun cleared = run(lm, H);
    check_equal("LlamaModel cleared window, prefill", cleared.prefill, base.prefill);
    check_equal("LlamaModel cleared window, decode", cleared.decode, base.decode);
    bool bad_size = false;
    try {
        lm->setAttentionWindow({W}, 0);
    } catch (const std::runtime_error &) {
        bad_size = true;
    }
    verdict(bad_size, "LlamaModel one window per layer is required");
    model.reset();

    // a model that runs the per-kernel loops (a matrix not in HF layout) must refuse, not ignore, a window
    std::unique_ptr<BaseModel> loop_model = make_model(false);
    bool refused = false;
    try {
        static_cast<LlamaModel<half> *>(loop_model.get())->setAttentionWindow({W, W}, 0);
    } catch (const std::runtime_error &e) {
        refused = std::string(e.what()).find("a window needs the fused engine") != std::string::npos;
    }
    verdict(refused, "LlamaModel without the fused engine refuses a window");
}

// out[b][h][:] of the masked softmax, double, on the values as stored; sum + 1e-6 denominator
std::vector<float> attention_loop(const std::vector<float> &qkv, const std::vector<float> &kc, const std::vector<float> &vc, const std::vector<int> &ctx,
                                  int NH, int KVH, int HS, int MAXS, int W, int S) {
    const int B = static_cast<int>(ctx.size()), rep = NH / KVH, heads = NH + 2 * KVH;
    std::vector<float> out(static_cast<size_t>(B) * NH * HS);
    for (int b = 0; b < B; ++b)
        for (int h = 0; h < NH; ++h) {
            const int g = h / rep, n = ctx[b];
            const float *q = &qkv[(static_cast<size_t>(b) * heads + h) * HS];
            auto krow = [&](int t) { return t == n - 1 ? &qkv[(static_cast<size_t>(b) * heads + NH + g) * HS] : &kc[((static_cast<size_t>(b) * KVH + g) * MAXS + t) * HS]; };
            auto vrow = [&](int t) { return t == n - 1 ? &qkv[(static_cast<size_t>(b) * heads + NH + KVH + g) * HS] : &vc[((static_cast<size_t>(b) * KVH + g) * MAXS + t) * HS]; };
            auto vis = [&](int t) { return W <= 0 || t >= n - W || t < S; };
            std::vector<double> lg(n, -std::numeric_limits<double>::infinity());
            double mx = -std::numeric_limits<double>::infinity(), sum = 0;
            for (int t = 0; t < n; ++t)
                if (vis(t)) {
                    double d = 0;
                    for (int e = 0; e < HS; ++e) d += double(q[e]) * krow(t)[e];
                    lg[t] = d / std::sqrt(double(HS));
                    mx = std::max(mx, lg[t]);
                }
            std::vector<double> o(HS, 0.0);
            for (int t = 0; t < n; ++t)
                if (vis(t)) {
                    const double p = std::exp(lg[t] - mx);
                    sum += p;
                    for (int e = 0; e < HS; ++e) o[e] += p * vrow(t)[e];
                }
            for (int e = 0; e < HS; ++e) out[(static_cast<size_t>(b) * NH + h) * HS + e] = static_cast<float>(o[e] / (sum + 1e-6));
        }
    return out;
}

void run_attention() {
    const int B = 3, NH = 4, KVH = 2, HS = 128, MAXS = 384, W = 17, S = 3;
    const std::vector<int> ctx = {300, 5, 140};
    std::mt19937_64 rng(5);
    const std::vector<float> qkv = storage_round<half>(randn(rng, static_cast<size_t>(B) * (NH + 2 * KVH) * HS, 1.f));
    const std::vector<float> kc = storage_round<half>(randn(rng, static_cast<size_t>(B) * KVH * MAXS * HS, 0.5f));
    const std::vector<float> vc = storage_round<half>(randn(rng, static_cast<size_t>(B) * KVH * MAXS * HS, 0.5f));
    // every row the mask hides (and every row past the context) is NaN in the windowed call's caches
    std::vector<float> kn = kc, vn = vc;
    size_t hidden = 0;
    for (int b = 0; b < B; ++b)
        for (int g = 0; g < KVH; ++g)
            for (int t = 0; t < MAXS; ++t)
                if (t >= ctx[b] || (t < ctx[b] - W && t >= S)) {
                    ++hidden;
                    for (int e = 0; e < HS; ++e) kn[((static_cast<size_t>(b) * KVH + g) * MAXS + t) * HS + e] = vn[((static_cast<size_t>(b) * KVH + g) * MAXS + t) * HS + e] = std::nanf("");
                }
    DeviceArray<half> d_qkv(to_half(qkv)), d_out(static_cast<size_t>(B) * NH * HS);
    DeviceArray<int> d_ctx(ctx);
    const DataType th = getTensorType<half>();
    TensorWrapper<half> t_qkv(Device::GPU, th, {B, NH + 2 * KVH, HS}, d_qkv.d), t_out(Device::GPU, th, {B, NH * HS}, d_out.d);
    TensorWrapper<int> t_ctx(Device::GPU, getTensorType<int>(), {B}, d_ctx.d);
    for (int windowed = 1; windowed >= 0; --windowed) {
        DeviceArray<half> d_k(to_half(windowed ? kn : kc)), d_v(to_half(windowed ? vn : vc));
        TensorWrapper<half> t_k(Device::GPU, th, {1, B, KVH, MAXS, HS}, d_k.d), t_v(Device::GPU, th, {1, B, KVH, MAXS, HS}, d_v.d);
        launchDecoderWindowAttention<half>(&t_qkv, nullptr, 0, &t_k, &t_v, &t_ctx, nullptr, 0, nullptr, 0, windowed ? W : 0, windowed ? S : 0, &t_out);
        CHECK(hipStreamSynchronize(llmie_api::st()));
        const std::vector<float> exp = attention_loop(qkv, kc, vc, ctx, NH, KVH, HS, MAXS, windowed ? W : 0, windowed ? S : 0);
        check_close(windowed ? "DecoderWindowAttention W=17 S=3 over NaN dead rows" : "DecoderWindowAttention window 0 is full attention",
                    to_float(d_out.download()), exp, 3e-3f, 2e-3f);
        // the step's k / v landed in the cache slot ctx - 1
        const std::vector<float> kafter = to_float(d_k.download());
        bool appended = true;
        for (int b = 0; b < B; ++b)
            for (int g = 0; g < KVH; ++g)
                for (int e = 0; e < HS; ++e)
                    appended &= kafter[((static_cast<size_t>(b) * KVH + g) * MAXS + ctx[b] - 1) * HS + e] == qkv[(static_cast<size_t>(b) * (NH + 2 * KVH) + NH + g) * HS + e];
        verdict(appended, windowed ? "DecoderWindowAttention append (windowed)" : "DecoderWindowAttention append (window 0)");
    }
    verdict(hidden > 1000, "DecoderWindowAttention case hides rows");
}

void run_ring() {
    const int B = 4, MP = 6, W = 200, S = 4;
    //            dead page 1 recycled for page 4     no dead page yet         past the table            page already mapped
    std::vector<int> table = {10, 11, 12, 13, -1, -1, 20, 21, 22, -1, -1, -1, 30, 31, 32, 33, 34, 35, 40, 41, 42, 43, -1, -1};
    const std::vector<int> cached = {512, 384, 768, 400};
    const std::vector<int> e_table = {10, -1, 12, 13, 11, -1, 20, 21, 22, -1, -1, -1, 30, 31, 32, 33, 34, 35, 40, 41, 42, 43, -1, -1};
    const std::vector<int> e_status = {0, 1, 2, 0};
    DeviceArray<int> d_table(table), d_cached(cached), d_status(std::vector<int>(B, -7));
    const DataType ti = getTensorType<int>();
    TensorWrapper<int> t_table(Device::GPU, ti, {B, MP}, d_table.d), t_cached(Device::GPU, ti, {B}, d_cached.d), t_status(Device::GPU, ti, {B}, d_status.d);
    launchKvWindowAdvance(&t_table, &t_cached, nullptr, W, S, &t_status);
    CHECK(hipStreamSynchronize(llmie_api::st()));
    check_equal("KvWindowAdvance table", d_table.download(), e_table);
    check_equal("KvWindowAdvance status", d_status.download(), e_status);
}
}  // namespace

int main() {
    run_attention();
    run_ring();
    run_model();
    std::printf(g_failures ? "%d FAILED\n" : "all passed (%d failures)\n", g_failures);
    return g_failures ? 1 : 0;
}
