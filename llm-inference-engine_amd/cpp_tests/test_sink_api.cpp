// Learned per-head attention sink logits and RoPE scaling through the C++ API mirror:
//   launchDecoderSinkAttention (api/kernels.hpp)  a ragged fp16 batch (head size 128, head ratio 2, contexts 300 / 5 / 140, no RoPE)
//       against a plain double loop with one extra softmax column per head -- logits -inf, negligible, comparable and dominant within
//       one KV group --, without a window and under W = 17, S = 3; head_sink = null and sinks of -inf give the bits of
//       launchDecoderWindowAttention;
//   LlamaModel::setAttentionSinks / setRopeScaling  a small fp16 model (both decoders on the fused engine): sinks of -inf keep the
//       bits of a model without them, real sinks move prefill and decode rows, clearing restores the bits; a YaRN table moves the rows
//       behind the first (which attends to itself alone), kind NONE restores the bits; a struct llmie_rope_table_fill refuses is
//       refused; a model on the per-kernel loops refuses both.
// Run on the GPU by tests/test_sink_cpp_gpu.py; exit code != 0 on any failure.
#include <limits>
#include <memory>
#include <stdexcept>

#include "../src/kernels/includes/linear.cuh"   // all launchers arrive through api/kernels.hpp
#include "../src/utils/model_utils.h"
#include "test_common.hpp"

namespace {
const std::vector<int> kPrompt = {1, 17, 499, 5, 5, 123, 42, 7, 200, 3, 11, 8, 90, 301, 44, 12, 6, 77};
const float kNinf = -std::numeric_limits<float>::infinity();
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
        // (the dummy model's attention gammas are below 0.1: its logits are ~0 and its attention uniform whatever the rotation)
        llmie_api::upload(lw->attention_norm_weight.gamma, to_half(std::vector<float>(H, 1.f)));
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
    const int H = 512, NH = 4, L = 2;
    std::unique_ptr<BaseModel> plain_model = make_model(true);
    const ModelRun base = run(static_cast<LlamaModel<half> *>(plain_model.get()), H);
    plain_model.reset();

    std::unique_ptr<BaseModel> model = make_model(true);
    LlamaModel<half> *lm = static_cast<LlamaModel<half> *>(model.get());
    DeviceArray<float> d_none(std::vector<float>(L * NH, kNinf));
    lm->setAttentionSinks(d_none.d);
    const ModelRun none = run(lm, H);
    check_equal("LlamaModel sinks of -inf, prefill", none.prefill, base.prefill);
    check_equal("LlamaModel sinks of -inf, decode", none.decode, base.decode);
    DeviceArray<float> d_sinks(std::vector<float>{2.f, kNinf, 4.f, 1.f, 3.f, 5.f, kNinf, 2.5f});
    lm->setAttentionSinks(d_sinks.d);
    const ModelRun sunk = run(lm, H);
    const double moved_p = max_abs_diff(sunk.prefill, base.prefill, 0, sunk.prefill.size());
    const double moved_d = max_abs_diff(sunk.decode, base.decode, 0, sunk.decode.size());
    std::printf("LlamaModel head sinks: rows move by up to %.4g (prefill) / %.4g (decode)\n", moved_p, moved_d);
    verdict(moved_p > 0.02 && moved_d > 0.02, "LlamaModel head sinks move the rows");   // (fp16 noise on these rows: ~5e-3)
    lm->setAttentionSinks(nullptr);
    const ModelRun cleared = run(lm, H);
    check_equal("LlamaModel cleared sinks, prefill", cleared.prefill, base.prefill);
    check_equal("LlamaModel cleared sinks, decode", cleared.decode, base.decode);

    llmie_rope_scaling yarn{};
    yarn.kind = LLMIE_ROPE_YARN, yarn.factor = 32.f, yarn.original_max_pos = 4096, yarn.beta_fast = 32.f, yarn.beta_slow = 1.f;
    lm->setRopeScaling(yarn);
    const ModelRun scaled = run(lm, H);
    const double rope_p = max_abs_diff(scaled.prefill, base.prefill, static_cast<size_t>(H), scaled.prefill.size());
    const double rope_d = max_abs_diff(scaled.decode, base.decode, 0, scaled.decode.size());
    std::printf("LlamaModel YaRN table: rows move by up to %.4g (prefill) / %.4g (decode)\n", rope_p, rope_d);
    verdict(rope_p > 0.02 && rope_d > 0.02, "LlamaModel a scaled table moves the rows");
    llmie_rope_scaling off{};
    lm->setRopeScaling(off);
    const ModelRun unscaled = run(lm, H);
    check_equal("LlamaModel table restored, prefill", unscaled.prefill, base.prefill);
    check_equal("LlamaModel table restored, decode", unscaled.decode, base.decode);
    bool bad_factor = false;
    try {
        yarn.factor = 0.5f;
        lm->setRopeScaling(yarn);
    } catch (const std::runtime_error &e) {
        bad_factor = std::string(e.what()).find("factor") != std::string::npos;
    }
    verdict(bad_factor, "LlamaModel a factor below 1 is refused");
    model.reset();

    // a model that runs the per-kernel loops (a matrix not in HF layout) must refuse, not ignore, either
    std::unique_ptr<BaseModel> loop_model = make_model(false);
    int refused = 0;
    try {
        static_cast<LlamaModel<half> *>(loop_model.get())->setAttentionSinks(d_sinks.d);
    } catch (const std::runtime_error &e) {
        refused += std::string(e.what()).find("head sinks need the fused engine") != std::string::npos;
    }
    try {
        yarn.factor = 32.f;
        static_cast<LlamaModel<half> *>(loop_model.get())->setRopeScaling(yarn);
    } catch (const std::runtime_error &e) {
        refused += std::string(e.what()).find("a scaled table needs the fused engine") != std::string::npos;
    }
    verdict(refused == 2, "LlamaModel without the fused engine refuses sinks and scaling");
}

// out[b][h][:] of the masked softmax with the sink column, double, on the values as stored; sum + 1e-6 denominator
std::vector<float> attention_loop(const std::vector<float> &qkv, const std::vector<float> &kc, const std::vector<float> &vc, const std::vector<int> &ctx,
                                  const std::vector<float> &sink, int NH, int KVH, int HS, int MAXS, int W, int S) {
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
            double mx = sink[h], sum = 0;
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
            sum += std::exp(double(sink[h]) - mx);   // the column without a value row (exp(-inf) = 0)
            for (int e = 0; e < HS; ++e) out[(static_cast<size_t>(b) * NH + h) * HS + e] = static_cast<float>(o[e] / (sum + 1e-6));
        }
    return out;
}

void run_attention() {
    const int B = 3, NH = 4, KVH = 2, HS = 128, MAXS = 384;
    const std::vector<int> ctx = {300, 5, 140};
    // logits of these inputs are N(0, 0.5) with a row maximum near 1.5: per KV group one head without a sink or a negligible one,
    // and one comparable or dominant one
    const std::vector<float> sink = {kNinf, 6.f, -9.f, 10.f};
    std::mt19937_64 rng(5);
    const std::vector<float> qkv = storage_round<half>(randn(rng, static_cast<size_t>(B) * (NH + 2 * KVH) * HS, 1.f));
    const std::vector<float> kc = storage_round<half>(randn(rng, static_cast<size_t>(B) * KVH * MAXS * HS, 0.5f));
    const std::vector<float> vc = storage_round<half>(randn(rng, static_cast<size_t>(B) * KVH * MAXS * HS, 0.5f));
    DeviceArray<half> d_qkv(to_half(qkv)), d_out(static_cast<size_t>(B) * NH * HS), d_ref(static_cast<size_t>(B) * NH * HS);
    DeviceArray<int> d_ctx(ctx);
    DeviceArray<float> d_sink(sink), d_ninf(std::vector<float>(NH, kNinf));
    const DataType th = getTensorType<half>();
    TensorWrapper<half> t_qkv(Device::GPU, th, {B, NH + 2 * KVH, HS}, d_qkv.d), t_out(Device::GPU, th, {B, NH * HS}, d_out.d),
        t_ref(Device::GPU, th, {B, NH * HS}, d_ref.d);
    TensorWrapper<int> t_ctx(Device::GPU, getTensorType<int>(), {B}, d_ctx.d);
    TensorWrapper<float> t_sink(Device::GPU, getTensorType<float>(), {NH}, d_sink.d), t_ninf(Device::GPU, getTensorType<float>(), {NH}, d_ninf.d);
    for (int windowed = 0; windowed < 2; ++windowed) {
        const int W = windowed ? 17 : 0, S = windowed ? 3 : 0;
        auto call = [&](TensorWrapper<float> *hs, TensorWrapper<half> *out, bool plain) {
            DeviceArray<half> d_k(to_half(kc)), d_v(to_half(vc));
            TensorWrapper<half> t_k(Device::GPU, th, {1, B, KVH, MAXS, HS}, d_k.d), t_v(Device::GPU, th, {1, B, KVH, MAXS, HS}, d_v.d);
            if (plain) launchDecoderWindowAttention<half>(&t_qkv, nullptr, 0, &t_k, &t_v, &t_ctx, nullptr, 0, nullptr, 0, W, S, out);
            else launchDecoderSinkAttention<half>(&t_qkv, nullptr, 0, &t_k, &t_v, &t_ctx, nullptr, 0, nullptr, 0, W, S, hs, out);
            CHECK(hipStreamSynchronize(llmie_api::st()));
        };
        call(&t_sink, &t_out, false);
        const std::vector<float> exp = attention_loop(qkv, kc, vc, ctx, sink, NH, KVH, HS, MAXS, W, S);
        check_close(windowed ? "DecoderSinkAttention W=17 S=3" : "DecoderSinkAttention full attention", to_float(d_out.download()), exp, 3e-3f, 2e-3f);
        call(nullptr, &t_ref, true);
        const std::vector<float> plain = to_float(d_ref.download());
        verdict(max_abs_diff(plain, exp, 0, exp.size()) > 0.02, windowed ? "DecoderSinkAttention the sinks matter (windowed)" : "DecoderSinkAttention the sinks matter");
        call(nullptr, &t_out, false);
        check_equal(windowed ? "DecoderSinkAttention null sinks are the window launcher's bits (windowed)" : "DecoderSinkAttention null sinks are the window launcher's bits",
                    to_float(d_out.download()), plain);
        call(&t_ninf, &t_out, false);
        check_equal(windowed ? "DecoderSinkAttention sinks of -inf are the window launcher's bits (windowed)" : "DecoderSinkAttention sinks of -inf are the window launcher's bits",
                    to_float(d_out.download()), plain);
    }
}
}  // namespace

int main() {
    run_attention();
    run_model();
    std::printf(g_failures ? "%d FAILED\n" : "all passed (%d failures)\n", g_failures);
    return g_failures ? 1 : 0;
}
