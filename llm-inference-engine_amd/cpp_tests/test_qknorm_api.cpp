// QK-norm (per-head q/k RMSNorm in front of RoPE; Qwen3 q_norm / k_norm) through the C++ API mirror:
//   launchQkNorm (api/kernels.hpp)  packed fp16 rows (head size 128, 4 heads over 2) against a plain double loop with one fp16
//       rounding, |got - ref| <= 2^-10 |ref| + 2^-24; the v heads keep their bits;
//   launchDecoderQkNormAttention    a ragged fp16 batch (contexts 300 / 5 / 140) equals launchQkNorm followed by
//       launchDecoderSinkAttention bit for bit (output and caches); null gammas give the sink launcher's bits;
//   LlamaModel::setQkNorm           a small fp16 model (both decoders on the fused engine): the gammas move prefill and decode rows,
//       clearing restores the bits; a model on the per-kernel loops refuses.
// Run on the GPU by tests/test_qknorm_cpp_gpu.py; exit code != 0 on any failure.
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
        llmie_api::upload(lw->attention_norm_weight.gamma, to_half(std::vector<float>(H, 1.f)));
        lw->self_attention_weight.output.is_transposed = hf_layout;
    }
    return model;
}
double max_abs_diff(const std::vector<float> &a, const std::vector<float> &b) {
    double m = 0;
    for (size_t i = 0; i < a.size(); ++i) m = std::max(m, std::fabs(double(a[i]) - b[i]));
    return m;
}
void verdict(bool ok, const char *what) {
    if (ok) std::printf("%s passed\n", what);
    else { std::printf("FAIL %s\n", what); ++g_failures; }
}
// gammas in [0.5, 2], log-uniform
std::vector<float> gammas(std::mt19937_64 &rng, size_t n) {
    std::vector<float> g = randu(rng, n, 1.f);
    for (float &v : g) v = std::exp2(v);
    return storage_round<half>(g);
}

void run_model() {
    llm::ModelConfig &c = llm::config();
    c.head_num = 4; c.kv_head_num = 4; c.head_size = 128; c.inter_size = 352; c.num_layers = 2;
    c.max_seq_len = 64; c.vocab_size = 500; c.rotary_embedding_dim = 128;
    const int H = 512, HS = 128, L = 2;
    std::unique_ptr<BaseModel> plain_model = make_model(true);
    const ModelRun base = run(static_cast<LlamaModel<half> *>(plain_model.get()), H);
    plain_model.reset();

    std::mt19937_64 rng(11);
    DeviceArray<half> d_q(to_half(gammas(rng, static_cast<size_t>(L) * HS))), d_k(to_half(gammas(rng, static_cast<size_t>(L) * HS)));
    std::unique_ptr<BaseModel> model = make_model(true);
    LlamaModel<half> *lm = static_cast<LlamaModel<half> *>(model.get());
    lm->setQkNorm(d_q.d, d_k.d, 1e-6f);
    const ModelRun normed = run(lm, H);
    const double moved_p = max_abs_diff(normed.prefill, base.prefill), moved_d = max_abs_diff(normed.decode, base.decode);
    std::printf("LlamaModel QK-norm: rows move by up to %.4g (prefill) / %.4g (decode)\n", moved_p, moved_d);
    verdict(moved_p > 0.02 && moved_d > 0.02, "LlamaModel QK-norm moves the rows");   // (fp16 noise on these rows: ~5e-3)
    lm->setQkNorm(nullptr, nullptr, 0.f);
    const ModelRun cleared = run(lm, H);
    check_equal("LlamaModel cleared gammas, prefill", cleared.prefill, base.prefill);
    check_equal("LlamaModel cleared gammas, decode", cleared.decode, base.decode);
    model.reset();

    // a model that runs the per-kernel loops (a matrix not in HF layout) must refuse, not ignore
    std::unique_ptr<BaseModel> loop_model = make_model(false);
    bool refused = false;
    try {
        static_cast<LlamaModel<half> *>(loop_model.get())->setQkNorm(d_q.d, d_k.d, 1e-6f);
    } catch (const std::runtime_error &e) {
        refused = std::string(e.what()).find("QK-norm needs the fused engine") != std::string::npos;
    }
    verdict(refused, "LlamaModel without the fused engine refuses QK-norm");
}

void run_kernels() {
    const int B = 3, NH = 4, KVH = 2, HS = 128, MAXS = 384, HEADS = NH + 2 * KVH;
    const float eps = 1e-6f;
    const std::vector<int> ctx = {300, 5, 140};
    std::mt19937_64 rng(5);
    std::vector<float> qkv = randn(rng, static_cast<size_t>(B) * HEADS * HS, 1.f);
    for (int b = 0; b < B; ++b)   // every head at its own scale, one q head with a mean square near eps
        for (int h = 0; h < HEADS; ++h)
            for (int e = 0; e < HS; ++e) qkv[(static_cast<size_t>(b) * HEADS + h) * HS + e] *= h == 1 ? 1e-3f : std::exp2(float(h % 5) - 2.f);
    qkv = storage_round<half>(qkv);
    const std::vector<float> qg = gammas(rng, HS), kg = gammas(rng, HS);
    const std::vector<float> kc = storage_round<half>(randn(rng, static_cast<size_t>(B) * KVH * MAXS * HS, 0.5f));
    const std::vector<float> vc = storage_round<half>(randn(rng, static_cast<size_t>(B) * KVH * MAXS * HS, 0.5f));
    DeviceArray<half> d_qkv(to_half(qkv)), d_normed(to_half(qkv)), d_qg(to_half(qg)), d_kg(to_half(kg));
    DeviceArray<half> d_out(static_cast<size_t>(B) * NH * HS), d_ref(static_cast<size_t>(B) * NH * HS);
    DeviceArray<int> d_ctx(ctx);
    const DataType th = getTensorType<half>();
    TensorWrapper<half> t_qkv(Device::GPU, th, {B, HEADS, HS}, d_qkv.d), t_normed(Device::GPU, th, {B, HEADS, HS}, d_normed.d);
    TensorWrapper<half> t_qg(Device::GPU, th, {HS}, d_qg.d), t_kg(Device::GPU, th, {HS}, d_kg.d);
    TensorWrapper<half> t_out(Device::GPU, th, {B, NH * HS}, d_out.d), t_ref(Device::GPU, th, {B, NH * HS}, d_ref.d);
    TensorWrapper<int> t_ctx(Device::GPU, getTensorType<int>(), {B}, d_ctx.d);

    // the operator against a plain loop
    launchQkNorm<half>(&t_normed, KVH, &t_qg, &t_kg, eps);
    CHECK(hipStreamSynchronize(llmie_api::st()));
    const std::vector<float> normed = to_float(d_normed.download());
    bool ok = true;
    double worst = 0;
    for (int b = 0; b < B; ++b)
        for (int h = 0; h < HEADS; ++h) {
            const float *x = &qkv[(static_cast<size_t>(b) * HEADS + h) * HS], *y = &normed[(static_cast<size_t>(b) * HEADS + h) * HS];
            if (h >= NH + KVH) {
                for (int e = 0; e < HS; ++e) ok = ok && x[e] == y[e];
                continue;
            }
            double ss = 0;
            for (int e = 0; e < HS; ++e) ss += double(x[e]) * x[e];
            const double inv = 1.0 / std::sqrt(ss / HS + eps);
            for (int e = 0; e < HS; ++e) {
                const double ref = x[e] * inv * (h < NH ? qg[e] : kg[e]);
                const double r = std::fabs(y[e] - ref) / (std::ldexp(std::fabs(ref), -10) + std::ldexp(1.0, -24));
                worst = std::max(worst, r);
            }
        }
    std::printf("QkNorm: largest error / bound %.3f\n", worst);
    verdict(ok && worst <= 1.0, "QkNorm against a plain loop");

    // fused = the operator, then the sink launcher (no sinks): bit for bit, output and caches
    auto call = [&](int form, TensorWrapper<half> *out, std::vector<half> *k_after) {
        DeviceArray<half> d_k(to_half(kc)), d_v(to_half(vc));
        TensorWrapper<half> t_k(Device::GPU, th, {1, B, KVH, MAXS, HS}, d_k.d), t_v(Device::GPU, th, {1, B, KVH, MAXS, HS}, d_v.d);
        if (form == 0) launchDecoderQkNormAttention<half>(&t_qkv, nullptr, 0, &t_k, &t_v, &t_ctx, nullptr, 0, nullptr, 0, 0, 0, nullptr, &t_qg, &t_kg, eps, out);
        else if (form == 1) launchDecoderSinkAttention<half>(&t_normed, nullptr, 0, &t_k, &t_v, &t_ctx, nullptr, 0, nullptr, 0, 0, 0, nullptr, out);
        else if (form == 2) launchDecoderQkNormAttention<half>(&t_qkv, nullptr, 0, &t_k, &t_v, &t_ctx, nullptr, 0, nullptr, 0, 0, 0, nullptr, nullptr, nullptr, 0.f, out);
        else launchDecoderSinkAttention<half>(&t_qkv, nullptr, 0, &t_k, &t_v, &t_ctx, nullptr, 0, nullptr, 0, 0, 0, nullptr, out);
        CHECK(hipStreamSynchronize(llmie_api::st()));
        if (k_after) *k_after = d_k.download();
    };
    std::vector<half> k_fused, k_composed;
    call(0, &t_out, &k_fused);
    call(1, &t_ref, &k_composed);
    const std::vector<float> fused = to_float(d_out.download()), composed = to_float(d_ref.download());
    const bool same = check_equal("DecoderQkNormAttention output", fused, composed) & check_equal("DecoderQkNormAttention k cache", to_float(k_fused), to_float(k_composed));
    verdict(same, "DecoderQkNormAttention equals QkNorm + DecoderSinkAttention");
    call(2, &t_out, nullptr);
    call(3, &t_ref, nullptr);
    const std::vector<float> null_gammas = to_float(d_out.download()), plain = to_float(d_ref.download());
    check_equal("DecoderQkNormAttention null gammas are the sink launcher's bits", null_gammas, plain);
    verdict(max_abs_diff(plain, composed) > 0.02, "DecoderQkNormAttention the norm matters");
}
}  // namespace

int main() {
    run_kernels();
    run_model();
    std::printf(g_failures ? "%d FAILED\n" : "all passed (%d failures)\n", g_failures);
    return g_failures ? 1 : 0;
}
