// The mixture-of-experts entries through the C++ API mirror:
//   launchMoeRoute (api/kernels.hpp)  rows of small integers against a router of small integers (every logit exact in fp32): the ids
//       against a host ranking by (logit descending, id ascending), exact ties included, the weights against a double softmax;
//   launchMoeFfn  7 rows (grouped route) and 2 rows (GEMV route), H = 128, Ie = 64, E = 4, k = 2, with a residual, against a double
//       loop over the selected experts;
//   LlamaModel::attachExperts / detachExperts  a small fp16 model (both decoders on the fused engine): ONE expert holding the dense
//       FFN's matrices stays within fp16 noise of the model without experts; four random experts move the rows; detachExperts restores
//       the bits; a model on the per-kernel loops refuses experts.
// Run on the GPU by tests/test_moe_cpp_gpu.py; exit code != 0 on any failure.
#include <algorithm>
#include <memory>
#include <numeric>
#include <stdexcept>

#include "../src/kernels/includes/linear.cuh"   // all launchers arrive through api/kernels.hpp
#include "../src/utils/model_utils.h"
#include "test_common.hpp"

namespace {
void verdict(bool ok, const char *what) {
    if (ok) std::printf("%s passed\n", what);
    else { std::printf("FAIL %s\n", what); ++g_failures; }
}

struct Routing {
    std::vector<int> ids;
    std::vector<double> w;
};
// x [rows, H], router [E, H] as stored
Routing host_route(const std::vector<float> &x, const std::vector<float> &router, int rows, int H, int E, int k) {
    Routing r;
    for (int m = 0; m < rows; ++m) {
        std::vector<double> lg(E, 0.0);
        for (int e = 0; e < E; ++e)
            for (int i = 0; i < H; ++i) lg[e] += double(x[size_t(m) * H + i]) * router[size_t(e) * H + i];
        std::vector<int> order(E);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lg[a] > lg[b]; });
        double den = 0;
        for (int j = 0; j < k; ++j) den += std::exp(lg[order[j]] - lg[order[0]]);
        for (int j = 0; j < k; ++j) r.ids.push_back(order[j]), r.w.push_back(std::exp(lg[order[j]] - lg[order[0]]) / den);
    }
    return r;
}

void run_route() {
    const int rows = 9, H = 64, E = 8, k = 2;
    std::mt19937_64 rng(3);
    std::uniform_int_distribution<int> d(-3, 3);
    std::vector<float> x(size_t(rows) * H), router(size_t(E) * H);
    for (auto &v : x) v = float(d(rng));
    for (auto &v : router) v = float(d(rng)) / 32.f;
    for (int i = 0; i < H; ++i) router[size_t(1) * H + i] = router[size_t(2) * H + i] = router[i], router[size_t(4) * H + i] = router[size_t(3) * H + i];   // exact ties
    DeviceArray<half> d_x(to_half(x)), d_r(to_half(router));
    DeviceArray<int> d_ids(size_t(rows) * k);
    DeviceArray<float> d_w(size_t(rows) * k);
    const DataType th = getTensorType<half>();
    TensorWrapper<half> t_x(Device::GPU, th, {rows, H}, d_x.d), t_r(Device::GPU, th, {E, H}, d_r.d);
    TensorWrapper<int> t_ids(Device::GPU, getTensorType<int>(), {rows, k}, d_ids.d);
    TensorWrapper<float> t_w(Device::GPU, getTensorType<float>(), {rows, k}, d_w.d);
    launchMoeRoute(&t_x, &t_r, &t_ids, &t_w);
    CHECK(hipStreamSynchronize(llmie_api::st()));
    const Routing exp = host_route(x, router, rows, H, E, k);
    check_equal("MoeRoute expert ids", d_ids.download(), exp.ids);
    check_close("MoeRoute weights", d_w.download(), std::vector<float>(exp.w.begin(), exp.w.end()), 1e-6f, 0.f);
    bool tie = false;
    for (int m = 0; m < rows; ++m) tie |= exp.w[size_t(m) * k] == exp.w[size_t(m) * k + 1];
    verdict(tie, "MoeRoute case has an exact tie");
}

void run_ffn() {
    const int H = 128, Ie = 64, E = 4, k = 2;
    std::mt19937_64 rng(5);
    std::uniform_int_distribution<int> d(-3, 3);
    std::vector<float> router(size_t(E) * H);
    for (auto &v : router) v = float(d(rng)) / 64.f;   // exact logits: the device routes as the host does
    const std::vector<float> gu = storage_round<half>(randn(rng, size_t(E) * 2 * Ie * H, 1.f / std::sqrt(float(H))));
    const std::vector<float> dn = storage_round<half>(randn(rng, size_t(E) * H * Ie, 1.f / std::sqrt(float(Ie))));
    DeviceArray<half> d_r(to_half(router)), d_gu(to_half(gu)), d_dn(to_half(dn));
    const DataType th = getTensorType<half>();
    TensorWrapper<half> t_r(Device::GPU, th, {E, H}, d_r.d), t_gu(Device::GPU, th, {E, 2 * Ie, H}, d_gu.d), t_dn(Device::GPU, th, {E, H, Ie}, d_dn.d);
    for (int rows : {7, 2}) {
        std::vector<float> x(size_t(rows) * H);
        for (auto &v : x) v = float(d(rng)) / 2.f;
        const std::vector<float> resid = storage_round<half>(randn(rng, size_t(rows) * H, 1.f));
        DeviceArray<half> d_x(to_half(x)), d_res(to_half(resid)), d_y(size_t(rows) * H);
        TensorWrapper<half> t_x(Device::GPU, th, {rows, H}, d_x.d), t_res(Device::GPU, th, {rows, H}, d_res.d), t_y(Device::GPU, th, {rows, H}, d_y.d);
        launchMoeFfn(&t_x, &t_r, &t_gu, &t_dn, &t_res, &t_y, k);
        CHECK(hipStreamSynchronize(llmie_api::st()));
        const Routing rt = host_route(x, router, rows, H, E, k);
        std::vector<float> exp(size_t(rows) * H);
        for (int m = 0; m < rows; ++m) {
            std::vector<double> y(H, 0.0);
            for (int j = 0; j < k; ++j) {
                const int e = rt.ids[size_t(m) * k + j];
                std::vector<double> a(Ie);
                for (int n = 0; n < Ie; ++n) {
                    double g = 0, u = 0;
                    for (int i = 0; i < H; ++i) {
                        g += double(x[size_t(m) * H + i]) * gu[(size_t(e) * 2 * Ie + n) * H + i];
                        u += double(x[size_t(m) * H + i]) * gu[(size_t(e) * 2 * Ie + Ie + n) * H + i];
                    }
                    a[n] = g / (1.0 + std::exp(-g)) * u;
                }
                for (int c = 0; c < H; ++c) {
                    double s = 0;
                    for (int n = 0; n < Ie; ++n) s += a[n] * dn[(size_t(e) * H + c) * Ie + n];
                    y[c] += rt.w[size_t(m) * k + j] * s;
                }
            }
            for (int c = 0; c < H; ++c) exp[size_t(m) * H + c] = float(y[c] + resid[size_t(m) * H + c]);
        }
        // the per-kernel fp16 bar (2e-3 relative / absolute) once for each of the two roundings of the arithmetic, a_j and y
        check_close(rows > 4 ? "MoeFfn grouped route" : "MoeFfn GEMV route", to_float(d_y.download()), exp, 4e-3f, 4e-3f);
    }
}

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
double max_abs_diff(const std::vector<float> &a, const std::vector<float> &b) {
    double m = 0;
    for (size_t i = 0; i < a.size(); ++i) m = std::max(m, std::fabs(double(a[i]) - b[i]));
    return m;
}

void run_model() {
    llm::ModelConfig &c = llm::config();
    c.head_num = 4; c.kv_head_num = 4; c.head_size = 128; c.inter_size = 384; c.num_layers = 2;
    c.max_seq_len = 64; c.vocab_size = 500; c.rotary_embedding_dim = 128;
    const int H = 512, I = 384, E = 4, k = 2, Ie = 128;
    std::unique_ptr<BaseModel> model = make_model(true);
    LlamaModel<half> *lm = static_cast<LlamaModel<half> *>(model.get());
    const ModelRun base = run(lm, H);

    // ONE expert = the layer's own dense matrices: weight 1, the dense FFN
    DeviceArray<half> d_one(to_half(std::vector<float>(H, 0.25f)));
    std::vector<llmie_moe_layer> own;
    for (auto &lw : lm->weights()->llama_layer_weight) own.push_back(llmie_moe_layer{d_one.d, lw->ffn_weight.gate_and_up.data, lw->ffn_weight.down.data});
    lm->attachExperts(own, I, 1, 1);
    const ModelRun same = run(lm, H);
    // (the dummy model's FFN moves a hidden row by about 1e-2 in all: the per-kernel fp16 bar, not the multi-layer one, or a dropped
    // FFN would pass)
    check_close("LlamaModel one expert with the dense matrices, prefill", same.prefill, base.prefill, 2e-3f, 2e-3f);
    check_close("LlamaModel one expert with the dense matrices, decode", same.decode, base.decode, 2e-3f, 2e-3f);
    const double noise_p = std::max(max_abs_diff(same.prefill, base.prefill), 1e-3), noise_d = std::max(max_abs_diff(same.decode, base.decode), 1e-3);

    // four random experts on layer 1, layer 0 dense
    std::mt19937_64 rng(11);
    DeviceArray<half> d_r(to_half(randn(rng, size_t(E) * H, 8.f / std::sqrt(float(H)))));
    DeviceArray<half> d_gu(to_half(randu(rng, size_t(E) * 2 * Ie * H, 2.f / std::sqrt(float(H)))));
    DeviceArray<half> d_dn(to_half(randu(rng, size_t(E) * H * Ie, 2.f / std::sqrt(float(Ie)))));
    lm->attachExperts({llmie_moe_layer{nullptr, nullptr, nullptr}, llmie_moe_layer{d_r.d, d_gu.d, d_dn.d}}, Ie, E, k);
    const ModelRun routed = run(lm, H);
    const ModelRun again = run(lm, H);
    check_equal("LlamaModel experts, two runs agree, prefill", again.prefill, routed.prefill);
    check_equal("LlamaModel experts, two runs agree, decode", again.decode, routed.decode);
    const double moved_p = max_abs_diff(routed.prefill, base.prefill), moved_d = max_abs_diff(routed.decode, base.decode);
    std::printf("LlamaModel experts move the rows by up to %.4g (prefill) / %.4g (decode); fp16 noise of the same sequence %.4g / %.4g\n", moved_p,
                moved_d, noise_p, noise_d);
    verdict(moved_p > 4 * noise_p && moved_d > 4 * noise_d, "LlamaModel experts move the hidden rows");
    bool finite = true;
    for (float v : routed.prefill) finite &= std::isfinite(v);
    verdict(finite, "LlamaModel experts give finite rows");

    lm->detachExperts();
    const ModelRun back = run(lm, H);
    check_equal("LlamaModel detached experts, prefill", back.prefill, base.prefill);
    check_equal("LlamaModel detached experts, decode", back.decode, base.decode);
    bool bad_size = false;
    try {
        lm->attachExperts({llmie_moe_layer{d_r.d, d_gu.d, d_dn.d}}, Ie, E, k);
    } catch (const std::runtime_error &) {
        bad_size = true;
    }
    verdict(bad_size, "LlamaModel one expert entry per layer is required");
    model.reset();

    std::unique_ptr<BaseModel> loop_model = make_model(false);
    bool refused = false;
    try {
        static_cast<LlamaModel<half> *>(loop_model.get())->attachExperts({llmie_moe_layer{nullptr, nullptr, nullptr}, llmie_moe_layer{d_r.d, d_gu.d, d_dn.d}}, Ie, E, k);
    } catch (const std::runtime_error &e) {
        refused = std::string(e.what()).find("experts need the fused engine") != std::string::npos;
    }
    verdict(refused, "LlamaModel without the fused engine refuses experts");
}
}  // namespace

int main() {
    run_route();
    run_ffn();
    run_model();
    std::printf(g_failures ? "%d FAILED\n" : "all passed (%d failures)\n", g_failures);
    return g_failures ? 1 : 0;
}
