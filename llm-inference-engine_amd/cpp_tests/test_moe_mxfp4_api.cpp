// The _ex mixture-of-experts entries through the C++ API mirror:
//   launchMoeFfnEx (api/kernels.hpp)  MXFP4 experts given as random codes and scale bytes, with a router bias, gate/up and down biases
//       and the clamped SwiGLU, 7 rows (forced grouped route) and 2 rows (GEMV route), H = 128, Ie = 64, E = 4, k = 2, against a double
//       loop over the exact values of the codes; an fp16 descriptor without biases returns the bits of launchMoeFfn;
//   LlamaModel::attachExperts(descriptors)  a small fp16 model: four MXFP4 experts with the epilogue on layer 1 move the rows, two runs
//       agree, detachExperts restores the bits; fp16 descriptors give the bits of the llmie_moe_layer overload.
// Run on the GPU by tests/test_moe_mxfp4_cpp_gpu.py; exit code != 0 on any failure.
#include <algorithm>
#include <cstdint>
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
const double kMag[8] = {0, 0.5, 1, 1.5, 2, 3, 4, 6};
// exact value of weight i of a matrix stored as codes (two per byte, low nibble = even k) + one e8m0 byte per 32
double weight_at(const std::vector<uint8_t> &wq, const std::vector<uint8_t> &sc, size_t i) {
    const unsigned code = (wq[i / 2] >> (4 * (i % 2))) & 0xF;
    return (code & 8 ? -1.0 : 1.0) * kMag[code & 7] * std::ldexp(1.0, int(sc[i / 32]) - 127);
}
struct Mx4 {
    std::vector<uint8_t> q, s;
};
// random codes; block exponents base .. base + 3, neighbouring blocks and rows differ
Mx4 random_mx4(std::mt19937_64 &rng, size_t rows, int K, int base) {
    Mx4 m;
    m.q.resize(rows * K / 2), m.s.resize(rows * K / 32);
    for (auto &b : m.q) b = static_cast<uint8_t>(rng() & 0xFF);
    for (size_t n = 0; n < rows; ++n)
        for (int b = 0; b < K / 32; ++b) m.s[n * (K / 32) + b] = static_cast<uint8_t>(127 + base + (b * 3 + n) % 4);
    return m;
}

struct Routing {
    std::vector<int> ids;
    std::vector<double> w;
};
Routing host_route(const std::vector<float> &x, const std::vector<float> &router, const std::vector<float> &bias, int rows, int H, int E, int k) {
    Routing r;
    for (int m = 0; m < rows; ++m) {
        std::vector<double> lg(E, 0.0);
        for (int e = 0; e < E; ++e) {
            for (int i = 0; i < H; ++i) lg[e] += double(x[size_t(m) * H + i]) * router[size_t(e) * H + i];
            lg[e] += bias[e];
        }
        std::vector<int> order(E);
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lg[a] > lg[b]; });
        double den = 0;
        for (int j = 0; j < k; ++j) den += std::exp(lg[order[j]] - lg[order[0]]);
        for (int j = 0; j < k; ++j) r.ids.push_back(order[j]), r.w.push_back(std::exp(lg[order[j]] - lg[order[0]]) / den);
    }
    return r;
}

void run_ffn() {
    const int H = 128, Ie = 64, E = 4, k = 2;
    const float alpha = 1.702f, limit = 1.0f;
    std::mt19937_64 rng(5);
    std::uniform_int_distribution<int> d(-3, 3);
    std::vector<float> router(size_t(E) * H), rbias(E);
    for (auto &v : router) v = float(d(rng)) / 64.f;   // exact logits, with the bias too: the device routes as the host does
    for (auto &v : rbias) v = float(d(rng)) / 128.f;
    const Mx4 gu = random_mx4(rng, size_t(E) * 2 * Ie, H, -7), dn = random_mx4(rng, size_t(E) * H, Ie, -6);
    const std::vector<float> gub = storage_round<half>(randn(rng, size_t(E) * 2 * Ie, 0.25f)), dnb = storage_round<half>(randn(rng, size_t(E) * H, 0.5f));
    DeviceArray<half> d_r(to_half(router)), d_rb(to_half(rbias)), d_gub(to_half(gub)), d_dnb(to_half(dnb));
    DeviceArray<uint8_t> d_guq(gu.q), d_gus(gu.s), d_dnq(dn.q), d_dns(dn.s);
    llmie_moe_experts ex{};
    ex.format = LLMIE_W_MXFP4, ex.router = d_r.d, ex.router_bias = d_rb.d, ex.gate_up = d_guq.d, ex.gate_up_scale = d_gus.d, ex.gate_up_bias = d_gub.d;
    ex.down = d_dnq.d, ex.down_scale = d_dns.d, ex.down_bias = d_dnb.d, ex.act = LLMIE_MOE_ACT_SWIGLU_CLAMPED, ex.alpha = alpha, ex.limit = limit;
    const DataType th = getTensorType<half>();
    for (int rows : {7, 2}) {
        std::vector<float> x(size_t(rows) * H);
        for (auto &v : x) v = float(d(rng)) / 2.f;
        const std::vector<float> resid = storage_round<half>(randn(rng, size_t(rows) * H, 1.f));
        DeviceArray<half> d_x(to_half(x)), d_res(to_half(resid)), d_y(size_t(rows) * H);
        TensorWrapper<half> t_x(Device::GPU, th, {rows, H}, d_x.d), t_res(Device::GPU, th, {rows, H}, d_res.d), t_y(Device::GPU, th, {rows, H}, d_y.d);
        launchMoeFfnEx(&t_x, ex, &t_res, &t_y, Ie, E, k, rows > 4 ? LLMIE_MOE_FORCE_GROUPED : 0u);
        CHECK(hipStreamSynchronize(llmie_api::st()));
        const Routing rt = host_route(x, router, rbias, rows, H, E, k);
        std::vector<float> exp(size_t(rows) * H);
        size_t clamped = 0;
        for (int m = 0; m < rows; ++m) {
            std::vector<double> y(H, 0.0);
            for (int j = 0; j < k; ++j) {
                const int e = rt.ids[size_t(m) * k + j];
                std::vector<double> a(Ie);
                for (int n = 0; n < Ie; ++n) {
                    double g = gub[size_t(e) * 2 * Ie + n], u = gub[size_t(e) * 2 * Ie + Ie + n];
                    for (int i = 0; i < H; ++i) {
                        g += double(x[size_t(m) * H + i]) * weight_at(gu.q, gu.s, (size_t(e) * 2 * Ie + n) * H + i);
                        u += double(x[size_t(m) * H + i]) * weight_at(gu.q, gu.s, (size_t(e) * 2 * Ie + Ie + n) * H + i);
                    }
                    clamped += g > limit || std::fabs(u) > limit;
                    g = std::min(g, double(limit)), u = std::max(std::min(u, double(limit)), -double(limit));
                    a[n] = (u + 1.0) * g / (1.0 + std::exp(-double(alpha) * g));
                }
                for (int c = 0; c < H; ++c) {
                    double s = dnb[size_t(e) * H + c];
                    for (int n = 0; n < Ie; ++n) s += a[n] * weight_at(dn.q, dn.s, (size_t(e) * H + c) * Ie + n);
                    y[c] += rt.w[size_t(m) * k + j] * s;
                }
            }
            for (int c = 0; c < H; ++c) exp[size_t(m) * H + c] = float(y[c] + resid[size_t(m) * H + c]);
        }
        // the per-kernel fp16 bar (2e-3 relative / absolute) once for each of the two roundings of the arithmetic, a_j and y
        check_close(rows > 4 ? "MoeFfnEx MXFP4 grouped route" : "MoeFfnEx MXFP4 GEMV route", to_float(d_y.download()), exp, 4e-3f, 4e-3f);
        verdict(clamped > size_t(rows) * k * Ie / 10 && clamped < size_t(rows) * k * Ie * 9 / 10, "MoeFfnEx case clamps some pairs and not others");
    }
    // an fp16 descriptor without biases under the plain act: the bits of launchMoeFfn
    const int rows = 7;
    const std::vector<float> gu16 = storage_round<half>(randn(rng, size_t(E) * 2 * Ie * H, 1.f / std::sqrt(float(H))));
    const std::vector<float> dn16 = storage_round<half>(randn(rng, size_t(E) * H * Ie, 1.f / std::sqrt(float(Ie))));
    std::vector<float> x(size_t(rows) * H);
    for (auto &v : x) v = float(d(rng)) / 2.f;
    DeviceArray<half> d_gu(to_half(gu16)), d_dn(to_half(dn16)), d_x(to_half(x)), d_y0(size_t(rows) * H), d_y1(size_t(rows) * H);
    TensorWrapper<half> t_r(Device::GPU, th, {E, H}, d_r.d), t_gu(Device::GPU, th, {E, 2 * Ie, H}, d_gu.d), t_dn(Device::GPU, th, {E, H, Ie}, d_dn.d);
    TensorWrapper<half> t_x(Device::GPU, th, {rows, H}, d_x.d), t_y0(Device::GPU, th, {rows, H}, d_y0.d), t_y1(Device::GPU, th, {rows, H}, d_y1.d);
    launchMoeFfn(&t_x, &t_r, &t_gu, &t_dn, nullptr, &t_y0, k);
    llmie_moe_experts f16{};
    f16.format = LLMIE_W_F16, f16.router = d_r.d, f16.gate_up = d_gu.d, f16.down = d_dn.d, f16.act = LLMIE_MOE_ACT_SWIGLU;
    launchMoeFfnEx(&t_x, f16, nullptr, &t_y1, Ie, E, k);
    CHECK(hipStreamSynchronize(llmie_api::st()));
    check_equal("MoeFfnEx fp16 descriptor against MoeFfn", d_y1.download(), d_y0.download());
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
std::unique_ptr<BaseModel> make_model() {
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
        lw->self_attention_weight.output.is_transposed = true;
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
    const int H = 512, E = 4, k = 2, Ie = 128;
    std::unique_ptr<BaseModel> model = make_model();
    LlamaModel<half> *lm = static_cast<LlamaModel<half> *>(model.get());
    const ModelRun base = run(lm, H);

    std::mt19937_64 rng(11);
    DeviceArray<half> d_r(to_half(randn(rng, size_t(E) * H, 8.f / std::sqrt(float(H)))));
    DeviceArray<half> d_rb(to_half(randn(rng, size_t(E), 0.5f)));
    const Mx4 gu = random_mx4(rng, size_t(E) * 2 * Ie, H, -8), dn = random_mx4(rng, size_t(E) * H, Ie, -7);
    DeviceArray<uint8_t> d_guq(gu.q), d_gus(gu.s), d_dnq(dn.q), d_dns(dn.s);
    DeviceArray<half> d_gub(to_half(randn(rng, size_t(E) * 2 * Ie, 0.25f))), d_dnb(to_half(randn(rng, size_t(E) * H, 0.1f)));
    llmie_moe_experts ex{};
    ex.format = LLMIE_W_MXFP4, ex.router = d_r.d, ex.router_bias = d_rb.d, ex.gate_up = d_guq.d, ex.gate_up_scale = d_gus.d, ex.gate_up_bias = d_gub.d;
    ex.down = d_dnq.d, ex.down_scale = d_dns.d, ex.down_bias = d_dnb.d, ex.act = LLMIE_MOE_ACT_SWIGLU_CLAMPED, ex.alpha = 1.702f, ex.limit = 7.f;
    lm->attachExperts(std::vector<llmie_moe_experts>{llmie_moe_experts{}, ex}, Ie, E, k);   // layer 0 dense
    const ModelRun routed = run(lm, H);
    const ModelRun again = run(lm, H);
    check_equal("LlamaModel MXFP4 experts, two runs agree, prefill", again.prefill, routed.prefill);
    check_equal("LlamaModel MXFP4 experts, two runs agree, decode", again.decode, routed.decode);
    const double moved_p = max_abs_diff(routed.prefill, base.prefill), moved_d = max_abs_diff(routed.decode, base.decode);
    std::printf("LlamaModel MXFP4 experts move the rows by up to %.4g (prefill) / %.4g (decode)\n", moved_p, moved_d);
    verdict(moved_p > 4e-3 && moved_d > 4e-3, "LlamaModel MXFP4 experts move the hidden rows");
    bool finite = true;
    for (float v : routed.prefill) finite &= std::isfinite(v);
    for (float v : routed.decode) finite &= std::isfinite(v);
    verdict(finite, "LlamaModel MXFP4 experts give finite rows");
    lm->detachExperts();
    const ModelRun back = run(lm, H);
    check_equal("LlamaModel detached MXFP4 experts, prefill", back.prefill, base.prefill);
    check_equal("LlamaModel detached MXFP4 experts, decode", back.decode, base.decode);

    // fp16 descriptors: the bits of the llmie_moe_layer overload
    DeviceArray<half> d_gu(to_half(randu(rng, size_t(E) * 2 * Ie * H, 2.f / std::sqrt(float(H)))));
    DeviceArray<half> d_dn(to_half(randu(rng, size_t(E) * H * Ie, 2.f / std::sqrt(float(Ie)))));
    lm->attachExperts({llmie_moe_layer{nullptr, nullptr, nullptr}, llmie_moe_layer{d_r.d, d_gu.d, d_dn.d}}, Ie, E, k);
    const ModelRun by_layers = run(lm, H);
    llmie_moe_experts f16{};
    f16.format = LLMIE_W_F16, f16.router = d_r.d, f16.gate_up = d_gu.d, f16.down = d_dn.d, f16.act = LLMIE_MOE_ACT_SWIGLU;
    lm->attachExperts(std::vector<llmie_moe_experts>{llmie_moe_experts{}, f16}, Ie, E, k);
    const ModelRun by_desc = run(lm, H);
    check_equal("LlamaModel fp16 descriptors against llmie_moe_layer, prefill", by_desc.prefill, by_layers.prefill);
    check_equal("LlamaModel fp16 descriptors against llmie_moe_layer, decode", by_desc.decode, by_layers.decode);
    bool refused = false;
    try {
        llmie_moe_experts bad = ex;
        bad.down_scale = nullptr;
        lm->attachExperts(std::vector<llmie_moe_experts>{llmie_moe_experts{}, bad}, Ie, E, k);
        run(lm, H);
    } catch (const std::runtime_error &e) {
        refused = true;
    }
    verdict(refused, "LlamaModel MXFP4 experts without a scale are refused");
}
}  // namespace

int main() {
    run_ffn();
    run_model();
    std::printf(g_failures ? "%d FAILED\n" : "all passed (%d failures)\n", g_failures);
    return g_failures ? 1 : 0;
}
