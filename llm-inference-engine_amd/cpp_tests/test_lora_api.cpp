// launchLoraApply (api/kernels.hpp) on a small mixed batch: two adapters of rank 8 and 32 on a three-block projection, rows without
// an adapter, an empty slot and a slot outside the table; the expected values are computed by plain loops in double.  Run on the GPU
// by tests/test_lora_engine_gpu.py; exit code != 0 on any failure.
#include <memory>
#include <stdexcept>

#include "../src/kernels/includes/linear.cuh"   // all launchers arrive through api/kernels.hpp
#include "../src/utils/model_utils.h"
#include "test_common.hpp"

// LlamaModel::loadAdapter / selectAdapter: a small fp16 model (head_size 128, HF-layout matrices: both decoders run the fused engine)
// with random weights.  Checked on the hidden rows of a prefill and of one decode step: slot -1 agrees with a model that never saw
// an adapter (another launch sequence, same mathematics); a loaded slot moves them far; the same adapter in another slot gives the
// same bits; an emptied slot gives the bits of -1.  A model whose layers are not all in HF layout refuses the adapter.
namespace {
struct ModelRun {
    std::vector<float> prefill, decode;
};
double rel_fro(const std::vector<float> &a, const std::vector<float> &b) {
    double num = 0, den = 1e-30;
    for (size_t i = 0; i < a.size(); ++i) num += (double(a[i]) - b[i]) * (double(a[i]) - b[i]), den += double(b[i]) * b[i];
    return std::sqrt(num / den);
}
const std::vector<int> kPrompt = {1, 17, 499, 5, 5, 123, 42, 7, 200, 3, 11, 8, 90, 301, 44, 12, 6, 77};
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
void run_model() {
    llm::ModelConfig &c = llm::config();
    c.head_num = 4; c.kv_head_num = 4; c.head_size = 128; c.inter_size = 352; c.num_layers = 2;
    c.max_seq_len = 64; c.vocab_size = 500; c.rotary_embedding_dim = 128;
    const int H = 512, QKV = 3 * H, I = 352, L = 2, RANK = 8;
    std::mt19937_64 rng(21);
    // one adapter on all four modules of both layers
    const int blocks[4] = {3, 1, 2, 1}, Ns[4] = {QKV, H, 2 * I, H}, Ks[4] = {H, H, H, I};
    std::vector<std::unique_ptr<DeviceArray<half>>> keep;
    llmie_lora_layer layers[L] = {};
    for (int l = 0; l < L; ++l)
        for (int mo = 0; mo < 4; ++mo) {
            keep.push_back(std::make_unique<DeviceArray<half>>(to_half(randn(rng, static_cast<size_t>(blocks[mo]) * RANK * Ks[mo], 1.f / std::sqrt(float(Ks[mo]))))));
            layers[l].a[mo] = keep.back()->d;
            keep.push_back(std::make_unique<DeviceArray<half>>(to_half(randn(rng, static_cast<size_t>(Ns[mo]) * RANK, 0.5f / std::sqrt(float(RANK))))));
            layers[l].b[mo] = keep.back()->d;
        }
    const llmie_lora_adapter desc{RANK, 16.f, L, layers};

    std::unique_ptr<BaseModel> plain_model = make_model(true);
    const ModelRun base = run(static_cast<LlamaModel<half> *>(plain_model.get()), H);
    plain_model.reset();

    std::unique_ptr<BaseModel> model = make_model(true);
    LlamaModel<half> *lm = static_cast<LlamaModel<half> *>(model.get());
    lm->loadAdapter(3, &desc);
    lm->selectAdapter(-1);
    const ModelRun none = run(lm, H);
    lm->selectAdapter(3);
    const ModelRun with3 = run(lm, H);
    lm->loadAdapter(5, &desc);
    lm->selectAdapter(5);
    const ModelRun with5 = run(lm, H);
    lm->loadAdapter(3, nullptr);
    lm->selectAdapter(3);
    const ModelRun emptied = run(lm, H);
    const double near_p = rel_fro(none.prefill, base.prefill), near_d = rel_fro(none.decode, base.decode);
    const double far_p = rel_fro(with3.prefill, base.prefill), far_d = rel_fro(with3.decode, base.decode);
    std::printf("LlamaModel adapters: slot -1 vs no table %.4g / %.4g (prefill / decode), loaded slot vs no table %.4g / %.4g\n", near_p, near_d, far_p, far_d);
    if (near_p <= 2e-2 && near_d <= 2e-2) std::printf("LlamaModel slot -1 agrees with the base model passed\n");
    else { std::printf("FAIL LlamaModel slot -1 agrees with the base model\n"); ++g_failures; }
    if (far_p >= 0.1 && far_d >= 0.1) /* five times the bar the slot -1 rows are held to */ std::printf("LlamaModel loaded slot moves the hidden rows passed\n");
    else { std::printf("FAIL LlamaModel loaded slot moves the hidden rows\n"); ++g_failures; }
    check_equal("LlamaModel same adapter in another slot, prefill", with5.prefill, with3.prefill);
    check_equal("LlamaModel same adapter in another slot, decode", with5.decode, with3.decode);
    check_equal("LlamaModel emptied slot, prefill", emptied.prefill, none.prefill);
    check_equal("LlamaModel emptied slot, decode", emptied.decode, none.decode);
    model.reset();

    // a model that runs the per-kernel loops (a matrix not in HF layout) must refuse, not ignore, an adapter
    std::unique_ptr<BaseModel> loop_model = make_model(false);
    bool refused = false;
    try {
        static_cast<LlamaModel<half> *>(loop_model.get())->loadAdapter(0, &desc);
    } catch (const std::runtime_error &e) {
        refused = std::string(e.what()).find("adapters need the fused engine") != std::string::npos;
    }
    if (refused) std::printf("LlamaModel without the fused engine refuses adapters passed\n");
    else { std::printf("FAIL LlamaModel without the fused engine refuses adapters\n"); ++g_failures; }
}
}  // namespace

int main() {
    const int ROWS = 21, K = 96, SLOTS = 3, LAYERS = 2, LAYER = 1;
    const std::vector<int> widths = {32, 16, 16};
    const int N = 64, ranks[2] = {8, 32};
    const float scales[2] = {2.f, 0.5f};
    std::mt19937_64 rng(11);
    const std::vector<float> x = storage_round<half>(randn(rng, static_cast<size_t>(ROWS) * K, 1.f));
    const std::vector<float> y = storage_round<half>(randn(rng, static_cast<size_t>(ROWS) * N, 0.1f));
    std::vector<float> A[2], B[2];
    for (int s = 0; s < 2; ++s) {
        A[s] = storage_round<half>(randn(rng, static_cast<size_t>(3) * ranks[s] * K, 1.f / std::sqrt(static_cast<float>(K))));
        B[s] = storage_round<half>(randn(rng, static_cast<size_t>(N) * ranks[s], 1.f / std::sqrt(static_cast<float>(ranks[s]))));
    }
    std::vector<int> slot(ROWS);
    const int pattern[7] = {0, 1, -1, 1, 2 /* empty */, 0, 7 /* outside the table */};
    for (int m = 0; m < ROWS; ++m) slot[m] = m < 17 && m % 2 == 0 ? 1 : pattern[m % 7];   // slot 1 in more than 8 rows

    std::vector<float> expect = y, bound(y.size(), 0.f);
    for (int m = 0; m < ROWS; ++m) {
        const int s = slot[m];
        if (s < 0 || s > 1) continue;
        const int r = ranks[s];
        int c0 = 0;
        for (int j = 0; j < 3; ++j) {
            std::vector<double> t(r, 0.0);
            for (int q = 0; q < r; ++q)
                for (int k = 0; k < K; ++k) t[q] += static_cast<double>(x[m * K + k]) * A[s][(static_cast<size_t>(j) * r + q) * K + k];
            for (int n = c0; n < c0 + widths[j]; ++n) {
                double d = 0.0, mag = 0.0;
                for (int q = 0; q < r; ++q) {
                    d += static_cast<double>(B[s][n * r + q]) * t[q];
                    mag += std::fabs(static_cast<double>(B[s][n * r + q]) * t[q]);
                }
                expect[m * N + n] = static_cast<float>(y[m * N + n] + scales[s] * d);
                bound[m * N + n] = static_cast<float>(scales[s] * mag);
            }
            c0 += widths[j];
        }
    }

    DeviceArray<half> d_x(to_half(x)), d_y(to_half(y)), d_a0(to_half(A[0])), d_b0(to_half(B[0])), d_a1(to_half(A[1])), d_b1(to_half(B[1]));
    DeviceArray<int> d_slot(slot);
    DeviceArray<unsigned char> d_table(llmie_lora_table_bytes(SLOTS, LAYERS));
    CHECK(hipMemset(d_table.d, 0, d_table.n));
    const half *as[2] = {d_a0.d, d_a1.d}, *bs[2] = {d_b0.d, d_b1.d};
    for (int s = 0; s < 2; ++s) {
        llmie_lora_layer layers[LAYERS] = {};
        layers[LAYER].a[LLMIE_LORA_QKV] = as[s];
        layers[LAYER].b[LLMIE_LORA_QKV] = bs[s];
        const llmie_lora_adapter desc{ranks[s], scales[s], LAYERS, layers};
        LLMIE_CALL(llmie_lora_slot_load(d_table.d, SLOTS, LAYERS, s, &desc, llmie_api::st()));
    }
    TensorWrapper<half> t_x(Device::GPU, getTensorType<half>(), {ROWS, K}, d_x.d), t_y(Device::GPU, getTensorType<half>(), {ROWS, N}, d_y.d);
    TensorWrapper<int> t_slot(Device::GPU, getTensorType<int>(), {ROWS}, d_slot.d);
    launchLoraApply(&t_x, &t_y, &t_slot, d_table.d, SLOTS, LAYERS, LAYER, LLMIE_LORA_QKV, widths);
    CHECK(hipStreamSynchronize(llmie_api::st()));
    const std::vector<half> got_h = d_y.download(), y_h = to_half(y);
    const std::vector<float> got = to_float(got_h);

    // adapted rows: |got - ref| <= 2e-3 (|ref| + scale sum |B| |t|) + 1e-6; the others: their input bits
    std::vector<half> untouched_got, untouched_exp;
    bool ok = true, moved = false;
    for (int m = 0; m < ROWS; ++m) {
        const bool adapted = slot[m] == 0 || slot[m] == 1;
        for (int n = 0; n < N; ++n) {
            const size_t i = static_cast<size_t>(m) * N + n;
            if (!adapted) {
                untouched_got.push_back(got_h[i]);
                untouched_exp.push_back(y_h[i]);
                continue;
            }
            moved = moved || std::fabs(expect[i] - y[i]) > 0.05f;
            if (!(std::fabs(got[i] - expect[i]) <= 2e-3f * (std::fabs(expect[i]) + bound[i]) + 1e-6f)) {
                if (ok) std::printf("FAIL LoraApply adapted rows: row %d column %d expected %g got %g\n", m, n, expect[i], got[i]);
                ok = false;
            }
        }
    }
    if (ok && moved) std::printf("LoraApply adapted rows passed\n");
    else ++g_failures;
    if (!moved) std::printf("FAIL LoraApply adapted rows: the case changes nothing\n");
    check_equal("LoraApply untouched rows", untouched_got, untouched_exp);
    run_model();
    std::printf(g_failures ? "%d FAILED\n" : "all passed (%d failures)\n", g_failures);
    return g_failures ? 1 : 0;
}
