// launchBeamSearchStep and launchForkKVPages (api/kernels.hpp) on a tiny case each; the expected values are computed by plain
// loops here.  Run on the GPU by tests/test_beam_cpp_gpu.py; exit code != 0 on any failure.
#include <algorithm>
#include <array>

#include "../src/kernels/includes/topk.cuh"   // all launchers arrive through api/kernels.hpp
#include "test_common.hpp"

static void run_step() {
    const int G = 2, W = 3, V = 11, END = 4;
    std::vector<float> logits(static_cast<size_t>(G) * W * V);
    for (int r = 0; r < G * W; ++r)
        for (int v = 0; v < V; ++v) logits[r * V + v] = 0.25f * static_cast<float>((7 * v + 3 * (r < W ? 0 : r)) % 13) - 1.f;   // group 0: identical rows
    const float inf = INFINITY;
    std::vector<float> cum = {0.f, -inf, -inf, -1.5f, -0.25f, -2.f};
    std::vector<int> len = {0, 0, 0, 3, 2, 3};
    std::vector<uint8_t> fin = {0, 0, 0, 0, 1, 0};   // group 1: live, finished, live

    // expected, by the rules of include/llmie.h in double
    std::vector<int> e_parent(G * W), e_token(G * W), e_len(G * W);
    std::vector<uint8_t> e_fin(G * W);
    std::vector<float> e_cum(G * W);
    for (int g = 0; g < G; ++g) {
        std::vector<std::array<double, 6>> cands;   // score, w, k, token, len, fin
        for (int w = 0; w < W; ++w) {
            const int r = g * W + w;
            if (!(cum[r] > -inf)) continue;
            if (fin[r]) { cands.push_back({cum[r], double(w), 0, double(END), double(len[r]), 1}); continue; }
            double mx = -1e300, sum = 0;
            for (int v = 0; v < V; ++v) mx = std::max(mx, double(logits[r * V + v]));
            for (int v = 0; v < V; ++v) sum += std::exp(double(logits[r * V + v]) - mx);
            const double lse = mx + std::log(sum);
            std::vector<int> ids(V);
            for (int v = 0; v < V; ++v) ids[v] = v;
            std::stable_sort(ids.begin(), ids.end(), [&](int a, int b) { return logits[r * V + a] > logits[r * V + b]; });
            for (int k = 0; k < W; ++k)
                cands.push_back({cum[r] + (logits[r * V + ids[k]] - lse), double(w), double(k), double(ids[k]), double(len[r] + 1), double(ids[k] == END)});
        }
        std::stable_sort(cands.begin(), cands.end(), [](const std::array<double, 6> &a, const std::array<double, 6> &b) { return a[0] > b[0]; });
        for (int j = 0; j < W; ++j) {
            const int r = g * W + j;
            e_parent[r] = g * W + int(cands[j][1]); e_token[r] = int(cands[j][3]); e_cum[r] = float(cands[j][0]);
            e_len[r] = int(cands[j][4]); e_fin[r] = uint8_t(cands[j][5]);
        }
    }

    DeviceArray<float> d_logits(logits), d_cum(cum);
    DeviceArray<int> d_len(len), d_parent(G * W), d_token(G * W);
    DeviceArray<uint8_t> d_fin(fin);
    TensorWrapper<float> t_logits(Device::GPU, getTensorType<float>(), {G * W, V}, d_logits.d), t_cum(Device::GPU, getTensorType<float>(), {G, W}, d_cum.d);
    TensorWrapper<int> t_len(Device::GPU, getTensorType<int>(), {G, W}, d_len.d), t_parent(Device::GPU, getTensorType<int>(), {G, W}, d_parent.d),
        t_token(Device::GPU, getTensorType<int>(), {G, W}, d_token.d);
    TensorWrapper<bool> t_fin(Device::GPU, getTensorType<bool>(), {G, W}, reinterpret_cast<bool *>(d_fin.d));
    launchBeamSearchStep(&t_logits, &t_cum, &t_len, &t_fin, &t_parent, &t_token, END);
    CHECK(hipStreamSynchronize(llmie_api::st()));
    check_equal("BeamSearchStep parent", d_parent.download(), e_parent);
    check_equal("BeamSearchStep token", d_token.download(), e_token);
    check_equal("BeamSearchStep gen_len", d_len.download(), e_len);
    check_equal("BeamSearchStep finished", d_fin.download(), e_fin);
    check_close("BeamSearchStep cum_logprob", d_cum.download(), e_cum, 0.f, 1e-4f);
}

static void run_fork() {
    const int L = 2, P = 7, KVH = 2, HS = 8, ROWS = 3, MP = 2;
    const size_t page = static_cast<size_t>(KVH) * 128 * HS, n = static_cast<size_t>(L) * P * page;
    std::vector<float> k(n), v(n);
    for (size_t i = 0; i < n; ++i) { k[i] = static_cast<float>(i % 1009); v[i] = -static_cast<float>(i % 997); }
    std::vector<int> table = {3, 5, 0, 6, 1, 2}, own = {3, 5, 0, 6, 1, 2}, parent = {0, 0, 1}, lens = {130, 5, 0};
    // row 1 forks from row 0 (130 tokens: page 3 shared, 2 token rows of page 5 copied into page 6); row 2 from row 1 (5 rows of page 0 into page 1)
    std::vector<float> ek = k, ev = v;
    std::vector<int> e_table = table, e_lens = lens;
    for (int j = 0; j < ROWS; ++j) {
        const int q = parent[j];
        if (q == j) continue;
        const int cnt = lens[q], pc = cnt / 128, r = cnt % 128;
        e_lens[j] = cnt;
        for (int p = 0; p < MP; ++p) e_table[j * MP + p] = p < pc ? table[q * MP + p] : own[j * MP + p];
        for (int l = 0; l < L && r > 0; ++l)
            for (int h = 0; h < KVH; ++h)
                for (int i = 0; i < r * HS; ++i) {
                    const size_t s = (static_cast<size_t>(l) * P + table[q * MP + pc]) * page + static_cast<size_t>(h) * 128 * HS + i;
                    const size_t d = (static_cast<size_t>(l) * P + own[j * MP + pc]) * page + static_cast<size_t>(h) * 128 * HS + i;
                    ek[d] = k[s]; ev[d] = v[s];
                }
    }
    DeviceArray<float> d_k(k), d_v(v);
    DeviceArray<int> d_table(table), d_own(own), d_parent(parent), d_lens(lens);
    const DataType tf = getTensorType<float>(), ti = getTensorType<int>();
    TensorWrapper<float> t_k(Device::GPU, tf, {L, P, KVH, 128, HS}, d_k.d), t_v(Device::GPU, tf, {L, P, KVH, 128, HS}, d_v.d);
    TensorWrapper<int> t_table(Device::GPU, ti, {ROWS, MP}, d_table.d), t_own(Device::GPU, ti, {ROWS, MP}, d_own.d),
        t_parent(Device::GPU, ti, {ROWS}, d_parent.d), t_lens(Device::GPU, ti, {ROWS}, d_lens.d);
    launchForkKVPages(&t_k, &t_v, &t_table, &t_own, &t_parent, &t_lens);
    CHECK(hipStreamSynchronize(llmie_api::st()));
    check_equal("ForkKVPages K pool", d_k.download(), ek);
    check_equal("ForkKVPages V pool", d_v.download(), ev);
    check_equal("ForkKVPages block table", d_table.download(), e_table);
    check_equal("ForkKVPages cached lengths", d_lens.download(), e_lens);
    if (ek == k) { std::printf("FAIL ForkKVPages: the case copies nothing\n"); ++g_failures; }
}

int main() {
    run_step();
    run_fork();
    std::printf(g_failures ? "%d FAILED\n" : "all passed (%d failures)\n", g_failures);
    return g_failures ? 1 : 0;
}
