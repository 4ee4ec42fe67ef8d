// launchSpecVerifySampled (api/kernels.hpp) on a tiny case whose outcome plain loops here can tell without restating the sampler:
//   sequence 0  greedy target, greedy drafter: the point masses meet on the arg-maxima, so the walk accepts while the two models'
//               arg-maxima agree and emits the target's at the first disagreement;
//   sequence 1  the drafter IS the target (its rows, its parameters): P == Q, every draft is accepted whatever it is, then the bonus;
//   sequence 2  finished on entry: left alone;
//   sequence 3  greedy target, a drafter sampling at temperature 1 whose draft is not the target's arg-maximum: P_d = 0, rejected,
//               and the residual is the target's arg-maximum.
// Run on the GPU by tests/test_spec_sampled_cpp_gpu.py; exit code != 0 on any failure.
#include <algorithm>
#include <cstdlib>

#include "../api/kernels.hpp"
#include "test_common.hpp"

static int argmax_row(const float *row, int V) {   // ties -> the lower id
    int best = 0;
    for (int v = 1; v < V; ++v)
        if (row[v] > row[best]) best = v;
    return best;
}

int main() {
    const int B = 4, K = 3, V = 11, END = 4;
    std::vector<float> logits(static_cast<size_t>(B) * (K + 1) * V), dlogits(static_cast<size_t>(B) * K * V);
    for (int r = 0; r < B * (K + 1); ++r)
        for (int v = 0; v < V; ++v) logits[r * V + v] = 0.25f * static_cast<float>((7 * v + 5 * r) % 13) - 1.f;
    for (int r = 0; r < B * (K + 1); ++r) logits[r * V + END] = -9.f;   // (no walk ends by chance)
    // the drafter's rows: the target's, but sequence 0 prefers another token at position 2
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < K; ++i) std::copy(&logits[(b * (K + 1) + i) * V], &logits[(b * (K + 1) + i + 1) * V], &dlogits[(b * K + i) * V]);
    const int other = (argmax_row(&logits[2 * V], V) + 3) % V == END ? 0 : (argmax_row(&logits[2 * V], V) + 3) % V;
    dlogits[(0 * K + 2) * V + other] = 5.f;
    std::vector<int> drafts(B * K);
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < K; ++i) drafts[b * K + i] = argmax_row(&dlogits[(b * K + i) * V], V);
    const int seq1[] = {7, 0, 9};   // any tokens do for sequence 1
    std::copy(seq1, seq1 + K, &drafts[1 * K]);
    drafts[3 * K] = (argmax_row(&logits[3 * (K + 1) * V], V) + 1) % V == END ? 0 : (argmax_row(&logits[3 * (K + 1) * V], V) + 1) % V;

    const llmie_sampling_params greedy{0.f, 0, 1.f, 0.f, 1.f, 0.f, 0.f, 0u}, warm{1.f, 0, 1.f, 0.f, 1.f, 0.f, 0.f, 77u},
        warm_draft{1.f, 0, 1.f, 0.f, 1.f, 0.f, 0.f, 78u};
    std::vector<llmie_sampling_params> params = {greedy, warm, warm, greedy}, dparams = {greedy, warm, warm, warm_draft};
    std::vector<int> seq = {10, 20, 30, 40}, last = {-7, -7, -7, -7}, cached = {100, 200, 300, 400}, steps = {5, 6, 7, 8};
    std::vector<uint8_t> fin = {0, 0, 1, 0};

    // the plain loops
    std::vector<int> e_tok(B * (K + 1), -1), e_cnt(B, 0), e_acc(B, 0);
    for (int b : {0, 3})
        for (int i = 0; i <= K; ++i) {
            const int t = argmax_row(&logits[(b * (K + 1) + i) * V], V);
            e_tok[b * (K + 1) + i] = t;
            ++e_cnt[b];
            if (i == K || t != drafts[b * K + i]) break;
            ++e_acc[b];
        }
    std::copy(&drafts[K], &drafts[2 * K], &e_tok[K + 1]);
    e_cnt[1] = K + 1;
    e_acc[1] = K;
    std::vector<int> e_seq = seq, e_cached = cached, e_steps = steps;
    for (int b = 0; b < B; ++b) { e_seq[b] += e_cnt[b]; e_cached[b] += e_cnt[b]; e_steps[b] += e_cnt[b]; }

    DeviceArray<float> d_logits(logits), d_dlogits(dlogits);
    DeviceArray<int> d_drafts(drafts), d_seq(seq), d_last(last), d_cached(cached), d_steps(steps), d_tok(B * (K + 1)), d_cnt(B), d_acc(B);
    DeviceArray<uint8_t> d_fin(fin);
    DeviceArray<llmie_sampling_params> d_params(params), d_dparams(dparams);
    const DataType ti = getTensorType<int>();
    TensorWrapper<float> t_logits(Device::GPU, getTensorType<float>(), {B * (K + 1), V}, d_logits.d),
        t_dlogits(Device::GPU, getTensorType<float>(), {B, K, V}, d_dlogits.d);
    TensorWrapper<int> t_drafts(Device::GPU, ti, {B, K}, d_drafts.d), t_seq(Device::GPU, ti, {B}, d_seq.d), t_last(Device::GPU, ti, {B}, d_last.d),
        t_cached(Device::GPU, ti, {B}, d_cached.d), t_steps(Device::GPU, ti, {B}, d_steps.d), t_tok(Device::GPU, ti, {B, K + 1}, d_tok.d),
        t_cnt(Device::GPU, ti, {B}, d_cnt.d), t_acc(Device::GPU, ti, {B}, d_acc.d);
    TensorWrapper<bool> t_fin(Device::GPU, getTensorType<bool>(), {B}, reinterpret_cast<bool *>(d_fin.d));
    TensorWrapper<int> *none = nullptr;
    launchSpecVerifySampled(&t_logits, &t_dlogits, &t_drafts, none, d_params.d, d_dparams.d, none, none, false, &t_seq, &t_fin, &t_tok, &t_cnt,
                            &t_acc, static_cast<TensorWrapper<float> *>(nullptr), &t_last, &t_cached, &t_steps, 0, END);
    CHECK(hipStreamSynchronize(llmie_api::st()));
    std::vector<int> tok = d_tok.download();
    const int bonus = tok[1 * (K + 1) + K];   // sequence 1's bonus token is the sampler's draw: any token but the one END's logit rules out
    if (bonus < 0 || bonus >= V) { std::printf("FAIL SpecVerifySampled: bonus token %d\n", bonus); ++g_failures; }
    e_tok[1 * (K + 1) + K] = bonus;
    std::vector<int> e_last = last;
    for (int b = 0; b < B; ++b)
        if (e_cnt[b]) e_last[b] = e_tok[b * (K + 1) + e_cnt[b] - 1];
    check_equal("SpecVerifySampled tokens", tok, e_tok);
    check_equal("SpecVerifySampled counts", d_cnt.download(), e_cnt);
    check_equal("SpecVerifySampled accepted", d_acc.download(), e_acc);
    check_equal("SpecVerifySampled seq_len", d_seq.download(), e_seq);
    check_equal("SpecVerifySampled finished", d_fin.download(), fin);
    check_equal("SpecVerifySampled last_token", d_last.download(), e_last);
    check_equal("SpecVerifySampled cached_len", d_cached.download(), e_cached);
    check_equal("SpecVerifySampled step_rows", d_steps.download(), e_steps);
    if (e_cnt != std::vector<int>{3, K + 1, 0, 1} || e_acc != std::vector<int>{2, K, 0, 0}) {
        std::printf("FAIL SpecVerifySampled: the case does not cover accept / residual / all accepted / finished / rejected at once\n");
        ++g_failures;
    }
    std::printf(g_failures ? "%d FAILED\n" : "all passed (%d failures)\n", g_failures);
    return g_failures ? 1 : 0;
}
