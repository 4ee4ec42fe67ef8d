// Tree speculative decoding through the C++ API mirror:
//   launchSpecTreePrepare + launchSpecVerifyTree (api/kernels.hpp)  a small batch of greedy trees against plain loops here: depth and
//       ancestor masks, the walk (the lowest live child that carries the pick), a dead child, a finished sequence, the state;
//   launchKvTreeCommit      a dense fp16 cache of known rows against a host gather, one path whose destination is a later source;
//   launchNgramDraftTree    the prefix-sharing example of the header's rule against a host trie;
//   LlamaModel::speculativeTreeStep  a small fp16 model on the fused engine: every chunk carries the plain greedy continuation as
//       ONE branch (not the first child) beside corrupted siblings; the emitted tokens must be the walk over the arg-maxima of the
//       step's own logits rows; afterwards the K cache rows of every cached token -- the accepted nodes, moved into place by the
//       commit -- must equal those of a one-shot prefill of the final sequence within 2e-2 (the bound of tests/test_spec_tree_gpu.py: a
//       row left at its node's slot, a sibling's row or a rotation by index instead of depth is off by O(1)); a model on the per-kernel
//       loops refuses.
// Run on the GPU by tests/test_spec_tree_cpp_gpu.py; exit code != 0 on any failure.
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <stdexcept>

#include "../src/kernels/includes/linear.cuh"   // all launchers arrive through api/kernels.hpp
#include "../src/utils/model_utils.h"
#include "test_common.hpp"

static int argmax_row(const float *row, int V) {   // ties -> the lower id
    int best = 0;
    for (int v = 1; v < V; ++v)
        if (row[v] > row[best]) best = v;
    return best;
}

// llmie_spec_tree_prepare's rule for one sequence
static void prepare_ref(const int *parent, int n, int count, int *depth, uint64_t *anc) {
    depth[0] = 0;
    anc[0] = 1;
    for (int i = 1; i < n; ++i) {
        const int p = parent[i];
        const bool live = i < count && p >= 0 && p < i && (anc[p] & 1);
        depth[i] = live ? depth[p] + 1 : 0;
        anc[i] = live ? (anc[p] | (1ull << i)) : (1ull << i);
    }
}

static void run_verify() {
    const int B = 3, N = 7, V = 13, END = 4;
    std::vector<float> logits(static_cast<size_t>(B) * N * V);
    for (int r = 0; r < B * N; ++r)
        for (int v = 0; v < V; ++v) logits[r * V + v] = 0.25f * static_cast<float>((7 * v + 5 * r) % 11) - 1.f + (v == END ? -9.f : 0.f);
    std::vector<int> pick(B * N);
    for (int r = 0; r < B * N; ++r) pick[r] = argmax_row(&logits[r * V], V);
    //                           0  1  2  3  4  5  6
    const int par[B][N] = {{-1, 0, 0, 2, 2, 4, 1},    // the second child is right at every level: 0 2 4 5
                           {-1, 0, 0, 1, 5, 2, 2},    // the child that carries the pick (node 4) names a later parent: dead, the walk stops at 1
                           {-1, 0, 1, 2, 3, 4, 5}};   // finished on entry
    std::vector<int> parent(B * N), ids(B * N, -3), count = {N, N, N};
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < N; ++i) parent[b * N + i] = par[b][i];
    auto wrong = [&](int t) { return (t + 1) % V; };
    // sequence 0
    ids[1] = wrong(pick[0]); ids[2] = pick[0];
    ids[3] = wrong(pick[2]); ids[4] = pick[2];
    ids[5] = pick[4]; ids[6] = pick[1];
    // sequence 1: nodes 1 and 2 both carry the root's pick (the lowest wins); below node 1 only the dead node 4 carries its pick
    ids[N + 1] = pick[N]; ids[N + 2] = pick[N];
    ids[N + 3] = wrong(pick[N + 1]); ids[N + 4] = pick[N + 1];
    ids[N + 5] = pick[N + 2]; ids[N + 6] = pick[N + 2];
    for (int i = 1; i < N; ++i) ids[2 * N + i] = pick[2 * N + i - 1];
    std::vector<int> e_depth(B * N);
    std::vector<uint64_t> e_anc(B * N);
    for (int b = 0; b < B; ++b) prepare_ref(&parent[b * N], N, count[b], &e_depth[b * N], &e_anc[b * N]);
    std::vector<int> seq = {10, 20, 30}, last = {-7, -7, -7}, cached = {100, 200, 300}, steps = {5, 6, 7};
    std::vector<uint8_t> fin = {0, 0, 1};
    std::vector<int> e_tok(B * N, -1), e_path(B * N, -1), e_cnt(B, 0), e_seq = seq, e_last = last, e_cached = cached, e_steps = steps;
    std::vector<uint8_t> e_fin = fin;
    for (int b = 0; b < B; ++b) {
        if (fin[b]) continue;
        int cur = 0;
        for (;;) {
            const int t = pick[b * N + cur];
            e_tok[b * N + e_cnt[b]] = t;
            e_path[b * N + e_cnt[b]] = cur;
            ++e_cnt[b];
            e_fin[b] = t == END;
            int next = -1;
            for (int j = cur + 1; j < N && next < 0; ++j)
                if ((e_anc[b * N + j] & 1) && parent[b * N + j] == cur && ids[b * N + j] == t) next = j;
            if (t == END || next < 0) break;
            cur = next;
        }
        e_seq[b] += e_cnt[b]; e_cached[b] += e_cnt[b]; e_steps[b] += e_cnt[b];
        e_last[b] = e_tok[b * N + e_cnt[b] - 1];
    }
    std::vector<llmie_sampling_params> params(B, llmie_sampling_params{0.f, 0, 1.f, 0.f, 1.f, 0.f, 0.f, 0u});   // greedy
    DeviceArray<float> d_logits(logits);
    DeviceArray<int> d_parent(parent), d_ids(ids), d_count(count), d_depth(B * N), d_seq(seq), d_last(last), d_cached(cached), d_steps(steps),
        d_tok(B * N), d_cnt(B), d_path(B * N);
    DeviceArray<uint64_t> d_anc(B * N);
    DeviceArray<uint8_t> d_fin(fin);
    DeviceArray<llmie_sampling_params> d_params(params);
    const DataType ti = getTensorType<int>();
    TensorWrapper<float> t_logits(Device::GPU, getTensorType<float>(), {B * N, V}, d_logits.d);
    TensorWrapper<int> t_parent(Device::GPU, ti, {B, N}, d_parent.d), t_ids(Device::GPU, ti, {B, N}, d_ids.d), t_count(Device::GPU, ti, {B}, d_count.d),
        t_depth(Device::GPU, ti, {B, N}, d_depth.d), t_seq(Device::GPU, ti, {B}, d_seq.d), t_last(Device::GPU, ti, {B}, d_last.d),
        t_cached(Device::GPU, ti, {B}, d_cached.d), t_steps(Device::GPU, ti, {B}, d_steps.d), t_tok(Device::GPU, ti, {B, N}, d_tok.d),
        t_cnt(Device::GPU, ti, {B}, d_cnt.d), t_path(Device::GPU, ti, {B, N}, d_path.d);
    TensorWrapper<bool> t_fin(Device::GPU, getTensorType<bool>(), {B}, reinterpret_cast<bool *>(d_fin.d));
    launchSpecTreePrepare(&t_parent, &t_count, &t_depth, d_anc.d);
    launchSpecVerifyTree(&t_logits, &t_ids, &t_parent, &t_depth, d_anc.d, d_params.d, static_cast<TensorWrapper<int> *>(nullptr),
                         static_cast<TensorWrapper<int> *>(nullptr), false, &t_seq, &t_fin, &t_tok, &t_cnt, &t_path,
                         static_cast<TensorWrapper<float> *>(nullptr), &t_last, &t_cached, &t_steps, 0, END);
    CHECK(hipStreamSynchronize(llmie_api::st()));
    check_equal("SpecTreePrepare depth", d_depth.download(), e_depth);
    check_equal("SpecTreePrepare anc", d_anc.download(), e_anc);
    check_equal("SpecVerifyTree tokens", d_tok.download(), e_tok);
    check_equal("SpecVerifyTree path", d_path.download(), e_path);
    check_equal("SpecVerifyTree counts", d_cnt.download(), e_cnt);
    check_equal("SpecVerifyTree seq_len", d_seq.download(), e_seq);
    check_equal("SpecVerifyTree finished", d_fin.download(), e_fin);
    check_equal("SpecVerifyTree last_token", d_last.download(), e_last);
    check_equal("SpecVerifyTree cached_len", d_cached.download(), e_cached);
    check_equal("SpecVerifyTree step_rows", d_steps.download(), e_steps);
    if (e_cnt != std::vector<int>{4, 2, 0} || e_path[1] != 2 || e_path[N + 1] != 1 || (e_anc[N + 4] & 1)) {
        std::printf("FAIL SpecVerifyTree: the case does not cover a deep path / the lowest twin / a dead child / finished (counts %d %d %d)\n", e_cnt[0], e_cnt[1], e_cnt[2]);
        ++g_failures;
    }
}

static void run_commit() {
    const int L = 2, B = 2, KVH = 2, S = 160, HS = 64, N = 8;
    std::vector<float> vals(static_cast<size_t>(L) * B * KVH * S * HS);
    for (size_t i = 0; i < vals.size(); ++i) vals[i] = static_cast<float>(i % 2039) * 0.25f;   // every row differs from its neighbours
    const std::vector<half> k0 = to_half(vals);
    std::vector<half> v0 = k0;
    std::reverse(v0.begin(), v0.end());
    const std::vector<int> path = {0, 2, 3, 5, -1, -1, -1, -1, 0, 7, -1, -1, -1, -1, -1, -1}, count = {4, 2}, base = {126, 3};
    auto expect = [&](const std::vector<half> &c0) {
        std::vector<half> e = c0;
        for (int l = 0; l < L; ++l)
            for (int b = 0; b < B; ++b)
                for (int g = 0; g < KVH; ++g)
                    for (int m = 0; m < count[b]; ++m) {
                        const size_t row = (static_cast<size_t>(l) * B + b) * KVH + g;
                        std::copy(c0.begin() + (row * S + base[b] + path[b * N + m]) * HS, c0.begin() + (row * S + base[b] + path[b * N + m] + 1) * HS,
                                  e.begin() + (row * S + base[b] + m) * HS);
                    }
        return e;
    };
    DeviceArray<half> d_k(k0), d_v(v0);
    DeviceArray<int> d_path(path), d_count(count), d_base(base);
    const DataType ti = getTensorType<int>(), th = getTensorType<half>();
    TensorWrapper<half> t_k(Device::GPU, th, {L, B, KVH, S, HS}, d_k.d), t_v(Device::GPU, th, {L, B, KVH, S, HS}, d_v.d);
    TensorWrapper<int> t_path(Device::GPU, ti, {B, N}, d_path.d), t_count(Device::GPU, ti, {B}, d_count.d), t_base(Device::GPU, ti, {B}, d_base.d);
    launchKvTreeCommit(&t_k, &t_v, static_cast<TensorWrapper<int> *>(nullptr), &t_base, &t_path, &t_count);
    CHECK(hipStreamSynchronize(llmie_api::st()));
    check_equal("KvTreeCommit K rows", to_float(d_k.download()), to_float(expect(k0)));
    check_equal("KvTreeCommit V rows", to_float(d_v.download()), to_float(expect(v0)));
}

static void run_ngram_tree() {
    const int N = 16, K = 3, PAD = -5;
    // suffix "1 2 3": the 3-gram match continues 7 8 9, the later 2-gram match 7 8 5, the 1-gram match 6 6 6
    const std::vector<int> row = {1, 2, 3, 7, 8, 9, 0, 2, 3, 7, 8, 5, 0, 0, 3, 6, 6, 6, 0, 1, 2, 3};
    std::vector<int> tokens = row, len = {static_cast<int>(row.size()), 1};
    tokens.resize(2 * row.size(), 9);
    std::vector<int> e_ids(2 * N, PAD), e_parent(2 * N, -1), e_count = {8, 1};
    const int ids0[] = {3, 7, 8, 9, 5, 6, 6, 6}, par0[] = {-1, 0, 1, 2, 2, 0, 5, 6};
    std::copy(ids0, ids0 + 8, e_ids.begin());
    std::copy(par0, par0 + 8, e_parent.begin());
    e_ids[N] = 9;   // a row of one token: its last token, no drafts
    DeviceArray<int> d_tokens(tokens), d_len(len), d_ids(2 * N), d_parent(2 * N), d_count(2);
    const DataType ti = getTensorType<int>();
    TensorWrapper<int> t_tokens(Device::GPU, ti, {2, static_cast<int>(row.size())}, d_tokens.d), t_len(Device::GPU, ti, {2}, d_len.d),
        t_ids(Device::GPU, ti, {2, N}, d_ids.d), t_parent(Device::GPU, ti, {2, N}, d_parent.d), t_count(Device::GPU, ti, {2}, d_count.d);
    launchNgramDraftTree(&t_tokens, &t_len, static_cast<TensorWrapper<bool> *>(nullptr), K, 4, 3, 1, PAD, &t_ids, &t_parent, &t_count);
    CHECK(hipStreamSynchronize(llmie_api::st()));
    check_equal("NgramDraftTree ids", d_ids.download(), e_ids);
    check_equal("NgramDraftTree parents", d_parent.download(), e_parent);
    check_equal("NgramDraftTree node counts", d_count.download(), e_count);
}

static std::unique_ptr<BaseModel> make_model(bool hf_layout) {
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

static void run_model() {
    llm::ModelConfig &c = llm::config();
    c.head_num = 4; c.kv_head_num = 4; c.head_size = 128; c.inter_size = 352; c.num_layers = 2;
    c.max_seq_len = 96; c.vocab_size = 500; c.rotary_embedding_dim = 128;
    const int V = c.vocab_size, DEPTH = 3, NEW = 14;
    const std::vector<int> prompt = {1, 17, 499, 5, 5, 123, 42, 7, 200, 3, 11, 8, 90, 301, 44, 12, 6, 77};
    // the plain greedy loop: the continuation one branch of every tree is taken from
    std::unique_ptr<BaseModel> plain_model = make_model(true);
    LlamaModel<half> *plain = static_cast<LlamaModel<half> *>(plain_model.get());
    std::vector<int> cont = {plain->generateFirstToken(prompt, 0)};
    while (static_cast<int>(cont.size()) < NEW + DEPTH + 1) cont.push_back(plain->continueWith(cont.back()));
    plain_model.reset();

    std::unique_ptr<BaseModel> model = make_model(true);
    LlamaModel<half> *lm = static_cast<LlamaModel<half> *>(model.get());
    std::vector<int> out = {lm->generateFirstToken(prompt, 0)};
    bool walk_ok = out[0] == cont[0], path_ok = true;
    int steps = 0, accepted = 0, cut = 0, off_first = 0;
    while (static_cast<int>(out.size()) < NEW && walk_ok) {
        const int at = static_cast<int>(out.size());
        // per level two siblings: a corrupted one FIRST, then the continuation's token; the next level hangs on the right one.  Every
        // third step the right node of level 1 is missing (both siblings wrong): the walk must stop behind the root.
        std::vector<int> drafts, parent = {-1};
        int hang = 0;
        for (int d = 0; d < DEPTH; ++d) {
            const int right = cont[at + d];
            const bool missing = d == 1 && steps % 3 == 2;
            drafts.push_back((right + 1) % V);
            parent.push_back(hang);
            drafts.push_back(missing ? (right + 2) % V : right);
            parent.push_back(hang);
            hang = static_cast<int>(parent.size()) - 1;
        }
        const int n = static_cast<int>(parent.size());
        std::vector<int> path;
        const std::vector<int> got = lm->speculativeTreeStep(out.back(), drafts, parent, &path);
        std::vector<half> rows(static_cast<size_t>(n) * V);
        CHECK(hipMemcpy(rows.data(), lm->lastLogits(), sizeof(half) * rows.size(), hipMemcpyDeviceToHost));
        const std::vector<float> f = to_float(rows);
        std::vector<int> expect, epath;
        for (int cur = 0;;) {
            const int t = argmax_row(&f[static_cast<size_t>(cur) * V], V);
            expect.push_back(t);
            epath.push_back(cur);
            int next = -1;
            for (int j = cur + 1; j < n && next < 0; ++j)
                if (parent[j] == cur && drafts[j - 1] == t) next = j;
            if (t == 2 /* EOS */ || next < 0) break;
            cur = next;
        }
        walk_ok = got == expect;
        path_ok = path_ok && path == epath;
        accepted += static_cast<int>(got.size()) - 1;
        cut += got.size() < static_cast<size_t>(DEPTH + 1) ? 1 : 0;
        for (size_t m = 1; m < path.size(); ++m) off_first += path[m] != static_cast<int>(m) ? 1 : 0;
        out.insert(out.end(), got.begin(), got.end());
        std::printf("speculativeTreeStep %d: %zu tokens\n", steps, got.size());
        ++steps;
        if (std::find(got.begin(), got.end(), 2) != got.end()) break;
    }
    if (!walk_ok) { std::printf("FAIL speculativeTreeStep: a step's tokens are not the walk over its logits' arg-maxima\n"); ++g_failures; }
    else std::printf("speculativeTreeStep emits the walk over its logits passed\n");
    if (!path_ok) { std::printf("FAIL speculativeTreeStep: a step's path is not the walk's\n"); ++g_failures; }
    else std::printf("speculativeTreeStep path passed\n");
    if (accepted < 2 || cut < 1 || off_first < 2) { std::printf("FAIL speculativeTreeStep: %d nodes accepted, %d steps cut short, %d accepted nodes off the first-child chain: the loop covers too little\n", accepted, cut, off_first); ++g_failures; }
    else std::printf("speculativeTreeStep accepted %d nodes in %d steps, %d cut short, %d moved by the commit passed\n", accepted, steps, cut, off_first);
    // the accepted rows were moved into place and the rejected siblings' rows never read again: the loop follows the plain greedy loop
    // as far as chunked and one-token forwards round alike (reported; a stale or misplaced row ends the agreement within a step)
    const size_t n = std::min(out.size(), cont.size());
    size_t same = 0;
    while (same < n && out[same] == cont[same]) ++same;
    std::printf("tree loop agrees with the plain greedy loop on the first %zu of %zu tokens\n", same, n);
    // the K rows of the cached tokens (prompt, then every emitted token but the last) against a one-shot prefill of that sequence
    {
        std::vector<int> cached_ids = prompt;
        cached_ids.insert(cached_ids.end(), out.begin(), out.end() - 1);
        const int len = lm->cachedLength();
        const size_t cache = static_cast<size_t>(c.num_layers) * c.kv_head_num * c.max_seq_len * c.head_size;
        std::vector<half> loop_k(cache), shot_k(cache);
        CHECK(hipMemcpy(loop_k.data(), lm->keyCache(), sizeof(half) * cache, hipMemcpyDeviceToHost));
        std::unique_ptr<BaseModel> shot_model = make_model(true);
        LlamaModel<half> *shot = static_cast<LlamaModel<half> *>(shot_model.get());
        shot->generateFirstToken(cached_ids, 0);
        CHECK(hipMemcpy(shot_k.data(), shot->keyCache(), sizeof(half) * cache, hipMemcpyDeviceToHost));
        double worst = 0;
        for (int row = 0; row < c.num_layers * c.kv_head_num; ++row)
            for (int t = 0; t < len; ++t)
                for (int d = 0; d < c.head_size; ++d) {
                    const size_t i = (static_cast<size_t>(row) * c.max_seq_len + t) * c.head_size + d;
                    worst = std::max(worst, std::fabs(double(__half2float(loop_k[i])) - __half2float(shot_k[i])));
                }
        std::printf("max |K tree loop - K one shot| = %.4g over %d cached tokens\n", worst, len);
        if (len != static_cast<int>(cached_ids.size()) || len <= static_cast<int>(prompt.size()) + 4 || !(worst <= 2e-2)) {
            std::printf("FAIL speculativeTreeStep: the cached K rows are not those of a one-shot prefill (%d cached, %zu expected)\n", len, cached_ids.size());
            ++g_failures;
        } else std::printf("speculativeTreeStep cached K rows passed\n");
    }
    model.reset();

    // the per-kernel loops (an output projection that is not in HF layout) know no tree
    std::unique_ptr<BaseModel> loops = make_model(false);
    LlamaModel<half> *ll = static_cast<LlamaModel<half> *>(loops.get());
    const int first = ll->generateFirstToken(prompt, 0);
    bool refused = false;
    try {
        ll->speculativeTreeStep(first, {5, 6}, {-1, 0, 0});
    } catch (const std::exception &) {
        refused = true;
    }
    if (!refused) { std::printf("FAIL speculativeTreeStep: a model on the per-kernel loops took a tree\n"); ++g_failures; }
    else std::printf("speculativeTreeStep refusal passed\n");
}

int main() {
    run_verify();
    run_commit();
    run_ngram_tree();
    run_model();
    std::printf(g_failures ? "%d FAILED\n" : "all passed (%d failures)\n", g_failures);
    return g_failures ? 1 : 0;
}
