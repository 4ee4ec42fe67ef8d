"""Speculative decoding with a SAMPLED draft model, end to end on the paged engines: the two-model loop of INTEGRATION.md.

Target: 2 layers; drafter: 1 layer (the target's first, with its embedding and LM head); 4 heads of 128, V = 1000, paged fp16
caches, k = 3, prompts of 120 tokens so that the chunks cross the 128-token page boundary.  Per step the drafter runs k + 1 single-token steps on its own cache (the last one only caches
the last draft), sampling each draft with lm_head_sample_params and writing the step's logits into its row of draft_logits; the
target runs prefill_paged of k + 1 inputs on top of cached_len, rmsnorm + linear, and spec_verify_sampled moves the one
SpecState both engines read.

(a) after 40 steps each engine's K cache over [0, cached_len) equals a one-shot prefill of the final sequences within 2e-2 (the
    bound tests/test_speculative_gpu.py uses): an off-by-one in either engine's length or a stale rejected row moves it by O(1);
(b) with the target's temperature 0 the emitted text equals the plain greedy loop bit for bit;
(c) with the drafter built on the target's own weights and parameters every chunk emits k + 1 tokens;
(d) one captured step replayed 8 times equals the eager loop."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16
NH, KVH, HS, INTER, V = 4, 4, 128, 512, 1000
B, PROMPT, K, STEPS = 3, 120, 3, 40
H, MAX_PAGES, EPS = NH * HS, 3, 1e-5
MAX_SEQ = MAX_PAGES * 128


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


class Model:
    """an engine with its embedding, final norm and LM head"""

    def __init__(self, llmie, rng, layers, weights=None):
        self.llmie, self.nl = llmie, layers
        QKV = (NH + 2 * KVH) * HS
        u = lambda shape, s: torch.from_numpy((rng.uniform(-1, 1, shape) * s).astype(np.float32)).to(DEV).to(F16)
        if weights is None:
            lw = [dict(attn_norm=u((H,), 0.2) + 1, qkv=dict(data=u((QKV, H), 2 / np.sqrt(H))), o=dict(data=u((H, H), 2 / np.sqrt(H))),
                       ffn_norm=u((H,), 0.2) + 1, gate_up=dict(data=u((2 * INTER, H), 2 / np.sqrt(H))),
                       down=dict(data=u((H, INTER), 2 / np.sqrt(INTER)))) for _ in range(layers)]
            for w in lw[1:]:      # the later layers move the residual stream less: a drafter of the first layer alone is a fair guess
                w["o"]["data"] *= 0.5
                w["down"]["data"] *= 0.5
            weights = (lw, u((V, H), 1.0), u((V, H), 3 / np.sqrt(H)), u((H,), 0.2) + 1)
        self.weights = weights
        lw, self.embed, self.lm_head, self.gamma = weights
        cfg = dict(head_num=NH, kv_head_num=KVH, head_size=HS, inter_size=INTER, num_layers=layers, vocab_size=V, max_seq_len=MAX_SEQ,
                   max_batch=B, rotary_dim=HS, rotary_base=10000.0, rms_eps=EPS, dtype=llmie.F16, wfmt=llmie.W_F16, int4_group=128,
                   kv_fmt=llmie.KV_NATIVE, k_scale=1.0, v_scale=1.0)
        self.dec = llmie.Decoder(cfg, lw)
        self.num_pages = B * MAX_PAGES + 2

    def pages(self, rng):
        z = lambda: torch.zeros((self.nl, self.num_pages, KVH, 128, HS), dtype=F16, device=DEV)
        table = torch.from_numpy(rng.permutation(self.num_pages)[:B * MAX_PAGES].astype(np.int32)).reshape(B, MAX_PAGES).to(DEV)
        return z(), z(), table

    def chunk(self, ids, kp, vp, table, in_len, hist_len, max_q, hidden=None, logits=None):
        T = ids.numel()
        x = torch.empty((T, H), dtype=F16, device=DEV) if hidden is None else hidden
        self.llmie.input_embedding(ids, self.embed, x)
        out = self.dec.prefill_paged(x, torch.empty_like(x), kp, vp, table, in_len, hist_len, max_q)
        self.llmie.rmsnorm(out, None, self.gamma, EPS)
        logits = torch.empty((T, V), dtype=F16, device=DEV) if logits is None else logits
        self.llmie.linear(out, self.lm_head, logits)
        return logits

    def dense_k(self, kp, table, lens):
        kd = torch.zeros((self.nl, B, KVH, MAX_SEQ, HS), dtype=kp.dtype, device=DEV)
        self.llmie.kv_pages_copy(kd, kp, table, lens, False)
        return kd


class Loop:
    """the two-model loop: every buffer lives here, so that step() allocates nothing and can be captured"""

    def __init__(self, llmie, target, drafter, params, dparams, rng, prompt):
        self.llmie, self.t, self.d = llmie, target, drafter
        self.params, self.dparams = llmie.sampling_params(params), llmie.sampling_params(dparams)
        self.kp, self.vp, self.table = target.pages(rng)
        self.dkp, self.dvp, self.dtable = drafter.pages(rng)
        self.seq, self.fin = _i32([0] * B), torch.zeros(B, dtype=torch.uint8, device=DEV)
        lens, zero = _i32([PROMPT] * B), _i32([0] * B)
        logits = target.chunk(prompt, self.kp, self.vp, self.table, lens, zero, PROMPT)
        drafter.chunk(prompt, self.dkp, self.dvp, self.dtable, lens, zero, PROMPT)
        first = torch.empty(B, dtype=torch.int32, device=DEV)
        llmie.sample_logits(logits[PROMPT - 1::PROMPT].contiguous(), self.params, self.seq, self.fin, first, 0, -1)
        self.state = llmie.spec_state(first, [PROMPT] * B, [1] * B)
        T = B * (K + 1)
        e = lambda shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=DEV)
        self.ids_t, self.ids, self.drafts = e((K + 1, B)), e((B, K + 1)), e((B, K))
        self.draft_logits, self.row_logits = e((B, K, V), F16), e((B, V), F16)
        self.dx, self.dy, self.d_lens = e((B, H), F16), e((B, H), F16), e(B)
        self.d_seq, self.d_fin, self.d_step = e(B), e(B, torch.uint8), e(1)
        self.hidden, self.logits = e((T, H), F16), e((T, V), F16)
        self.tok, self.cnt, self.acc, self.total = e((B, K + 1)), e(B), e(B), e(B)
        self.in_len = _i32([K + 1] * B)
        self.ws_s = e(llmie.sample_logits_workspace_bytes(B, V), torch.uint8)
        self.ws_v = e(llmie.spec_verify_sampled_workspace_bytes(B, K, V), torch.uint8)

    def step(self):
        llmie, st = self.llmie, self.state
        self.ids_t[0].copy_(st.last_token)
        for i in range(K + 1):     # the drafter: one token per step on top of cached_len + i tokens; the last step only caches draft k - 1
            llmie.input_embedding(self.ids_t[i], self.d.embed, self.dx)
            torch.add(st.cached_len, i + 1, out=self.d_lens)
            self.d.dec.forward_paged_ragged(self.dx, self.dy, self.dkp, self.dvp, self.dtable, self.d_lens)
            if i < K:
                self.d.dec.lm_head_sample_params(self.dy, self.d.gamma, self.d.lm_head, llmie.W_F16, self.row_logits, self.dparams, self.d_seq,
                                                 self.d_fin, self.ids_t[i + 1], -1, -1, step_dev=self.d_step, advance=True, workspace=self.ws_s)
                self.draft_logits[:, i].copy_(self.row_logits)
        self.ids.copy_(self.ids_t.t())
        self.drafts.copy_(self.ids_t[1:].t())
        self.t.chunk(self.ids.view(-1), self.kp, self.vp, self.table, self.in_len, st.cached_len, K + 1, hidden=self.hidden, logits=self.logits)
        llmie.spec_verify_sampled(self.logits, self.draft_logits, self.drafts, self.params, self.dparams, self.seq, self.fin, -1, state=st,
                                  out_accepted=self.acc, workspace=self.ws_v, out=(self.tok, self.cnt))
        self.total += self.cnt

    def snapshot(self):
        names = ("kp", "vp", "dkp", "dvp", "seq", "fin", "d_seq", "d_fin", "d_step", "tok", "cnt", "acc", "total")
        snap = {n: getattr(self, n).clone() for n in names}
        snap.update(last=self.state.last_token.clone(), cached=self.state.cached_len.clone(), steps=self.state.step_rows.clone())
        return snap

    def restore(self, snap):
        for n, t in snap.items():
            dst = dict(last=self.state.last_token, cached=self.state.cached_len, steps=self.state.step_rows).get(n)
            (getattr(self, n) if dst is None else dst).copy_(t)


def _pair(llmie, rng):
    """the 2-layer target and its 1-layer drafter: the target's first layer, embedding, final norm and LM head (two random models
    would agree on nothing, and no draft would ever be accepted)"""
    target = Model(llmie, rng, 2)
    lw, embed, lm_head, gamma = target.weights
    return target, Model(llmie, rng, 1, weights=(lw[:1], embed, lm_head, gamma))


def _run(loop, steps):
    """eager steps with a host read after each -> emitted tokens per sequence (the first token included), counts per step"""
    out = [[t] for t in loop.state.last_token.tolist()]
    counts, accepted = [], []
    for _ in range(steps):
        cached = loop.state.cached_len.tolist()
        loop.step()
        tok, cnt = loop.tok.tolist(), loop.cnt.tolist()
        for b in range(B):
            assert 1 <= cnt[b] <= K + 1 and tok[b][cnt[b]:] == [-1] * (K + 1 - cnt[b])
            out[b] += tok[b][:cnt[b]]
        assert loop.state.cached_len.tolist() == [cached[b] + cnt[b] for b in range(B)]
        assert loop.state.last_token.tolist() == [o[-1] for o in out] and loop.acc.tolist() == [c - 1 for c in cnt]
        counts.append(cnt)
        accepted.append(loop.acc.tolist())
    return out, np.array(counts)


SAMPLED = [dict(temperature=0.9, top_k=40, seed=11 + b) for b in range(B)]
DRAFT = [dict(temperature=1.0, top_k=60, seed=900 + b) for b in range(B)]


def test_both_caches_equal_a_one_shot_prefill_of_the_final_sequences(llmie):
    rng = np.random.default_rng(2026)
    target, drafter = _pair(llmie, rng)
    prompt = _i32(rng.integers(3, V, B * PROMPT))
    loop = Loop(llmie, target, drafter, SAMPLED, DRAFT, rng, prompt)
    out, counts = _run(loop, STEPS)
    lens = loop.state.cached_len.tolist()
    assert lens == [PROMPT + len(o) - 1 for o in out] and min(lens) > 128 and loop.seq.tolist() == [len(o) for o in out]
    print("tokens per step: mean %.2f; chunks by count 1 .. k + 1: %s" % (counts.mean(), np.bincount(counts.reshape(-1), minlength=K + 2)[1:].tolist()))
    assert counts.min() == 1 and counts.max() >= 3     # rejections, and runs of acceptances, both happen
    p = prompt.reshape(B, PROMPT).tolist()
    flat = _i32([t for b in range(B) for t in p[b] + out[b][:-1]])      # the cached tokens: all but the last emitted one
    dl = _i32(lens)
    for name, m, kp, table in (("target", target, loop.kp, loop.table), ("drafter", drafter, loop.dkp, loop.dtable)):
        kp2, vp2, table2 = m.pages(rng)
        m.chunk(flat, kp2, vp2, table2, dl, _i32([0] * B), max(lens))
        ka, kb = m.dense_k(kp, table, dl).float(), m.dense_k(kp2, table2, dl).float()
        for b in range(B):
            diff = (ka[:, b, :, :lens[b]] - kb[:, b, :, :lens[b]]).abs().max().item()
            print("%s, sequence %d: max |K loop - K one shot| = %.4g over %d tokens" % (name, b, diff, lens[b]))
            assert diff <= 2e-2
    target.dec.close()
    drafter.dec.close()


def test_a_greedy_target_emits_the_plain_greedy_text(llmie):
    rng = np.random.default_rng(2027)
    target, drafter = _pair(llmie, rng)
    prompt = _i32(rng.integers(3, V, B * PROMPT))
    greedy = [dict(temperature=0.0)] * B
    loop = Loop(llmie, target, drafter, greedy, DRAFT, rng, prompt)
    out, counts = _run(loop, STEPS)
    n_new = min(len(o) for o in out)
    # the plain loop: no drafter, one token per step through the same chunk forward
    kp, vp, table = target.pages(rng)
    params = llmie.sampling_params(greedy)
    seq, fin, cur = _i32([0] * B), torch.zeros(B, dtype=torch.uint8, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV)
    logits = target.chunk(prompt, kp, vp, table, _i32([PROMPT] * B), _i32([0] * B), PROMPT)[PROMPT - 1::PROMPT].contiguous()
    lens, one = _i32([PROMPT] * B), _i32([1] * B)
    plain = []
    for s in range(n_new):
        llmie.sample_logits(logits, params, seq, fin, cur, s, -1)
        plain.append(cur.tolist())
        logits = target.chunk(cur, kp, vp, table, one, lens, 1)
        lens += 1
    plain = np.array(plain).T
    agree = [next((i for i in range(n_new) if out[b][i] != plain[b, i]), n_new) for b in range(B)]
    print("greedy target: %s tokens per sequence, mean %.2f per step; agreement with the plain loop: first %s of %d"
          % ([len(o) for o in out], counts.mean(), agree, n_new))
    assert counts.max() > 1
    for b in range(B):
        assert out[b][:n_new] == plain[b].tolist(), "sequence %d leaves the plain greedy text at token %d" % (b, agree[b])
    target.dec.close()
    drafter.dec.close()


def test_the_targets_twin_as_drafter_has_every_draft_accepted(llmie):
    rng = np.random.default_rng(2028)
    target = Model(llmie, rng, 2)
    twin = Model(llmie, rng, 2, weights=target.weights)
    prompt = _i32(rng.integers(3, V, B * PROMPT))
    twin_params = [dict(p, seed=500 + b) for b, p in enumerate(SAMPLED)]   # the target's controls; its own draws
    loop = Loop(llmie, target, twin, SAMPLED, twin_params, rng, prompt)
    out, counts = _run(loop, STEPS)
    short = int((counts < K + 1).sum())
    print("twin drafter: %d of %d chunks short of k + 1" % (short, counts.size))
    assert short == 0
    target.dec.close()
    twin.dec.close()


def test_captured_step_equals_eager_loop(llmie):
    REPLAYS = 8
    rng = np.random.default_rng(2029)
    target, drafter = _pair(llmie, rng)
    prompt = _i32(rng.integers(3, V, B * PROMPT))
    loop = Loop(llmie, target, drafter, SAMPLED, DRAFT, rng, prompt)
    init = loop.snapshot()
    for _ in range(REPLAYS):
        loop.step()
    torch.cuda.synchronize()
    eager = loop.snapshot()
    assert (eager["total"] >= REPLAYS).all() and eager["cached"].tolist() == [PROMPT + t for t in eager["total"].tolist()]
    loop.restore(init)
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            loop.step()
    loop.restore(init)   # (capturing runs nothing; the state is the initial one either way)
    for _ in range(REPLAYS):
        graph.replay()
    torch.cuda.synchronize()
    got = loop.snapshot()
    for n in ("last", "cached", "steps", "seq", "fin", "tok", "cnt", "acc", "total", "d_step"):
        assert torch.equal(got[n], eager[n]), n
    target.dec.close()
    drafter.dec.close()
