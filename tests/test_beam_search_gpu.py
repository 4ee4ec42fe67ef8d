"""Beam search end to end on the paged engine: prefill once per request, then 14 steps of forward_paged_ragged -> LM head ->
beam_step -> kv_pages_fork -> embedding of the chosen tokens, across the page boundary at 128 tokens.  Afterwards every row is
replayed teacher-forced -- the same engine and batch, private pages, no fork, each row fed the tokens of the hypothesis that ended
up in it -- and must match bit for bit: the caches over the cached length and the last step's logits (rows are independent in
every decode path).  Every cumulative log-probability equals the float64 sum of the replay's per-step log-softmax values."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16
NH, KVH, HS, INTER, LAYERS, V = 8, 8, 128, 512, 2, 1000
G, W, PROMPT, STEPS, END_ID = 2, 4, 120, 14, 2
ROWS, H, MAX_SEQ, MAX_PAGES = G * W, NH * HS, 256, 2


def _engine(llmie, rng, kv8):
    QKV = (NH + 2 * KVH) * HS
    u = lambda shape, s: torch.from_numpy((rng.uniform(-1, 1, shape) * s).astype(np.float32)).to(DEV).to(F16)
    layers = [dict(attn_norm=u((H,), 0.2) + 1, qkv=dict(data=u((QKV, H), 2 / np.sqrt(H))), o=dict(data=u((H, H), 2 / np.sqrt(H))),
                   ffn_norm=u((H,), 0.2) + 1, gate_up=dict(data=u((2 * INTER, H), 2 / np.sqrt(H))),
                   down=dict(data=u((H, INTER), 2 / np.sqrt(INTER)))) for _ in range(LAYERS)]
    cfg = dict(head_num=NH, kv_head_num=KVH, head_size=HS, inter_size=INTER, num_layers=LAYERS, vocab_size=V, max_seq_len=MAX_SEQ,
               max_batch=ROWS, rotary_dim=HS, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=llmie.W_F16, int4_group=128,
               kv_fmt=llmie.KV_FP8 if kv8 else llmie.KV_NATIVE, k_scale=1 / 32, v_scale=1 / 16)
    return llmie.Decoder(cfg, layers), u((V, H), 1.0), u((V, H), 2 / np.sqrt(H))


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _to_dense(llmie, kp, vp, table, lens):
    kd = torch.zeros((LAYERS, ROWS, KVH, MAX_SEQ, HS), dtype=kp.dtype, device=DEV)
    vd = torch.zeros_like(kd)
    llmie.kv_pages_copy(kd, kp, table, lens, False)
    llmie.kv_pages_copy(vd, vp, table, lens, False)
    return kd, vd


@pytest.mark.parametrize("kv8", [False, True])
def test_beam_search_equals_its_teacher_forced_replay(llmie, kv8):
    rng = np.random.default_rng(2024)
    dec, embed, lm_head = _engine(llmie, rng, kv8)
    cdt = torch.uint8 if kv8 else F16
    num_pages = ROWS * MAX_PAGES + 3
    prompt = _i32(rng.integers(3, V, G * PROMPT))

    def pools():
        return torch.zeros((LAYERS, num_pages, KVH, 128, HS), dtype=cdt, device=DEV), torch.zeros((LAYERS, num_pages, KVH, 128, HS), dtype=cdt, device=DEV)

    def prefill(kp, vp, table):
        """the G prompts into the pages of rows 0, W, ...; -> the last prompt token's hidden state, once per beam row"""
        x = torch.empty((G * PROMPT, H), dtype=F16, device=DEV)
        llmie.input_embedding(prompt, embed, x)
        out = dec.prefill_paged(x, torch.empty_like(x), kp, vp, table[::W].contiguous(), _i32([PROMPT] * G), _i32([0] * G), PROMPT)
        return out[PROMPT - 1::PROMPT].repeat_interleave(W, dim=0).contiguous()

    def lm(hidden):
        return llmie.linear(hidden, lm_head, torch.empty((ROWS, V), dtype=F16, device=DEV))

    def decode(tokens, kp, vp, table, lens):
        """one step on all rows: embeds `tokens`, appends their K / V (lens += 1); -> hidden"""
        x = torch.empty((ROWS, H), dtype=F16, device=DEV)
        llmie.input_embedding(tokens.reshape(-1).contiguous(), embed, x)
        lens += 1
        return dec.forward_paged_ragged(x, torch.empty_like(x), kp, vp, table, lens)

    # ---- beam search
    kp, vp = pools()
    own = torch.from_numpy(rng.permutation(num_pages)[:ROWS * MAX_PAGES].astype(np.int32)).reshape(ROWS, MAX_PAGES).to(DEV)
    table = own.clone()
    lens = _i32([PROMPT if j % W == 0 else 0 for j in range(ROWS)])
    hidden = prefill(kp, vp, table)
    state = llmie.beam_state(G, W, DEV)
    hist = [[] for _ in range(ROWS)]
    crossed = False
    for s in range(STEPS):
        parent, token = llmie.beam_step(lm(hidden), state, END_ID)
        llmie.kv_pages_fork(kp, vp, table, own, parent.reshape(-1), lens)
        p, t = parent.reshape(-1).tolist(), token.reshape(-1).tolist()
        assert all(p[j] // W == j // W for j in range(ROWS))
        crossed |= s >= 1 and any(p[j] != j for j in range(ROWS))
        hist = [hist[p[j]] + [t[j]] for j in range(ROWS)]
        hidden = decode(token, kp, vp, table, lens)
    assert crossed, "no row ever continued another row's hypothesis: pick another seed"
    assert lens.tolist() == [PROMPT + STEPS] * ROWS and PROMPT + STEPS > 128
    last_logits = lm(hidden)
    kd, vd = _to_dense(llmie, kp, vp, table, lens)

    # ---- replay: private pages, the same prefill call, no fork
    kp2, vp2 = pools()
    table2 = torch.from_numpy(rng.permutation(num_pages)[:ROWS * MAX_PAGES].astype(np.int32)).reshape(ROWS, MAX_PAGES).to(DEV)
    hidden2 = prefill(kp2, vp2, table2)
    lens2 = _i32([PROMPT if j % W == 0 else 0 for j in range(ROWS)])
    k0, v0 = _to_dense(llmie, kp2, vp2, table2, lens2)
    for j in range(ROWS):   # every row gets a private copy of its request's prompt cache
        k0[:, j], v0[:, j] = k0[:, j - j % W].clone(), v0[:, j - j % W].clone()
    lens2 = _i32([PROMPT] * ROWS)
    llmie.kv_pages_copy(k0, kp2, table2, lens2, True)
    llmie.kv_pages_copy(v0, vp2, table2, lens2, True)
    logprob = np.zeros(ROWS)
    for s in range(STEPS):
        lsm = torch.log_softmax(lm(hidden2).double(), dim=-1).cpu().numpy()
        for j in range(ROWS):
            if END_ID not in hist[j][:s]:
                logprob[j] += lsm[j, hist[j][s]]
        hidden2 = decode(_i32([hist[j][s] for j in range(ROWS)]), kp2, vp2, table2, lens2)
    kd2, vd2 = _to_dense(llmie, kp2, vp2, table2, lens2)
    n = PROMPT + STEPS
    assert torch.equal(kd[:, :, :, :n], kd2[:, :, :, :n]) and torch.equal(vd[:, :, :, :n], vd2[:, :, :, :n])
    assert torch.equal(last_logits, lm(hidden2))
    if not kv8:
        cum = state.cum.reshape(-1).cpu().numpy().astype(np.float64)
        print("max |cum - replay| = %.3g" % np.abs(cum - logprob).max())
        assert np.isfinite(cum).all() and (np.abs(cum - logprob) <= 1e-4 * STEPS).all(), (cum, logprob)
        assert state.gen_len.reshape(-1).tolist() == [hist[j].index(END_ID) + 1 if END_ID in hist[j] else STEPS for j in range(ROWS)]
    dec.close()
