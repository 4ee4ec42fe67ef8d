"""llmie_score_tokens on the GPU against numpy float64 on the same fp16 inputs.  The normalised rows of the reference are what
llmie.rmsnorm leaves on a copy of the hidden states, so the comparison isolates the new kernels (and pins that the call normalises
to those very bits).

Bound: |got - ref| <= 2e-5 * max(1, |ref|) for the log-probability, the log-sum-exp and the arg-max log-probability.  fp32-accumulated
logits reduced in fp32 are within 1.0e-6 of float64 on these shapes (measured with numpy on the CPU), so the bound leaves 20x; logits
rounded to fp16 first -- the rmsnorm + linear + log_softmax composition -- are off by 1.3e-4 .. 7e-4 and miss it 6x, which
test_parity asserts on the (130, 512, 1003) case."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2e-5
EPS = 1e-5
# (rows, H, V): one row / one partial tile; several rows; two row tiles; three row tiles x 17 spans of two column tiles with a
# ragged last tile; and three row tiles x 22 spans of three column tiles (more than one span and more than one row tile)
SHAPES = [(1, 256, 129), (17, 256, 1003), (130, 512, 1003), (300, 256, 4099), (260, 512, 8200)]


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def _inputs(rows, H, V, seed=0, x_scale=1.0):
    rng = np.random.default_rng([seed, rows, H, V])
    x = (rng.standard_normal((rows, H)) * x_scale).astype(np.float16)
    w = (rng.standard_normal((V, H)) * (1.2 / np.sqrt(H))).astype(np.float16)
    gamma = (1.0 + 0.1 * rng.uniform(-1, 1, H)).astype(np.float16)
    bias = (0.5 * rng.standard_normal(V)).astype(np.float16)
    targets = rng.integers(0, V, rows).astype(np.int32)
    forced = [0, 127, 128, V - 1, -1, V]   # tile edges, the last column, and both kinds of "no target"
    targets[:min(rows, len(forced))] = forced[:rows]
    return x, w, gamma, bias, targets


def _reference(xn, w, bias, targets):
    """float64 on the fp16 values: (logprob, lse, argmax, argmax logprob, top-two gap)"""
    z = xn.astype(np.float64) @ w.astype(np.float64).T
    if bias is not None:
        z = z + bias.astype(np.float64)
    mx = z.max(axis=1)
    lse = mx + np.log(np.exp(z - mx[:, None]).sum(axis=1))
    V = z.shape[1]
    has = (targets >= 0) & (targets < V)
    lp = np.where(has, z[np.arange(len(z)), np.clip(targets, 0, V - 1)] - lse, 0.0)
    top2 = np.partition(z, V - 2, axis=1)[:, V - 2:]
    return lp, lse, z.argmax(axis=1), mx - lse, top2[:, 1] - top2[:, 0]


def _normalised(llmie, x_dev, gamma_dev):
    xn = x_dev.clone()
    llmie.rmsnorm(xn, None, gamma_dev, EPS)
    return xn


_CASES = {}


def _case(llmie, rows, H, V, use_gamma, use_bias):
    """device inputs, the call's outputs and the float64 reference of one parity case: computed once, shared, left unchanged"""
    key = (rows, H, V, use_gamma, use_bias)
    if key not in _CASES:
        x, w, gamma, bias, targets = _inputs(rows, H, V)
        d = dict(x=torch.from_numpy(x).to(DEV), w=torch.from_numpy(w).to(DEV), targets=torch.from_numpy(targets).to(DEV),
                 gamma=torch.from_numpy(gamma).to(DEV) if use_gamma else None, bias=torch.from_numpy(bias).to(DEV) if use_bias else None)
        d["xn"] = _normalised(llmie, d["x"], d["gamma"]) if use_gamma else d["x"]
        d["ref"] = _reference(d["xn"].cpu().numpy(), w, bias if use_bias else None, targets)
        got = llmie.score_tokens(d["x"], d["w"], d["targets"], gamma=d["gamma"], eps=EPS, bias=d["bias"], want_lse=True, want_argmax=True)
        torch.cuda.synchronize()
        d["got"] = tuple(t.cpu().numpy() for t in got)
        d["np"] = (x, w, gamma, bias, targets)
        _CASES[key] = d
    return _CASES[key]


@pytest.mark.parametrize("use_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("use_gamma", [False, True], ids=["nonorm", "norm"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity(llmie, shape, use_gamma, use_bias):
    rows, H, V = shape
    c = _case(llmie, rows, H, V, use_gamma, use_bias)
    lp, lse, amax, amax_lp = c["got"]
    r_lp, r_lse, _, r_amax_lp, _ = c["ref"]
    errs = dict(logprob=_rel(lp, r_lp), lse=_rel(lse, r_lse), argmax_logprob=_rel(amax_lp, r_amax_lp))
    print("score_tokens %s gamma=%s bias=%s: %s" % (shape, use_gamma, use_bias, errs))
    assert np.isfinite(lp).all() and np.isfinite(lse).all() and np.isfinite(amax_lp).all()
    assert max(errs.values()) <= BOUND, errs
    assert ((amax >= 0) & (amax < V)).all()
    if shape == (130, 512, 1003):
        # the accuracy claim: the composition that rounds the logits to fp16 first misses the same bound
        logits = torch.empty((rows, V), dtype=torch.float16, device=DEV)
        llmie.linear(c["xn"], c["w"], logits, bias=c["bias"])
        z = logits.cpu().numpy().astype(np.float64)
        mx = z.max(axis=1)
        c_lse = mx + np.log(np.exp(z - mx[:, None]).sum(axis=1))
        t = c["np"][4]
        has = (t >= 0) & (t < V)
        c_lp = np.where(has, z[np.arange(rows), np.clip(t, 0, V - 1)] - c_lse, 0.0)
        comp = _rel(c_lp, r_lp)
        print("fp16-logits composition: logprob error %.3g" % comp)
        assert comp > BOUND, comp


def test_large_logits_do_not_overflow(llmie):
    rows, H, V = 130, 512, 1003
    x, w, _, bias, targets = _inputs(rows, H, V, seed=1, x_scale=30.0)
    xd, wd = torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV)
    lp, lse, amax, amax_lp = (t.cpu().numpy() for t in llmie.score_tokens(xd, wd, torch.from_numpy(targets).to(DEV), want_lse=True,
                                                                          want_argmax=True))
    r_lp, r_lse, r_amax, r_amax_lp, gap = _reference(x, w, None, targets)
    assert np.abs(x.astype(np.float64) @ w.astype(np.float64).T).max() > 120   # exp() of these overflows fp32 without a running maximum
    for a in (lp, lse, amax_lp):
        assert np.isfinite(a).all()
    errs = dict(logprob=_rel(lp, r_lp), lse=_rel(lse, r_lse), argmax_logprob=_rel(amax_lp, r_amax_lp))
    print("large logits:", errs)
    assert max(errs.values()) <= BOUND, errs
    sure = gap >= 1e-3
    assert np.array_equal(amax[sure], r_amax[sure])


def test_argmax_matches_float64(llmie):
    total = clear = 0
    for rows, H, V in SHAPES:
        for use_gamma, use_bias in ((False, False), (True, True)):
            c = _case(llmie, rows, H, V, use_gamma, use_bias)
            sure = c["ref"][4] >= 1e-3   # rows whose float64 top two are further apart than fp32 accumulation can move them
            assert np.array_equal(c["got"][2][sure], c["ref"][2][sure]), (rows, H, V)
            total += rows
            clear += int(sure.sum())
    assert clear >= 0.98 * total, (clear, total)


@pytest.mark.parametrize("shape", [(130, 512, 1003), (260, 512, 8200)], ids=lambda s: "x".join(map(str, s)))
def test_argmax_tie_goes_to_the_lower_id(llmie, shape):
    """weight row 5 copied to rows 131 (the next column tile) and V - 3 (the last tile, another span): three bit-equal logits,
    pushed above all others by adding a multiple of that weight row to every x -- every row must answer 5"""
    rows, H, V = shape
    x, w, _, _, targets = _inputs(rows, H, V, seed=2)
    w[131] = w[5]
    w[V - 3] = w[5]
    w5 = w[5].astype(np.float64)
    x = (x.astype(np.float64) + (12.0 / np.dot(w5, w5)) * w5).astype(np.float16)   # + 12 on that logit; the others are N(0, 1.2^2)
    z = x.astype(np.float64) @ w.astype(np.float64).T
    assert (z.argmax(axis=1) == 5).all() and (z[:, 5] == z[:, 131]).all() and (z[:, 5] == z[:, V - 3]).all()
    _, amax, amax_lp = llmie.score_tokens(torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV), torch.from_numpy(targets).to(DEV),
                                          want_argmax=True)
    assert (amax.cpu().numpy() == 5).all(), amax.cpu().numpy()
    mx = z.max(axis=1)
    assert _rel(amax_lp.cpu().numpy(), -np.log(np.exp(z - mx[:, None]).sum(axis=1))) <= BOUND


def _raw_call(llmie, x, gamma, w, bias, targets, lp, lse, amax, amax_lp, rows, ws):
    def p(t):
        return None if t is None else t.data_ptr()
    rc = llmie.lib().llmie_score_tokens(p(x), p(gamma), EPS, p(w), p(bias), p(targets), p(lp), p(lse), p(amax), p(amax_lp), rows,
                                        x.shape[1], w.shape[0], p(ws), ws.numel(), llmie.F16, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, llmie.lib().llmie_last_error()


def test_no_target_rows_untouched_tail_and_hidden(llmie):
    rows, H, V = 130, 512, 1003
    c = _case(llmie, rows, H, V, True, True)
    lp = c["got"][0]
    t = c["np"][4]
    none = (t < 0) | (t >= V)
    assert none.sum() == 2
    assert (lp[none] == 0.0).all() and not np.signbit(lp[none]).any()
    assert (lp[~none] < 0).all()
    # over-allocated outputs: rows past `rows` keep their sentinel; the hidden states keep their bits
    extra, sent = 70, -12345.0
    x0 = c["x"].clone()
    o_lp, o_lse, o_alp = (torch.full((rows + extra,), sent, dtype=torch.float32, device=DEV) for _ in range(3))
    o_am = torch.full((rows + extra,), -777, dtype=torch.int32, device=DEV)
    ws = torch.empty(llmie.score_tokens_workspace_bytes(rows, H, V), dtype=torch.uint8, device=DEV)
    _raw_call(llmie, c["x"], c["gamma"], c["w"], c["bias"], c["targets"], o_lp, o_lse, o_am, o_alp, rows, ws)
    torch.cuda.synchronize()
    assert torch.equal(c["x"], x0)
    for o in (o_lp, o_lse, o_alp):
        assert (o[rows:] == sent).all()
    assert (o_am[rows:] == -777).all()
    assert np.array_equal(o_lp[:rows].cpu().numpy(), lp) and np.array_equal(o_am[:rows].cpu().numpy(), c["got"][2])
    # the optional outputs really are optional
    only = torch.full((rows,), sent, dtype=torch.float32, device=DEV)
    _raw_call(llmie, c["x"], c["gamma"], c["w"], c["bias"], c["targets"], only, None, None, None, rows, ws)
    assert np.array_equal(only.cpu().numpy(), lp)


def test_deterministic_and_independent_of_the_other_rows(llmie):
    rows, H, V = 130, 512, 1003
    c = _case(llmie, rows, H, V, True, True)

    def run(x, targets):
        out = llmie.score_tokens(x, c["w"], targets, gamma=c["gamma"], eps=EPS, bias=c["bias"], want_lse=True, want_argmax=True)
        return [o.cpu().numpy() for o in out]

    again = run(c["x"], c["targets"])
    for a, b in zip(again, c["got"]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    for t in (0, 3, 64, 127, 128, 129):
        alone = run(c["x"][t:t + 1].contiguous(), c["targets"][t:t + 1].contiguous())
        # as row 0 of a 17-row call whose other rows are other rows of the batch
        idx = torch.tensor([t] + [(t + 7 * k) % rows for k in range(1, 17)], device=DEV)
        first = run(c["x"][idx].contiguous(), c["targets"][idx].contiguous())
        for full, a, f in zip(c["got"], alone, first):
            assert full[t:t + 1].view(np.int32) == a[0:1].view(np.int32), t
            assert full[t:t + 1].view(np.int32) == f[0:1].view(np.int32), t


def test_first_call_under_graph_capture():
    """a fresh process captures its FIRST score_tokens call into a graph (nothing on the path may allocate or synchronise), replays it
    twice and compares with the eager call"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "score_capture.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["replay1_equal"] == [True] * 4 and out["replay2_equal"] == [True] * 4, out
    assert out["finite"] and out["logprob_min"] < 0, out


def test_through_the_engine(llmie):
    """one-layer fp16 decoder: a 20-token prefill, then the scores of its output rows against float64 on the same rows.  (The
    engine's prefill serves head_size 128 only, so the decoder is 8 heads of 128 rather than the 4 x 32 of the sampling tests'
    helper; V = 1003 and the 20 tokens are as there.)"""
    rng = np.random.default_rng(4)
    nh, hs, inter, V, n, max_seq = 8, 128, 512, 1003, 20, 384
    H = nh * hs

    def mk(shape, scale):
        return torch.from_numpy((rng.uniform(-1, 1, shape) * scale).astype(np.float16)).to(DEV)

    layers = [dict(attn_norm=mk((H,), 0.1) + 1, ffn_norm=mk((H,), 0.1) + 1, qkv=mk((3 * H, H), 0.05), o=mk((H, H), 0.05),
                   gate_up=mk((2 * inter, H), 0.05), down=mk((H, inter), 0.05))]
    cfg = dict(head_num=nh, kv_head_num=nh, head_size=hs, inter_size=inter, num_layers=1, vocab_size=V, max_seq_len=max_seq, max_batch=1,
               rotary_dim=hs, rotary_base=10000.0, rms_eps=EPS, dtype=llmie.F16, wfmt=llmie.W_F16, int4_group=128)
    dec = llmie.Decoder(cfg, layers)
    gamma, lm, embed = mk((H,), 0.1) + 1, mk((V, H), 0.1), mk((V, H), 1.0)
    ids = rng.integers(0, V, n).astype(np.int32)
    hidden = torch.empty((n, H), dtype=torch.float16, device=DEV)
    llmie.input_embedding(torch.from_numpy(ids).to(DEV), embed, hidden)
    out = torch.empty_like(hidden)
    kc = torch.zeros((1, 1, nh, max_seq, hs), dtype=torch.float16, device=DEV)
    vc = torch.zeros_like(kc)
    dec.prefill(hidden, out, kc, vc, torch.tensor([n], dtype=torch.int32, device=DEV), torch.tensor([0], dtype=torch.int32, device=DEV), n)
    targets = np.append(ids[1:], -1).astype(np.int32)
    lp, lse = llmie.score_tokens(out, lm, torch.from_numpy(targets).to(DEV), gamma=gamma, eps=EPS, want_lse=True)
    torch.cuda.synchronize()
    assert out.float().abs().max().item() > 0
    xn = _normalised(llmie, out, gamma).cpu().numpy()
    r_lp, r_lse, _, _, _ = _reference(xn, lm.cpu().numpy(), None, targets)
    dec.close()
    errs = dict(logprob=_rel(lp.cpu().numpy(), r_lp), lse=_rel(lse.cpu().numpy(), r_lse))
    print("engine:", errs)
    assert max(errs.values()) <= BOUND, errs
    assert lp[-1].item() == 0.0 and (lp[:-1] < 0).all()
