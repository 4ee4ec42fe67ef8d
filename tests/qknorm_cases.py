"""Inputs and float64 references of the QK-norm tests (llmie_qk_norm, llmie_decoder_mha_qknorm, llmie_decoder_set_qk_norm).  Plain
module, no fixtures: tests/test_qknorm_cpu.py checks what it claims on the CPU, the *_gpu.py files run the device against it.

head_norm is the operator as include/llmie.h states it, in float64 with the one fp16 rounding at the end.  op_inputs draws QKV rows
on which the mistakes a kernel can make show: a sum shared between the heads of a KV head, eps outside the root or missing, a sum of
squares kept in fp16.  gammas draws per-layer q and k gammas whose rotate-half partners differ, so that a norm placed behind RoPE
is a different function.  layer_restatement is sink_engine_cases.layer_restatement with head_norm on q and k in front of rope_rows
(full attention, no sink column), with the defects a test holds the engine against.
"""
import numpy as np

import model_param_cases as mpc
import sink_engine_cases as se

DEFECTS = ("none", "after_rope", "gammas_swapped", "k_raw", "v_too")
EPS = 1e-6
# Gamma ranges of the engine cases.  An engine that prefills attends to the K / V rows it projected itself and every defect moves its
# hidden output by 0.18 .. 0.34 (relative Frobenius) at [0.5, 2].  A decode-only case attends to DRAWN caches (uniform +-0.5): at
# [0.5, 2] its logits have a standard deviation of 0.3, the softmax is nearly uniform over 150 keys and a wrongly normalised q
# moves the first step's output by 0.013 .. 0.033 only -- below 10 x the engine bound of 3e-3.  At [0.5, 8] the logits have a
# standard deviation of about 1, the choice of keys matters, and the least visible defect moves it by 0.15
# (tests/test_qknorm_cpu.py asserts both on the CPU).
GAMMA_RANGE = {"prefill": (0.5, 2.0), "decode_only": (0.5, 8.0)}


def head_norm(x, g, eps, rounded=True):
    """x [..., hs] normalised over the last axis with the gamma g [hs]: float64, then one fp16 rounding (returned as float64)"""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    inv = 1.0 / np.sqrt((x * x).sum(axis=-1, keepdims=True) / x.shape[-1] + eps)
    n = (x * inv) * g
    return n.astype(np.float16).astype(np.float64) if rounded else n


def tiny_heads(nh, kvh):
    """the q head and the k head (column head indices) of op_inputs whose mean square is about eps"""
    return nh - 1, nh + kvh - 1


def op_inputs(rows, nh, kvh, hs, seed):
    """fp16 QKV rows [rows, nh + 2 kvh, hs]: head h is N(0, 1) scaled by 2^((h % 5) - 2); the last q head and the last k head are
    ~1e-3 N(0, 1) (mean square about eps = 1e-6); q head 0 is uniform in +-300 (squares above the fp16 range)"""
    rng = np.random.default_rng(seed)
    heads = nh + 2 * kvh
    x = rng.standard_normal((rows, heads, hs)) * (2.0 ** ((np.arange(heads) % 5) - 2))[None, :, None]
    tq, tk = tiny_heads(nh, kvh)
    x[:, tq] = 1e-3 * rng.standard_normal((rows, hs))
    x[:, tk] = 1e-3 * rng.standard_normal((rows, hs))
    x[:, 0] = rng.uniform(-300.0, 300.0, (rows, hs))
    return x.astype(np.float16)


def gammas(layers, hs, seed, lo=0.5, hi=2.0):
    """(q_gamma, k_gamma), fp16 [layers, hs] each: log-uniform in [lo, hi] per dimension, q and k and every layer drawn apart, and
    g[d] != g[d + hs/2] for every d (as fp16 values)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        g = np.exp(rng.uniform(np.log(lo), np.log(hi), (layers, hs))).astype(np.float16)
        while True:
            same = g[:, :hs // 2] == g[:, hs // 2:]
            if not same.any():
                break
            g[:, :hs // 2][same] = np.exp(rng.uniform(np.log(lo), np.log(hi), int(same.sum()))).astype(np.float16)
        out.append(g)
    return out[0], out[1]


def normed_qkv(qkv, nh, kvh, qg, kg, eps):
    """llmie_qk_norm on fp16 rows [rows, nh + 2 kvh, hs]: the expected rows as float64 (v columns as they are)"""
    out = np.asarray(qkv, np.float64).copy()
    out[:, :nh] = head_norm(out[:, :nh], qg, eps)
    out[:, nh:nh + kvh] = head_norm(out[:, nh:nh + kvh], kg, eps)
    return out


def qk_of(qkv, nh, kvh, tab, pos, qg, kg, eps, defect="none", rounded=True):
    """q, k, v [T, heads, hs] float64 of packed rows qkv [T, nh + 2 kvh, hs]: head_norm on q and k, then the rotation by the table at
    the positions pos -- or one of the DEFECTS.  qg None: no norm at all"""
    assert defect in DEFECTS
    q, k, v = qkv[:, :nh], qkv[:, nh:nh + kvh], qkv[:, nh + kvh:]
    if qg is None:
        return se.rope_rows(q, tab, pos), se.rope_rows(k, tab, pos), v
    if defect == "gammas_swapped":
        qg, kg = kg, qg
    hn = lambda x, g: head_norm(x, g, eps, rounded)
    if defect == "after_rope":
        return hn(se.rope_rows(q, tab, pos), qg), hn(se.rope_rows(k, tab, pos), kg), v
    return (se.rope_rows(hn(q, qg), tab, pos), se.rope_rows(k if defect == "k_raw" else hn(k, kg), tab, pos),
            hn(v, kg) if defect == "v_too" else v)


def layer_restatement(cfg, layers, x, k_cache, v_cache, lens, hist, tab, q_gamma, k_gamma, qk_eps=EPS, defect="none", store=None, stored=None):
    """float64 numpy; caches [L, bs, kvh, max_seq, hs] updated in place.  q_gamma / k_gamma: [L, hs] (None: an engine without
    QK-norm); tab: the (cos, sin) table; store / stored as in sink_engine_cases.layer_restatement"""
    nh, kvh, hs, inter, eps = cfg["head_num"], cfg["kv_head_num"], cfg["head_size"], cfg["inter_size"], cfg["rms_eps"]
    rep, H, T = nh // kvh, nh * hs, int(sum(lens))
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    pos = np.concatenate([hist[b] + np.arange(lens[b]) for b in range(len(lens))])
    h = np.asarray(x, np.float64).copy()
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    store = store or (lambda rows, which: rows)
    for l, w in enumerate(layers):
        resid = h
        hn = mpc._norm(h, f(w["attn_norm"]), eps, "attn", l, frozenset())
        qkv = (hn @ f(w["qkv"]).T).reshape(T, nh + 2 * kvh, hs)
        q, k, v = qk_of(qkv, nh, kvh, tab, pos, None if q_gamma is None else q_gamma[l], None if k_gamma is None else k_gamma[l], qk_eps, defect)
        att = np.empty((T, nh, hs))
        for b in range(len(lens)):
            s0, s1, h0 = starts[b], starts[b + 1], hist[b]
            k_cache[l, b, :, h0:h0 + lens[b]] = store(k[s0:s1].transpose(1, 0, 2), 0)
            v_cache[l, b, :, h0:h0 + lens[b]] = store(v[s0:s1].transpose(1, 0, 2), 1)
            if stored is not None:
                for cache, dev in ((k_cache, stored[0]), (v_cache, stored[1])):
                    mine, theirs = cache[l, b, :, h0:h0 + lens[b]], np.asarray(dev[l, b, :, h0:h0 + lens[b]], np.float64)
                    tol = 0.126 * np.abs(theirs) + 2.0 ** -6 * np.abs(theirs).max(axis=-1, keepdims=True)
                    assert (np.abs(mine - theirs) <= tol).all(), "layer %d sequence %d: stored rows off by %.3g" % (l, b, (np.abs(mine - theirs) - tol).max())
                    cache[l, b, :, h0:h0 + lens[b]] = theirs
            ctx = h0 + lens[b]
            K, V = k_cache[l, b, np.arange(nh) // rep, :ctx], v_cache[l, b, np.arange(nh) // rep, :ctx]
            sc = np.einsum("qhd,htd->hqt", q[s0:s1], K) / np.sqrt(hs)
            vis = np.arange(ctx)[None, :] <= (h0 + np.arange(lens[b]))[:, None]
            att[s0:s1] = np.einsum("hqt,htd->qhd", se.sink_softmax(np.where(vis[None], sc, -np.inf), np.full(nh, -np.inf)), V)
        resid = resid + att.reshape(T, H) @ f(w["o"]).T
        hn2 = mpc._norm(resid, f(w["ffn_norm"]), eps, "ffn", l, frozenset())
        gu = hn2 @ f(w["gate_up"]).T
        g, u = gu[:, :inter], gu[:, inter:]
        h = resid + ((g * 0.5 * (1.0 + np.tanh(0.5 * g))) * u) @ f(w["down"]).T
    return h


def moe_decode(b, rounded, q_gamma, k_gamma, qk_eps, flags, tab):
    """moe_engine_ref.decode for a native (fp16) cache with head_norm on q and k in front of the rotation (q_gamma None: without it)
    and the router flags `flags` (moe_cases.SOFTMAX_ALL) -> (hidden_out [rows, H] fp32, [logits per sparse layer])"""
    import moe_cases as mc
    import moe_engine_ref as er
    import oracle as orc
    case = b["case"]
    assert case["kind"] == "decode" and case["cache"] != "e4m3" and not case["window"]
    hs = case["hs"]
    nh, kvh = er.geometry(hs)
    kf, vf = er._float_caches(b)
    ctx = np.array(er.contexts(case))
    out = np.zeros((case["rows"], er.H), np.float32)
    logit_rows = [np.zeros((case["rows"], case["E"])) for s in case["sparse"] if s]
    r = er._r
    for step in np.unique(ctx):
        idx = np.nonzero(ctx == step)[0]
        n, step = len(idx), int(step)
        h = b["x"][idx].astype(np.float32)
        logits = []
        for l, (lw, sparse) in enumerate(zip(b["weights"], case["sparse"])):
            hn, resid = orc.rmsnorm(h, lw["attn_norm"], er.EPS)
            qkv = r(orc.linear(r(hn, rounded), lw["qkv"]), rounded).reshape(n, nh + 2 * kvh, hs).astype(np.float64)
            pos = np.full(n, step - 1)
            q, k, v = qk_of(qkv, nh, kvh, tab, pos, None if q_gamma is None else q_gamma[l], None if k_gamma is None else k_gamma[l], qk_eps,
                            rounded=rounded)
            q, k = r(q, rounded), r(k, rounded)
            att = np.empty((n, nh, hs))
            for i, row in enumerate(idx):
                K = np.concatenate([kf[l][row][:, :step - 1], k[i][:, None]], axis=1).astype(np.float64)[np.arange(nh) // (nh // kvh)]
                V = np.concatenate([vf[l][row][:, :step - 1], v[i][:, None]], axis=1).astype(np.float64)[np.arange(nh) // (nh // kvh)]
                sc = np.einsum("hd,htd->ht", q[i].astype(np.float64), K)[:, None, :] / np.sqrt(hs)
                att[i] = np.einsum("hqt,htd->qhd", se.sink_softmax(sc, np.full(nh, -np.inf)), V)[0]
            att = r(att.reshape(n, er.H).astype(np.float32), rounded)
            o = r(orc.linear(att, lw["o"]), rounded)
            hn2, resid2 = orc.fused_add_bias_residual_rmsnorm(resid, o, None, lw["ffn_norm"], er.EPS)
            hn2, resid2 = r(hn2, rounded), r(resid2, rounded)
            if sparse:
                bb = dict(x=hn2, router=lw["router"], gate_up=lw["e_gate_up"], down=lw["e_down"], resid=resid2)
                ids, wts, rr = mc.route(hn2, lw["router"], case["k"], flags=flags)
                logits.append(rr)
                h = mc.ffn(bb, ids, wts, rounded).astype(np.float32)
            else:
                h = er._ffn(hn2, resid2, lw, False, case, rounded, logits)
        out[idx] = h
        for dst, src in zip(logit_rows, logits):
            dst[idx] = src
    return out, logit_rows
