"""References of tests/test_sink_engine_gpu.py: an engine with head sinks (llmie_decoder_set_head_sinks), per-layer windows and a
scaled RoPE table (llmie_decoder_set_rope_scaling).  Plain module, no fixtures.

layer_restatement: window_attn_cases.window_layer_restatement (float64 numpy) with the rotation taken from a (cos, sin) TABLE -- the
one llmie_rope_table_fill computed, as the device reads it -- and one sink column per (layer, query head) in every softmax.
moe_decode: moe_engine_ref.decode (the oracle's per-kernel composition around the experts) with the same two changes to its
attention, for the gpt-oss layer: MXFP4 experts, a window, head sinks and YaRN on one engine.
"""
import numpy as np

import model_param_cases as mpc
import window_attn_cases as wc

GPT_OSS_YARN = dict(kind="yarn", factor=32.0, original_max_pos=4096, beta_fast=32.0, beta_slow=1.0, truncate=0)
GPT_OSS_BASE = 150000.0


def rope_rows(x, tab, pos):
    """x [T, heads, hs] rotated at the positions pos [T] by the table [max_pos, hs/2, 2]: rotate-half pairs (d, d + hs/2)"""
    half = x.shape[-1] // 2
    c, s = tab[pos][:, None, :, 0].astype(np.float64), tab[pos][:, None, :, 1].astype(np.float64)
    a, b = x[..., :half], x[..., half:]
    return np.concatenate([a * c - b * s, b * c + a * s], axis=-1)


def sink_softmax(sc, sink):
    """sc [heads, q, t] masked logits (-inf = masked), sink [heads] -> probabilities of the real keys under the sink column"""
    s = np.asarray(sink, np.float64)[:, None, None]
    m = np.maximum(sc.max(axis=2, keepdims=True), s)
    p = np.exp(sc - m)
    return p / (p.sum(axis=2, keepdims=True) + np.exp(s - m) + 1e-6)


def layer_restatement(cfg, layers, x, k_cache, v_cache, lens, hist, layer_window, sinks, head_sinks, tab, store=None, stored=None):
    """float64 numpy; caches [L, bs, kvh, max_seq, hs] updated in place.  head_sinks: [L, head_num] (None: no sink column);
    tab: the (cos, sin) table; layer_window / sinks / store / stored as in window_attn_cases.window_layer_restatement"""
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
        q, k, v = rope_rows(qkv[:, :nh], tab, pos), rope_rows(qkv[:, nh:nh + kvh], tab, pos), qkv[:, nh + kvh:]
        att = np.empty((T, nh, hs))
        sink = np.full(nh, -np.inf) if head_sinks is None else np.asarray(head_sinks[l], np.float64)
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
            vis = wc.prefill_visible(h0 + np.arange(lens[b]), ctx, layer_window[l], sinks)
            att[s0:s1] = np.einsum("hqt,htd->qhd", sink_softmax(np.where(vis[None], sc, -np.inf), sink), V)
        resid = resid + att.reshape(T, H) @ f(w["o"]).T
        hn2 = mpc._norm(resid, f(w["ffn_norm"]), eps, "ffn", l, frozenset())
        gu = hn2 @ f(w["gate_up"]).T
        g, u = gu[:, :inter], gu[:, inter:]
        h = resid + ((g * 0.5 * (1.0 + np.tanh(0.5 * g))) * u) @ f(w["down"]).T
    return h


def moe_decode(b, rounded, head_sinks, tab, layer_window, sinks):
    """moe_engine_ref.decode for a native (fp16) cache with the experts of moe_mxfp4_engine_ref, the rotation by `tab`, the window
    layer_window[l] on layer l and the sink column head_sinks[l] in every softmax -> (hidden_out [rows, H] fp32, [logits per sparse
    layer])"""
    import moe_engine_ref as er
    import moe_mxfp4_engine_ref as xr
    import oracle as orc
    case = b["case"]
    assert case["kind"] == "decode" and case["cache"] != "e4m3"
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
            q, k, v = r(rope_rows(qkv[:, :nh], tab, pos), rounded), r(rope_rows(qkv[:, nh:nh + kvh], tab, pos), rounded), qkv[:, nh + kvh:]
            vis = er._visible(step, layer_window[l], sinks)
            att = np.empty((n, nh, hs))
            for i, row in enumerate(idx):
                K = np.concatenate([kf[l][row][:, vis], k[i][:, None]], axis=1).astype(np.float64)[np.arange(nh) // (nh // kvh)]
                V = np.concatenate([vf[l][row][:, vis], v[i][:, None]], axis=1).astype(np.float64)[np.arange(nh) // (nh // kvh)]
                sc = np.einsum("hd,htd->ht", q[i].astype(np.float64), K)[:, None, :] / np.sqrt(hs)
                att[i] = np.einsum("hqt,htd->qhd", sink_softmax(sc, head_sinks[l]), V)[0]
            att = r(att.reshape(n, er.H).astype(np.float32), rounded)
            o = r(orc.linear(att, lw["o"]), rounded)
            hn2, resid2 = orc.fused_add_bias_residual_rmsnorm(resid, o, None, lw["ffn_norm"], er.EPS)
            h = xr._ffn(r(hn2, rounded), r(resid2, rounded), lw, sparse, case, rounded, logits)
        out[idx] = h
        for dst, src in zip(logit_rows, logits):
            dst[idx] = src
    return out, logit_rows
