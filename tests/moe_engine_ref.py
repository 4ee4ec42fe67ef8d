"""The engine cases of the mixture-of-experts tests and their reference (numpy + the oracle only; read by test_moe_cpu.py, which asserts
what the cases claim, by moe_engine_cases.py / test_moe_engine_gpu.py, which run them on the device, and by moe_capture.py).

Reference: one layer after the other from the oracle's per-kernel functions (rmsnorm, linear, rope_decode, decoder_mha,
qkv_bias_transpose_rope, concat_kv / repeat_kv, scale_mask_softmax, batched_gemm, fused_add_bias_residual_rmsnorm, silu_and_mul,
add_residual -- the order of oracle.self_decoder / oracle.context_decoder), with moe_cases.route + moe_cases.ffn as the FFN of a
sparse layer.  Two evaluations: `rounded=False`, the oracle's fp32 kernels and the float64 expert FFN as they are; `rounded=True`,
every activation that an engine keeps in an fp16 buffer between two kernels rounded to fp16 and the expert
FFN with its own two roundings.  The device is compared with the rounded evaluation.

Routing stability: a row is compared only if, at every sparse layer, both evaluations select the same expert set and the gap
between its k-th and (k + 1)-th logit (unrounded evaluation) is at least 8 times the largest logit difference between the two
evaluations at that layer in that case.  At most 10 % of a case's rows may be unstable; router gain and seeds are chosen so that
this holds, and test_moe_cpu.py asserts it for every case, from these functions alone.

Geometry: hidden 256, expert inter 192, dense inter 320, head_size 64 (4 / 2 heads, decode entries) or 128 (2 / 1 heads:
llmie_decoder_prefill takes head_size 128 only)."""
import zlib

import numpy as np

import moe_cases as mc
import oracle as orc
from exact_linear_cases import E4M3

H, IE, INTER, MAX_SEQ, MAX_BATCH = 256, 192, 320, 384, 32
ROUTER_GAIN = 8.0
EPS, ROPE_BASE = 1e-5, 10000.0
K_SCALE, V_SCALE = 1 / 32, 1 / 16


def geometry(hs):
    return (4, 2) if hs == 64 else (2, 1)


def layer_weights(hs, layers, E, seed, inter=INTER):
    """per layer: the dense matrices (fp16 numpy) and the experts' (router, gate_up, down)"""
    rng = np.random.default_rng(seed)
    nh, kvh = geometry(hs)
    u = lambda shape, s: (rng.uniform(-1, 1, shape) * s).astype(np.float16)
    out = []
    for _ in range(layers):
        out.append(dict(attn_norm=u((H,), 0.2) + np.float16(1), ffn_norm=u((H,), 0.2) + np.float16(1),
                        qkv=u(((nh + 2 * kvh) * hs, H), 2 / np.sqrt(H)), o=u((H, H), 2 / np.sqrt(H)),
                        gate_up=u((2 * inter, H), 2 / np.sqrt(H)), down=u((H, inter), 2 / np.sqrt(inter)),
                        router=(ROUTER_GAIN * rng.standard_normal((E, H)) / np.sqrt(H)).astype(np.float16),
                        e_gate_up=u((E, 2 * IE, H), 2 / np.sqrt(H)), e_down=u((E, H, IE), 2 / np.sqrt(IE))))
    return out


def _c(id, kind, cache, E, k, sparse, hs, seed, rows=None, lens=None, hist=None, step=131, window=0, sinks=0):
    return dict(id=id, kind=kind, cache=cache, E=E, k=k, sparse=sparse, hs=hs, seed=seed, rows=rows, lens=lens, hist=hist, step=step,
                window=window, sinks=sinks)


# decode: 32 rows take the grouped route, 3 rows the GEMV route; prefill: a dense layer in front of the sparse one
CASES = []
for E, k in ((8, 2), (4, 1)):
    for cache in ("dense", "paged", "ragged", "e4m3"):
        for rows in (32, 3):
            CASES.append(_c("decode_%s_e%d_r%d" % (cache, E, rows), "decode", cache, E, k, (True, True), 64, seed=100 + E + rows, rows=rows))
    for cache in ("dense", "paged"):
        for lens, hist in (((5,), (0,)), ((33,), (17,)), ((130,), (140,)), ((5, 33, 130), (0, 17, 140))):
            CASES.append(_c("prefill_%s_e%d_t%d" % (cache, E, sum(lens)), "prefill", cache, E, k, (False, True), 128, seed=200 + E + sum(lens), lens=lens,
                            hist=hist if cache == "paged" else tuple(0 for _ in lens)))
CASES.append(_c("decode_stack_e8", "decode", "dense", 8, 2, (True, False, True), 64, seed=301, rows=32))
CASES.append(_c("decode_window_e8", "decode", "ragged", 8, 2, (True, True), 64, seed=302, rows=24, step=200, window=64, sinks=4))
BY_ID = {c["id"]: c for c in CASES}
# inputs redrawn until the reference alone meets the stability cap (a 3-row case has room for no unstable row)
SALT = {"decode_paged_e8_r3": "/1"}


def n_rows(case):
    return case["rows"] if case["kind"] == "decode" else sum(case["lens"])


def contexts(case):
    """decode: the context length of every row including this step's token"""
    return [case["step"] - (b % 5) * 7 if case["cache"] == "ragged" else case["step"] for b in range(case["rows"])]


def build(case):
    """weights, hidden rows (fp16) and caches of a case: k / v [L, bs, kvh, MAX_SEQ, hs] fp16, or e4m3 bytes"""
    rng = np.random.default_rng(zlib.crc32((case["id"] + SALT.get(case["id"], "")).encode()))
    L, hs = len(case["sparse"]), case["hs"]
    nh, kvh = geometry(hs)
    bs = case["rows"] if case["kind"] == "decode" else len(case["lens"])
    w = layer_weights(hs, L, case["E"], case["seed"])
    x = rng.standard_normal((n_rows(case), H)).astype(np.float16)
    shape = (L, bs, kvh, MAX_SEQ, hs)
    if case["cache"] == "e4m3":
        kc, vc = rng.integers(0, 0x58, shape).astype(np.uint8), rng.integers(0, 0x58, shape).astype(np.uint8)
    else:
        kc, vc = (0.5 * rng.standard_normal(shape)).astype(np.float16), (0.5 * rng.standard_normal(shape)).astype(np.float16)
    return dict(case=case, weights=w, x=x, k=kc, v=vc)


def _r(a, rounded):
    return a.astype(np.float16).astype(np.float32) if rounded else a


def _ffn(hn2, resid2, lw, sparse, case, rounded, logits):
    if sparse:
        b = dict(x=hn2, router=lw["router"], gate_up=lw["e_gate_up"], down=lw["e_down"], resid=resid2)
        ids, wts, r = mc.route(hn2, lw["router"], case["k"])
        logits.append(r)
        return mc.ffn(b, ids, wts, rounded).astype(np.float32)
    n = hn2.shape[0]
    act = _r(orc.silu_and_mul(orc.linear(hn2, lw["gate_up"]).reshape(n, 2, -1)), rounded)
    return _r(orc.add_residual(resid2, orc.linear(act, lw["down"])), rounded)


def _float_caches(b):
    if b["case"]["cache"] == "e4m3":
        return (E4M3[b["k"]] * K_SCALE).astype(np.float32), (E4M3[b["v"]] * V_SCALE).astype(np.float32)
    return b["k"].astype(np.float32), b["v"].astype(np.float32)


def _e4m3_round(x, scale):
    """e4m3(x / scale) * scale: what an e4m3 cache holds of a new row (round to nearest, ties to the even code, saturating at 448)"""
    pos = E4M3[:127]
    a = np.minimum(np.abs(x.astype(np.float64) / scale), 448.0)
    idx = np.clip(np.searchsorted(pos, a), 1, 126)
    lo, hi = pos[idx - 1], pos[idx]
    up = (a - lo > hi - a) | ((a - lo == hi - a) & (idx % 2 == 0))
    return (np.sign(x) * np.where(up, hi, lo) * scale).astype(np.float32)


def _visible(ctx, window, sinks):
    """cached positions a decode query at position ctx - 1 sees"""
    j = np.arange(ctx - 1)
    return j if window <= 0 else j[(ctx - 1 - j < window) | (j < sinks)]


def decode(b, rounded):
    """(hidden_out [rows, H] fp32, [logits per sparse layer])"""
    case = b["case"]
    hs = case["hs"]
    nh, kvh = geometry(hs)
    kf, vf = _float_caches(b)
    ctx = np.array(contexts(case))
    out = np.zeros((case["rows"], H), np.float32)
    L = len(case["sparse"])
    logit_rows = [np.zeros((case["rows"], case["E"])) for s in case["sparse"] if s]
    for step in np.unique(ctx):
        idx = np.nonzero(ctx == step)[0]
        h = b["x"][idx].astype(np.float32)
        logits = []
        for l, (lw, sparse) in enumerate(zip(b["weights"], case["sparse"])):
            hn, resid = orc.rmsnorm(h, lw["attn_norm"], EPS)
            hn = _r(hn, rounded)
            qkv = _r(orc.linear(hn, lw["qkv"]), rounded)
            qkv = orc.rope_decode(qkv, nh, kvh, hs, int(step), hs, ROPE_BASE)
            if case["cache"] == "e4m3":   # the step's own k / v rows are attended to as the cache stores them
                ko, vo = nh * hs, (nh + kvh) * hs
                qkv[:, ko:vo], qkv[:, vo:] = _e4m3_round(qkv[:, ko:vo], K_SCALE), _e4m3_round(qkv[:, vo:], V_SCALE)
            # a window on the first layer: the visible cached keys (rotated when they were appended), packed to the front
            vis = _visible(int(step), case["window"] if l == 0 else 0, case["sinks"])
            kc = np.zeros((1, len(idx), kvh, MAX_SEQ, hs), np.float32)
            vc = np.zeros_like(kc)
            kc[0, :, :, :len(vis)], vc[0, :, :, :len(vis)] = kf[l][idx][:, :, vis], vf[l][idx][:, :, vis]
            att = _r(orc.decoder_mha(qkv, None, kc, vc, 0, nh, kvh, hs, len(vis) + 1), rounded)
            o = _r(orc.linear(att, lw["o"]), rounded)
            hn2, resid2 = orc.fused_add_bias_residual_rmsnorm(resid, o, None, lw["ffn_norm"], EPS)
            hn2, resid2 = _r(hn2, rounded), _r(resid2, rounded)
            h = _ffn(hn2, resid2, lw, sparse, case, rounded, logits)
        out[idx] = h
        for dst, src in zip(logit_rows, logits):
            dst[idx] = src
    return out, logit_rows


def prefill(b, rounded):
    """oracle.context_decoder's layer loop with the FFN of a sparse layer replaced; `hist` cached tokens per sequence"""
    case = b["case"]
    hs, lens, hist = case["hs"], case["lens"], case["hist"]
    nh, kvh = geometry(hs)
    kc, vc = (np.ascontiguousarray(a) for a in _float_caches(b))
    bs, T, mq = len(lens), int(sum(lens)), int(max(lens))
    ctx = np.array([l + h for l, h in zip(lens, hist)], np.int32)
    mk = int(ctx.max())
    off, _ = orc.cal_padding_offset(lens, mq, fill=0)
    off = off.reshape(-1)[:T]
    mask = orc.build_causal_mask(lens, ctx, mq, mk)
    h = b["x"].astype(np.float32)
    logits = []
    for l, (lw, sparse) in enumerate(zip(b["weights"], case["sparse"])):
        hn, resid = orc.rmsnorm(h, lw["attn_norm"], EPS)
        hn = _r(hn, rounded)
        qkv = _r(orc.linear(hn, lw["qkv"]), rounded).reshape(T, nh + 2 * kvh, hs)
        q, k, v = orc.qkv_bias_transpose_rope(qkv, None, off, hist, bs, mq, nh, kvh, hs, hs, ROPE_BASE, fill=0.0)
        orc.concat_kv(_r(k, rounded), kc, lens, hist, l)
        orc.concat_kv(_r(v, rounded), vc, lens, hist, l)
        kr, vr = orc.repeat_kv(kc, ctx, l, nh, mk), orc.repeat_kv(vc, ctx, l, nh, mk)
        p = orc.scale_mask_softmax(orc.batched_gemm(_r(q, rounded), kr, True), mask, 1.0 / np.sqrt(hs))
        att = _r(orc.transpose_remove_padding(orc.batched_gemm(p, vr, False), off, T).reshape(T, H), rounded)
        o = _r(orc.linear(att, lw["o"]), rounded)
        hn2, resid2 = orc.fused_add_bias_residual_rmsnorm(resid, o, None, lw["ffn_norm"], EPS)
        hn2, resid2 = _r(hn2, rounded), _r(resid2, rounded)
        h = _ffn(hn2, resid2, lw, sparse, case, rounded, logits)
    return h, logits


def dense_twin(b, rounded=True):
    """the same case on an engine that ignored its experts (every layer dense): how far that lies from the reference"""
    twin = dict(b, case=dict(b["case"], sparse=tuple(False for _ in b["case"]["sparse"])))
    return (decode if b["case"]["kind"] == "decode" else prefill)(twin, rounded)[0]


_done = {}


def reference(case):
    """(operands, rounded hidden_out, unrounded hidden_out, stable rows [rows] bool), computed once per case"""
    if case["id"] not in _done:
        b = build(case)
        run = decode if case["kind"] == "decode" else prefill
        y64, la = run(b, False)
        y16, lb = run(b, True)
        _done[case["id"]] = (b, y16, y64, stable_rows(la, lb, case["k"]))
    return _done[case["id"]]


def stable_rows(la, lb, k):
    stable = np.ones(la[0].shape[0], bool)
    for a, b in zip(la, lb):
        E = a.shape[1]
        if k >= E:
            continue
        delta = np.abs(a - b).max()
        sa = -np.sort(-a, axis=1)
        ia, ib = np.argsort(-a, axis=1, kind="stable")[:, :k], np.argsort(-b, axis=1, kind="stable")[:, :k]
        same = np.array([set(p) == set(q) for p, q in zip(ia.tolist(), ib.tolist())])
        stable &= same & (sa[:, k - 1] - sa[:, k] >= 8 * delta)
    return stable
