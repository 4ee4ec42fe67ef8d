"""Engine parity OFF the one (rms_eps, rotary_base, rotary_dim) point the other engine tests build with: the parameter points, the
engine cases, their inputs and their references, shared by tests/test_model_params_cpu.py (the inputs can fail, shown on the host) and
tests/test_model_params_gpu.py (the engines against the oracle at those inputs).

Points   P0 = (eps 1e-5, base 10000, rot = hs): the control, where the new references and bounds must reproduce what the existing
         tests measure; P1 = (0.5, 500000, hs / 2), with eps 2.0 on the fp8 engines (point_params);
         P2 = (1e-6, 77, hs / 4).
Cases    two layers (one for the fp8 and e4m3-cache engines, layers_of): the eight decode forms of tests/test_decoder_plan_gpu.py and the twelve prefill forms of tests/test_prefill_plan_gpu.py
         (imported, not copied), plus int4 decode at batch 1 / 7, an fp32 engine of 4 heads x 32, a GQA decode on a paged e4m3 cache at
         head size 64 and a prefill behind history on a paged e4m3 cache.  Every case names the launch sequence it must take.
Inputs   weights, gammas, caches and hidden rows as tests/test_decoder_gpu.py draws them (uniform, fp16-representable; the caches
         of the fp8 and e4m3-cache cases are larger, see draw_caches, and the fp8 prefill runs behind 64 cached tokens); a second family multiplies hidden row b (token t) by
         GAINS[b % 5] = 2^-9 .. 2^11.
Refs     orc.self_decoder / orc.context_decoder with the point in their config (de-quantised weights for int8 / int4, de-quantised
         caches for e4m3); fp8 weights: the oracle kernels composed with emulated e4m3 activations; layer_restatement(): the same
         layer in float64 numpy, equal to the oracle to 1e-5 (asserted on the host), with a switch per seeded defect.
"""
import numpy as np

import oracle as orc
from test_kvfp8_gpu import TAB, _to_e4m3 as to_e4m3   # the e4m3fn table and round-to-nearest-even onto it, defined once

FRO_F16, PROJ_F16 = 3e-3, 2e-4      # tests/test_decoder_gpu.py, tests/test_prefill_gpu.py
L, MAX_SEQ, STEP = 2, 64, 33        # decode: the geometry of tests/test_decoder_plan_gpu.py; the new token sits at position 32

POINTS = {"P0": dict(eps=1e-5, base=10000.0, rot_div=1), "P1": dict(eps=0.5, base=500000.0, rot_div=2),
          "P2": dict(eps=1e-6, base=77.0, rot_div=4)}
P1_EPS_FP8 = 2.0
GAINS = 2.0 ** np.array([-9.0, -3.0, 0.0, 4.0, 11.0])


def layers_of(wfmt, cache="dense"):
    """Layers of a case's engine.  Two, as the planner tests build them -- except the two engine kinds whose rounding is chaotic at
    the element level (per-token e4m3 activations of fp8 weights; e4m3 cache rows: an fp16 ulp moves a value across an e4m3 boundary,
    a 6 % step).  The project's bounds for those are defined on ONE layer (tests/test_quant_gpu.py, tests/test_kvfp8_gpu.py: a second
    layer doubles the quantisation stages), so they are held there; the launch sequence does not depend on the layer count."""
    return 1 if wfmt == "fp8" or cache == "paged_e4m3" else L


def point_params(point, hs, wfmt="f16"):
    """the three engine parameters of a point.  fp8 engines take P1_EPS_FP8 at P1: their bound is 0.03 on one layer, and eps placed
    outside the square root moves a unit row by 15 % at eps 0.5 (5 bounds) and by 40 % at 2.0."""
    p = POINTS[point]
    eps = P1_EPS_FP8 if (point, wfmt) == ("P1", "fp8") else p["eps"]
    return dict(rms_eps=eps, rotary_base=p["base"], rotary_dim=hs // p["rot_div"])


def h16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ cases
def decode_cases():
    """id, weight format, (heads, kv heads, head size, I), batch, engine flags, launch sequence, cache ("dense" / "paged_e4m3")"""
    from test_decoder_plan_gpu import CASES
    out = [(n, wfmt, geom, batch, flags, path, "dense") for n, wfmt, geom, batch, flags, path, _ in CASES]
    out += [("int4_b1", "int4", (8, 8, 128, 1024), 1, 0, "gemv", "dense"),
            ("int4_b7", "int4", (16, 4, 128, 1024), 7, 0, "packed", "dense"),
            ("fp32_4x32", "f32", (4, 4, 32, 344), 5, 0, "unfused", "dense"),
            ("gqa_kvfp8_paged_hs64", "f16", (8, 2, 64, 768), 5, 0, "gemv", "paged_e4m3")]
    return out


PREFILL_HISTORY_CASE = ("history_paged_e4m3", "f16", (8, 8, 768), [100, 64], dict(hist=[150, 200], cache="paged_e4m3"),
                        dict(path="lean", attn="q64w4t1", kv="e4m3"))


# The fp8 prefill keeps its tokens and its form but runs behind 64 cached tokens (drawn as draw_caches draws them for fp8): a
# wrongly rotated q shows in the hidden output only, and without cached rows whose choice matters it moves an fp8 layer's output by
# 5-6 bounds of 0.03, not 10 (tests/test_model_params_cpu.py).
PREFILL_HISTORY = {"general_fp8_quant_norms": dict(hist=[64])}


def prefill_cases():
    """id, weight format, (heads, kv heads, I), sequence lengths, options, the forms the planner must name (head size 128)"""
    from test_prefill_plan_gpu import CASES
    return [(n, wfmt, geom, lens, dict(opts, **PREFILL_HISTORY.get(n, {})), forms) for n, wfmt, geom, lens, opts, forms, _ in CASES] + \
        [PREFILL_HISTORY_CASE]


P2_DECODE = ("gemv", "packed", "splitk")
P2_PREFILL = ("short_splitk_rope_and_plain", "lean_rope_f16_513")
GAIN_PREFILL = ("short_splitk_rope_and_plain", "lean_plain_150", "lean_rope_f16_513", "general_o_bias", "general_fp8_quant_norms",
                "packed_only_rope_unpacked")
KS, VS = 1.0 / 32, 1.0 / 16          # e4m3 cache scales (tests/test_kvfp8_gpu.py)
FP8_K_SCALE, FP8_V_SCALE, E4M3_TOP = 8.0, 1.0, 0x68


def bounds(wfmt, cache="dense"):
    """the project's own bounds by engine kind.  elem: element-wise (rtol, atol) of the hidden output; fro / proj: systematic_error;
    max: largest element error (fp8); cache: appended rows, max abs; row: the per-row relative bound of the row-gain family (hidden
    rows, and K / V rows: row_kv)"""
    if wfmt == "f32":       # tests/test_decoder_gpu.py
        return dict(elem=(2e-4, 2e-4), fro=1e-5, proj=1e-6, cache=1e-4, row=1e-5, row_kv=1e-5)
    if wfmt == "fp8":       # against the emulated composition (tests/test_quant_gpu.py); the K / V rows are held like the hidden rows
        return dict(fro=0.03, max=0.3, row=0.03, row_kv=0.03)
    b = dict(elem=(2e-2, 2e-2), fro=FRO_F16, proj=PROJ_F16, cache=2e-2, row=FRO_F16, row_kv=FRO_F16)
    if cache == "paged_e4m3":
        # an fp16 engine whose reference quantises the new rows as the device does: the fp16 bounds on the hidden output; rows as
        # tests/test_kvfp8_gpu.py bounds them (codes equal up to ties, values within an e4m3 step: 0.13 abs, 0.07 relative)
        b.update(cache=0.13, row_kv=0.07)
    return b


# ------------------------------------------------------------------------------------------------------------------ inputs
def uniform(rng, shape, scale, f16=True):
    a = (rng.uniform(-1, 1, shape) * scale).astype(np.float32)
    return h16(a) if f16 else a


def draw_layers(rng, nh, kvh, hs, inter, layers, f16=True, qkv_bias=False, o_bias=False):
    """as tests/test_decoder_gpu.py _model: gammas 1 +- 0.2, matrices uniform * 2 / sqrt(K), biases * 0.1"""
    H, QKV = nh * hs, (nh + 2 * kvh) * hs
    out = []
    for _ in range(layers):
        w = dict(attn_norm=uniform(rng, (H,), 0.2, f16) + 1, qkv=uniform(rng, (QKV, H), 2.0 / np.sqrt(H), f16),
                 qkv_bias=uniform(rng, (QKV,), 0.1, f16) if qkv_bias else None,
                 o=uniform(rng, (H, H), 2.0 / np.sqrt(H), f16), o_bias=uniform(rng, (H,), 0.1, f16) if o_bias else None,
                 ffn_norm=uniform(rng, (H,), 0.2, f16) + 1, gate_up=uniform(rng, (2 * inter, H), 2.0 / np.sqrt(H), f16),
                 down=uniform(rng, (H, inter), 2.0 / np.sqrt(inter), f16))
        if f16:
            w["attn_norm"], w["ffn_norm"] = h16(w["attn_norm"]), h16(w["ffn_norm"])
        out.append(w)
    return out


def draw_caches(rng, shape, wfmt, cache="dense"):
    """(K, V) cache contents as float32, and their e4m3 bytes where the cache is e4m3.  Dense caches of the fp16 / fp32 / int engines:
    uniform * 0.5 as tests/test_decoder_gpu.py draws them.  fp8 weights: K uniform * FP8_K_SCALE, V uniform * FP8_V_SCALE -- at 0.5
    a wrongly rotated q moves the output by 9 % (a different average of 33 small V rows), three times the fp8 bound of 0.03 and not
    ten; a peaked softmax (logits of std 3.5) over larger V rows makes the choice of keys matter.  e4m3: random bytes up to E4M3_TOP (tests/test_kvfp8_gpu.py draws
    up to 0x58), de-quantised with KS / VS."""
    if cache == "paged_e4m3":
        code = lambda: rng.integers(0, E4M3_TOP, shape).astype(np.uint8) | (rng.integers(0, 2, shape).astype(np.uint8) << 7)
        kq, vq = code(), code()
        return TAB[kq] * np.float32(KS), TAB[vq] * np.float32(VS), kq, vq
    ks, vs = (FP8_K_SCALE, FP8_V_SCALE) if wfmt == "fp8" else (0.5, 0.5)
    return uniform(rng, shape, ks, wfmt != "f32"), uniform(rng, shape, vs, wfmt != "f32"), None, None


def row_gains(rows, first=0):
    return GAINS[(first + np.arange(rows)) % len(GAINS)].astype(np.float32)


MATS = ("qkv", "o", "gate_up", "down")


def engine_layers(llmie, layers, wfmt, misaligned_bias_layer=None):
    """(engine layers on the device, oracle layers): the oracle gets the de-quantised weights of a quantised format.
    misaligned_bias_layer: that layer's QKV bias is a view 4 bytes into its tensor (tests/test_prefill_plan_gpu.py)"""
    import torch
    from test_prefill_gpu import _quantise as quantise
    dt = torch.float32 if wfmt == "f32" else torch.float16
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    eng, ref = [], []
    for w in layers:
        e, o = dict(attn_norm=d(w["attn_norm"]).to(dt), ffn_norm=d(w["ffn_norm"]).to(dt)), dict(w)
        for m in MATS:
            if wfmt in ("f16", "f32"):
                e[m] = dict(data=d(w[m]).to(dt))
            elif wfmt == "fp8":
                n, k = w[m].shape
                q, sc = torch.empty((n, k), dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
                llmie.quantize_fp8(d(w[m]).to(dt), q, sc)
                e[m], o[m] = dict(data=q, scale=sc), TAB[q.cpu().numpy()] * sc.cpu().numpy()[:, None]
            else:
                q, s, deq = quantise(w[m], wfmt)   # the numpy definition the device quantisers are held to bit for bit
                e[m], o[m] = dict(data=d(q), scale=d(s)), deq
        if w.get("qkv_bias") is not None:
            off = 2 if len(eng) == misaligned_bias_layer else 0
            n = w["qkv_bias"].size
            buf = torch.zeros(n + 4, dtype=dt, device="cuda")
            buf[off:off + n] = d(w["qkv_bias"]).to(dt)
            e["qkv"]["bias"] = buf[off:off + n]
            assert e["qkv"]["bias"].data_ptr() % 8 == 2 * off
        if w.get("o_bias") is not None:
            e["o"]["bias"] = d(w["o_bias"]).to(dt)
        eng.append(e)
        ref.append(o)
    return eng, ref


def wfmt_code(llmie, wfmt):
    return dict(f16=llmie.W_F16, f32=llmie.W_F32, int8=llmie.W_INT8, int4=llmie.W_INT4, fp8=llmie.W_FP8)[wfmt]


def decode_engine_config(llmie, wfmt, geom, batch, flags, point, cache="dense"):
    nh, kvh, hs, inter = geom
    cfg = dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=inter, num_layers=layers_of(wfmt, cache), vocab_size=100, max_seq_len=MAX_SEQ,
               max_batch=batch, dtype=llmie.F32 if wfmt == "f32" else llmie.F16, wfmt=wfmt_code(llmie, wfmt), int4_group=128,
               flags=flags, **point_params(point, hs, wfmt))
    if cache == "paged_e4m3":
        cfg.update(kv_fmt=llmie.KV_FP8, k_scale=KS, v_scale=VS)
    return cfg


def prefill_engine_config(llmie, wfmt, geom, lens, opts, point, hs=128):
    nh, kvh, inter = geom
    hist = opts.get("hist", [0] * len(lens))
    max_seq = max(l + h for l, h in zip(lens, hist))
    if opts.get("cache") == "paged_e4m3":
        max_seq = -(-max_seq // 128) * 128
    cfg = dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=inter, num_layers=layers_of(wfmt, opts.get("cache", "dense")), vocab_size=100, max_seq_len=max_seq,
               max_batch=len(lens), dtype=llmie.F16, wfmt=wfmt_code(llmie, wfmt), int4_group=128,
               flags=llmie.DEC_PACKED_ONLY if opts.get("packed_only") else 0, **point_params(point, hs, wfmt))
    if opts.get("cache") == "paged_e4m3":
        cfg.update(kv_fmt=llmie.KV_FP8, k_scale=KS, v_scale=VS)
    return cfg


def oracle_config(geom4, point, max_seq, layers=L, wfmt="f16"):
    nh, kvh, hs, inter = geom4
    return dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=inter, num_layers=layers, vocab=100, max_seq_len=max_seq,
                **point_params(point, hs, wfmt))


# ------------------------------------------------------------------------------------------------------------------ fp8 reference
def fp8_linear(x, wdeq):
    """an fp8 projection as the engine defines it: per-token e4m3 activations (scale amax / 448) x de-quantised e4m3 weights"""
    xs = (np.abs(x).max(axis=1) / np.float32(448.0)).astype(np.float32)
    xs[xs == 0] = 1.0
    xq = TAB[to_e4m3(x / xs[:, None])]
    return orc.linear(xq * xs[:, None], wdeq)


def e4m3_cache_rounding(a, scale):
    """what an e4m3 cache of that scale holds of the fp16 rows a, de-quantised"""
    return TAB[to_e4m3(h16(a) / np.float32(scale))] * np.float32(scale)


def composed_self_decoder(ocfg, layers, x, kc, vc, step, lin=None, rnd=None, kv_scales=None, raw=None):
    """orc.self_decoder as a composition of the oracle's kernels (self_decoder.cpp:69-119 order) for any number of layers and any
    parameter point -- tests/test_quant_gpu.py test_fp8_decoder_matches_oracle_composition, generalised.  lin: the projection
    (default orc.linear; fp8_linear for fp8 weights); rnd: applied wherever the engine stores fp16 (default: nothing);
    kv_scales: (k, v) scales of an e4m3 cache -- the new rows are quantised before they are attended to, as the device does
    (tests/test_kvfp8_gpu.py); raw: a list that receives, per layer, the (K, V) rows [T, kvh, hs] BEFORE that quantisation.
    Caches (de-quantised float32) updated in place."""
    lin, rnd = lin or orc.linear, rnd or (lambda a: a)
    nh, kvh, hs, inter = ocfg["head_num"], ocfg["kv_head_num"], ocfg["head_size"], ocfg["inter_size"]
    eps, rot, base = ocfg["rms_eps"], ocfg["rotary_dim"], ocfg["rotary_base"]
    bs, H = x.shape
    hid = x
    for l, w in enumerate(layers):
        h = rnd(orc.rmsnorm(hid, w["attn_norm"], eps)[0])
        qkv = rnd(orc.rope_decode(rnd(lin(h, w["qkv"])), nh, kvh, hs, step, rot, base))
        ko, vo = nh * hs, (nh + kvh) * hs
        if raw is not None:
            raw.append((qkv[:, ko:vo].reshape(bs, kvh, hs).copy(), qkv[:, vo:].reshape(bs, kvh, hs).copy()))
        if kv_scales:
            qkv[:, ko:vo], qkv[:, vo:] = e4m3_cache_rounding(qkv[:, ko:vo], kv_scales[0]), e4m3_cache_rounding(qkv[:, vo:], kv_scales[1])
        mha = rnd(orc.decoder_mha(qkv, None, kc, vc, l, nh, kvh, hs, step))
        h1 = rnd(rnd(lin(mha.reshape(bs, H), w["o"])) + hid)
        h2 = rnd(orc.rmsnorm(h1, w["ffn_norm"], eps)[0])
        act = rnd(orc.silu_and_mul(lin(h2, w["gate_up"]).reshape(bs, 2, inter)))
        hid = rnd(lin(act.reshape(bs, inter), w["down"])) + h1
        if l + 1 < len(layers):
            hid = rnd(hid)
    return hid


def composed_context_decoder(cfg, layers, x, kc, vc, lens, hist, lin=None, rnd=None, kv_scales=None, raw=None):
    """orc.context_decoder with the hooks of composed_self_decoder (same kernels, same order)"""
    lin, rnd = lin or orc.linear, rnd or (lambda a: a)
    nh, kvh, hs, inter = cfg["head_num"], cfg["kv_head_num"], cfg["head_size"], cfg["inter_size"]
    eps = cfg["rms_eps"]
    bs, T, mq = len(lens), int(sum(lens)), int(max(lens))
    ctx = np.array([l + h for l, h in zip(lens, hist)], np.int32)
    mk, H = int(ctx.max()), nh * hs
    off, _ = orc.cal_padding_offset(lens, mq, fill=0)
    off = off.reshape(-1)[:T]
    mask = orc.build_causal_mask(lens, ctx, mq, mk)
    h = x.copy()
    for l, w in enumerate(layers):
        hn, resid = orc.rmsnorm(h, w["attn_norm"], eps)
        qkv = rnd(lin(rnd(hn), w["qkv"])).reshape(T, nh + 2 * kvh, hs)
        q, k, v = orc.qkv_bias_transpose_rope(qkv, w.get("qkv_bias"), off, hist, bs, mq, nh, kvh, hs, cfg["rotary_dim"],
                                              cfg["rotary_base"], fill=0.0)
        q, k, v = rnd(q), rnd(k), rnd(v)
        if raw is not None:
            tok = lambda a: np.concatenate([a[b, :, :lens[b]].transpose(1, 0, 2) for b in range(bs)], axis=0)
            raw.append((tok(k), tok(v)))
        if kv_scales:
            k, v = e4m3_cache_rounding(k, kv_scales[0]), e4m3_cache_rounding(v, kv_scales[1])
        orc.concat_kv(k, kc, lens, hist, l)
        orc.concat_kv(v, vc, lens, hist, l)
        kr, vr = orc.repeat_kv(kc, ctx, l, nh, mk), orc.repeat_kv(vc, ctx, l, nh, mk)
        p = orc.scale_mask_softmax(orc.batched_gemm(q, kr, True), mask, 1.0 / np.sqrt(hs))
        att = rnd(orc.transpose_remove_padding(orc.batched_gemm(p, vr, False), off, T).reshape(T, H))
        o = rnd(lin(att, w["o"]))
        hn2, resid2 = orc.fused_add_bias_residual_rmsnorm(resid, o, w.get("o_bias"), w["ffn_norm"], eps)
        hn2, resid2 = rnd(hn2), rnd(resid2)
        act = rnd(orc.silu_and_mul(lin(hn2, w["gate_up"]).reshape(T, 2, inter)))
        h = orc.add_residual(resid2, rnd(lin(act, w["down"])))
        if l + 1 < len(layers):
            h = rnd(h)
    return h


# ------------------------------------------------------------------------------------------------------------------ restatement
DEFECTS = ("no_eps:attn", "no_eps:ffn", "no_eps:final", "eps_in_sum", "eps_outside", "eps_fixed", "q_base", "k_base", "q_full", "k_full",
           "exp_hs", "pair_rot", "neighbour_rms", "fp16_squares")
EPS_DEFECTS = DEFECTS[:6]
ROPE_DEFECTS = DEFECTS[6:12]


def _norm(x, gamma, eps, which, layer, defects):
    """RMSNorm rows of x (float64); `which` in attn / ffn / final names the norm for the defects that pick one"""
    sq = x * x
    if "fp16_squares" in defects:
        sq = np.minimum(sq, 65504.0)
    ss = sq.sum(axis=1)
    n = x.shape[1]
    if "eps_fixed" in defects:
        eps = 1e-5
    if "no_eps:" + which in defects or ("no_eps:attn0" in defects and which == "attn" and layer == 0):
        inv = 1.0 / np.sqrt(ss / n)
    elif "eps_in_sum" in defects:
        inv = 1.0 / np.sqrt((ss + eps) / n)
    elif "eps_outside" in defects:
        inv = 1.0 / (np.sqrt(ss / n) + eps)
    else:
        inv = 1.0 / np.sqrt(ss / n + eps)
    if "neighbour_rms" in defects:
        m = np.arange(x.shape[0]) ^ 1
        m = np.where(m < x.shape[0], m, np.arange(x.shape[0]))
        inv = inv[m]
    return x * inv[:, None] * gamma[None, :]


def _rope(x, pos, hs, rot, base, which, defects):
    """x [T, heads, hs] rotated at positions pos [T]: pairs (d, d + hs / 2) for d < rot / 2, angle pos / base^(2d / rot)
    (oracle/llmie_oracle.c rope_pair)"""
    exp_den, pair = rot, hs // 2
    if which + "_base" in defects:
        base = 10000.0
    if which + "_full" in defects:
        rot, exp_den = hs, hs
    if "exp_hs" in defects:
        exp_den = hs
    if "pair_rot" in defects:
        pair = rot // 2
    d = np.arange(rot // 2)
    ang = pos[:, None].astype(np.float64) / base ** (2.0 * d / exp_den)[None, :]
    c, s = np.cos(ang)[:, None, :], np.sin(ang)[:, None, :]
    out = x.copy()
    x0, x1 = x[:, :, d], x[:, :, d + pair]
    out[:, :, d] = x0 * c - x1 * s
    out[:, :, d + pair] = x1 * c + x0 * s
    return out


def layer_restatement(cfg, layers, x, k_cache, v_cache, lens, hist, defects=(), final_gamma=None):
    """The layers of orc.context_decoder in float64 numpy (a decode step is one new token per sequence behind step - 1 cached ones:
    orc.self_decoder computes the same for layers without a QKV bias).  cfg: head_num, kv_head_num, head_size, inter_size, rms_eps,
    rotary_dim, rotary_base; caches [L, bs, kvh, max_seq, hs] float64, updated in place.  Returns the hidden rows [T, H], behind the
    final norm where final_gamma is given.  defects: names of DEFECTS (or "no_eps:attn0": layer 0's attention norm only)."""
    nh, kvh, hs, inter = cfg["head_num"], cfg["kv_head_num"], cfg["head_size"], cfg["inter_size"]
    eps, rot, base = cfg["rms_eps"], cfg["rotary_dim"], cfg["rotary_base"]
    defects = frozenset(defects)
    rep, H = nh // kvh, nh * hs
    T = int(sum(lens))
    starts = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    pos = np.concatenate([hist[b] + np.arange(lens[b]) for b in range(len(lens))])
    h = np.asarray(x, np.float64).copy()
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    for l, w in enumerate(layers):
        resid = h
        hn = _norm(h, f(w["attn_norm"]), eps, "attn", l, defects)
        qkv = hn @ f(w["qkv"]).T
        if w.get("qkv_bias") is not None:
            qkv = qkv + f(w["qkv_bias"])[None, :]
        qkv = qkv.reshape(T, nh + 2 * kvh, hs)
        q = _rope(qkv[:, :nh], pos, hs, rot, base, "q", defects)
        k = _rope(qkv[:, nh:nh + kvh], pos, hs, rot, base, "k", defects)
        v = qkv[:, nh + kvh:]
        att = np.empty((T, nh, hs))
        for b in range(len(lens)):
            s0, s1, h0 = starts[b], starts[b + 1], hist[b]
            k_cache[l, b, :, h0:h0 + lens[b]] = k[s0:s1].transpose(1, 0, 2)
            v_cache[l, b, :, h0:h0 + lens[b]] = v[s0:s1].transpose(1, 0, 2)
            ctx = h0 + lens[b]
            K, V = k_cache[l, b, np.arange(nh) // rep, :ctx], v_cache[l, b, np.arange(nh) // rep, :ctx]     # [nh, ctx, hs]
            sc = np.einsum("qhd,htd->hqt", q[s0:s1], K) / np.sqrt(hs)
            sc = np.where(np.arange(ctx)[None, None, :] <= (h0 + np.arange(lens[b]))[None, :, None], sc, -np.inf)
            p = np.exp(sc - sc.max(axis=2, keepdims=True))
            p = p / (p.sum(axis=2, keepdims=True) + 1e-6)
            att[s0:s1] = np.einsum("hqt,htd->qhd", p, V)
        o = att.reshape(T, H) @ f(w["o"]).T
        resid = resid + o                               # (the reference keeps the O bias out of the residual stream)
        pre = resid + f(w["o_bias"])[None, :] if w.get("o_bias") is not None else resid
        hn2 = _norm(pre, f(w["ffn_norm"]), eps, "ffn", l, defects)
        gu = hn2 @ f(w["gate_up"]).T
        g, u = gu[:, :inter], gu[:, inter:]
        h = resid + ((g * 0.5 * (1.0 + np.tanh(0.5 * g))) * u) @ f(w["down"]).T    # g * sigmoid(g), without exp overflow
    if final_gamma is not None:
        h = _norm(h, f(final_gamma), eps, "final", len(layers), defects)
    return h


def final_norm_inputs(rng, rows, H, V, f16=True, lm_scale=0.3):
    """hidden rows under the row gains, final gamma and LM head of the final-norm cases (statistics of the existing LM-head tests)"""
    x = uniform(rng, (rows, H), 1.0, f16) * row_gains(rows)[:, None]
    return (h16(x) if f16 else x), uniform(rng, (H,), 0.2, f16) + 1, uniform(rng, (V, H), lm_scale, f16)


def final_norm_logits(x, gamma, lm, eps, defects=()):
    """float64 logits of the LM head behind the final norm"""
    f = lambda a: np.asarray(a, np.float64)
    return _norm(f(x), f(gamma), eps, "final", 0, frozenset(defects)) @ f(lm).T


def logprob_of(logits, ids):
    z = np.asarray(logits, np.float64)
    mx = z.max(axis=1)
    return z[np.arange(len(z)), ids] - (mx + np.log(np.exp(z - mx[:, None]).sum(axis=1)))


def fp8_dequantised(w):
    """numpy emulation of llmie_quantize_fp8 (per-row scale amax / 448, e4m3 codes), de-quantised: for host-side stand-ins; the
    GPU tests de-quantise the device's own codes"""
    s = (np.abs(w).max(axis=1) / np.float32(448.0)).astype(np.float32)
    s[s == 0] = 1.0
    return TAB[to_e4m3(w / s[:, None])] * s[:, None]


def chaotic_reference(compose, wfmt, kc, vc, rows):
    """Reference for the two engine kinds whose rounding is chaotic at the element level (layers_of), and the reference's OWN error.
    compose(kc, vc, **hooks) runs composed_self_decoder / composed_context_decoder on the given caches; rows(cache) picks the
    appended rows.  The reference is the composition with an fp16 rounding wherever the engine stores fp16, as the one-layer
    references of tests/test_quant_gpu.py (e4m3 activations emulated) and tests/test_kvfp8_gpu.py (new rows quantised before they
    are attended to) have it: an fp16 rounding ahead of an e4m3 rounding decides 0.8 % of the bytes.
    Returns (expected hidden, expected K rows, V rows, raw (unquantised) K rows, V rows or None, own): own() computes, from the
    oracle alone, the error of the rounded composition against the unrounded one -- dict(fro, max, row), each a list over (hidden,
    K rows, V rows) -- for a case that misses a project bound OFF the control point: twice that is then allowed (the factor 2
    covers summation order)."""
    k2, v2 = kc.copy(), vc.copy()
    raw = []
    if wfmt == "fp8":
        exp = compose(kc, vc, lin=fp8_linear, rnd=h16)
    else:
        exp = compose(kc, vc, kv_scales=(KS, VS), raw=raw, rnd=h16)
    a = (exp, rows(kc), rows(vc))
    memo = []

    def own():
        if not memo:
            alt = compose(k2, v2, lin=fp8_linear) if wfmt == "fp8" else compose(k2, v2, kv_scales=(KS, VS))
            b = (alt, rows(k2), rows(v2))
            memo.append(dict(fro=[rel_fro(x, y) for x, y in zip(a, b)], max=[float(np.abs(x - y).max()) for x, y in zip(a, b)],
                             row=[row_rel(x, y) for x, y in zip(a, b)]))
        return memo[0]

    rk = np.stack([r[0] for r in raw], axis=1) if raw else None
    rv = np.stack([r[1] for r in raw], axis=1) if raw else None
    return exp, a[1], a[2], rk, rv, own


def rel_fro(got, exp):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    return float(np.linalg.norm(got - exp) / (np.linalg.norm(exp) + 1e-300))


def row_rel(got, exp):
    """per row ||got_b - exp_b|| / ||exp_b|| (rows = the leading axis)"""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    got, exp = got.reshape(got.shape[0], -1), exp.reshape(exp.shape[0], -1)
    return np.linalg.norm(got - exp, axis=1) / (np.linalg.norm(exp, axis=1) + 1e-300)


def appended_rows(cache, lens, hist):
    """the appended rows of a [L, bs, kvh, max_seq, hs] cache as [T, L, kvh, hs] (token-major, like the hidden rows)"""
    return np.concatenate([cache[:, b, :, hist[b]:hist[b] + lens[b]].transpose(2, 0, 1, 3) for b in range(len(lens))], axis=0)
