"""QK-norm without a GPU: the exports, every host-side refusal of llmie_qk_norm / llmie_decoder_mha_qknorm, the plan texts of the
decode attention launch and of a prefill layer under the new form bits, the cases of tests/qknorm_cases.py themselves, and the
resources of the new kernels in the built objects.

The prefill layer plans are held to tests/golden/prefill_layer_plans.txt through tests/test_prefill_layer_plan_cpu.py's own
recording(): without LLMIE_PLAN_QK_NORM every line of the golden comes back unchanged; with it a layer whose golden form rotates in
the QKV projection plans the form without the epilogue and the RoPE + append launch, which normalises.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import attn_cases as ac
import model_param_cases as mpc
import qknorm_cases as qc
import test_prefill_layer_plan_cpu as plp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("llmie_qk_norm", "llmie_decoder_mha_qknorm", "llmie_decoder_mha_qknorm_plan", "llmie_decoder_set_qk_norm")
PLAN_QK_NORM = 8192


@pytest.fixture(scope="module")
def lib(llmie):
    llmie.build()
    return llmie.lib()


def test_new_entries_are_exported(lib, llmie):
    for n in NEW:
        assert hasattr(lib, n) and n in llmie.EXPORTS, n
    assert llmie.PLAN_QK_NORM == PLAN_QK_NORM and llmie.ATTN_FORMS["qk_norm"] == 1024
    hdr = open(os.path.join(ROOT, "include", "llmie.h")).read()
    assert "#define LLMIE_PLAN_QK_NORM 8192u" in hdr and "#define LLMIE_ATTN_QK_NORM 1024u" in hdr
    for name in ("qk_norm", "decoder_mha_qknorm", "decoder_mha_qknorm_plan"):
        assert callable(getattr(llmie, name))
    assert callable(llmie.Decoder.set_qk_norm)


def test_qk_norm_refusals(lib):
    one, odd = C.c_void_p(16), C.c_void_p(24)   # never dereferenced: every check here fails on the host
    f = lambda qkv, rows, nh, kvh, hs, qg, kg, eps, dt=1: lib.llmie_qk_norm(qkv, rows, nh, kvh, hs, qg, kg, eps, dt, None)
    err = lambda: lib.llmie_last_error().decode()
    for args in ((None, 1, 4, 2, 128, one, one, 1e-6), (one, 1, 4, 2, 128, None, one, 1e-6), (one, 1, 4, 2, 128, one, None, 1e-6)):
        assert f(*args) == -1 and "NULL" in err()
    for args in ((one, 0, 4, 2, 128, one, one, 1e-6), (one, 1, 0, 2, 128, one, one, 1e-6), (one, 1, 4, 0, 128, one, one, 1e-6),
                 (one, 1, 4, 2, 0, one, one, 1e-6), (one, -3, 4, 2, 128, one, one, 1e-6)):
        assert f(*args) == -1 and "bad shape" in err()
    assert f(one, 1, 3, 2, 128, one, one, 1e-6) == -1 and "kv_head_num" in err()
    for eps in (-1e-6, float("nan")):
        assert f(one, 1, 4, 2, 128, one, one, eps) == -1 and "eps" in err()
    for args in ((odd, 1, 4, 2, 128, one, one, 1e-6), (one, 1, 4, 2, 128, odd, one, 1e-6), (one, 1, 4, 2, 128, one, odd, 1e-6)):
        assert f(*args) == -1 and "16-byte aligned" in err()
    assert f(one, 1, 4, 2, 128, one, one, 1e-6, 0) == -2 and "fp16 only" in err()
    for hs in (32, 256, 96):
        assert f(one, 1, 4, 2, hs, one, one, 1e-6) == -2 and "head_size 64 / 128" in err()
    assert f(one, 1, 4, 2, 128, one, one, 0.0, 7) == -2   # unknown dtype


def _mha(lib, qkv=16, bias=None, nh=4, kvh=2, hs=128, window=0, head_sink=None, e4m3=0, qg=16, kg=16, eps=1e-6, dt=1, tickets=None):
    p = lambda v: None if v is None else C.c_void_p(v)
    return lib.llmie_decoder_mha_qknorm(p(qkv), p(bias), p(16), p(16), p(16), 0, 3, nh, kvh, hs, 1024, p(16), p(16), 1 << 40, p(16), hs, None, 0, 0,
                                        window, 0, p(tickets), e4m3, 0.5, 0.5, p(head_sink), p(qg), p(kg), eps, dt, None)


def test_decoder_mha_qknorm_refusals(lib):
    """never-dereferenced pointers: every refusal is decided on the host, in front of any launch"""
    err = lambda: lib.llmie_last_error().decode()
    assert _mha(lib, qg=None) == -1 and "go together" in err()
    assert _mha(lib, kg=None) == -1 and "go together" in err()
    assert _mha(lib, qg=24) == -1 and "16-byte aligned" in err()
    assert _mha(lib, eps=-1.0) == -1 and "qk_eps" in err()
    assert _mha(lib, eps=float("nan")) == -1 and "qk_eps" in err()
    for kw in (dict(bias=16), dict(window=64), dict(head_sink=16), dict(dt=0), dict(hs=32), dict(hs=256), dict(qkv=24), dict(nh=6)):
        assert _mha(lib, **kw) == -2 and "QK-norm needs" in err(), (kw, err())
    assert _mha(lib, nh=16, e4m3=1) == -2 and "head ratio 1/2/4" in err()        # rep 8 over e4m3
    assert _mha(lib, e4m3=1, tickets=16) == -2 and "fp8 KV" in err()


def test_decode_plan_text(llmie, lib):
    forms = ("rope", "ragged", "step_dev")
    n = 0
    for hs in (64, 128):
        for ratio, e4m3 in ((1, False), (2, False), (4, False), (8, False), (1, True), (2, True), (4, True)):
            for extra in ((), ("paged",), ("tickets",)):
                if e4m3 and "tickets" in extra:
                    continue
                kw = dict(kv_e4m3=e4m3, forms=forms + extra, max_pages=8 if extra == ("paged",) else 0, num_pages=40 if extra == ("paged",) else 0)
                sink, st0 = llmie.decoder_mha_sink_plan(llmie.F16, 3, 2 * ratio, 2, hs, 1024, **kw)
                with_bit, st1 = llmie.decoder_mha_qknorm_plan(llmie.F16, 3, 2 * ratio, 2, hs, 1024, **dict(kw, forms=kw["forms"] + ("qk_norm",)))
                without, st2 = llmie.decoder_mha_qknorm_plan(llmie.F16, 3, 2 * ratio, 2, hs, 1024, **kw)
                assert st0 == st1 == st2 == 0 and with_bit == sink + " qk_norm" and without == sink, (hs, ratio, e4m3, extra, sink, with_bit)
                # the three older queries mask the bit: their texts do not change
                older = dict(kw, forms=kw["forms"] + ("qk_norm",))
                assert llmie.decoder_mha_sink_plan(llmie.F16, 3, 2 * ratio, 2, hs, 1024, **older)[0] == sink
                assert llmie.decoder_mha_window_plan(llmie.F16, 3, 2 * ratio, 2, hs, 1024, 0, **older)[0] == sink
                assert llmie.decoder_mha_plan(llmie.F16, 3, 2 * ratio, 2, hs, 1024, **older)[0] == sink
                n += 1
    assert n == 36
    q = ("rope", "ragged", "step_dev", "qk_norm")
    assert llmie.decoder_mha_qknorm_plan(llmie.F16, 3, 4, 2, 32, 1024, forms=q) == (None, -2)
    assert llmie.decoder_mha_qknorm_plan(llmie.F32, 3, 4, 2, 128, 1024, forms=q) == (None, -2)
    assert llmie.decoder_mha_qknorm_plan(llmie.F16, 3, 4, 2, 128, 1024, window=64, forms=q) == (None, -2)
    assert llmie.decoder_mha_qknorm_plan(llmie.F16, 3, 16, 2, 128, 1024, kv_e4m3=True, forms=q) == (None, -2)
    assert llmie.decoder_mha_qknorm_plan(llmie.F16, 3, 4, 2, 128, 1024, forms=q + ("bias",)) == (None, -2)
    assert llmie.decoder_mha_qknorm_plan(llmie.F16, 3, 4, 2, 128, 1024, forms=q + ("head_sink",)) == (None, -2)
    assert llmie.decoder_mha_qknorm_plan(llmie.F16, 3, 4, 2, 128, 1024, forms=q, residues={"qkv": 8}) == (None, -2)


ROPE_FORMS = {"rope_f16": "plain", "rope_w8": "plain", "rope_image": "plain", "rope_e4m3": "plain_e4m3", "rope_unpacked": "unpack_plain",
              "splitk_rope": "splitk"}


def test_prefill_layer_plans(llmie, lib):
    plan = plp.ctypes_plan(lib, lib.llmie_decoder_prefill_layer_plan)
    # without the flag: the golden, line for line (every query of the golden's grid, through its own recording())
    assert plp.recording(llmie, plan) == plp._fixture()
    seen, refused, kept = {k: 0 for k in ROPE_FORMS}, 0, 0
    field = lambda text: dict(w.split("=") for w in text.split(" ") if "=" in w)
    for engine, heads, calls in plp.grid(llmie):
        for _, points in calls:
            for cfg, T, batch, mq, cf, sw in points:
                text, status, _ = plan(cfg, T, batch, mq, cf, sw)
                got, gst, gerr = plan(cfg, T, batch, mq, cf | PLAN_QK_NORM, sw)
                if text is None:
                    assert got is None
                    continue
                if cfg.head_num // cfg.kv_head_num == 3:   # no QKN instantiation of the decode kernel: set_qk_norm refuses the engine
                    assert got is None and gst == -2 and "QK-norm needs" in gerr
                    refused += 1
                    continue
                a, b = field(text), field(got)
                assert got.endswith(" qk_norm=1") and b["rope_done"] == "0" and b["rope_append"] == "1" and b["token_table"] == "0", got
                assert b["qkv"] == ROPE_FORMS.get(a["qkv"], a["qkv"]), (engine, T, text, got)
                if a["qkv"] in ROPE_FORMS:
                    seen[a["qkv"]] += 1
                else:   # a layer that did not rotate in the projection keeps every form
                    assert got == text.replace("token_table=1", "token_table=0") + " qk_norm=1", (text, got)
                    kept += 1
                for key in ("attn_norm", "ffn_norm", "gate_up", "attn", "kv", "grid"):
                    assert a[key] == b[key], (key, text, got)
    assert all(seen.values()) and refused > 100 and kept > 1000, (seen, refused, kept)


def test_plan_names(llmie, lib):
    cfg = plp._config(llmie, plp.W_F16, 128, (32, 8, 128, 11008), 0)
    name = lambda c, prefill, rows, flags: lib.llmie_decoder_plan_name(C.byref(c), prefill, rows, flags, 0)
    for rows in (1, 4, 8):
        assert name(cfg, 0, rows, PLAN_QK_NORM) == name(cfg, 0, rows, 0) is not None
    for T in (64, 300, 2048):
        assert name(cfg, 1, T, PLAN_QK_NORM) == name(cfg, 1, T, 0) is not None
    bad = plp._config(llmie, plp.W_F16, 128, (32, 8, 32, 11008), 0)
    assert name(bad, 0, 1, 0) is not None and name(bad, 0, 1, PLAN_QK_NORM) is None and b"QK-norm needs" in lib.llmie_last_error()
    # a window or head sinks with QK-norm: no such engine
    for other in (llmie.PLAN_WINDOW, llmie.PLAN_HEAD_SINK):
        assert name(cfg, 0, 1, PLAN_QK_NORM | other) is None and b"QK-norm needs" in lib.llmie_last_error()


def test_head_norm_and_op_inputs():
    for rows, nh, kvh, hs in ((3, 8, 1, 128), (5, 4, 4, 128), (4, 4, 2, 64)):
        x = qc.op_inputs(rows, nh, kvh, hs, seed=1)
        assert x.dtype == np.float16 and x.shape == (rows, nh + 2 * kvh, hs) and np.isfinite(x).all()
        n = qc.head_norm(x[:, :nh + kvh], np.ones(hs), 0.0)
        assert np.abs((n * n).mean(axis=-1) - 1.0).max() <= 2.0 ** -9
        x64 = x.astype(np.float64)
        tq, tk = qc.tiny_heads(nh, kvh)
        for t in (tq, tk):   # mean square about eps: eps outside the root, or missing, is another function there
            ms = (x64[:, t] ** 2).mean(axis=-1)
            assert (ms > 0.5e-6).all() and (ms < 2e-6).all()
            exact = qc.head_norm(x[:, t], np.ones(hs), 1e-6, rounded=False)
            for other in (x64[:, t] / np.sqrt(ms)[:, None], x64[:, t] / (np.sqrt(ms)[:, None] + 1e-6)):
                assert (np.abs(other - exact).max(axis=-1) > 0.1 * np.abs(exact).max(axis=-1)).all()
        assert (x64[:, 0] ** 2).max() > 65504.0   # a sum in fp16 overflows
        ms = (x64[:, 1:nh - 1] ** 2).mean(axis=-1)
        if nh >= 4:   # one inv shared by the heads of a KV head: their mean squares differ by 4x from one head to the next
            assert (np.maximum(ms[:, 1:] / ms[:, :-1], ms[:, :-1] / ms[:, 1:]) > 2.0).all()
    qg, kg = qc.gammas(3, 128, seed=2)
    for g in (qg, kg):
        assert g.dtype == np.float16 and g.shape == (3, 128) and (g >= 0.5).all() and (g <= 2.0).all()
        assert (g[:, :64] != g[:, 64:]).all() and len({g[l].tobytes() for l in range(3)}) == 3
    assert (qg != kg).mean() > 0.9


def test_defects_move_a_one_layer_restatement():
    """4 heads over 2 of 64, 150 tokens, one layer: every defect of layer_restatement moves the hidden output of the layer's attention
    block -- measured on the attention output itself -- by more than 0.1 in relative Frobenius norm"""
    nh, kvh, hs, T = 4, 2, 64, 150
    rng = np.random.default_rng(11)
    w = mpc.draw_layers(rng, nh, kvh, hs, 512, 1)[0]
    x = mpc.h16(rng.standard_normal((T, nh * hs)).astype(np.float32)).astype(np.float64)
    hn = mpc._norm(x, w["attn_norm"].astype(np.float64), 1e-5, "attn", 0, frozenset())
    qkv = (hn @ w["qkv"].astype(np.float64).T).reshape(T, nh + 2 * kvh, hs)
    qg, kg = qc.gammas(1, hs, seed=3)
    tab = ac.rope_table(256, hs, hs)

    def attend(defect, gam=True):
        q, k, v = qc.qk_of(qkv, nh, kvh, tab, np.arange(T), qg[0] if gam else None, kg[0] if gam else None, qc.EPS, defect)
        sc = np.einsum("qhd,thd->hqt", q, k[:, np.arange(nh) // (nh // kvh)]) / np.sqrt(hs)
        sc = np.where(np.arange(T)[None, :] <= np.arange(T)[:, None], sc, -np.inf)
        p = np.exp(sc - sc.max(axis=2, keepdims=True))
        return np.einsum("hqt,thd->qhd", p / (p.sum(axis=2, keepdims=True) + 1e-6), v[:, np.arange(nh) // (nh // kvh)])

    exp = attend("none")
    rel = lambda a: np.linalg.norm(a - exp) / np.linalg.norm(exp)
    moved = {d: rel(attend(d)) for d in qc.DEFECTS[1:]}
    moved["no norm"] = rel(attend("none", gam=False))
    print({k: round(float(v), 3) for k, v in moved.items()})
    assert all(v > 0.1 for v in moved.values()), moved
    # eps 1e-5 against 1e-6 moves it far less: eps is tested on the operator, not on an engine
    q5, k5, _ = qc.qk_of(qkv, nh, kvh, tab, np.arange(T), qg[0], kg[0], 1e-5)
    q6, k6, _ = qc.qk_of(qkv, nh, kvh, tab, np.arange(T), qg[0], kg[0], 1e-6)
    assert np.linalg.norm(q5 - q6) / np.linalg.norm(q6) < 1e-3


def _resources():
    spec = importlib.util.spec_from_file_location("ckr", os.path.join(ROOT, "tools", "check_kernel_resources.py"))
    ckr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ckr)
    obj = lambda n: os.path.join(ROOT, "llm-inference-engine_amd", "csrc", "_obj", n + ".hip.o")
    return {n: ckr.kernel_metadata(obj(n)) for n in ("attention_decode", "prefill", "qk_norm")}


def test_qkn_kernels_are_there_and_do_not_spill(lib):
    """14 QKN forms of the split kernel (head size 64 / 128 x ratios 1 / 2 / 4 / 8 over fp16, 1 / 2 / 4 over e4m3; rep 8 fits), the two
    QKN forms of the RoPE + append kernel, the operator's two head sizes: no scratch and no spilled vector register in any of them (the
    project's meaning of "does not spill", as in tests/test_abi_cpu.py), and the split forms stay within the 512 registers of a wave"""
    ks = _resources()
    # template arguments <.., KT, WIN = false, SINK = false, QKN = true, const half *, const half *, float>
    split = [k for k in ks["attention_decode"] if "decode_attn_split_kernel" in k["name"] and "Lb0ELb0ELb1EJPKDF16_" in k["name"]]
    names = sorted(k["name"] for k in split)
    assert len(split) == 14, names
    for hs in (64, 128):
        for rep, kt in [(r, "DF16_") for r in (1, 2, 4, 8)] + [(r, "NS_7fp8kv_tE") for r in (1, 2, 4)]:
            assert any("IDF16_Li%dELi%dELi4ELi8E%sLb0ELb0ELb1E" % (hs, rep, kt) in n for n in names), (hs, rep, kt)
    append = [k for k in ks["prefill"] if "prefill_rope_append_kernel" in k["name"] and "Lb1EJPKDF16_" in k["name"]]
    assert len(append) == 2, [k["name"] for k in append]
    op = [k for k in ks["qk_norm"] if "qk_norm_kernel" in k["name"]]
    assert len(op) == 2
    for k in split + append + op:
        print("%-100s vgpr %3d sgpr %3d spill v%d s%d scratch %d" % (k["name"][:100], k["vgpr"], k["sgpr"], k["vgpr_spill"], k["sgpr_spill"], k["scratch"]))
    bad = [k for k in split + append + op if k["vgpr_spill"] or k["scratch"]]
    assert not bad, bad
    # the kernels that existed keep their count: 88 in the object (80 of them split forms) beside the 14
    assert len(ks["attention_decode"]) == 88 + 14
    assert len([k for k in ks["attention_decode"] if "decode_attn_split_kernel" in k["name"]]) == 80 + 14


@pytest.mark.parametrize("hs,nh,kvh,L,prefill", [(128, 4, 2, 2, True), (64, 4, 2, 4, False)], ids=["A_prefill", "B_decode_only"])
def test_defects_clear_the_engine_bar(hs, nh, kvh, L, prefill):
    """the first case of each engine of tests/test_qknorm_engine_gpu.py on the CPU: the restatement without the norm and the ones with
    a defect lie more than 10 x bounds["fro"] from the engine's, on the hidden output, at the gamma range the case draws from"""
    from conftest import systematic_error
    lens, inter, max_seq = [150, 70, 129], 512, 1024
    rng = np.random.default_rng(7)
    layers = mpc.draw_layers(rng, nh, kvh, hs, inter, L)
    cfg = dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=inter, rms_eps=1e-5)
    qg, kg = qc.gammas(L, hs, 13, *qc.GAMMA_RANGE["prefill" if prefill else "decode_only"])
    tab = ac.rope_table(max_seq, hs, hs)
    shape = (L, len(lens), kvh, max_seq, hs)
    k0, v0, _, _ = mpc.draw_caches(rng, shape, "f16")
    if prefill:
        k0, v0 = np.zeros(shape), np.zeros(shape)
        x, q_lens, hist = rng.standard_normal((sum(lens), nh * hs)), lens, [0] * len(lens)
    else:
        x, q_lens, hist = rng.standard_normal((len(lens), nh * hs)), [1] * len(lens), lens
    out = {}
    for name in ("exp", "no norm", "after_rope", "gammas_swapped", "k_raw"):
        g = (None, None) if name == "no norm" else (qg, kg)
        out[name] = qc.layer_restatement(cfg, layers, mpc.h16(x.astype(np.float32)), k0.astype(np.float64).copy(), v0.astype(np.float64).copy(), q_lens,
                                         hist, tab, g[0], g[1], qc.EPS, name if name in qc.DEFECTS else "none")
    exp = out.pop("exp")
    moved = {n: float(systematic_error(o, exp)[0]) for n, o in out.items()}
    print({k: round(v, 3) for k, v in moved.items()})
    assert all(v > 10 * mpc.bounds("f16")["fro"] for v in moved.values()), moved
