"""The forms llmie_decoder_prefill_layer_plan names are the launches llmie_decoder_prefill makes: for one small 2-layer engine per form,
the query names the form and one profiled prefill pass makes the launches of that sequence, op by op, and leaves a finite output.

The expected launch counts are those of the commit BEFORE plan_prefill_layer existed, written down here as literals: the profiled
(TIMED) launches of the sequence the ladders inside PrefillPass took for each case, counted from that commit's source for two layers
-- short_splitk: one leading norm + one row-norm launch per layer under attn_norm, projection + slab consumer under qkv_gemm and
gate_up_swiglu; lean / general: one launch per op and layer (qkv_proj is one TIMED launch whatever it runs), two under gate_up_swiglu
where the SwiGLU is a launch of its own; packed_only with the RoPE epilogue: unpack and projection are two TIMED launches.  They are
not taken from the code under test.  Every case sits at the smallest token count at which the planner gives the form on a model of at
most 16 heads (asked on the CPU: 16 heads fill the QKV grid from 513 tokens, the 3072-wide SwiGLU grid from 1793; the fused fp16 SwiGLU
case sits at 2048, beside the two-launch one at 1024).  Counts cannot tell
a RoPE epilogue from the two launches behind one TIMED bracket -- tests/test_qkv_rope_fusion_gpu.py tells them apart by bit-identity."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16
L, HS = 2, 128
QKV_BIAS_MISALIGNED = 128   # LLMIE_PLAN_QKV_BIAS_MISALIGNED

ONE = dict(attn_norm=2, qkv_gemm=2, mha=2, o_gemm=2, ffn_norm=2, gate_up_swiglu=2, down_gemm=2)   # one launch per op and layer
TWO_GU = dict(ONE, gate_up_swiglu=4)
SPLITK = dict(attn_norm=3, qkv_gemm=4, mha=2, o_gemm=2, ffn_norm=2, gate_up_swiglu=4, down_gemm=2)

# id, weight format, heads / kv heads / I, sequence lengths, options, the forms the query names (layer 0; "layer1": what differs in
# layer 1), launches by op of ONE pass (2 layers)
CASES = [
    ("short_splitk_rope_and_plain", "f16", (16, 16, 1024), [64], dict(bias_misaligned_in_layer=1),
     dict(path="short_splitk", attn_norm="none", qkv="splitk_rope", rope_done="1", ffn_norm="rownorm", gate_up="splitk", attn="q64w4t1",
          layer1=dict(qkv="splitk", rope_done="0", rope_append="1")), SPLITK),
    ("lean_plain_150", "f16", (16, 16, 1024), [150], {},
     dict(path="lean", token_table="0", attn_norm="oop", qkv="plain", rope_done="0", rope_append="1", ffn_norm="oop", gate_up="fused"), ONE),
    ("lean_rope_f16_513", "f16", (16, 16, 1024), [513], {},
     dict(path="lean", token_table="1", qkv="rope_f16", pre="none", rope_done="1", rope_append="0", gate_up="two_launch", attn="q64w4t1"), TWO_GU),
    ("lean_int8_rope_w8", "int8", (16, 16, 1024), [513], {},
     dict(path="lean", qkv="rope_w8", pre="none", rope_done="1", gate_up="two_launch"), TWO_GU),
    ("lean_int4_rope_image", "int4", (16, 16, 1024), [513], {},
     dict(path="lean", qkv="rope_image", pre="dequant", rope_done="1", gate_up="two_launch"), TWO_GU),
    ("general_o_bias", "f16", (16, 16, 1024), [150], dict(o_bias=True),
     dict(path="general", attn_norm="inplace", qkv="plain", ffn_norm="inplace", gate_up="fused"), ONE),
    ("general_fp8_quant_norms", "fp8", (16, 16, 3072), [1793], {},
     dict(path="general", attn_norm="quant", qkv="rope_e4m3", rope_done="1", ffn_norm="quant", gate_up="e4m3_swiglu", attn="q64w4t1"), ONE),
    ("packed_only_rope_unpacked", "int8", (16, 16, 1024), [513], dict(packed_only=True),
     dict(path="packed_only", attn_norm="inplace", qkv="rope_unpacked", pre="unpack", rope_done="1", gate_up="unpack_two_launch"),
     dict(TWO_GU, qkv_gemm=4)),
    ("f16_swiglu_fused_2048", "f16", (16, 16, 3072), [2048], {}, dict(path="lean", qkv="rope_f16", gate_up="fused", attn="q128w8t1"), ONE),
    ("f16_swiglu_two_launch_1024", "f16", (16, 16, 3072), [1024], {}, dict(path="lean", qkv="rope_f16", gate_up="two_launch", attn="q64w4t1"),
     TWO_GU),
    # the three forms of the flash kernel: 64 query rows per workgroup (above: one short sequence), 4 waves x 2 row tiles, 8 waves
    ("attn_4_waves_2_tiles", "f16", (16, 16, 1024), [512] * 4, {}, dict(path="lean", attn="q128w4t2", grid="4x16x4", kv="f16"), TWO_GU),
    ("attn_8_waves", "f16", (16, 16, 1024), [1024, 1024], {}, dict(path="lean", attn="q128w8t1", grid="8x16x2", kv="f16"), TWO_GU),
]


def quantised(llmie, w, wfmt):
    if wfmt == "f16":
        return dict(data=w)
    n, k = w.shape
    if wfmt == "int8":
        q, sc = torch.empty((n, k), dtype=torch.int8, device=DEV), torch.empty(n, dtype=F16, device=DEV)
        llmie.quantize_w8(w, q, sc)
    elif wfmt == "int4":
        q, sc = torch.empty((n, k // 2), dtype=torch.uint8, device=DEV), torch.empty((n, k // 128), dtype=F16, device=DEV)
        llmie.quantize_w4(w, q, sc, 128)
    else:
        q, sc = torch.empty((n, k), dtype=torch.uint8, device=DEV), torch.empty(n, dtype=torch.float32, device=DEV)
        llmie.quantize_fp8(w, q, sc)
    return dict(data=q, scale=sc)


def engine_config(llmie, wfmt, geom, lens, opts):
    nh, kvh, inter = geom
    fmt = dict(f16=llmie.W_F16, int8=llmie.W_INT8, int4=llmie.W_INT4, fp8=llmie.W_FP8)[wfmt]
    return dict(head_num=nh, kv_head_num=kvh, head_size=HS, inter_size=inter, num_layers=L, vocab_size=100, max_seq_len=max(lens),
                max_batch=len(lens), rotary_dim=HS, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=fmt, int4_group=128,
                flags=llmie.DEC_PACKED_ONLY if opts.get("packed_only") else 0)


def profiled_pass(llmie, wfmt, geom, lens, opts):
    """{op: launches} of one prefill pass through a fresh 2-layer engine (ops that did not run are left out)"""
    nh, kvh, inter = geom
    H, QKV, T, bs = nh * HS, (nh + 2 * kvh) * HS, sum(lens), len(lens)
    rng = np.random.default_rng(5)
    u = lambda shape, s: torch.from_numpy((rng.uniform(-1, 1, shape) * s).astype(np.float32)).to(DEV).to(F16)
    layers = []
    for l in range(L):
        qkv, o = quantised(llmie, u((QKV, H), 2 / np.sqrt(H)), wfmt), quantised(llmie, u((H, H), 2 / np.sqrt(H)), wfmt)
        if "bias_misaligned_in_layer" in opts:   # a view 4 bytes into its tensor in that layer, at the tensor's start in the other
            off = 2 if l == opts["bias_misaligned_in_layer"] else 0
            qkv["bias"] = u((QKV + 4,), 0.3)[off:off + QKV]
            assert qkv["bias"].data_ptr() % 8 == 2 * off
        if opts.get("o_bias"):
            o["bias"] = u((H,), 0.3)
        layers.append(dict(attn_norm=u((H,), 0.2) + 1, ffn_norm=u((H,), 0.2) + 1, qkv=qkv, o=o,
                           gate_up=quantised(llmie, u((2 * inter, H), 2 / np.sqrt(H)), wfmt), down=quantised(llmie, u((H, inter), 2 / np.sqrt(inter)), wfmt)))
    dec = llmie.Decoder(engine_config(llmie, wfmt, geom, lens, opts), layers)
    kc, vc = torch.zeros((L, bs, kvh, max(lens), HS), dtype=F16, device=DEV), torch.zeros((L, bs, kvh, max(lens), HS), dtype=F16, device=DEV)
    x = u((T, H), 1.0)
    dec.profile_begin(64)
    y = dec.prefill(x, torch.empty_like(x), kc, vc, torch.tensor(lens, dtype=torch.int32, device=DEV),
                    torch.zeros(bs, dtype=torch.int32, device=DEV), max(lens))
    counts = {op: n for op, (_, n) in dec.profile_end().items() if n}
    assert torch.isfinite(y.float()).all()
    dec.close()
    return counts


def named_forms(llmie, wfmt, geom, lens, opts, call_flags=0):
    cfg = dict(engine_config(llmie, wfmt, geom, lens, opts), kv_fmt=0, k_scale=0.0, v_scale=0.0)
    text, status = llmie.decoder_prefill_layer_plan(cfg, sum(lens), len(lens), max(lens), call_flags | (32 if opts.get("o_bias") else 0))
    assert text is not None, (status, llmie.lib().llmie_last_error())
    return llmie.plan_fields(text)


@pytest.mark.parametrize("name,wfmt,geom,lens,opts,forms,counts", CASES, ids=[c[0] for c in CASES])
def test_named_forms_make_their_launches(llmie, name, wfmt, geom, lens, opts, forms, counts):
    forms = dict(forms)
    layer1 = forms.pop("layer1", {})
    named = named_forms(llmie, wfmt, geom, lens, opts)
    assert {k: named[k] for k in forms} == forms
    if layer1:
        named1 = named_forms(llmie, wfmt, geom, lens, opts, QKV_BIAS_MISALIGNED)
        assert {k: named1[k] for k in layer1} == layer1
        assert named1["launches"] == named["launches"]
    # (the query counts one layer; the split-K sequence adds its leading norm once per pass)
    per_pass = {op: L * n + (1 if forms["path"] == "short_splitk" and op == "attn_norm" else 0) for op, n in named["launches"].items()}
    got = profiled_pass(llmie, wfmt, geom, lens, opts)
    print(name, got)
    assert got == counts
    assert per_pass == counts
