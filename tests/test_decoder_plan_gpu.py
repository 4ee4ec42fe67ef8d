"""The names llmie_decoder_plan_name gives are the launch sequences llmie_decoder_forward runs: for one small engine per decode path,
the query names the path and one profiled decode step makes the launches of that path, op by op.

The expected launch counts are those of the commit BEFORE the planners existed, written down here as literals: the profiled (TIMED)
launches of the sequence the ladder inside llmie_decoder_forward took for each case, counted from that commit's source for two layers
(e.g. split-K: one leading norm + one row-norm launch per layer under attn_norm, projection + finalize under gate_up_swiglu; fp8 adds
the quantise launches).  They are not taken from the code under test.  gemv and packed
have the same counts -- tests/test_packed_only_gpu.py tells them apart by bit-identity; the chain path is per process and covered by
tests/test_path_switches_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16
L, MAX_SEQ, STEP = 2, 64, 33

# id, weight format, heads / kv heads / head size / I, batch, engine flags, path, launches by op of ONE step (2 layers)
CASES = [
    ("gemv", "f16", (8, 8, 64, 768), 2, 0, "gemv", dict(qkv_gemm=2, mha=2, o_gemm=2, gate_up_swiglu=2, down_gemm=2)),
    ("packed", "f16", (16, 4, 128, 1024), 7, 0, "packed", dict(qkv_gemm=2, mha=2, o_gemm=2, gate_up_swiglu=2, down_gemm=2)),
    ("no_packed_copy", "f16", (16, 4, 128, 1024), 7, 1, "splitk", dict(attn_norm=3, qkv_gemm=2, mha=2, o_gemm=2, ffn_norm=2, gate_up_swiglu=4, down_gemm=2)),
    ("splitk", "f16", (8, 8, 64, 768), 40, 0, "splitk", dict(attn_norm=3, qkv_gemm=2, mha=2, o_gemm=2, ffn_norm=2, gate_up_swiglu=4, down_gemm=2)),
    ("unfused", "f16", (8, 8, 64, 768), 130, 0, "unfused", dict(attn_norm=2, qkv_gemm=2, mha=2, o_gemm=2, ffn_norm=2, gate_up_swiglu=2, down_gemm=2)),
    ("unfused_rope", "f16", (6, 2, 48, 768), 2, 0, "unfused", dict(attn_norm=2, qkv_gemm=2, rope=2, mha=2, o_gemm=2, ffn_norm=2, gate_up_swiglu=2, down_gemm=2)),
    ("int8_packed", "int8", (16, 4, 128, 1024), 7, 0, "packed", dict(qkv_gemm=2, mha=2, o_gemm=2, gate_up_swiglu=2, down_gemm=2)),
    ("fp8_splitk", "fp8", (8, 8, 64, 768), 40, 0, "splitk", dict(attn_norm=4, qkv_gemm=2, mha=2, o_gemm=4, ffn_norm=2, gate_up_swiglu=4, down_gemm=4)),
]


def engine_config(llmie, wfmt, geom, batch, flags):
    nh, kvh, hs, inter = geom
    fmt = dict(f16=llmie.W_F16, int8=llmie.W_INT8, fp8=llmie.W_FP8)[wfmt]
    return dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=inter, num_layers=L, vocab_size=100, max_seq_len=MAX_SEQ,
                max_batch=batch, rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=fmt, int4_group=128, flags=flags)


def launch_counts(llmie, wfmt, geom, batch, flags):
    """{op: launches} of one decode step at STEP through a fresh 2-layer engine (ops that did not run are left out)"""
    nh, kvh, hs, inter = geom
    H, QKV = nh * hs, (nh + 2 * kvh) * hs
    rng = np.random.default_rng(3)
    u = lambda shape, s: torch.from_numpy((rng.uniform(-1, 1, shape) * s).astype(np.float32)).to(DEV).to(F16)

    def q(w):
        n, k = w.shape
        if wfmt == "f16":
            return dict(data=w)
        if wfmt == "int8":
            d, sc = torch.empty((n, k), dtype=torch.int8, device=DEV), torch.empty(n, dtype=F16, device=DEV)
            llmie.quantize_w8(w, d, sc)
        else:
            d, sc = torch.empty((n, k), dtype=torch.uint8, device=DEV), torch.empty(n, dtype=torch.float32, device=DEV)
            llmie.quantize_fp8(w, d, sc)
        return dict(data=d, scale=sc)

    layers = [dict(attn_norm=u((H,), 0.2) + 1, ffn_norm=u((H,), 0.2) + 1, qkv=q(u((QKV, H), 2 / np.sqrt(H))), o=q(u((H, H), 2 / np.sqrt(H))),
                   gate_up=q(u((2 * inter, H), 2 / np.sqrt(H))), down=q(u((H, inter), 2 / np.sqrt(inter)))) for _ in range(L)]
    dec = llmie.Decoder(engine_config(llmie, wfmt, geom, batch, flags), layers)
    kc, vc = u((L, batch, kvh, MAX_SEQ, hs), 0.5), u((L, batch, kvh, MAX_SEQ, hs), 0.5)
    x = u((batch, H), 1.0)
    dec.profile_begin(64)
    y = dec.forward(x, torch.empty_like(x), kc, vc, STEP)
    counts = {op: n for op, (_, n) in dec.profile_end().items() if n}
    assert torch.isfinite(y.float()).all()
    dec.close()
    return counts


@pytest.mark.parametrize("name,wfmt,geom,batch,flags,path,counts", CASES, ids=[c[0] for c in CASES])
def test_named_path_makes_its_launches(llmie, name, wfmt, geom, batch, flags, path, counts):
    cfg = llmie.DecoderConfig(**dict(engine_config(llmie, wfmt, geom, batch, flags), kv_fmt=0, k_scale=0.0, v_scale=0.0))
    named = llmie.lib().llmie_decoder_plan_name(C.byref(cfg), 0, batch, 0, 0)
    assert named is not None and named.decode() == path
    got = launch_counts(llmie, wfmt, geom, batch, flags)
    print(name, got)
    assert got == counts
