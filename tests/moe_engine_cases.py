"""Shared by tests/test_moe_engine_gpu.py and tests/moe_capture.py: the device side of the engine cases of tests/moe_engine_ref.py
(small engines with experts, and one call of a case on the entry point its cache form names)."""
import numpy as np
import torch

from moe_engine_ref import H, IE, INTER, MAX_SEQ, MAX_BATCH, K_SCALE, V_SCALE, geometry, layer_weights, contexts  # noqa: F401

DEV, F16 = "cuda", torch.float16


def make_engine(llmie, weights, hs, kv8=False, zero_down=False, inter=INTER, int8=False):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    nh, kvh = geometry(hs)
    layers = []
    for lw in weights:
        e = dict(attn_norm=d(lw["attn_norm"]), ffn_norm=d(lw["ffn_norm"]))
        for m in ("qkv", "o", "gate_up", "down"):
            w = d(np.zeros_like(lw[m]) if (zero_down and m == "down") else lw[m])
            if int8:
                wq, sc = torch.empty(w.shape, dtype=torch.int8, device=DEV), torch.empty(w.shape[0], dtype=F16, device=DEV)
                llmie.quantize_w8(w, wq, sc)
                e[m] = dict(data=wq, scale=sc)
            else:
                e[m] = dict(data=w)
        layers.append(e)
    cfg = dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=inter, num_layers=len(weights), vocab_size=100, max_seq_len=MAX_SEQ,
               max_batch=MAX_BATCH, rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=llmie.W_INT8 if int8 else llmie.W_F16,
               int4_group=128, flags=0, kv_fmt=llmie.KV_FP8 if kv8 else llmie.KV_NATIVE, k_scale=K_SCALE, v_scale=V_SCALE)
    return llmie.Decoder(cfg, layers)


def experts_of(weights, sparse):
    """the `layers` argument of Decoder.moe_attach: sparse[l] says whether layer l has experts"""
    d = lambda a: torch.from_numpy(a).to(DEV)
    return [dict(router=d(lw["router"]), gate_up=d(lw["e_gate_up"]), down=d(lw["e_down"])) if s else None for lw, s in zip(weights, sparse)]


def moe_engine(llmie, weights, sparse, hs, k, max_tokens, kv8=False, flags=0, int8=False):
    dec = make_engine(llmie, weights, hs, kv8=kv8, int8=int8)
    dec.moe_attach(experts_of(weights, sparse), k, flags=flags, max_tokens=max_tokens)
    return dec


def i32(v):
    return torch.tensor(list(v), dtype=torch.int32, device=DEV)


def run_case(llmie, eng, b):
    """one call of the built case b (moe_engine_ref.build) on engine eng: hidden_out [rows, H] as float32 numpy"""
    case = b["case"]
    hs = case["hs"]
    nh, kvh = geometry(hs)
    x = torch.from_numpy(b["x"]).to(DEV)
    y = torch.empty_like(x)
    k, v = torch.from_numpy(b["k"]).to(DEV), torch.from_numpy(b["v"]).to(DEV)
    bs = k.shape[1]
    max_pages = (MAX_SEQ + 127) // 128
    if case["kind"] == "decode":
        ctx = contexts(case)
        if case["cache"] in ("dense", "e4m3"):
            eng.forward(x, y, k, v, case["step"])
        elif case["cache"] == "ragged":
            eng.forward_ragged(x, y, k, v, i32(ctx))
        else:
            bt = torch.arange(bs * max_pages, dtype=torch.int32, device=DEV).flip(0).reshape(bs, max_pages).contiguous()
            kp = torch.zeros((k.shape[0], bs * max_pages, kvh, 128, hs), dtype=F16, device=DEV)
            vp = torch.zeros_like(kp)
            full = i32(c - 1 for c in ctx)
            llmie.kv_pages_copy(k, kp, bt, full, True)
            llmie.kv_pages_copy(v, vp, bt, full, True)
            eng.forward_paged(x, y, kp, vp, bt, case["step"])
    else:
        lens, hist = case["lens"], case["hist"]
        if case["cache"] == "dense":
            eng.prefill(x, y, k, v, i32(lens), i32(hist), max(lens))
        else:
            bt = torch.from_numpy(np.random.default_rng(2).permutation(bs * max_pages).astype(np.int32)).reshape(bs, max_pages).to(DEV)
            kp = torch.zeros((k.shape[0], bs * max_pages, kvh, 128, hs), dtype=F16, device=DEV)
            vp = torch.zeros_like(kp)
            llmie.kv_pages_copy(k, kp, bt, i32(hist), True)
            llmie.kv_pages_copy(v, vp, bt, i32(hist), True)
            eng.prefill_paged(x, y, kp, vp, bt, i32(lens), i32(hist), max(lens))
    torch.cuda.synchronize()
    return y.float().cpu().numpy()
