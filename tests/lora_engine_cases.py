"""Shared by tests/test_lora_engine_gpu.py and tests/lora_capture.py: a small engine, three adapters and the merged weights
fp16(W + scale B A) a second engine without a table runs for each of them."""
import numpy as np
import torch

DEV, F16 = "cuda", torch.float16
NH, KVH, INTER, LAYERS, MAX_SEQ, MAX_BATCH = 4, 2, 704, 2, 384, 8
MODULES = ("qkv", "o", "gate_up", "down")
# three adapters: ranks 8 / 16 / 64; the second carries only q and v (a zero k block, no o / gate_up / down)
ADAPTERS = ((8, 1.0, MODULES), (16, 4.0, ("q", "v")), (64, 0.5, MODULES))
GAIN = 0.5   # B ~ GAIN N(0, 1/rank): delta W about GAIN / 1.15 of W's own spread


def shapes(hs):
    H = NH * hs
    return H, dict(qkv=((NH * hs, KVH * hs, KVH * hs), H), o=((H,), H), gate_up=((INTER, INTER), H), down=((H,), INTER))


def base_weights(hs, seed=5):
    rng = np.random.default_rng(seed)
    H, shp = shapes(hs)
    u = lambda shape, s: (rng.uniform(-1, 1, shape) * s).astype(np.float16)
    return [dict(attn_norm=u((H,), 0.2) + np.float16(1), ffn_norm=u((H,), 0.2) + np.float16(1),
                 **{m: u((sum(w), K), 2 / np.sqrt(K)) for m, (w, K) in shp.items()}) for _ in range(LAYERS)]


def adapters(hs, seed=9):
    """per adapter, per layer, per module: (A [blocks * rank, K], B [N, rank]) fp16, or None"""
    rng = np.random.default_rng(seed)
    _, shp = shapes(hs)
    out = []
    for rank, scale, mods in ADAPTERS:
        layers = []
        for _ in range(LAYERS):
            lw = {}
            for m, (w, K) in shp.items():
                A = (rng.standard_normal((len(w) * rank, K)) / np.sqrt(K)).astype(np.float16)
                B = (GAIN * rng.standard_normal((sum(w), rank)) / np.sqrt(rank)).astype(np.float16)
                if m in mods:
                    lw[m] = (A, B)
                elif m == "qkv" and "q" in mods:   # q and v only: the k block of A and B is zero
                    A[rank:2 * rank] = 0
                    B[w[0]:w[0] + w[1]] = 0
                    lw[m] = (A, B)
            layers.append(lw)
        out.append(dict(rank=rank, scale=scale, layers=layers))
    return out


def merged_weights(base, adapter, hs):
    """fp16(W + scale B A) per module, the column blocks each with their rows of A"""
    _, shp = shapes(hs)
    out = []
    for lw, al in zip(base, adapter["layers"]):
        new = dict(lw)
        for m, ab in al.items():
            w, K = shp[m]
            A, B = ab[0].astype(np.float64), ab[1].astype(np.float64)
            r, delta, c0 = adapter["rank"], np.zeros((sum(w), K)), 0
            for j, wj in enumerate(w):
                delta[c0:c0 + wj] = B[c0:c0 + wj] @ A[j * r:(j + 1) * r]
                c0 += wj
            new[m] = (lw[m].astype(np.float64) + adapter["scale"] * delta).astype(np.float16)
        out.append(new)
    return out


def make_engine(llmie, weights, hs, int8, fmt=None, flags=0, kv8=False):
    """fmt: None (fp16, or int8 where `int8`), "fp8" or "f32"; flags: LLMIE_DEC_*; kv8: an e4m3 KV cache"""
    d = lambda a: torch.from_numpy(a).to(DEV)
    layers = []
    for lw in weights:
        e = dict(attn_norm=d(lw["attn_norm"]), ffn_norm=d(lw["ffn_norm"]))
        for m in MODULES:
            w = d(lw[m])
            if fmt == "fp8":
                wq, sc = torch.empty(w.shape, dtype=torch.uint8, device=DEV), torch.empty(w.shape[0], dtype=torch.float32, device=DEV)
                llmie.quantize_fp8(w, wq, sc)
                e[m] = dict(data=wq, scale=sc)
            elif fmt == "f32":
                e[m] = dict(data=w.float())
            elif int8:
                wq, sc = torch.empty(w.shape, dtype=torch.int8, device=DEV), torch.empty(w.shape[0], dtype=F16, device=DEV)
                llmie.quantize_w8(w, wq, sc)
                e[m] = dict(data=wq, scale=sc)
            else:
                e[m] = dict(data=w)
        if fmt == "f32":
            e["attn_norm"], e["ffn_norm"] = e["attn_norm"].float(), e["ffn_norm"].float()
        layers.append(e)
    wfmt = {"fp8": llmie.W_FP8, "f32": llmie.W_F32}.get(fmt, llmie.W_INT8 if int8 else llmie.W_F16)
    cfg = dict(head_num=NH, kv_head_num=KVH, head_size=hs, inter_size=INTER, num_layers=LAYERS, vocab_size=100, max_seq_len=MAX_SEQ,
               max_batch=MAX_BATCH, rotary_dim=hs, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F32 if fmt == "f32" else llmie.F16,
               wfmt=wfmt, int4_group=128, flags=flags, kv_fmt=llmie.KV_FP8 if kv8 else llmie.KV_NATIVE, k_scale=1 / 32, v_scale=1 / 16)
    return llmie.Decoder(cfg, layers)


def load_slot(llmie, table, slot, adapter):
    d = lambda a: torch.from_numpy(a).to(DEV)
    llmie.lora_slot_load(table, slot, [{m: (d(ab[0]), d(ab[1])) for m, ab in lw.items()} for lw in adapter["layers"]], scale=adapter["scale"])


def lora_engine(llmie, base, ads, hs, int8, max_tokens, slots=4, kv8=False):
    """(engine with the table attached, table, seq_slot [MAX_BATCH] on the device): slot i holds adapter i, the last slot is empty"""
    dec = make_engine(llmie, base, hs, int8, kv8=kv8)
    table = llmie.lora_table(slots, LAYERS)
    for i, ad in enumerate(ads):
        load_slot(llmie, table, i, ad)
    seq_slot = torch.full((MAX_BATCH,), -1, dtype=torch.int32, device=DEV)
    dec.lora_attach(table, seq_slot, max_tokens=max_tokens)
    return dec, table, seq_slot
