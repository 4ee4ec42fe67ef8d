"""Recorded results of the engine's projections: a decode step and a prefill pass give, bit for bit, what they gave when
golden/projection_family.json was recorded (`python tests/test_projection_family_gpu.py --record` on the GPU, at the commit whose
behaviour is to be kept; a case enters the file only after a second process has reproduced its hashes).  test_exact_linear_gpu.py
holds every kernel route to an exact answer; this one holds the shell around the kernels -- which operand, scratch area and epilogue
flag reaches which launch in every sequence of the engine -- so that the host side of the projection family can be rearranged
without a silent swap.

One 2-layer model (4 heads of 128 on 2 KV heads, inter_size 768: H = 512, QKV = 1024; max_batch 130, max_seq_len 256) as eight
engines: fp16, int8, int4 (group 128), fp8 and MXFP4 weights, an int8 LLMIE_DEC_PACKED_ONLY engine (max_batch 32: its limit), an fp16
engine with an O bias and an fp16 engine with an adapter attached.  The cases are chosen by the planners, on the host: the smallest
batch at which llmie_decoder_plan_name gives each decode sequence, and the smallest token count at which
llmie_decoder_prefill_layer_plan gives each plan text (every count up to 1100, then the multiples of 128 and the counts one above
them, where the row tiles and split-K passes change, up to what the engine holds).  The recorded file names each case's rows and plan,
so a plan that moves reads as "the cases differ".  Stored: a SHA-256 of hidden_out per case, and of both KV caches for the smallest
decode and prefill case of each engine.  Inputs come from one seeded numpy generator and the device quantisers; the file stores their
checksum, so a changed generator reads as "inputs differ" and not as a failure of the code."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "projection_family.json")
DEV, F16 = "cuda", torch.float16
NH, KVH, HS, INTER, LAYERS, MAX_BATCH, MAX_SEQ, STEP = 4, 2, 128, 768, 2, 130, 256, 131
H, QKV = NH * HS, (NH + 2 * KVH) * HS
SHAPES = dict(qkv=(QKV, H), o=(H, H), gate_up=(2 * INTER, H), down=(H, INTER))
HIDDEN_ROWS, KV_SEQS, LORA_RANK, LORA_ROWS = 4096, 8, 8, 300
PLAN_O_BIAS, PLAN_LORA = 32, 1024
# Row counts every engine runs beside the planners' choices: the plan texts do not name the kernel route of a projection, and these
# move it inside one sequence (past the GEMVs' 8 rows, past 64 rows, the split-K passes from 129 rows, the mid-sized tile grids)
EXTRA_ROWS = (9, 70, 130, 300)
# name -> (weight format, engine flags, max_batch, O bias, adapter)
ENGINES = {"f16": ("f16", 0, MAX_BATCH, False, False), "int8": ("int8", 0, MAX_BATCH, False, False), "int4": ("int4", 0, MAX_BATCH, False, False),
           "fp8": ("fp8", 0, MAX_BATCH, False, False), "mxfp4": ("mxfp4", 0, MAX_BATCH, False, False),
           "int8_packed_only": ("int8", 2, 32, False, False), "f16_o_bias": ("f16", 0, MAX_BATCH, True, False),
           "f16_lora": ("f16", 0, MAX_BATCH, False, True)}


class Inputs:
    def __init__(self):
        rng = np.random.default_rng(20261020)
        u = lambda shape, s: (rng.uniform(-1, 1, shape) * s).astype(np.float16)
        self.layers = [dict(attn_norm=u((H,), 0.2) + np.float16(1), ffn_norm=u((H,), 0.2) + np.float16(1), o_bias=u((H,), 0.1),
                            **{m: u(s, 2 / np.sqrt(s[1])) for m, s in SHAPES.items()}) for _ in range(LAYERS)]
        blocks = dict(qkv=3, o=1, gate_up=2, down=1)
        self.lora = [{m: ((rng.standard_normal((blocks[m] * LORA_RANK, s[1])) / np.sqrt(s[1])).astype(np.float16),
                          (0.5 * rng.standard_normal((s[0], LORA_RANK)) / np.sqrt(LORA_RANK)).astype(np.float16)) for m, s in SHAPES.items()}
                     for _ in range(LAYERS)]
        self.hidden = rng.standard_normal((HIDDEN_ROWS, H)).astype(np.float16)
        self.k = (rng.standard_normal((LAYERS, KV_SEQS, KVH, MAX_SEQ, HS)) * 0.5).astype(np.float16)
        self.v = (rng.standard_normal((LAYERS, KV_SEQS, KVH, MAX_SEQ, HS)) * 0.5).astype(np.float16)
        h = hashlib.sha256()
        for lw, ad in zip(self.layers, self.lora):
            for name in sorted(lw):
                h.update(lw[name].tobytes())
            for name in sorted(ad):
                h.update(ad[name][0].tobytes() + ad[name][1].tobytes())
        for a in (self.hidden, self.k, self.v):
            h.update(a.tobytes())
        self.sha256 = h.hexdigest()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _sha(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _quantised(llmie, w, fmt):
    n, k = w.shape
    e = lambda shape, dt: torch.empty(shape, dtype=dt, device=DEV)
    if fmt == "f16":
        return dict(data=w)
    if fmt == "int8":
        wq, sc = e((n, k), torch.int8), e((n,), F16)
        llmie.quantize_w8(w, wq, sc)
    elif fmt == "int4":
        wq, sc = e((n, k // 2), torch.uint8), e((n, k // 128), F16)
        llmie.quantize_w4(w, wq, sc, 128)
    elif fmt == "fp8":
        wq, sc = e((n, k), torch.uint8), e((n,), torch.float32)
        llmie.quantize_fp8(w, wq, sc)
    else:
        wq, sc = e((n, k // 2), torch.uint8), e((n, k // 32), torch.uint8)
        llmie.quantize_mxfp4(w, wq, sc)
    return dict(data=wq, scale=sc)


def config(llmie, name):
    fmt, flags, max_batch, _, _ = ENGINES[name]
    wfmt = dict(f16=llmie.W_F16, int8=llmie.W_INT8, int4=llmie.W_INT4, fp8=llmie.W_FP8, mxfp4=llmie.W_MXFP4)[fmt]
    return dict(head_num=NH, kv_head_num=KVH, head_size=HS, inter_size=INTER, num_layers=LAYERS, vocab_size=100, max_seq_len=MAX_SEQ,
                max_batch=max_batch, rotary_dim=HS, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=wfmt,
                int4_group=0 if fmt == "mxfp4" else 128, flags=flags)


def engine(llmie, inp, name):
    fmt, _, _, o_bias, lora = ENGINES[name]
    layers = []
    for lw in inp.layers:
        e = dict(attn_norm=_dev(lw["attn_norm"]), ffn_norm=_dev(lw["ffn_norm"]))
        for m in SHAPES:
            e[m] = _quantised(llmie, _dev(lw[m]), fmt)
        if o_bias:
            e["o"]["bias"] = _dev(lw["o_bias"])
        layers.append(e)
    dec = llmie.Decoder(config(llmie, name), layers)
    if lora:
        table = llmie.lora_table(2, LAYERS)
        llmie.lora_slot_load(table, 0, [{m: (_dev(ab[0]), _dev(ab[1])) for m, ab in ad.items()} for ad in inp.lora], scale=1.0)
        slots = torch.zeros(MAX_BATCH, dtype=torch.int32, device=DEV)
        slots[1::3] = -1                               # every third row / sequence has no adapter
        dec.lora_attach(table, slots, max_tokens=LORA_ROWS)
    return dec


def _lens(T):
    n = -(-T // MAX_SEQ)
    return [MAX_SEQ] * (n - 1) + [T - MAX_SEQ * (n - 1)]


def cases(llmie, name):
    """{case id: dict(kind, rows, plan, kv)} of one engine, chosen on the host by the planners"""
    _, _, max_batch, o_bias, lora = ENGINES[name]
    cfg = config(llmie, name)
    flags = (PLAN_O_BIAS if o_bias else 0) | (PLAN_LORA if lora else 0)
    out, seen = {}, set()
    for b in range(1, max_batch + 1):
        plan = llmie.decoder_plan_name(cfg, False, b, flags)
        if plan is not None and (plan not in seen or b in EXTRA_ROWS):
            seen.add(plan)
            out["%s:decode:%s@%d" % (name, plan, b)] = dict(kind="decode", rows=b, plan=plan, kv=not out)
    top = LORA_ROWS if lora else max_batch * MAX_SEQ
    counts = list(range(1, min(top, 1100) + 1)) + [t + d for t in range(1152, top, 128) for d in (0, 1)]
    first = True
    for T in counts:
        lens = _lens(T)
        plan, _ = llmie.decoder_prefill_layer_plan(cfg, T, len(lens), max(lens), flags)
        if plan is not None:   # the forms the projections take: not the attention launch, whose grid grows with every tile
            plan = " ".join(w for w in plan.split(" launches")[0].split(" ") if w.split("=")[0] not in ("attn", "kv", "grid", "rope_append"))
        if plan is not None and (plan not in seen or T in EXTRA_ROWS):
            seen.add(plan)
            out["%s:prefill:%d" % (name, T)] = dict(kind="prefill", rows=T, plan=plan, kv=first)
            first = False
    return out


def run_case(dec, inp_dev, case):
    hidden, k, v = inp_dev
    rows = case["rows"]
    x = hidden[torch.arange(rows, device=DEV) % HIDDEN_ROWS].contiguous()
    out = torch.full_like(x, 7.0)
    seqs = rows if case["kind"] == "decode" else len(_lens(rows))
    idx = torch.arange(seqs, device=DEV) % KV_SEQS
    kd, vd = k[:, idx].contiguous(), v[:, idx].contiguous()
    try:
        if case["kind"] == "decode":
            dec.forward(x, out, kd, vd, STEP)
        else:
            lens = _lens(rows)
            dec.prefill(x, out, kd, vd, torch.tensor(lens, dtype=torch.int32, device=DEV),
                        torch.zeros(len(lens), dtype=torch.int32, device=DEV), max(lens))
    except Exception as e:   # a call the engine refuses is recorded by the whole text of its refusal
        return dict(rows=rows, plan=case["plan"], refused=str(e))
    res = dict(rows=rows, plan=case["plan"], hidden=_sha(out))
    if case["kv"]:
        res["kv"] = _sha(kd, vd)
    return res


def run_engine(llmie, inp, name):
    dec = engine(llmie, inp, name)
    inp_dev = (_dev(inp.hidden), _dev(inp.k), _dev(inp.v))
    got = {cid: run_case(dec, inp_dev, case) for cid, case in cases(llmie, name).items()}
    dec.close()
    return got


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def inputs():
    return Inputs()


def test_inputs_are_the_recorded_ones(recorded, inputs):
    assert inputs.sha256 == recorded["inputs"]


def test_the_planners_choose_the_recorded_cases(llmie, recorded):
    for name in ENGINES:
        exp = {cid: (c["rows"], c["plan"]) for cid, c in recorded["cases"].items() if cid.startswith(name + ":")}
        assert {cid: (c["rows"], c["plan"]) for cid, c in cases(llmie, name).items()} == exp, name
    kinds = {c["plan"].split(" ")[0] for c in recorded["cases"].values()}
    assert {"gemv", "packed", "splitk", "unfused", "lora", "short_splitk", "lean", "general", "packed_only"} <= kinds, kinds
    fp8 = " ".join(c["plan"] for cid, c in recorded["cases"].items() if cid.startswith("fp8:prefill:"))
    for form in ("attn_norm=quant", "qkv=rope_e4m3", "gate_up=two_launch", "gate_up=e4m3_swiglu"):
        assert form in fp8, form


@pytest.mark.parametrize("name", sorted(ENGINES))
def test_engine_reproduces_the_recording(llmie, recorded, inputs, name):
    got = run_engine(llmie, inputs, name)
    exp = {cid: c for cid, c in recorded["cases"].items() if cid.startswith(name + ":")}
    wrong = [cid for cid in exp if got.get(cid) != exp[cid]]
    assert sorted(got) == sorted(exp) and not wrong, "%d of %d cases differ: %s" % (len(wrong), len(exp), wrong)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from conftest import load_llmie
    mod = load_llmie()
    if sys.argv[1:] not in (["--record"], ["--run"]):
        sys.exit("usage: python tests/test_projection_family_gpu.py --record")
    inp, rec = Inputs(), {}
    for eng in ENGINES:
        rec.update(run_engine(mod, inp, eng))
        print("%s: %d cases so far" % (eng, len(rec)), file=sys.stderr, flush=True)
    if sys.argv[1:] == ["--run"]:   # the second process of a recording: every engine's results as JSON on the last line
        print(json.dumps(rec, sort_keys=True))
        sys.exit(0)
    again = json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--run"], check=True, stdout=subprocess.PIPE, text=True,
                                      timeout=400).stdout.strip().splitlines()[-1])
    unstable = [cid for cid in rec if rec[cid] != again.get(cid)]
    if unstable:
        sys.exit("NOT recorded: these cases did not reproduce in a second process: %s" % unstable)
    with open(GOLDEN, "w") as f:
        json.dump(dict(inputs=inp.sha256, cases=rec), f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d cases" % len(rec))
