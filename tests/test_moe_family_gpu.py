"""Recorded results of the mixture-of-experts family: the operator entries and an engine with experts give, bit for bit, what they
gave when golden/moe_family.json was recorded (`python tests/test_moe_family_gpu.py --record` on the GPU, at the commit whose
behaviour is to be kept; a case enters the file only after a second process has reproduced its hash).  Every output element of
moe.hip is computed by one lane chain (its header says why), so bit equality is the bar.  test_moe_ffn_gpu.py and
test_moe_mxfp4_gpu.py hold the kernels to their references; this one holds the shell around them -- which instantiation, grid,
workspace section and operand reaches which launch -- so that the host side of the family can be rearranged without a silent swap.

Operator level: (hidden, inter) with each of the two at the GEMV kernels' four chunk counts (64, 2112, 4160, 8256), as fp16 experts,
fp16 experts with the three biases under the clamped act, and MXFP4 experts with the same epilogue; rows 1 and 4 (GEMV), 5 and 17
(fp16: grouped RT 1; MXFP4: GEMV up to 16 rows), 16 under LLMIE_MOE_FORCE_GEMV, 4 under LLMIE_MOE_FORCE_GROUPED, and 80 rows on 4
experts with top_k 2 (40 pairs per expert: RT 4); with and without a residual; LLMIE_MOE_SOFTMAX_ALL once per format; the route
entries by their expert ids and weights.  The plan line of each case is stored with its hash, so a plan that moves reads as such.
Engine level: one 2-layer model (layer 0 sparse, layer 1 dense; 4 heads of 128 on 2 KV heads, inter 192, 8 experts, top_k 2) with
fp16 experts through llmie_decoder_moe_attach and with MXFP4 experts, biases and the clamped act through _attach_ex: decode at batch
1, 4, 5 and 17, prefill of 33 and 80 tokens, the KV caches of the smallest case, and the launches per op kind that
llmie_decoder_profile_end counts for one decode step and one prefill.  Also every refusal of the two attach entries on a live
engine, by code and whole text (test_moe_refusals_cpu.py has no engine to ask).
Inputs come from one seeded numpy generator and the device quantiser; the file stores their checksum."""
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
GOLDEN = os.path.join(ROOT, "tests", "golden", "moe_family.json")
DEV, F16 = "cuda", torch.float16
SOFTMAX_ALL, FORCE_GEMV, FORCE_GROUPED = 1, 2, 4
ALPHA, LIMIT = 1.702, 7.0
# (hidden, inter, experts, top_k): 4 experts with top_k 1 where a dimension is wide
GEOMETRIES = [(64, 64, 8, 2), (2112, 64, 4, 1), (64, 2112, 4, 1), (4160, 64, 4, 1), (64, 4160, 4, 1), (8256, 64, 4, 1), (64, 8256, 4, 1)]
RT4 = (256, 192, 4, 2)
VARIANTS = ("f16", "f16_epi", "mxfp4_epi")
# (rows, flags, with a residual)
CALLS = [(1, 0, False), (4, 0, True), (5, 0, False), (17, 0, True), (16, FORCE_GEMV, True), (4, FORCE_GROUPED, False)]
MAX_ROWS = 80
NH, KVH, HS, INTER, LAYERS, MAX_BATCH, MAX_SEQ, STEP, E_ENG, K_ENG = 4, 2, 128, 192, 2, 17, 256, 131, 8, 2
H_ENG, QKV_ENG = NH * HS, (NH + 2 * KVH) * HS
DECODE, PREFILL = (1, 4, 5, 17), (33, 80)
ENGINES = ("f16", "mxfp4_epi")


def _gid(g):
    return "%dx%d" % g[:2]


class Inputs:
    def __init__(self):
        rng = np.random.default_rng(20261021)
        u = lambda shape, s: (rng.uniform(-1, 1, shape) * s).astype(np.float16)
        n = lambda shape, s: (rng.standard_normal(shape) * s).astype(np.float16)
        experts = lambda Hh, Ie, E: dict(router=u((E, Hh), 4 / np.sqrt(Hh)), gate_up=u((E, 2 * Ie, Hh), 2 / np.sqrt(Hh)),
                                         down=u((E, Hh, Ie), 2 / np.sqrt(Ie)), router_bias=u((E,), 0.5), gate_up_bias=u((E, 2 * Ie), 0.5),
                                         down_bias=u((E, Hh), 0.5))
        self.ops = {}
        for g in GEOMETRIES + [RT4]:
            Hh, Ie, E, _ = g
            self.ops[_gid(g)] = dict(experts(Hh, Ie, E), x=n((MAX_ROWS, Hh), 1.0), resid=n((MAX_ROWS, Hh), 1.0))
        shapes = dict(qkv=(QKV_ENG, H_ENG), o=(H_ENG, H_ENG), gate_up=(2 * INTER, H_ENG), down=(H_ENG, INTER))
        self.layers = [dict(attn_norm=u((H_ENG,), 0.2) + np.float16(1), ffn_norm=u((H_ENG,), 0.2) + np.float16(1),
                            **{m: u(s, 2 / np.sqrt(s[1])) for m, s in shapes.items()}) for _ in range(LAYERS)]
        self.experts = experts(H_ENG, INTER, E_ENG)
        self.hidden = n((max(PREFILL), H_ENG), 1.0)
        self.k = n((LAYERS, MAX_BATCH, KVH, MAX_SEQ, HS), 0.5)
        self.v = n((LAYERS, MAX_BATCH, KVH, MAX_SEQ, HS), 0.5)
        h = hashlib.sha256()
        for d in list(self.ops.values()) + self.layers + [self.experts]:
            for name in sorted(d):
                h.update(d[name].tobytes())
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


def descriptor(llmie, w, variant):
    """MoeExperts of one variant from a dict of fp16 arrays"""
    d = {n: _dev(a) for n, a in w.items() if n not in ("x", "resid")}
    epi = {}
    if variant.endswith("_epi"):
        epi = dict(router_bias=d["router_bias"], gate_up_bias=d["gate_up_bias"], down_bias=d["down_bias"], act=llmie.MOE_ACT_SWIGLU_CLAMPED,
                   alpha=ALPHA, limit=LIMIT)
    if variant.startswith("mxfp4"):
        return llmie.MoeExperts.quantize(d["router"], d["gate_up"], d["down"], **epi)
    return llmie.MoeExperts(d["router"], d["gate_up"], d["down"], **epi)


def operator_calls(g):
    if g == RT4:
        return [(v, 80, 0, v == "f16") for v in VARIANTS]
    calls = [(v,) + c for v in VARIANTS for c in CALLS]
    if g == GEOMETRIES[0]:
        calls += [("f16", 5, SOFTMAX_ALL, False), ("mxfp4_epi", 5, SOFTMAX_ALL, True)]
    return calls


def run_operator(llmie, inp, g):
    """{case id: dict(plan, y)} of one geometry"""
    Hh, Ie, E, k = g
    w = inp.ops[_gid(g)]
    x, resid = _dev(w["x"]), _dev(w["resid"])
    out = {}
    ex = {v: descriptor(llmie, w, v) for v in VARIANTS}
    for v, rows, flags, with_resid in operator_calls(g):
        xs = x[:rows].contiguous()
        y = torch.full_like(xs, 7.0)
        r = resid[:rows].contiguous() if with_resid else None
        if v == "f16":   # the plain entry
            llmie.moe_ffn(xs, ex[v].router, ex[v].gate_up, ex[v].down, y, k, resid=r, flags=flags)
        else:
            llmie.moe_ffn_ex(xs, ex[v], y, k, resid=r, flags=flags)
        plan = llmie.moe_ffn_plan_ex(rows, Hh, Ie, E, k, flags, ex[v].format, ex[v].act)
        out["op:%s:%s:r%d:f%d:%s" % (_gid(g), v, rows, flags, "resid" if with_resid else "plain")] = dict(plan=plan, y=_sha(y))
    return out


def run_routes(llmie, inp):
    out = {}
    for g in (GEOMETRIES[0], GEOMETRIES[1], RT4):
        Hh, Ie, E, k = g
        w = inp.ops[_gid(g)]
        ex = descriptor(llmie, w, "f16_epi")
        for rows in (1, 5, 17, 80):
            for flags in (0, SOFTMAX_ALL):
                xs = _dev(w["x"][:rows])
                out["route:%s:r%d:f%d" % (_gid(g), rows, flags)] = _sha(*llmie.moe_route(xs, ex.router, k, flags))
                out["route_ex:%s:r%d:f%d" % (_gid(g), rows, flags)] = _sha(*llmie.moe_route_ex(xs, ex, k, flags))
    return out


def engine(llmie, inp, name):
    layers = [{m: _dev(a) for m, a in lw.items()} for lw in inp.layers]
    cfg = dict(head_num=NH, kv_head_num=KVH, head_size=HS, inter_size=INTER, num_layers=LAYERS, vocab_size=100, max_seq_len=MAX_SEQ,
               max_batch=MAX_BATCH, rotary_dim=HS, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16, wfmt=llmie.W_F16, int4_group=128)
    dec = llmie.Decoder(cfg, layers)
    if name == "f16":   # tuples: llmie_decoder_moe_attach
        w = {m: _dev(inp.experts[m]) for m in ("router", "gate_up", "down")}
        dec.moe_attach([(w["router"], w["gate_up"], w["down"]), None], K_ENG, max_tokens=max(PREFILL))
    else:
        dec.moe_attach([descriptor(llmie, inp.experts, name), None], K_ENG, max_tokens=max(PREFILL))
    return dec


def run_engine(llmie, inp, name):
    dec = engine(llmie, inp, name)
    hidden, k, v = _dev(inp.hidden), _dev(inp.k), _dev(inp.v)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
    out = {}
    for kind, sizes in (("decode", DECODE), ("prefill", PREFILL)):
        for rows in sizes:
            x = hidden[:rows].contiguous()
            y = torch.full_like(x, 7.0)
            seqs = rows if kind == "decode" else 1
            kd, vd = k[:, :seqs].contiguous(), v[:, :seqs].contiguous()
            first = rows == sizes[0]
            if first:
                dec.profile_begin(256)
            if kind == "decode":
                dec.forward(x, y, kd, vd, STEP)
            else:
                dec.prefill(x, y, kd, vd, i32([rows]), i32([0]), rows)
            res = dict(hidden=_sha(y))
            if first:
                res["launches_by_op"] = {op: n for op, (_, n) in dec.profile_end().items()}
                res["kv"] = _sha(kd, vd)
            out["engine:%s:%s:%d" % (name, kind, rows)] = res
    dec.close()
    return out


# ---- the attach entries on a live engine: [rc, whole text] of one broken rule each, and of pairs that say which check comes first ----
FAKE = 4096
ATTACH_BASE = dict(layers=True, Ie=INTER, E=E_ENG, k=K_ENG, flags=0, ws=0, short=0, lora=False, l0={}, l1=None)
ATTACH_COMMON = [dict(layers=None), dict(ws=None), dict(Ie=0), dict(E=0), dict(k=-1), dict(lora=True)]
ATTACH_CALL = [dict(E=129), dict(E=4, k=5), dict(E=16, k=9), dict(Ie=100), dict(flags=2 | 4), dict(flags=64), dict(flags=8 | 16)]
ATTACH_WS = [dict(short=1), dict(ws=16)]
ATTACH_RULES = {
    "decoder_moe_attach": ATTACH_COMMON + ATTACH_CALL +
    [dict(l0=dict(gate_up=None)), dict(l0=dict(down=None)), dict(l0=dict(router=FAKE + 8)), dict(l1=dict(down=FAKE + 2)), dict(l0=None)] + ATTACH_WS +
    [dict(E=129, short=1), dict(flags=64, l0=dict(router=FAKE + 8)), dict(Ie=100, l0=None), dict(l0=dict(gate_up=None), short=1), dict(lora=True, E=129)],
    "decoder_moe_attach_ex": ATTACH_COMMON +
    [dict(l0=dict(format=1)), dict(l0=dict(gate_up=None)), dict(l0=dict(format=5)), dict(l0=dict(gate_up_scale=FAKE)), dict(l0=dict(act=2)),
     dict(l0=dict(act=1, alpha=ALPHA, limit=-1.0)), dict(l0=dict(down=FAKE + 4)), dict(l0=dict(down_bias=FAKE + 1)), dict(l1=dict(act=1, alpha=ALPHA, limit=LIMIT)),
     dict(l1=dict(format=5, gate_up_scale=FAKE, down_scale=FAKE)), dict(l0=None)] + ATTACH_CALL + ATTACH_WS +
    [dict(l0=dict(format=1), E=129), dict(l0=None, E=129), dict(E=129, short=1), dict(l0=dict(act=2), l1=dict(format=5, gate_up_scale=FAKE, down_scale=FAKE)),
     dict(lora=True, l0=dict(format=1))],
}


def _attach_name(entry, kw):
    return "%s:%s" % (entry, ",".join("%s=%s" % (n, kw[n]) for n in sorted(kw)))


def run_attach_refusals(llmie, inp):
    """fake expert pointers: every call is refused before the engine keeps anything"""
    lib = llmie.lib()
    dec = engine(llmie, inp, "f16")
    dec.moe_detach()
    need = dec.moe_workspace_bytes(MAX_BATCH, INTER, E_ENG, K_ENG)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    table = llmie.lora_table(2, LAYERS)
    seq_slot = torch.full((MAX_BATCH,), -1, dtype=torch.int32, device=DEV)
    out = {}
    for entry, rules in ATTACH_RULES.items():
        ex = entry.endswith("_ex")
        for kw in rules:
            a = dict(ATTACH_BASE, **kw)
            arr = ((llmie.MoeExpertsDesc if ex else llmie.MoeLayer) * LAYERS)()
            for i, lw in enumerate((a["l0"], a["l1"])):
                if lw is not None:   # a sparse layer: fp16 experts at fake addresses, then the case's fields
                    arr[i].router, arr[i].gate_up, arr[i].down = FAKE, FAKE, FAKE
                    for n, val in lw.items():
                        setattr(arr[i], n, val)
            if a["lora"]:
                dec.lora_attach(table, seq_slot)
            fn = lib.llmie_decoder_moe_attach_ex if ex else lib.llmie_decoder_moe_attach
            rc = fn(dec.handle, arr if a["layers"] else None, a["Ie"], a["E"], a["k"], a["flags"], None if a["ws"] is None else ws.data_ptr() + a["ws"],
                    need - a["short"])
            out[_attach_name(entry, kw)] = [rc, lib.llmie_last_error().decode()]
            if a["lora"]:
                dec.lora_detach()
    dec.close()
    return out


def run_all(llmie, inp):
    rec = {}
    for g in GEOMETRIES + [RT4]:
        rec.update(run_operator(llmie, inp, g))
    rec.update(run_routes(llmie, inp))
    for name in ENGINES:
        rec.update(run_engine(llmie, inp, name))
    rec.update(run_attach_refusals(llmie, inp))
    return rec


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def inputs():
    return Inputs()


def _same(got, recorded, prefix):
    exp = {cid: c for cid, c in recorded["cases"].items() if cid.startswith(prefix)}
    wrong = [cid for cid in exp if got.get(cid) != exp[cid]]
    assert exp and sorted(got) == sorted(exp) and not wrong, "%d of %d cases differ: %s" % (len(wrong), len(exp), wrong)


def test_inputs_are_the_recorded_ones(recorded, inputs):
    assert inputs.sha256 == recorded["inputs"]


def test_the_recording_reaches_every_route_and_tile_height(recorded):
    plans = [c["plan"] for cid, c in recorded["cases"].items() if cid.startswith("op:")]
    for fmt in ("format=f16", "format=mxfp4"):
        for route in ("route=gemv", "route=grouped rt=1", "route=grouped rt=4"):
            assert any(route in p and fmt in p for p in plans), (fmt, route)
    # the GEMV kernels' chunk counts on both sides: a gate/up grid over 4 inter columns blocks = inter 64 beside every hidden, and back
    for g in GEOMETRIES:
        for v in VARIANTS:
            assert any(cid.startswith("op:%s:%s:r1:" % (_gid(g), v)) and "route=gemv" in c["plan"] for cid, c in recorded["cases"].items()), (g, v)
    refusals = [c for cid, c in recorded["cases"].items() if cid.startswith("decoder_moe_attach")]
    assert len(refusals) == sum(len(r) for r in ATTACH_RULES.values()) and all(rc in (-1, -2, -4) for rc, _ in refusals)
    assert {rc for rc, _ in refusals} == {-1, -2, -4}


@pytest.mark.parametrize("g", GEOMETRIES + [RT4], ids=_gid)
def test_operator_reproduces_the_recording(llmie, recorded, inputs, g):
    _same(run_operator(llmie, inputs, g), recorded, "op:%s:" % _gid(g))


def test_route_entries_reproduce_the_recording(llmie, recorded, inputs):
    _same(run_routes(llmie, inputs), recorded, "route")


@pytest.mark.parametrize("name", ENGINES)
def test_engine_reproduces_the_recording(llmie, recorded, inputs, name):
    _same(run_engine(llmie, inputs, name), recorded, "engine:%s:" % name)


def test_attach_refusals_are_the_recorded_ones(llmie, recorded, inputs):
    _same(run_attach_refusals(llmie, inputs), recorded, "decoder_moe_attach")


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from conftest import load_llmie
    mod = load_llmie()
    if sys.argv[1:] not in (["--record"], ["--run"]):
        sys.exit("usage: python tests/test_moe_family_gpu.py --record")
    inp = Inputs()
    rec = run_all(mod, inp)
    if sys.argv[1:] == ["--run"]:   # the second process of a recording: the results as JSON on the last line
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
