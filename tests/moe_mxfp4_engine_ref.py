"""Engine cases of the _ex mixture-of-experts tests (llmie_decoder_moe_attach_ex) and their reference (numpy + the oracle only; read
by test_moe_mxfp4_engine_cpu.py, which asserts what the cases claim, by test_moe_mxfp4_engine_gpu.py and by moe_mxfp4_capture.py).

Cases: the E = 8 cases of moe_engine_ref (decode on dense / paged / ragged / e4m3 caches at 32 and 3 rows, prefill at 5 / 33 / 130
tokens and the three together on dense caches and on pages with history), its stack and window cases -- all with MXFP4 experts, no
bias, plain SwiGLU -- and one decode and one prefill case with the full gpt-oss epilogue: router bias, gate/up and down biases and
the clamped SwiGLU (alpha 1.702, limit 7.0).

Reference: moe_engine_ref.decode / .prefill, the oracle's per-kernel composition, with the expert matrices replaced by the exact
values of their MXFP4 codes (mxfp4_cases.dequantize: every such value is an fp16 number, so the replacement is exact) and the FFN of
a sparse layer computed by moe_mxfp4_cases.ffn on logits + router bias.  Routing stability, the 10 % cap and the experts-ignoring
twin are those of moe_engine_ref; the inputs of a case are redrawn (SALT) until the reference alone meets the cap."""
import numpy as np

import moe_cases as mc
import moe_engine_ref as er
import moe_mxfp4_cases as mq
import mxfp4_cases as mx

ALPHA, LIMIT = 1.702, 7.0


def _case(base, epi=False, id=None):
    return dict(base, id=id or "mx4_" + base["id"], base_id=base["id"], epi=epi)


CASES = [_case(c) for c in er.CASES if c["E"] == 8]
CASES.append(_case(er.BY_ID["decode_ragged_e8_r32"], epi=True, id="mx4_gptoss_decode_r32"))
CASES.append(_case(er.BY_ID["prefill_paged_e8_t168"], epi=True, id="mx4_gptoss_prefill_t168"))
BY_ID = {c["id"]: c for c in CASES}
# inputs redrawn until the reference alone meets the stability cap (at most 10 % unstable rows; a 3-row case has room for none)
SALT = {"mx4_decode_e4m3_e8_r32": "/2"}


def build(case):
    """moe_engine_ref.build on redrawn inputs, plus per sparse layer: e_gate_up_q / e_gate_up_s / e_down_q / e_down_s (codes and scale
    bytes as the device takes them), e_gate_up / e_down replaced by the exact fp16 values of the codes, and the biases of an epilogue case"""
    b = er.build(dict(case, id=case["id"] + SALT.get(case["id"], "")))
    b["case"] = case
    E, H, IE = case["E"], er.H, er.IE
    rng = np.random.default_rng(case["seed"] + 7)
    for lw in b["weights"]:
        gq, gs = mx.quantize(lw["e_gate_up"].reshape(E * 2 * IE, H))
        dq, ds = mx.quantize(lw["e_down"].reshape(E * H, IE))
        lw.update(e_gate_up_q=gq.reshape(E, 2 * IE, H // 2), e_gate_up_s=gs.reshape(E, 2 * IE, H // 32), e_down_q=dq.reshape(E, H, IE // 2),
                  e_down_s=ds.reshape(E, H, IE // 32), e_gate_up=mx.dequantize_f16(gq, gs).reshape(E, 2 * IE, H),
                  e_down=mx.dequantize_f16(dq, ds).reshape(E, H, IE))
        assert np.array_equal(lw["e_gate_up"].astype(np.float64).reshape(E * 2 * IE, H), mx.dequantize(gq, gs))
        assert np.array_equal(lw["e_down"].astype(np.float64).reshape(E * H, IE), mx.dequantize(dq, ds))
        if case["epi"]:
            lw.update(router_bias=(0.5 * rng.standard_normal(E)).astype(np.float16), e_gate_up_bias=(0.25 * rng.standard_normal((E, 2 * IE))).astype(np.float16),
                      e_down_bias=(0.5 * rng.standard_normal((E, H))).astype(np.float16))
    return b


def _ffn(hn2, resid2, lw, sparse, case, rounded, logits):
    """moe_engine_ref._ffn with the FFN of a sparse layer by moe_mxfp4_cases"""
    if not sparse:
        return _dense_ffn(hn2, resid2, lw, sparse, case, rounded, logits)
    epi = case.get("epi", False)
    b = dict(x=hn2, router=lw["router"], resid=resid2, gate_up64=lw["e_gate_up"].astype(np.float64), down64=lw["e_down"].astype(np.float64),
             router_bias=lw["router_bias"] if epi else None, gate_up_bias=lw["e_gate_up_bias"] if epi else None,
             down_bias=lw["e_down_bias"] if epi else None, act=mq.ACT_CLAMPED if epi else mq.ACT_SWIGLU, alpha=ALPHA, limit=LIMIT)
    ids, wts, r = mc.route(hn2, lw["router"], case["k"], r=mq.biased_logits(b))
    logits.append(r)
    return mq.ffn(b, ids, wts, rounded).astype(np.float32)


_dense_ffn = er._ffn


def _run(b, rounded):
    """moe_engine_ref's layer loop with _ffn above in the place of its own"""
    er._ffn = _ffn
    try:
        return (er.decode if b["case"]["kind"] == "decode" else er.prefill)(b, rounded)
    finally:
        er._ffn = _dense_ffn


def dense_twin(b, rounded=True):
    """the same case on an engine that ignored its experts (every layer dense)"""
    return _run(dict(b, case=dict(b["case"], sparse=tuple(False for _ in b["case"]["sparse"]))), rounded)[0]


_done = {}


def reference(case):
    """(operands, rounded hidden_out, unrounded hidden_out, stable rows [rows] bool), computed once per case"""
    if case["id"] not in _done:
        b = build(case)
        y64, la = _run(b, False)
        y16, lb = _run(b, True)
        _done[case["id"]] = (b, y16, y64, er.stable_rows(la, lb, case["k"]))
    return _done[case["id"]]
