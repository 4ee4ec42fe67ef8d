"""The inputs of tests/test_model_params_gpu.py can fail, shown without a GPU.

1. layer_restatement (float64 numpy, tests/model_param_cases.py) equals orc.self_decoder / orc.context_decoder to 1e-5 relative at
   P0, P1 and P2 on a small-geometry stand-in of every engine case -- so the defect experiments below are about the oracle's
   semantics, not a private formula.
2. Each seeded defect (a switch of the restatement) moves at least one checked quantity -- the hidden output, the appended K rows,
   the appended V rows, measured as the GPU file measures them -- of every case by at least 10 x that case's project bound:
     at P1, every eps and every RoPE defect on every case;
     at P2, every RoPE defect on the cases the GPU file runs there.  With unit rows P2 is a RoPE-only point: its eps of 1e-6 is
     1.5e-6 of a unit row's mean square, below fp16 resolution.  Under the row gains it is not: on the 2^-9 rows (mean square 1.3e-6)
     eps omitted in the attention norm, added to the sum, or fixed at 1e-5 each move layer 0's K / V rows by 10 x the bound, asserted
     here and run on the GPU.  eps outside the root (1e-6 against a root of 1.1e-3) and eps omitted in the FFN norm (its input is of
     order 1 at every gain) stay invisible at P2 on any input; P1 is where they are held;
     on the row-gain family at P0: row m normalised with row m ^ 1's rms, squares saturating at the fp16 maximum, and eps omitted in
     layer 0's attention norm, each on the rows it affects, per row.
   Inputs that differ from a plain draw, each because a defect would otherwise stay below 10 x a bound: P1's eps is 0.5 (eps outside
   the root on the fp8 engines); the smallest gain is 2^-9 (an omitted production eps against the fp8 and e4m3-cache row bounds of
   0.03 / 0.07); the caches of the fp8 and e4m3-cache cases are larger, and the fp8 prefill runs behind 64 cached tokens (a wrongly
   rotated q, which shows through the attention output only).
3. The gap this work closes, written down: on the P0 control with unit rows every eps defect stays below 0.1 x the bound (fp16-class
   bounds; the fp32 engine's 1e-5 is tight enough to see eps at P0 and is left out of this one condition).

A stand-in keeps the head size, the rotary dimension, the GQA ratio, the biases, the layer count, the weight / cache statistics and
(decode) the position of its case; heads, I, batch and sequence lengths shrink."""
import numpy as np
import pytest

import oracle as orc
import model_param_cases as mc


def standins():
    out = []
    for name, wfmt, (nh, kvh, hs, inter), batch, flags, path, cache in mc.decode_cases():
        nhs = min(nh, 4)
        bs = min(batch, 10)
        out.append(dict(id="decode-" + name, kind="decode", wfmt=wfmt, cache=cache, geom=(nhs, max(1, nhs * kvh // nh), hs, 96),
                        lens=[1] * bs, hist=[mc.STEP - 1] * bs, qkv_bias=False, o_bias=False, p2=name in mc.P2_DECODE))
    for name, wfmt, (nh, kvh, inter), lens, opts, forms in mc.prefill_cases():
        lens_s = [min(l, 64 - 3 * i) for i, l in enumerate(lens[:3])]
        hist = [min(h, 64 + i) for i, h in enumerate(opts.get("hist", [0] * len(lens))[:3])]
        out.append(dict(id="prefill-" + name, kind="prefill", wfmt=wfmt, cache=opts.get("cache", "dense"),
                        geom=(2, max(1, 2 * kvh // nh), 128, 96), lens=lens_s, hist=hist, qkv_bias="bias_misaligned_in_layer" in opts,
                        o_bias=bool(opts.get("o_bias")), p2=name in mc.P2_PREFILL))
    return out


STANDINS = standins()
IDS = [s["id"] for s in STANDINS]
_INPUTS = {}


def inputs(s):
    """layers, hidden rows, caches of a stand-in: drawn once, never modified"""
    if s["id"] not in _INPUTS:
        rng = np.random.default_rng(1234)
        nh, kvh, hs, inter = s["geom"]
        f16 = s["wfmt"] != "f32"
        nl = mc.layers_of(s["wfmt"], s["cache"])
        layers = mc.draw_layers(rng, nh, kvh, hs, inter, nl, f16, s["qkv_bias"], s["o_bias"])
        max_seq = max(mc.MAX_SEQ, max(l + h for l, h in zip(s["lens"], s["hist"])))
        shape = (nl, len(s["lens"]), kvh, max_seq, hs)
        kc, vc, _, _ = mc.draw_caches(rng, shape, s["wfmt"], s["cache"])
        x = mc.uniform(rng, (sum(s["lens"]), nh * hs), 1.0, f16)
        final = mc.uniform(rng, (nh * hs,), 0.2, f16) + 1
        _INPUTS[s["id"]] = (layers, x, kc, vc, final)
    return _INPUTS[s["id"]]


def config(s, point):
    nh, kvh, hs, inter = s["geom"]
    return dict(head_num=nh, kv_head_num=kvh, head_size=hs, inter_size=inter, **mc.point_params(point, hs, s["wfmt"]))


def restated(s, point, defects=(), gains=None, final=False):
    """(hidden rows [T, H], appended K rows, appended V rows [T, L, kvh, hs]) of the restatement; gains: None, or the index of the
    first row's gain"""
    layers, x, kc, vc, fg = inputs(s)
    if gains is not None:
        x = mc.h16(x * mc.row_gains(x.shape[0], gains)[:, None])
    k, v = kc.astype(np.float64), vc.astype(np.float64)
    hid = mc.layer_restatement(config(s, point), layers, x, k, v, s["lens"], s["hist"], defects, fg if final else None)
    return hid, mc.appended_rows(k, s["lens"], s["hist"]), mc.appended_rows(v, s["lens"], s["hist"])


_CLEAN = {}


def clean(s, point, gains=None, final=False):
    key = (s["id"], point, gains, final)
    if key not in _CLEAN:
        _CLEAN[key] = restated(s, point, (), gains, final)
    return _CLEAN[key]


@pytest.mark.parametrize("point", list(mc.POINTS))
@pytest.mark.parametrize("s", STANDINS, ids=IDS)
def test_restatement_equals_the_oracle(s, point):
    layers, x, kc, vc, _ = inputs(s)
    nh, kvh, hs, inter = s["geom"]
    k, v = kc.copy(), vc.copy()
    if s["kind"] == "decode":
        ocfg = mc.oracle_config(s["geom"], point, kc.shape[3], len(layers), s["wfmt"])
        exp = orc.self_decoder(ocfg, layers, x, k, v, mc.STEP)
    else:
        exp = orc.context_decoder(config(s, point), layers, x, k, v, np.array(s["lens"], np.int32), np.array(s["hist"], np.int32))
    hid, kr, vr = clean(s, point)
    assert mc.rel_fro(hid, exp) <= 1e-5
    assert mc.rel_fro(kr, mc.appended_rows(k, s["lens"], s["hist"])) <= 1e-5
    assert mc.rel_fro(vr, mc.appended_rows(v, s["lens"], s["hist"])) <= 1e-5
    # and the composition with its hooks left empty is the oracle itself (the GPU file's fp8 / e4m3 references are built from it)
    k2, v2 = kc.copy(), vc.copy()
    if s["kind"] == "decode":
        comp = mc.composed_self_decoder(ocfg, layers, x, k2, v2, mc.STEP)
    else:
        comp = mc.composed_context_decoder(config(s, point), layers, x, k2, v2, np.array(s["lens"], np.int32), np.array(s["hist"], np.int32))
    assert mc.rel_fro(comp, exp) <= 1e-6 and np.array_equal(k2, k) and np.array_equal(v2, v)


def moved(s, got, ref):
    """by how many project bounds the defect moved the most-moved checked quantity, measured as the GPU file measures it: the hidden
    rows by relative Frobenius error; the K / V rows by max abs (fp8 weights: relative Frobenius, like their hidden rows)"""
    b = mc.bounds(s["wfmt"], s["cache"])
    out = [mc.rel_fro(got[0], ref[0]) / b["fro"]]
    for i in (1, 2):
        if "cache" not in b:
            out.append(mc.rel_fro(got[i], ref[i]) / b["fro"])
        else:
            out.append(np.abs(got[i] - ref[i]).max() / (b["cache"] * (max(1.0, np.abs(ref[i]).max()) if s["cache"] == "paged_e4m3" else 1.0)))
            if s["cache"] == "paged_e4m3":    # and the bytes of layer 0's rows, which the GPU file holds to < 2 % mismatches
                sc = np.float32(mc.KS if i == 1 else mc.VS)
                out.append((mc.to_e4m3(mc.h16(got[i][:, 0]) / sc) != mc.to_e4m3(mc.h16(ref[i][:, 0]) / sc)).mean() / 0.02)
    return max(out)


PER_CASE_EPS = [d for d in mc.EPS_DEFECTS if d != "no_eps:final"]     # the final norm has its own entries: see the test below
OFF_DEFAULT = [(s, "P1", d) for s in STANDINS for d in PER_CASE_EPS + list(mc.ROPE_DEFECTS)] + \
              [(s, "P2", d) for s in STANDINS if s["p2"] for d in mc.ROPE_DEFECTS]


@pytest.mark.parametrize("s,point,defect", OFF_DEFAULT, ids=["%s-%s-%s" % (s["id"], p, d) for s, p, d in OFF_DEFAULT])
def test_defect_shows_off_the_default_point(s, point, defect):
    m = moved(s, restated(s, point, (defect,)), clean(s, point))
    assert m >= 10.0, "%s at %s moves %s by %.3g bounds" % (defect, point, s["id"], m)


def per_row_moved(s, got, ref):
    b = mc.bounds(s["wfmt"], s["cache"])
    return np.max([mc.row_rel(got[i], ref[i]) / (b["row"] if i == 0 else b["row_kv"]) for i in range(3)], axis=0)


# (one row has no neighbour to take an rms from: that defect does not exist on a batch-1 case, which is left out)
UNDER_GAINS = [(s, "P0", d) for s in STANDINS for d in ("neighbour_rms", "fp16_squares", "no_eps:attn0")
               if not (d == "neighbour_rms" and sum(s["lens"]) == 1)] + \
              [(s, "P2", d) for s in STANDINS if s["p2"] for d in ("no_eps:attn", "eps_in_sum", "eps_fixed")]


@pytest.mark.parametrize("s,point,defect", UNDER_GAINS, ids=["%s-%s-%s" % (s["id"], p, d) for s, p, d in UNDER_GAINS])
def test_defect_shows_on_the_rows_it_affects_under_row_gains(s, point, defect):
    T = sum(s["lens"])
    seen = 0
    for first in range(0, len(mc.GAINS) if T < len(mc.GAINS) else 1, T):   # a batch below 5 cycles the gains over repeated calls
        g = (first + np.arange(T)) % len(mc.GAINS)
        if defect == "neighbour_rms":
            nb = np.arange(T) ^ 1
            rows = np.nonzero(nb < T)[0]
            rows = rows[g[rows] != g[nb[rows]]]
        else:
            rows = np.nonzero(g == (4 if defect == "fp16_squares" else 0))[0]
        if not len(rows):
            continue
        seen += len(rows)
        m = per_row_moved(s, restated(s, point, (defect,), gains=first), clean(s, point, gains=first))[rows]
        assert (m >= 10.0).all(), "%s at %s under row gains moves rows %s of %s by %s bounds" % (defect, point, rows, s["id"], m)
    assert seen


@pytest.mark.parametrize("defect", mc.EPS_DEFECTS)
@pytest.mark.parametrize("s", [s for s in STANDINS if s["wfmt"] != "f32"], ids=[s["id"] for s in STANDINS if s["wfmt"] != "f32"])
def test_eps_defects_hide_at_the_default_point(s, defect):
    """the gap: with unit rows at eps 1e-5 none of the eps defects comes near a bound"""
    final = defect == "no_eps:final"
    m = moved(s, restated(s, "P0", (defect,), final=final), clean(s, "P0", final=final))
    assert m <= 0.1, "%s at P0 moves %s by %.3g bounds" % (defect, s["id"], m)


@pytest.mark.parametrize("H,V,f16,tol", [(128, 1000, False, 1e-4), (1024, 3000, True, 2e-2), (128, 32000, True, 2e-2)],
                         ids=["fp32_4x32", "fp16_8x128", "fp16_4x32_v32000"])
def test_final_norm_eps_defect_shows_on_the_lm_head_values(H, V, f16, tol):
    """the final norm is applied by the LM-head entries only, so its eps defect is held against THEIR tolerances: at P1 under row
    gains an omitted eps moves the logits of every row whose mean square is not far above eps (gains 2^-9, 2^-3, 1) by at least 10 x
    the tolerance of the existing tests of those entries (1e-4 abs for fp32 logits, 2e-2 x max(1, |logits| max) for fp16)"""
    rng = np.random.default_rng(1234)
    x, gamma, lm = mc.final_norm_inputs(rng, 5, H, V, f16, 0.2 if not f16 else 0.3)
    eps = mc.POINTS["P1"]["eps"]
    ref = mc.final_norm_logits(x, gamma, lm, eps)
    bad = mc.final_norm_logits(x, gamma, lm, eps, ("no_eps:final",))
    bound = tol * (max(1.0, np.abs(ref).max()) if f16 else 1.0)
    m = np.abs(bad - ref).max(axis=1)[:3] / bound
    assert (m >= 10.0).all(), m
    # and at the default eps with unit rows it hides
    x1 = mc.uniform(rng, (5, H), 1.0, f16)
    m0 = np.abs(mc.final_norm_logits(x1, gamma, lm, 1e-5, ("no_eps:final",)) - mc.final_norm_logits(x1, gamma, lm, 1e-5)).max() / \
        (tol * (max(1.0, np.abs(mc.final_norm_logits(x1, gamma, lm, 1e-5)).max()) if f16 else 1.0))
    if f16:
        assert m0 <= 0.1, m0
