"""Every host refusal of the mixture-of-experts entries, by return code and by the WHOLE llmie_last_error() text (no GPU):
llmie_moe_ffn, _ffn_ex, _route, _route_ex, _ffn_plan, _ffn_plan_ex, and what llmie_decoder_moe_attach / _attach_ex refuse without
an engine (an engine cannot be made without a device: their rules on a live handle are recorded by test_moe_family_gpu.py).  Each
call breaks one rule -- the tables of test_moe_cpu.py and test_moe_mxfp4_cpu.py, the descriptor's rules and the workspace's -- or
two rules that the entry checks one behind the other, so that the recorded text also says which check comes first.  A pair is kept
only where it can say that: its two rules alone give different texts and the pair gives one of them (so two breakages of one rule,
whose text names both values, are dropped when the file is recorded).  The texts in golden/moe_refusals.json are what the library
printed when they were recorded (`python tests/test_moe_refusals_cpu.py --record`): a change to the host side of the family that
rewords or reorders a refusal fails here.  Pointers are never dereferenced: each call ends in the checks."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "moe_refusals.json")
FAKE, WS = 4096, 4096 * 16
W_F16, W_INT8, W_MXFP4 = 0, 1, 5
INF, NAN = float("inf"), float("nan")
DESC_FIELDS = ("format", "router", "router_bias", "gate_up", "gate_up_scale", "gate_up_bias", "down", "down_scale", "down_bias", "act", "alpha",
               "limit")
# the call every case starts from; "d.*": the fields of the _ex entries' descriptor (MXFP4 experts; scale bytes need no alignment)
BASE = dict(x=FAKE, router=FAKE, gate_up=FAKE, down=FAKE, resid=None, y=FAKE, rows=5, H=256, Ie=192, E=8, k=2, flags=0, ws=WS, ws_bytes=1 << 40,
            dtype=1, eo=FAKE, wo=FAKE, format=W_MXFP4, act=0, d=True, dec=FAKE, layers=FAKE)
BASE.update({"d.format": W_MXFP4, "d.router": FAKE, "d.gate_up": FAKE, "d.down": FAKE, "d.gate_up_scale": FAKE + 1, "d.down_scale": FAKE + 3})
F16_DESC = {"d.format": W_F16, "d.gate_up_scale": None, "d.down_scale": None}


def _desc(llmie, a):
    if not a["d"]:
        return None
    d = llmie.MoeExpertsDesc()
    for n in DESC_FIELDS:
        if a.get("d." + n) is not None:
            setattr(d, n, a["d." + n])
    return d


def _call(llmie, entry, kw):
    lib = llmie.lib()
    a = dict(BASE)
    a.update(kw)
    shape = (a["rows"], a["H"], a["Ie"], a["E"], a["k"], a["flags"])
    if a["ws_bytes"] == "need-1":   # one byte less than the call's own plan asks for
        fmt = a["d.format"] if entry == "moe_ffn_ex" else W_F16
        line = lib.llmie_moe_ffn_plan_ex(*(shape + (fmt, 0)))
        a["ws_bytes"] = int(dict(w.split("=") for w in line.decode().split())["ws"]) - 1 if line is not None else 0
    d = _desc(llmie, a)
    dref = C.byref(d) if d is not None else None
    tail = (a["ws"], a["ws_bytes"], a["dtype"], None)
    route = (a["rows"], a["H"], a["E"], a["k"], a["flags"], a["eo"], a["wo"], a["dtype"], None)
    if entry == "moe_ffn":
        rc = lib.llmie_moe_ffn(*((a["x"], a["router"], a["gate_up"], a["down"], a["resid"], a["y"]) + shape + tail))
    elif entry == "moe_ffn_ex":
        rc = lib.llmie_moe_ffn_ex(*((a["x"], dref, a["resid"], a["y"]) + shape + tail))
    elif entry == "moe_route":
        rc = lib.llmie_moe_route(*((a["x"], a["router"]) + route))
    elif entry == "moe_route_ex":
        rc = lib.llmie_moe_route_ex(*((a["x"], dref) + route))
    elif entry == "moe_ffn_plan":        # the plan queries return no code: null where they refuse
        rc = None if lib.llmie_moe_ffn_plan(*shape) is None else 0
    elif entry == "moe_ffn_plan_ex":
        rc = None if lib.llmie_moe_ffn_plan_ex(*(shape + (a["format"], a["act"]))) is None else 0
    else:
        fn = lib.llmie_decoder_moe_attach if entry == "decoder_moe_attach" else lib.llmie_decoder_moe_attach_ex
        rc = fn(a["dec"], a["layers"], a["Ie"], a["E"], a["k"], a["flags"], a["ws"], a["ws_bytes"])
    return [rc, lib.llmie_last_error().decode()]


def _d(**kw):
    return {"d." + k: v for k, v in kw.items()}


# one rule each, grouped by check, groups and rules in the order the entries check them
SHAPE = [dict(rows=0), dict(H=0), dict(Ie=-64), dict(E=0), dict(k=0), dict(E=129), dict(E=4, k=5), dict(E=16, k=9), dict(H=96), dict(Ie=200),
         dict(rows=1 << 22, k=8)]
ROUTE_SHAPE = [dict(rows=-1), dict(H=0), dict(E=0), dict(k=0), dict(E=129), dict(E=2, k=3), dict(E=16, k=9), dict(H=96), dict(rows=1 << 22, k=8)]
PLAN = [dict(flags=2 | 4), dict(flags=64), dict(flags=8 | 16), dict(rows=17, flags=2), dict(H=16448, Ie=64, flags=2), dict(H=64, Ie=16448, flags=2)]
WORKSPACE = [dict(ws=None), dict(ws_bytes="need-1"), dict(ws_bytes=1024), dict(ws=WS + 16)]
DESC_OWN = [[dict(d=False)], [_d(format=W_INT8), _d(format=7)], [_d(router=None), _d(gate_up=None), _d(down=None)],
            [_d(gate_up_scale=None), _d(down_scale=None)], [dict(F16_DESC, **_d(gate_up_scale=FAKE)), dict(F16_DESC, **_d(down_scale=FAKE))],
            [_d(act=2), _d(act=-1)],
            [_d(act=1, alpha=1.702, limit=0.0), _d(act=1, alpha=1.702, limit=-1.0), _d(act=1, alpha=1.702, limit=INF), _d(act=1, alpha=1.702, limit=NAN),
             _d(act=1, alpha=INF, limit=7.0), dict(F16_DESC, **_d(act=1, alpha=NAN, limit=7.0))]]
DESC_ALIGNED = [[_d(router=FAKE + 2), _d(gate_up=FAKE + 8), _d(down=FAKE + 4), dict(F16_DESC, **_d(down=FAKE + 2))],
                [_d(router_bias=FAKE + 1), _d(gate_up_bias=FAKE + 1), dict(F16_DESC, **_d(down_bias=FAKE + 3))]]
RULES = {
    "moe_ffn": [[dict(x=None), dict(y=None)], [dict(router=None), dict(gate_up=None), dict(down=None)], SHAPE, [dict(dtype=0), dict(dtype=7)],
                [dict(x=FAKE + 8), dict(resid=FAKE + 4), dict(y=FAKE + 2)], [dict(router=FAKE + 8), dict(gate_up=FAKE + 4), dict(down=FAKE + 2)],
                PLAN, WORKSPACE],
    "moe_ffn_ex": [[dict(x=None), dict(y=None)]] + DESC_OWN + [SHAPE, [dict(dtype=0)], [dict(x=FAKE + 2), dict(resid=FAKE + 4), dict(y=FAKE + 8)]] +
                  DESC_ALIGNED + [PLAN, WORKSPACE, [dict(F16_DESC, ws_bytes=1024, **_d(down_bias=FAKE + 2))]],
    "moe_route": [[dict(x=None), dict(router=None), dict(eo=None), dict(wo=None)], ROUTE_SHAPE, [dict(dtype=0)], [dict(x=FAKE + 8), dict(router=FAKE + 8)],
                  [dict(flags=1 << 9)]],
    "moe_route_ex": [[dict(x=None), dict(d=False), _d(router=None), dict(eo=None), dict(wo=None)], ROUTE_SHAPE, [dict(dtype=0)],
                     [dict(x=FAKE + 8), _d(router=FAKE + 8)], [_d(router_bias=FAKE + 1)], [dict(flags=1 << 9)]],
    "moe_ffn_plan": [SHAPE, PLAN],
    "moe_ffn_plan_ex": [[dict(format=W_INT8), dict(format=7)], [dict(act=2), dict(act=-1)], SHAPE, PLAN],
    "decoder_moe_attach": [[dict(dec=None), dict(layers=None), dict(ws=None)]],
    "decoder_moe_attach_ex": [[dict(dec=None), dict(layers=None), dict(ws=None)]],
}


def _merge(x, y):
    """both breakages in one call, or None where they set the same operand differently"""
    m = dict(x)
    for k, v in y.items():
        if k in m and m[k] != v:
            return None
        m[k] = v
    return m


def _name(entry, kw):
    return entry + ":" + ",".join("%s=%s" % (k, kw[k]) for k in sorted(kw))


def candidates():
    """{name: (entry, kw, None)} of the single rules and {x + y: (entry, kw, (x, y))} of the pairs: neighbours in the order, and the
    first rule of every check with the first rule of every later check"""
    out = {}
    for entry, groups in RULES.items():
        rules = [r for g in groups for r in g]
        for kw in rules:
            out[_name(entry, kw)] = (entry, kw, None)
        pairs = list(zip(rules, rules[1:])) + [(g[0], h[0]) for i, g in enumerate(groups) for h in groups[i + 1:]]
        for x, y in pairs:
            m = _merge(x, y)
            if m is not None:
                out[_name(entry, x) + " + " + _name(entry, y).split(":", 1)[1]] = (entry, m, (_name(entry, x), _name(entry, y)))
    return out


CANDIDATES = candidates()


def says_the_order(rec, name):
    x, y = CANDIDATES[name][2]
    return rec[x] != rec[y] and rec[name] in (rec[x], rec[y])


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_recording_covers_the_cases(recorded):
    singles = {n for n, c in CANDIDATES.items() if c[2] is None}
    assert singles <= set(recorded) <= set(CANDIDATES)
    pairs = [n for n in recorded if CANDIDATES[n][2] is not None]
    assert len(singles) > 150 and len(pairs) > 100, (len(singles), len(pairs))
    assert all(says_the_order(recorded, n) for n in pairs)
    assert {rc for rc, _ in recorded.values()} == {None, -1, -2, -4}
    for name, (rc, text) in recorded.items():
        assert text.startswith(name.split(":")[0] + ": "), (name, text)
    # neighbouring checks of llmie_moe_ffn_ex whose texts differ are there as a pair (the clamped act's constants cannot be paired with
    # an unknown act): the order of its checks is recorded end to end
    groups = RULES["moe_ffn_ex"][:-1]
    for g, h in zip(groups, groups[1:]):
        if recorded[_name("moe_ffn_ex", g[0])] != recorded[_name("moe_ffn_ex", h[0])] and _merge(g[0], h[0]) is not None:
            assert any(_name("moe_ffn_ex", x) + " + " + _name("moe_ffn_ex", y).split(":", 1)[1] in recorded for x in g for y in h), (g[0], h[0])


@pytest.mark.parametrize("entry", sorted(RULES))
def test_every_refusal_is_the_recorded_one(llmie, recorded, entry):
    llmie.build()
    for name in recorded:
        e, kw, _ = CANDIDATES[name]
        if e == entry:
            assert _call(llmie, e, kw) == recorded[name], name


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_moe_refusals_cpu.py --record")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from conftest import load_llmie
    mod = load_llmie()
    rec = {name: _call(mod, e, kw) for name, (e, kw, _) in sorted(CANDIDATES.items())}
    kept = {name: r for name, r in rec.items() if CANDIDATES[name][2] is None or says_the_order(rec, name)}
    with open(GOLDEN, "w") as f:
        json.dump(kept, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d refusals (%d pairs dropped)" % (len(kept), len(rec) - len(kept)))
