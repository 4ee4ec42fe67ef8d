"""Every refusal of llmie_sample_logits, llmie_sample_logits_ext, llmie_spec_verify and llmie_spec_verify_sampled, by return code
and by the WHOLE llmie_last_error() text (no GPU).  Each call breaks one rule -- the tables of test_spec_decode_cpu.py and
test_spec_sampled_cpu.py, and the sampler's own workspace rule -- or two rules that the entry checks one behind the other, so that
the recorded text also says which check comes first.  The texts in golden/sampler_refusals.json are what the library printed when
they were recorded (`python tests/test_sampler_refusals_cpu.py --record`): a change to the host side of the sampler family that
rewords or reorders a refusal fails here.  Pointers are never dereferenced: each call ends in the checks."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sampler_refusals.json")
FAKE = 0x1000
BIG = 1 << 40

SAMPLE = dict(logits=FAKE, batch=2, vocab=100, params=FAKE, history=None, stride=0, hlen=None, append=0, seq_len=FAKE, fin=FAKE, out=FAKE,
              logprob=None, step=0, step_dev=None, end_id=2, ws=FAKE, ws_bytes=BIG, dtype=1, ext=None)
VERIFY = dict(SAMPLE, k=4, drafts=FAKE, draft_len=None, count=FAKE, last=None, cached=None, step_rows=None)
SAMPLED = dict(VERIFY, dlogits=FAKE, dparams=FAKE, accepted=None)
ENTRIES = {"sample_logits": SAMPLE, "sample_logits_ext": SAMPLE, "spec_verify": VERIFY, "spec_verify_sampled": SAMPLED}


def _call(llmie, entry, kw):
    a = dict(ENTRIES[entry])
    a.update(kw)
    ext = None
    if a["ext"] is not None:
        e = llmie.SamplingExt()
        for k, v in a["ext"].items():
            setattr(e, k, v)
        ext = C.byref(e)
    lib = llmie.lib()
    state = (a["history"], a["stride"], a["hlen"], a["append"], a["seq_len"], a["fin"])
    tail = (a["step"], a["step_dev"], a["end_id"], a["ws"], a["ws_bytes"], a["dtype"], None)
    if entry.startswith("sample_logits"):
        args = (a["logits"], a["batch"], a["vocab"], a["params"]) + state + (a["out"], a["logprob"]) + tail
        rc = lib.llmie_sample_logits(*args) if entry == "sample_logits" else lib.llmie_sample_logits_ext(*(args + (ext,)))
    elif entry == "spec_verify":
        rc = lib.llmie_spec_verify(*((a["logits"], a["batch"], a["k"], a["vocab"], a["drafts"], a["draft_len"], a["params"]) + state +
                                     (a["out"], a["count"], a["logprob"], a["last"], a["cached"], a["step_rows"]) + tail + (ext,)))
    else:
        rc = lib.llmie_spec_verify_sampled(*((a["logits"], a["dlogits"], a["batch"], a["k"], a["vocab"], a["drafts"], a["draft_len"],
                                              a["params"], a["dparams"]) + state +
                                             (a["out"], a["count"], a["accepted"], a["logprob"], a["last"], a["cached"], a["step_rows"]) +
                                             tail + (ext,)))
    return [rc, lib.llmie_last_error().decode()]


def _merge(x, y):
    """both breakages in one call, or None where they set the same operand differently"""
    m = dict(x)
    for k, v in y.items():
        if k == "ext" and m.get("ext") is not None:
            if any(k2 in m["ext"] and m["ext"][k2] != v2 for k2, v2 in v.items()):
                return None
            m["ext"] = dict(m["ext"], **v)
        elif k in m and m[k] != v:
            return None
        else:
            m[k] = v
    return m


def _x(**kw):
    return dict(ext=kw)


# one rule each, in the order the entries check them
BASE = [dict(logits=None), dict(params=None), dict(seq_len=None), dict(fin=None), dict(out=None), dict(batch=0), dict(vocab=0),
        dict(stride=-1), dict(stride=8), dict(stride=8193, history=FAKE, hlen=FAKE), dict(dtype=7)]
WORKSPACE = [dict(ws=None), dict(ws_bytes=1000), dict(ws=FAKE + 4)]
EXT = [_x(top_n=-1), _x(bias_ids=FAKE), _x(stop_ids=FAKE), _x(mask_index=FAKE), _x(allowed_mask=FAKE, mask_stride=3, mask_rows=10),
       _x(allowed_mask=FAKE, mask_stride=4, mask_rows=0), _x(allowed_mask=FAKE, mask_stride=4, mask_rows=1), _x(top_n=3),
       _x(bias_ids=FAKE, bias_vals=FAKE, bias_len=FAKE, bias_stride=1025), _x(stop_ids=FAKE, stop_len=FAKE, stop_stride=17),
       _x(top_n=33, out_top_ids=FAKE, out_top_logprobs=FAKE)]
OWN = [dict(k=0), dict(k=-3), dict(drafts=None), dict(count=None)]
OWN_BOUNDS = [dict(k=16)]
RULES = {
    "sample_logits": BASE + WORKSPACE,
    "sample_logits_ext": BASE + WORKSPACE + EXT,
    "spec_verify": BASE + EXT + OWN + OWN_BOUNDS + [dict(batch=200000000, k=15)] + WORKSPACE,
    "spec_verify_sampled": BASE + EXT + OWN + [dict(dlogits=None), dict(dparams=None)] + OWN_BOUNDS +
                           [dict(vocab=(1 << 19) + 1), dict(batch=100000000, k=15)] + WORKSPACE,
}
# what the two spec tests pair with the sampler's rules, and the pairs among an entry's own rules
CROSS = [dict(vocab=0), dict(dtype=7), _x(stop_ids=FAKE)]
CROSS_OWN = {"spec_verify": [dict(k=0), dict(k=16), dict(drafts=None), dict(ws=None)],
             "spec_verify_sampled": [dict(k=0), dict(k=16), dict(drafts=None), dict(dlogits=None), dict(ws=None)]}
EXTRA = {"spec_verify": [dict(k=16, drafts=None, ws=None), dict(k=16, ws=None)],
         "spec_verify_sampled": [dict(k=16, dlogits=None, ws=None), dict(k=16, ws=None), dict(k=16, vocab=(1 << 19) + 1)]}


def _name(entry, kw):
    flat = dict(kw)
    flat.update({"ext." + k: v for k, v in (flat.pop("ext", None) or {}).items()})
    return entry + ":" + ",".join("%s=%s" % (k, flat[k]) for k in sorted(flat))


def cases():
    out = {}
    for entry, rules in RULES.items():
        calls = list(rules)
        calls += [m for x, y in zip(rules, rules[1:]) for m in [_merge(x, y)] if m is not None]           # neighbours in the order
        calls += [m for x in CROSS for y in CROSS_OWN.get(entry, []) for m in [_merge(x, y)] if m is not None]
        calls += EXTRA.get(entry, [])
        for kw in calls:
            out[_name(entry, kw)] = (entry, kw)
    return out


CASES = cases()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_recording_covers_the_cases(recorded):
    assert sorted(recorded) == sorted(CASES)
    assert len(CASES) > 150
    # every one is a refusal with its entry's name in front, and all three codes occur
    assert {rc for rc, _ in recorded.values()} == {-1, -2, -4}
    for name, (rc, text) in recorded.items():
        entry = name.split(":")[0]
        # (llmie_sample_logits_ext runs the sampler's checks under the sampler's name, its own under its own)
        assert text.startswith(entry + ": ") or (entry == "sample_logits_ext" and text.startswith("sample_logits: ")), (name, text)


@pytest.mark.parametrize("entry", sorted(RULES))
def test_every_refusal_is_the_recorded_one(llmie, recorded, entry):
    for name, (e, kw) in CASES.items():
        if e == entry:
            assert _call(llmie, e, kw) == recorded[name], name


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_sampler_refusals_cpu.py --record")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from conftest import load_llmie
    mod = load_llmie()
    with open(GOLDEN, "w") as f:
        json.dump({name: _call(mod, e, kw) for name, (e, kw) in sorted(CASES.items())}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d refusals" % len(CASES))
