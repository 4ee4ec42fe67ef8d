"""Recorded results of every entry of the sampler family: llmie_sample_logits, _ext, llmie_spec_verify, llmie_spec_verify_sampled
and the four llmie_lm_head_sample* entries give, bit for bit, what they gave when golden/sampler_family.json was recorded
(`python tests/test_sampler_family_gpu.py --record` on the GPU, at the commit whose behaviour is to be kept).  The other suites of
the family hold the kernels to their definitions; this one holds the shell around them -- which operand reaches which kernel
argument, which kernel runs, what is carved from the workspace -- so that the host side can be rearranged without a silent swap.

Inputs come from one seeded numpy generator; the fixture stores their checksum, so a changed generator reads as "inputs differ"
and not as a failure of the code.  Shapes are the smallest at which the shell can go wrong: vocab 2051 (no multiple of 64: the
workspace row is padded; above 1024: a thread sweeps more than one token), batch 3 (the advance ticket's last row is not row 0),
k = 3 with one draft_len of 1, one row finished on entry and one history row one slot short of its stride with append on; fp16
and fp32; the extension absent, present but inactive, and active (one bias entry, a mask row, top_n = 2, a stop id that a pick
hits); the position as `step`, as *step_dev and as step_rows.  The LM-head entries run on a one-layer decoder (2 heads of 64,
inter_size 256, max_batch 4), with next_hidden and advance_step on where an entry takes them, and their refusals behind the
decoder check are recorded as whole texts."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sampler_family.json")
DEV, END = "cuda", 2
V, B, K, STRIDE, STEP = 2051, 3, 3, 8, 41
ROWS = B * (K + 1)
HEADS, HEAD_SIZE, INTER, MAX_BATCH, TOPK = 2, 64, 256, 4, 5
H = HEADS * HEAD_SIZE
DTYPES = {"f16": torch.float16, "f32": torch.float32}
PARAMS = [dict(temperature=0.8, top_k=40, top_p=0.9, seed=11, repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.3),
          dict(temperature=0.0),
          dict(temperature=1.1, min_p=0.02, seed=5, repetition_penalty=1.5)]
DRAFT_PARAMS = [dict(temperature=0.8, top_k=40, top_p=0.9, seed=21), dict(temperature=1.0, seed=22), dict(temperature=0.9, top_k=50, seed=23)]


class Inputs:
    def __init__(self):
        rng = np.random.default_rng(20261020)
        u = lambda shape, scale: (rng.uniform(-1, 1, shape) * scale).astype(np.float32)
        self.logits = (rng.standard_normal((ROWS, V)) * 2.0).astype(np.float32)
        self.draft_logits = (rng.standard_normal((B, K, V)) * 2.0).astype(np.float32)
        self.logits[:, END] = -30.0            # no walk is cut short by chance
        self.draft_logits[0] = self.logits[0:K]   # sequence 0: the drafter's distribution is close to the target's
        self.history = rng.integers(0, V, (B, STRIDE)).astype(np.int32)
        self.history_len = np.array([3, 2, STRIDE - 1], np.int32)
        self.seq_len = np.array([10, 300, 7], np.int32)
        self.finished = np.array([0, 1, 0], np.uint8)
        self.draft_len = np.array([K, K, 1], np.int32)
        self.step_rows = np.array([STEP, 7, 100], np.int32)
        self.cached_len = np.array([120, 5, 77], np.int32)
        self.mask = np.ones((2, V), bool)
        self.mask[1, ::3] = False
        self.hidden = u((MAX_BATCH, H), 1.0)
        self.gamma = u((H,), 0.1) + 1
        self.lm_head = u((V, H), 0.3)
        self.embed = u((V, H), 1.0)
        self.layer = dict(attn_norm=u((H,), 0.1) + 1, ffn_norm=u((H,), 0.1) + 1, qkv=u((3 * H, H), 0.1), o=u((H, H), 0.1),
                          gate_up=u((2 * INTER, H), 0.1), down=u((H, INTER), 0.1))
        h = hashlib.sha256()
        for name in sorted(vars(self)):
            a = getattr(self, name)
            for x in ([a[k] for k in sorted(a)] if isinstance(a, dict) else [a]):
                h.update(np.ascontiguousarray(x).tobytes())
        self.sha256 = h.hexdigest()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype).contiguous()


def _ints(t):
    """a tensor as a flat list of ints: floats by their bit patterns"""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        t = t.view(torch.int32)
    elif t.dtype == torch.float16:
        t = t.view(torch.int16)
    return [int(x) for x in t.reshape(-1).tolist()]


class State:
    def __init__(self, inp, rows=B):
        self.seq, self.fin = _dev(inp.seq_len[:rows]), _dev(inp.finished[:rows])
        self.hist, self.hlen = _dev(inp.history[:rows]), _dev(inp.history_len[:rows])
        self.lp = torch.full((rows,), 7.0, dtype=torch.float32, device=DEV)
        self.out = torch.full((rows,), -5, dtype=torch.int32, device=DEV)

    def result(self):
        return dict(out_id=_ints(self.out), logprob=_ints(self.lp), seq_len=_ints(self.seq), finished=_ints(self.fin), history=_ints(self.hist),
                    history_len=_ints(self.hlen))


def _position(form):
    """-> (step argument, step_dev): the host step is wrong on purpose where the device's is to be read"""
    return (STEP, None) if form == "step" else (-1, torch.tensor([STEP], dtype=torch.int32, device=DEV))


def _ext(llmie, inp, kind, stop, rows, mask_index):
    if kind == "none":
        return None
    if kind == "inactive":
        return llmie.SamplingExt()
    return llmie.sampling_ext(B, V, masks=inp.mask, mask_index=mask_index, bias=[[(17, 4.0)], [], []], stops=[stop, [], []], top_n=2, rows=rows)


def _with_ext(res, ext):
    if hasattr(ext, "top_ids"):   # (the arrays of an active extension)
        res["top_ids"], res["top_logprobs"] = _ints(ext.top_ids), _ints(ext.top_logprobs)
    return res


def sample_case(llmie, inp, dt, kind, form):
    logits = _dev(inp.logits[:B], DTYPES[dt])
    pd = llmie.sampling_params(PARAMS)

    def run(stop):
        st, (step, step_dev) = State(inp), _position(form)
        ext = _ext(llmie, inp, kind, stop, B, [0, 0, 1])
        llmie.sample_logits(logits, pd, st.seq, st.fin, st.out, step, END, history=st.hist, history_len=st.hlen, append=True,
                            out_logprob=st.lp, step_dev=step_dev, ext=ext)
        torch.cuda.synchronize()
        res = _with_ext(st.result(), ext)
        if step_dev is not None:
            res["step_dev"] = _ints(step_dev)
        return res

    res = run([])
    return run([res["out_id"][0]]) if kind == "active" else res   # (the stop list does not move the pick: min_step is off)


def verify_case(llmie, inp, dt, kind, form, sampled):
    logits = _dev(inp.logits, DTYPES[dt])
    dlogits = _dev(inp.draft_logits, DTYPES[dt])
    pd, dpd = llmie.sampling_params(PARAMS), llmie.sampling_params(DRAFT_PARAMS)
    mask_index = [1 if r // (K + 1) == 2 else 0 for r in range(ROWS)]

    def run(drafts, stop, sampled, draft_len=inp.draft_len, finished=inp.finished):
        st = State(inp)
        st.fin = _dev(finished)
        step, step_dev = _position(form)
        state = llmie.SpecState(torch.full((B,), -9, dtype=torch.int32, device=DEV), _dev(inp.cached_len),
                                _dev(inp.step_rows) if form == "step_rows" else None)
        ext = _ext(llmie, inp, kind, stop, ROWS, mask_index)
        lp = torch.full((B, K + 1), 7.0, dtype=torch.float32, device=DEV)
        common = dict(state=state, draft_len=_dev(draft_len), history=st.hist, history_len=st.hlen, append=True, out_logprob=lp, step=step,
                      step_dev=step_dev, ext=ext)
        if sampled:
            accepted = torch.full((B,), -3, dtype=torch.int32, device=DEV)
            tokens, count = llmie.spec_verify_sampled(logits, dlogits, _dev(drafts), pd, dpd, st.seq, st.fin, END, out_accepted=accepted, **common)
        else:
            tokens, count = llmie.spec_verify(logits, _dev(drafts), pd, st.seq, st.fin, END, **common)
        torch.cuda.synchronize()
        res = dict(tokens=_ints(tokens), count=_ints(count), logprob=_ints(lp), seq_len=_ints(st.seq), finished=_ints(st.fin),
                   history=_ints(st.hist), history_len=_ints(st.hlen), last_token=_ints(state.last_token), cached_len=_ints(state.cached_len))
        if sampled:
            res["accepted"] = _ints(accepted)
        if state.step_rows is not None:
            res["step_rows"] = _ints(state.step_rows)
        if step_dev is not None:
            res["step_dev"] = _ints(step_dev)
        return _with_ext(res, ext)

    # the drafts: what exact-match verify itself emits with nothing finished and full draft lengths, found position by position
    # (position j's pick is final once the drafts in front of it are the picks), then one wrong draft in sequence 0
    drafts = np.full((B, K), -1, np.int32)
    nobody, full = np.zeros(B, np.uint8), np.full(B, K, np.int32)
    for j in range(K):
        tok = np.array(run(drafts, [], False, full, nobody)["tokens"], np.int32).reshape(B, K + 1)
        drafts[:, j] = tok[:, j]
    stop = [int(drafts[0, 1])] if kind == "active" else []   # sequence 0 finishes on its second token
    drafts[0, K - 1] = (drafts[0, K - 1] + 1) % V
    res = run(drafts, stop, sampled)
    res["drafts"] = [int(x) for x in drafts.reshape(-1)]
    return res


class Engine:
    def __init__(self, llmie, inp, dt):
        self.dtype = DTYPES[dt]
        d = lambda a: _dev(a, self.dtype)
        layers = [{k: d(v) for k, v in inp.layer.items()}]
        cfg = dict(head_num=HEADS, kv_head_num=HEADS, head_size=HEAD_SIZE, inter_size=INTER, num_layers=1, vocab_size=V, max_seq_len=16,
                   max_batch=MAX_BATCH, rotary_dim=HEAD_SIZE, rotary_base=10000.0, rms_eps=1e-5, dtype=llmie.F16 if dt == "f16" else llmie.F32,
                   wfmt=llmie.W_F16 if dt == "f16" else llmie.W_F32, int4_group=128)
        self.fmt = cfg["wfmt"]
        self.dec = llmie.Decoder(cfg, layers)
        self.hidden, self.gamma, self.lm_head, self.embed = d(inp.hidden), d(inp.gamma), d(inp.lm_head), d(inp.embed)


def lm_head_case(llmie, inp, eng, entry, rows=B, **bad):
    """one call of an LM-head entry; `bad` bends one operand for the refusals"""
    dec, dtype = eng.dec, eng.dtype
    st = State(inp)
    if rows != B:   # (only the refusals)
        st.seq, st.fin, st.out = (torch.zeros(rows, dtype=t.dtype, device=DEV) for t in (st.seq, st.fin, st.out))
    hidden = eng.hidden[:rows].clone() if rows <= MAX_BATCH else torch.zeros((rows, H), dtype=dtype, device=DEV)
    logits = torch.empty((rows, V), dtype=dtype, device=DEV)
    step_dev = None if bad.get("no_step_dev") else torch.tensor([STEP], dtype=torch.int32, device=DEV)
    embed = None if bad.get("no_table") else eng.embed
    next_hidden = torch.full((rows, H), 9.0, dtype=dtype, device=DEV)
    fmt = bad.get("fmt", eng.fmt)
    res = {}
    if entry in ("lm_head_sample", "lm_head_sample_next"):
        kk, bpr = bad.get("K", TOPK), bad.get("bpr", 8)
        tmp_ids = torch.full((rows, bpr * kk), -1, dtype=torch.int32, device=DEV)
        tmp_vals = torch.zeros((rows, bpr * kk), dtype=dtype, device=DEV)
        ids = torch.full((rows, kk), -1, dtype=torch.int32, device=DEV)
        vals = torch.zeros((rows, kk), dtype=dtype, device=DEV)
        nxt = entry == "lm_head_sample_next"
        dec.lm_head_sample(hidden, eng.gamma, eng.lm_head, fmt, logits, tmp_ids, tmp_vals, ids, vals, st.seq, st.fin, st.out, -1, END,
                           blocks_per_row=bpr, step_dev=step_dev, embed=embed if nxt else None, next_hidden=next_hidden if nxt else None,
                           advance=nxt, fused_tail=nxt)
        torch.cuda.synchronize()
        res = dict(out_id=_ints(st.out), seq_len=_ints(st.seq), finished=_ints(st.fin), topk_ids=_ints(ids), topk_vals=_ints(vals))
    else:
        ext = None
        if entry == "lm_head_sample_ext":
            ext = llmie.sampling_ext(B, V, masks=inp.mask, mask_index=[0, 0, 1], bias=[[(17, 4.0)], [], []], stops=[[], [], [5]], top_n=2)
        need = llmie.sample_logits_workspace_bytes(rows, V)
        ws = torch.empty(need - 16 if bad.get("short_ws") else need, dtype=torch.uint8, device=DEV)
        nxt = True
        dec.lm_head_sample_params(hidden, eng.gamma, eng.lm_head, fmt, logits, llmie.sampling_params((PARAMS + PARAMS)[:rows]), st.seq, st.fin,
                                  st.out, -1, END, history=st.hist, history_len=st.hlen, append=True, out_logprob=st.lp, step_dev=step_dev,
                                  embed=embed, next_hidden=next_hidden, advance=True, workspace=ws, ext=ext)
        torch.cuda.synchronize()
        res = _with_ext(st.result(), ext)
    if nxt:
        res["next_hidden"], res["step_dev"] = _ints(next_hidden), _ints(step_dev)
    return res


def lm_head_refusal(llmie, inp, eng, entry, rows=B, **bad):
    try:
        lm_head_case(llmie, inp, eng, entry, rows, **bad)
    except llmie.LlmieError as e:
        return str(e)
    return "no refusal"


ENTRIES = ("lm_head_sample", "lm_head_sample_next", "lm_head_sample_params", "lm_head_sample_ext")
TAILED = ENTRIES[1:]


def case_table():
    """name -> (kind, arguments)"""
    t = {}
    for dt in DTYPES:
        for kind in ("none", "inactive", "active"):
            for form in ("step", "step_dev"):
                t["sample_logits-%s-%s-%s" % (dt, kind, form)] = ("sample", (dt, kind, form))
            for form in ("step", "step_dev", "step_rows"):
                t["spec_verify-%s-%s-%s" % (dt, kind, form)] = ("verify", (dt, kind, form, False))
                t["spec_verify_sampled-%s-%s-%s" % (dt, kind, form)] = ("verify", (dt, kind, form, True))
    for e in ENTRIES:
        t[e + "-f16"] = ("lm_head", ("f16", e))
    t["lm_head_sample-f32"] = ("lm_head", ("f32", "lm_head_sample"))
    return t


def refusal_table(llmie):
    """name -> (entry, rows, bent operand)"""
    t = {}
    for e in ENTRIES:
        t[e + ":batch"] = (e, MAX_BATCH + 1, {})
        t[e + ":mxfp4"] = (e, B, dict(fmt=llmie.W_MXFP4))
    for e in TAILED:
        t[e + ":next_hidden without a table"] = (e, B, dict(no_table=True))
        t[e + ":advance without step_dev"] = (e, B, dict(no_step_dev=True))
    t["lm_head_sample_next:K"] = ("lm_head_sample_next", B, dict(K=33))
    t["lm_head_sample_next:blocks_per_row"] = ("lm_head_sample_next", B, dict(bpr=65))
    for e in ENTRIES[2:]:
        t[e + ":workspace"] = (e, B, dict(short_ws=True))
    return t


CASES = case_table()


class Runner:
    def __init__(self, llmie):
        self.llmie, self.inp, self.engines = llmie, Inputs(), {}

    def engine(self, dt):
        if dt not in self.engines:
            self.engines[dt] = Engine(self.llmie, self.inp, dt)
        return self.engines[dt]

    def case(self, name):
        kind, args = CASES[name]
        if kind == "sample":
            return sample_case(self.llmie, self.inp, *args)
        if kind == "verify":
            return verify_case(self.llmie, self.inp, *args)
        return lm_head_case(self.llmie, self.inp, self.engine(args[0]), args[1])

    def refusals(self):
        return {name: lm_head_refusal(self.llmie, self.inp, self.engine("f16"), e, rows, **bad)
                for name, (e, rows, bad) in refusal_table(self.llmie).items()}

    def close(self):
        for e in self.engines.values():
            e.dec.close()


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def runner(llmie, recorded):
    r = Runner(llmie)
    if r.inp.sha256 != recorded["inputs_sha256"]:
        pytest.fail("inputs differ from the recorded ones: the generator changed, not the code under test")
    yield r
    r.close()


def check_recording(recorded):
    c = recorded["cases"]
    assert sorted(c) == sorted(CASES)
    active = [v for n, v in c.items() if "-active-" in n]
    # the stop id is hit: sequence 0 ends on a token that is not END, and only where the extension is active
    assert all(v["finished"][0] == 1 for v in active) and all(END not in v.get("tokens", v.get("out_id"))[:2] for v in active)
    assert all(v["finished"][0] == 0 for n, v in c.items() if "-none-" in n or "-inactive-" in n)
    ver = [v for n, v in c.items() if n.startswith("spec_verify-")]
    assert {v["count"][0] for v in ver} == {3, 2} and all(v["count"][1] == 0 and v["count"][2] == 2 for v in ver)   # wrong draft / stop; finished; draft_len 1
    assert all(v["history_len"][2] == STRIDE for v in ver)
    smp = [v for n, v in c.items() if n.startswith("spec_verify_sampled-")]
    # drafts are accepted, and the wrong one is rejected
    assert any(a > 0 for v in smp for a in v["accepted"]) and any(v["accepted"][0] < K and v["finished"][0] == 0 for v in smp)
    for n, v in c.items():
        if "step_dev" in v:
            assert v["step_dev"] == [STEP + 1 if n.startswith("lm_head") else STEP], n
    assert all(t != "no refusal" for t in recorded["refusals"].values())


def test_the_recording_is_what_the_docstring_says(recorded):
    check_recording(recorded)


@pytest.mark.parametrize("name", sorted(CASES))
def test_entry_gives_the_recorded_result(runner, recorded, name):
    got, want = runner.case(name), recorded["cases"][name]
    assert sorted(got) == sorted(want)
    for field in want:
        assert got[field] == want[field], "%s: %s differs" % (name, field)


def test_lm_head_refusals_are_the_recorded_ones(runner, recorded):
    assert runner.refusals() == recorded["refusals"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_sampler_family_gpu.py --record   (on the GPU)")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from conftest import load_llmie
    r = Runner(load_llmie())
    cases = {name: r.case(name) for name in sorted(CASES)}
    again = {name: r.case(name) for name in sorted(CASES)}
    unstable = [n for n in cases if cases[n] != again[n]]
    if unstable:
        sys.exit("not reproducible from run to run: %s" % unstable)
    out = dict(inputs_sha256=r.inp.sha256, cases=cases, refusals=r.refusals())
    r.close()
    for n, v in cases.items():
        print(n, {k: v[k] for k in ("out_id", "tokens", "count", "accepted", "finished", "history_len", "step_dev", "step_rows") if k in v})
    for n, v in out["refusals"].items():
        print(n, "->", v)
    check_recording(out)
    with open(GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("recorded %d cases, %d refusals, %d bytes" % (len(cases), len(out["refusals"]), os.path.getsize(GOLDEN)))
