"""llmie_spec_verify_sampled against its restatement (tests/spec_sampled_cases.py: numpy float64 masses, the rule in Python
integers), and four exact properties that need no restatement.

Everything a call leaves is compared: tokens, counts, out_accepted, seq_len, finished, the history and its length, step_rows,
cached_len and last_token exactly, out_logprob within 1e-4 (the sampler tests' bound).  A sequence may differ from the
restatement only where the restatement itself reports a decision on a boundary (fragile), and at most max(1, 0.004 * sequences)
of a case may; tests/test_spec_sampled_cpu.py checks that the fragile share of every case stays under that cap.

The cases (spec_sampled_cases.matrix): V 7 / 1000 / 32003 x batch 1 / 5 x k 1 / 4 / 15 x fp16 / fp32 with parameter mixes drawn
independently for target and draft; a greedy target, a greedy draft, both; draft_len short of k and 0; drafts outside [0, V);
end_id and a stop id on an accepted draft; min_step inside the chunk; per-position masks and a bias that ban the draft; histories
that saturate inside the chunk with history_append 0 and 1; a finished sequence; all-NaN target and draft rows; the top-N of
every row; step_rows, *step_dev and the step argument."""
import numpy as np
import pytest
import torch

import spec_sampled_cases as R

pytestmark = pytest.mark.gpu
DEV, END, STRIDE = "cuda", R.END, R.STRIDE
MATRIX = R.matrix()
_cases = {}


def _case(name):
    if name not in _cases:
        _cases[name] = dict(MATRIX)[name]()
    return _cases[name]


def _t(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _ext(llmie, c):
    if not c.ctl and not c.top_n and c.masks is None:
        return None
    ctl = c.ctl or [dict()] * c.B
    any_of = lambda key: any(x.get(key) is not None for x in ctl)
    return llmie.sampling_ext(c.B, c.V, masks=c.masks, mask_index=c.mask_index, bias=[x.get("bias") or [] for x in ctl] if any_of("bias") else None,
                              stops=[x.get("stops") or [] for x in ctl] if any_of("stops") else None,
                              min_step=[x["min_step"] if x.get("min_step") is not None else 0 for x in ctl] if any_of("min_step") else None,
                              top_n=c.top_n, rows=c.B * (c.k + 1))


def run(llmie, c, order=None, step_mode="rows", drafts=None, raw_d=None, dparams=None):
    """one call on the sequences `order` of the case (default all, in place) -> dict of numpy outputs, per slot"""
    order = list(range(c.B)) if order is None else order
    B, k, V = len(order), c.k, c.V
    dt = torch.float16 if c.f16 else torch.float32
    sel = np.array(order)
    logits = _t(c.raw_t[sel], dt).reshape(B * (k + 1), V).contiguous()
    dlogits = _t((c.raw_d if raw_d is None else raw_d)[sel], dt).contiguous()
    d = _t((c.drafts if drafts is None else drafts)[sel].astype(np.int32))
    hist, hlen = _t(c.hist[sel]), _t(c.hlen[sel])
    seq, fin = _t(c.seq[sel]), _t(c.fin[sel])
    steps, cached = _t(c.steps[sel]), _t(c.cached[sel])
    last = torch.full((B,), -9, dtype=torch.int32, device=DEV)
    lp = torch.zeros((B, k + 1), dtype=torch.float32, device=DEV)
    acc = torch.full((B,), -5, dtype=torch.int32, device=DEV)
    dl = None if c.draft_len is None else _t(np.array(c.draft_len, np.int32)[sel])
    ext = _ext(llmie, c) if order == list(range(c.B)) else None
    kw = dict(step=0)
    state = llmie.SpecState(last, cached, steps)
    if c.shared_step is not None:
        state = llmie.SpecState(last, cached, None)
        kw = dict(step=c.shared_step) if step_mode == "arg" else dict(step=-77, step_dev=torch.tensor([c.shared_step], dtype=torch.int32, device=DEV))
    tok, cnt = llmie.spec_verify_sampled(logits, dlogits, d, llmie.sampling_params([c.params[b] for b in order]),
                                         llmie.sampling_params([(c.dparams if dparams is None else dparams)[b] for b in order]), seq, fin, END,
                                         state=state, draft_len=dl, history=hist, history_len=hlen, append=c.append, out_logprob=lp,
                                         out_accepted=acc, ext=ext, **kw)
    torch.cuda.synchronize()
    out = dict(tokens=tok, count=cnt, accepted=acc, logprob=lp, seq=seq, fin=fin, hist=hist, hlen=hlen, steps=steps, cached=cached, last=last)
    out = {n: t.cpu().numpy() for n, t in out.items()}
    out["ext"] = ext
    return out


def check(c, got):
    want = c.expected()
    bad = []
    for b, w in enumerate(want):
        n = w["count"]
        exact = dict(tokens=w["tokens"], count=n, accepted=w["accepted"], seq=c.seq[b] + n, fin=w["fin"], hist=w["hist"], hlen=w["hlen"],
                     cached=c.cached[b] + n, last=w["tokens"][n - 1] if n else -9)
        if c.shared_step is None:
            exact["steps"] = c.steps[b] + n
        diff = [name for name, v in exact.items() if not np.array_equal(np.asarray(got[name][b]), np.asarray(v))]
        if diff:
            assert w["fragile"] or c.draft_fragile[b], "sequence %d differs in %s: got %s count %d accepted %d, restatement %s" % (
                b, diff, got["tokens"][b].tolist(), got["count"][b], got["accepted"][b], w)
            bad.append(b)
            continue
        lp = np.array(w["logprob"], np.float64)
        assert np.array_equal(np.isneginf(got["logprob"][b]), np.isneginf(lp)), (b, got["logprob"][b], lp)
        fin = ~np.isneginf(lp)
        assert np.all(np.abs(got["logprob"][b][fin] - lp[fin]) <= 1e-4), (b, got["logprob"][b], lp)
    assert len(bad) <= R.fragile_cap(c.B), "%d of %d sequences differ from the restatement" % (len(bad), c.B)


@pytest.mark.parametrize("name", [n for n, _ in MATRIX])
def test_equals_the_restatement(llmie, name):
    c = _case(name)
    got = run(llmie, c)
    check(c, got)
    if c.top_n:
        # the top-N is a property of the raw row: one sampler call over all B * (k + 1) rows gives it for every position
        rows = c.B * (c.k + 1)
        e = llmie.sampling_ext(rows, c.V, top_n=c.top_n)
        dt = torch.float16 if c.f16 else torch.float32
        llmie.sample_logits(_t(c.raw_t, dt).reshape(rows, c.V).contiguous(), llmie.sampling_params([dict(temperature=0.0)] * rows),
                            torch.zeros(rows, dtype=torch.int32, device=DEV), torch.zeros(rows, dtype=torch.uint8, device=DEV),
                            torch.empty(rows, dtype=torch.int32, device=DEV), 0, END, ext=e)
        torch.cuda.synchronize()
        assert torch.equal(got["ext"].top_ids, e.top_ids)
        assert torch.equal(got["ext"].top_logprobs.view(torch.int32), e.top_logprobs.view(torch.int32))


def test_the_step_argument_and_step_dev_agree(llmie):
    c = _case("shared_step")
    a, b = run(llmie, c, step_mode="arg"), run(llmie, c, step_mode="dev")
    check(c, a)
    for name in a:
        if name != "ext":
            assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), name


def test_special_cases_reach_what_they_are_about():
    w = {n: _case(n).expected() for n in R.SPECIAL}
    assert [x["count"] for x in w["finished"]][1] == 0
    assert w["stops"][0]["tokens"][1] == END and w["stops"][0]["accepted"] == 2 and w["stops"][0]["fin"] == 1
    assert w["stops"][1]["tokens"][2] == 500 and w["stops"][1]["accepted"] == 3 and w["stops"][1]["fin"] == 1
    c = _case("min_step")
    # end_id named one step early: banned there (P_d = 0), rejected; the stop id named in time: accepted, and it finishes
    assert c.drafts[0, 1] == END and w["min_step"][0]["accepted"] == 1 and w["min_step"][0]["count"] == 2 and w["min_step"][0]["tokens"][1] != END
    assert w["min_step"][1]["tokens"][3] == 77 and w["min_step"][1]["accepted"] == 4 and w["min_step"][1]["fin"] == 1
    c = _case("mask_bans_draft")
    assert w["mask_bans_draft"][1]["accepted"] == 0 and w["mask_bans_draft"][1]["tokens"][0] != c.drafts[1, 0]
    c = _case("bias_ban")
    assert w["bias_ban"][0]["accepted"] <= 1 and c.drafts[0, 1] not in w["bias_ban"][0]["tokens"]
    assert w["nan_rows"][1]["tokens"][w["nan_rows"][1]["count"] - 1] == END and w["nan_rows"][1]["count"] == 3 and w["nan_rows"][1]["fin"] == 1
    assert w["nan_rows"][2]["accepted"] == 1 and w["nan_rows"][2]["count"] == 2      # S_Q = 0 at position 1: rejected, the pick emitted
    assert [x["count"] for x in w["draft_len"]][0] == 1 and [x["count"] for x in w["draft_len"]][3] == 1
    assert all(x["accepted"] == 0 for b, x in enumerate(w["draft_out_of_range"]) if b in (0, 2))


# ------------------------------------------------------------------------------------------------ exact, no restatement
@pytest.mark.parametrize("name", ["V32003-B5-k4-f16", "V1000-B5-k15-f32", "V7-B5-k4-f16"])
def test_the_targets_own_rows_as_the_draft_accept_everything(llmie, name):
    c = _case(name)
    # the drafter IS the target: its rows, its parameters (seed included), so P == Q at every position whatever the drafts are
    # along the accepted path; the drafts are the restated picks from those rows
    twin = R.make_case(900, c.V, c.B, c.k, c.f16, finalize=False)
    twin.raw_t, twin.params = c.raw_t, c.params
    twin.raw_d, twin.dparams = c.raw_t[:, :c.k].copy(), c.params
    R.draw(twin)
    got = run(llmie, twin)
    assert got["count"].tolist() == [c.k + 1] * c.B and got["accepted"].tolist() == [c.k] * c.B
    assert np.array_equal(got["tokens"][:, :c.k], twin.drafts)


@pytest.mark.parametrize("f16", [True, False])
def test_a_greedy_target_emits_what_exact_match_emits(llmie, f16):
    c = _case("greedy_target-%s" % ("f16" if f16 else "f32"))
    got = run(llmie, c)
    dt = torch.float16 if f16 else torch.float32
    seq, fin = _t(c.seq), _t(c.fin)
    tok, cnt = llmie.spec_verify(_t(c.raw_t, dt).reshape(-1, c.V).contiguous(), _t(c.drafts), llmie.sampling_params(c.params), seq, fin, END,
                                 state=llmie.SpecState(None, None, _t(c.steps)), history=_t(c.hist), history_len=_t(c.hlen), append=c.append)
    torch.cuda.synchronize()
    assert np.array_equal(got["tokens"], tok.cpu().numpy()) and np.array_equal(got["count"], cnt.cpu().numpy())
    assert np.array_equal(got["seq"], seq.cpu().numpy()) and np.array_equal(got["fin"], fin.cpu().numpy())
    assert len(set(got["count"].tolist())) > 1


def test_two_runs_give_equal_bits_and_a_sequence_keeps_them_in_another_slot(llmie):
    c = _case("V32003-B5-k4-f16")
    a, b = run(llmie, c), run(llmie, c)
    for name in a:
        if name != "ext":
            assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), name
    order = [3, 1, 4, 0]      # other slots, other neighbours, one sequence missing
    m = run(llmie, c, order=order)
    for slot, s in enumerate(order):
        for name in a:
            if name != "ext":
                assert np.array_equal(m[name][slot:slot + 1].view(np.uint8), a[name][s:s + 1].view(np.uint8)), (name, s)
    for s in range(c.B):
        solo = run(llmie, c, order=[s])
        for name in a:
            if name != "ext":
                assert np.array_equal(solo[name].view(np.uint8), a[name][s:s + 1].view(np.uint8)), (name, s)
