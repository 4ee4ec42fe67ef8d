"""llmie_spec_verify against its definition: the existing sampler, llmie.sample_logits (with ext), called ONE ROW AT A TIME on the
same device rows, position after position, until the header's stop rule ends the walk.  Everything is compared bit for bit:
tokens, counts, out_logprob, seq_len, finished, the history and its length, step_rows, cached_len, last_token and the top-N.

Construction: random logits [B, k + 1, V]; the reference chain run with "always continue" gives the picks c_0 .. c_k; the drafts
are c with one corrupted position a_b per sequence, chosen so that a count of 1, a middle count and k + 1 (all accepted + the
bonus token) occur -- asserted.  The logit of END is -30 in the matrix cases, so that no walk is cut short by chance.

The shape matrix is the full cross V x B x k x dtype; the five parameter mixes rotate through it (each meets every V, B, k and
dtype), and all five run in both dtypes at V = 1000, B = 5, k = 4."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV, END = "cuda", 2
STRIDE = 24
STEPS = [3, 100, 7, 1 << 20, 55]
MIXES = ["greedy", "truncate", "penal_append", "penal_keep", "penal_edge"]


def _params(mix, B):
    rows = []
    for b in range(B):
        if mix == "greedy":
            rows.append(dict(temperature=0.0))
        elif mix == "truncate":
            rows.append(dict(temperature=0.8, top_k=[0, 5, 40, 3, 0][b % 5], top_p=[0.9, 1.0, 0.7, 0.95, 0.5][b % 5],
                             min_p=[0.0, 0.05, 0.0, 0.02, 0.1][b % 5], seed=11 + b))
        else:
            rows.append(dict(temperature=0.8, repetition_penalty=1.5, presence_penalty=0.4, frequency_penalty=0.3, top_k=50, seed=5 + b))
    return rows


def _logits(rng, B, k, V, dtype, end_low=True):
    x = (rng.standard_normal((B, k + 1, V)) * 2.0).astype(np.float32)
    if end_low and V > END:
        x[:, :, END] = -30.0
    return torch.from_numpy(x).to(DEV).to(dtype).contiguous()


class State:
    def __init__(self, rng, B, V, hlen=None, steps=None):
        hist = rng.integers(0, V, (B, STRIDE)).astype(np.int32)
        hist[:, 1] = -1          # ids outside [0, V) are ignored
        hist[:, 3] = V + 3
        self.hist = torch.from_numpy(hist).to(DEV)
        self.hlen = torch.tensor([5, 0, 11, STRIDE // 2, 9][:B] if hlen is None else hlen, dtype=torch.int32, device=DEV)
        self.seq = torch.tensor([10, 0, 7, 300, 1][:B], dtype=torch.int32, device=DEV)
        self.fin = torch.zeros(B, dtype=torch.uint8, device=DEV)
        self.steps = torch.tensor(STEPS[:B] if steps is None else steps, dtype=torch.int32, device=DEV)
        self.cached = torch.tensor([120, 5, 77, 2000, 128][:B], dtype=torch.int32, device=DEV)
        self.last = torch.full((B,), -9, dtype=torch.int32, device=DEV)

    def clone(self):
        c = object.__new__(State)
        for n, t in vars(self).items():
            setattr(c, n, t.clone())
        return c

    def fields(self):
        return vars(self)


class Ext:
    """the controls of one case in Python terms: per-sequence bias / stops / min_step, per-position mask_index, top_n"""

    def __init__(self, B, k, V, masks=None, mask_index=None, bias=None, stops=None, min_step=None, top_n=0):
        self.B, self.k, self.V, self.masks, self.mask_index, self.bias, self.stops, self.min_step, self.top_n = B, k, V, masks, mask_index, bias, stops, min_step, top_n

    def for_verify(self, llmie):
        return llmie.sampling_ext(self.B, self.V, masks=self.masks, mask_index=self.mask_index, bias=self.bias, stops=self.stops,
                                  min_step=self.min_step, top_n=self.top_n, rows=self.B * (self.k + 1))

    def for_row(self, llmie, b, i):
        """what a single sampler call on row (b, i) is given"""
        mi = None
        masks = self.masks
        if masks is not None:
            mi = [self.mask_index[b * (self.k + 1) + i]] if self.mask_index is not None else [b]
        return llmie.sampling_ext(1, self.V, masks=masks, mask_index=mi, bias=None if self.bias is None else [self.bias[b]],
                                  stops=None if self.stops is None else [self.stops[b]],
                                  min_step=None if self.min_step is None else [self.min_step[b]], top_n=self.top_n)


def _reference(llmie, logits, prm, st, append, drafts=None, draft_len=None, ext=None, step=None, end_id=END):
    """the definition: per sequence, sampler calls on rows (b, 0), (b, 1), ... of `logits` [B, k + 1, V] until the stop rule ends
    the walk (drafts None: always continue, all k + 1 rows).  Moves `st` in place; -> tokens [B, k + 1], count [B], logprob"""
    B, n, V = logits.shape
    tokens = np.full((B, n), -1, np.int32)
    logprob = np.full((B, n), -np.inf, np.float32)
    count = np.zeros(B, np.int32)
    out, lp = torch.empty(1, dtype=torch.int32, device=DEV), torch.empty(1, dtype=torch.float32, device=DEV)
    entry_fin = st.fin.cpu().numpy().copy()
    steps = st.steps.cpu().numpy() if step is None else np.full(B, step)
    for b in range(B):
        if drafts is not None and entry_fin[b]:
            continue
        dl = n - 1 if draft_len is None else min(max(int(draft_len[b]), 0), n - 1)
        for i in range(n):
            llmie.sample_logits(logits[b, i:i + 1], prm[b], st.seq[b:b + 1], st.fin[b:b + 1], out, int(steps[b]) + i, end_id,
                                history=st.hist[b:b + 1], history_len=st.hlen[b:b + 1], append=append, out_logprob=lp,
                                ext=None if ext is None else ext.for_row(llmie, b, i))
            tokens[b, i], logprob[b, i] = int(out.item()), float(lp.item())
            count[b] += 1
            if drafts is not None and (i == dl or st.fin[b].item() or tokens[b, i] != drafts[b, i]):
                break
        if drafts is not None:
            st.last[b] = int(tokens[b, count[b] - 1])
            st.cached[b] += int(count[b])
            if step is None:
                st.steps[b] += int(count[b])
    return tokens, count, logprob


def _bits(t):
    t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(name, got, want):
    assert torch.equal(_bits(got), _bits(want)), "%s differs:\n%s\n%s" % (name, got, want)


def _run_case(llmie, logits, params, st0, append, corrupt, ext=None, draft_len=None, shared_step=None, step_dev=False, top_ref=True, end_id=END):
    """corrupt[b]: the draft position that is made wrong (>= k: none).  -> (count, tokens) after every comparison"""
    B, n, V = logits.shape
    k = n - 1
    prm = [llmie.sampling_params([p]) for p in params]
    chain, _, _ = _reference(llmie, logits, prm, st0.clone(), append, ext=ext, step=shared_step, end_id=end_id)
    drafts = chain[:, :k].copy()
    for b in range(B):
        if corrupt[b] < k:
            drafts[b, corrupt[b]] = (drafts[b, corrupt[b]] + 1) % V
    want = st0.clone()
    w_tok, w_cnt, w_lp = _reference(llmie, logits, prm, want, append, drafts=drafts, draft_len=draft_len, ext=ext, step=shared_step, end_id=end_id)

    got = st0.clone()
    vext = None if ext is None else ext.for_verify(llmie)
    d_drafts = torch.from_numpy(drafts).to(DEV)
    d_len = None if draft_len is None else torch.tensor(draft_len, dtype=torch.int32, device=DEV)
    lp = torch.zeros((B, n), dtype=torch.float32, device=DEV)
    state = llmie.SpecState(got.last, got.cached, None if shared_step is not None else got.steps)
    sdev = torch.tensor([shared_step], dtype=torch.int32, device=DEV) if step_dev else None
    tok, cnt = llmie.spec_verify(logits.reshape(B * n, V), d_drafts, llmie.sampling_params(params), got.seq, got.fin, end_id, state=state,
                                 draft_len=d_len, history=got.hist, history_len=got.hlen, append=append, out_logprob=lp,
                                 step=-77 if step_dev else (shared_step or 0), step_dev=sdev, ext=vext)
    torch.cuda.synchronize()
    _same("tokens", tok, w_tok)
    _same("count", cnt, w_cnt)
    _same("out_logprob", lp, w_lp)
    for name in want.fields():
        _same(name, getattr(got, name), getattr(want, name))
    if ext is not None and ext.top_n and top_ref:
        # the top-N is a property of the raw row: one sampler call over all B * (k + 1) rows gives it for every position
        R = B * n
        e = llmie.sampling_ext(R, V, top_n=ext.top_n)
        llmie.sample_logits(logits.reshape(R, V), llmie.sampling_params([dict(temperature=0.0)] * R), torch.zeros(R, dtype=torch.int32, device=DEV),
                            torch.zeros(R, dtype=torch.uint8, device=DEV), torch.empty(R, dtype=torch.int32, device=DEV), 0, end_id, ext=e)
        torch.cuda.synchronize()
        _same("top ids", vext.top_ids, e.top_ids)
        _same("top logprobs", vext.top_logprobs, e.top_logprobs)
    return cnt.cpu().numpy(), tok.cpu().numpy()


def _corrupt(B, k, case):
    """positions to corrupt: first, middle, none, last, second -- one sequence rotates through them by case number"""
    plan = [0, k // 2, k, k - 1, min(1, k)]
    return [plan[(b + (case if B == 1 else 0)) % 5] for b in range(B)]


SHAPES = list(itertools.product([7, 1000, 32003], [1, 5], [1, 4, 15], [torch.float16, torch.float32]))
MATRIX = [(V, B, k, dt, MIXES[i % 5]) for i, (V, B, k, dt) in enumerate(SHAPES)] + \
         [(1000, 5, 4, dt, m) for dt in (torch.float16, torch.float32) for m in MIXES]


@pytest.mark.parametrize("V,B,k,dtype,mix", MATRIX, ids=lambda v: str(v).replace("torch.", ""))
def test_verify_equals_sequential_sampler_calls(llmie, V, B, k, dtype, mix):
    case = MATRIX.index((V, B, k, dtype, mix))
    rng = np.random.default_rng(1000 + case)
    logits = _logits(rng, B, k, V, dtype)
    # penal_edge: histories within i of the stride -- the appends saturate inside the chunk, at the stride, and one is full on entry
    hlen = [STRIDE - 2, STRIDE, STRIDE - 1, STRIDE - k, 0][:B] if mix == "penal_edge" else None
    st0 = State(rng, B, V, hlen=hlen)
    corrupt = _corrupt(B, k, case)
    cnt, _ = _run_case(llmie, logits, _params(mix, B), st0, append=mix != "penal_keep", corrupt=corrupt)
    assert list(cnt) == [min(a, k) + 1 for a in corrupt], (cnt, corrupt)
    if B == 5:
        assert 1 in cnt and k + 1 in cnt and (k < 2 or any(1 < c < k + 1 for c in cnt))


def test_one_sequence_reaches_every_count(llmie):
    # B = 1 cases of the matrix take one count each; here every count 1 .. k + 1 of a single sequence
    k, V = 4, 1000
    rng = np.random.default_rng(7)
    logits = _logits(rng, 1, k, V, torch.float16)
    seen = [int(_run_case(llmie, logits, _params("penal_append", 1), State(rng, 1, V), True, [a])[0][0]) for a in range(k + 1)]
    assert seen == [1, 2, 3, 4, 5]


@pytest.mark.parametrize("k", [1, 4])
def test_draft_len(llmie, k):
    V, B = 1000, 5
    rng = np.random.default_rng(21 + k)
    logits = _logits(rng, B, k, V, torch.float16)
    # 0, 1, k, and values the device clamps (-3 -> 0, k + 9 -> k); no draft is wrong: only draft_len ends the walks
    dl = [0, 1, k, -3, k + 9]
    cnt, _ = _run_case(llmie, logits, _params("truncate", B), State(rng, B, V), True, [k] * B, draft_len=dl)
    assert list(cnt) == [1, 2, k + 1, 1, k + 1]
    cnt, _ = _run_case(llmie, logits, _params("truncate", B), State(rng, B, V), True, [k] * B, draft_len=None)
    assert list(cnt) == [k + 1] * B


def test_stop_id_and_end_id_on_an_accepted_draft(llmie):
    V, B, k = 1000, 3, 4
    rng = np.random.default_rng(33)
    logits = _logits(rng, B, k, V, torch.float32, end_low=False)
    lg = logits.clone()
    lg[0, 1, END] = 40.0     # sequence 0 picks end_id at position 1
    lg[1, 2, 500] = 40.0     # sequence 1 picks its stop id 500 at position 2
    lg[2, 3, 500] = 40.0     # 500 is no stop id of sequence 2: it goes on
    lg[:, 0, END] = -30.0
    ext = Ext(B, k, V, stops=[[], [9, 500], [501]])
    st0 = State(rng, B, V)
    cnt, tok = _run_case(llmie, lg, _params("greedy", B), st0, True, [k] * B, ext=ext)
    assert list(cnt) == [2, 3, k + 1] and tok[0, 1] == END and tok[1, 2] == 500 and tok[2, 3] == 500


def test_min_step_inside_the_chunk(llmie):
    V, B, k = 1000, 2, 4
    rng = np.random.default_rng(34)
    lg = _logits(rng, B, k, V, torch.float16)
    lg[:, :, END] = 40.0     # end_id wins wherever it is allowed
    lg[1, :, 77] = 41.0      # sequence 1: its stop id wins wherever it is allowed
    st0 = State(rng, B, V, steps=[10, 20])
    ext = Ext(B, k, V, stops=[[], [77]], min_step=[12, 23])   # held back at steps 10, 11 / 20, 21, 22
    cnt, tok = _run_case(llmie, lg, _params("greedy", B), st0, True, [k] * B, ext=ext)
    assert list(cnt) == [3, 4] and tok[0, 2] == END and tok[1, 3] == 77 and END not in tok[0, :2] and 77 not in tok[1, :3]


def test_finished_on_entry_is_left_alone(llmie):
    V, B, k = 1000, 3, 4
    rng = np.random.default_rng(35)
    logits = _logits(rng, B, k, V, torch.float16)
    st0 = State(rng, B, V)
    st0.fin[1] = 1
    before = st0.clone()
    got = st0.clone()
    drafts = torch.zeros((B, k), dtype=torch.int32, device=DEV)
    lp = torch.zeros((B, k + 1), dtype=torch.float32, device=DEV)
    tok, cnt = llmie.spec_verify(logits.reshape(-1, V), drafts, llmie.sampling_params(_params("penal_append", B)), got.seq, got.fin, END,
                                 state=llmie.SpecState(got.last, got.cached, got.steps), history=got.hist, history_len=got.hlen, append=True,
                                 out_logprob=lp)
    torch.cuda.synchronize()
    assert cnt.tolist()[1] == 0 and tok[1].tolist() == [-1] * (k + 1) and torch.isneginf(lp[1]).all()
    for name in before.fields():   # byte for byte
        a, b = getattr(got, name)[1].cpu().numpy().tobytes(), getattr(before, name)[1].cpu().numpy().tobytes()
        assert a == b, name
    assert cnt.tolist()[0] >= 1 and cnt.tolist()[2] >= 1 and got.seq[0].item() == before.seq[0].item() + cnt.tolist()[0]
    # and the whole call equals the reference, which skips the finished sequence
    _run_case(llmie, logits, _params("penal_append", B), st0, True, [1, 0, k])


def test_mask_per_position_forces_the_pick(llmie):
    V, B, k = 1000, 2, 4
    rng = np.random.default_rng(36)
    logits = _logits(rng, B, k, V, torch.float16)
    forced = rng.integers(3, V, B * (k + 1))
    masks = np.zeros((B * (k + 1) + 1, V), bool)
    for r, t in enumerate(forced):
        masks[r, t] = True
    masks[-1] = True
    index = list(rng.permutation(B * (k + 1)))   # position r uses mask row index[r]
    index[3] = -1                                # one position unconstrained
    ext = Ext(B, k, V, masks=masks, mask_index=index)
    cnt, tok = _run_case(llmie, logits, _params("truncate", B), State(rng, B, V), True, [k, 2], ext=ext)
    assert list(cnt) == [k + 1, 3]
    for b in range(B):
        for i in range(cnt[b]):
            r = b * (k + 1) + i
            assert r == 3 or tok[b, i] == forced[index[r]]


def test_bias_bans_a_draft(llmie):
    V, B, k = 1000, 2, 4
    rng = np.random.default_rng(37)
    logits = _logits(rng, B, k, V, torch.float32)
    prm = [llmie.sampling_params([p]) for p in _params("greedy", B)]
    chain, _, _ = _reference(llmie, logits, prm, State(rng, B, V), True)
    ban = int(chain[0, 2])                       # what sequence 0 would pick at position 2 ...
    assert ban not in chain[0, :2]
    ext = Ext(B, k, V, bias=[[(ban, float("-inf")), (5, 1.5)], [(7, -2.0)]])
    cnt, tok = _run_case(llmie, logits, _params("greedy", B), State(rng, B, V), True, [k, k], ext=ext)
    assert list(cnt) == [k + 1, k + 1] and ban not in tok[0]   # ... is never emitted: another token takes its place


@pytest.mark.parametrize("top_n", [1, 5])
def test_top_n_of_every_row(llmie, top_n):
    V, B, k = 1000, 5, 4
    rng = np.random.default_rng(38)
    logits = _logits(rng, B, k, V, torch.float16)
    st0 = State(rng, B, V)
    st0.fin[4] = 1    # rows of rejected positions and of a finished sequence carry their top-N too
    cnt, _ = _run_case(llmie, logits, _params("truncate", B), st0, True, [0, 1, k, 2, 0], ext=Ext(B, k, V, top_n=top_n))
    assert list(cnt) == [1, 2, k + 1, 3, 0]


@pytest.mark.parametrize("step_dev", [False, True])
def test_shared_step(llmie, step_dev):
    V, B, k = 1000, 5, 4
    rng = np.random.default_rng(39)
    logits = _logits(rng, B, k, V, torch.float16)
    cnt, _ = _run_case(llmie, logits, _params("truncate", B), State(rng, B, V), True, _corrupt(B, k, 0), shared_step=41, step_dev=step_dev)
    assert list(cnt) == [1, 3, 5, 4, 2]


def _call(llmie, logits, params, st, drafts, k):
    B = drafts.shape[0]
    lp = torch.zeros((B, k + 1), dtype=torch.float32, device=DEV)
    tok, cnt = llmie.spec_verify(logits.reshape(B * (k + 1), -1), drafts, llmie.sampling_params(params), st.seq, st.fin, END,
                                 state=llmie.SpecState(st.last, st.cached, st.steps), history=st.hist, history_len=st.hlen, append=True,
                                 out_logprob=lp)
    torch.cuda.synchronize()
    return dict(tok=tok, cnt=cnt, lp=lp, **st.fields())


def test_determinism_and_slot_invariance(llmie):
    V, B, k = 32003, 5, 4
    rng = np.random.default_rng(40)
    logits = _logits(rng, B, k, V, torch.float16)
    params = _params("penal_append", B)
    st0 = State(rng, B, V)
    prm = [llmie.sampling_params([p]) for p in params]
    chain, _, _ = _reference(llmie, logits, prm, st0.clone(), True)
    drafts = chain[:, :k].copy()
    drafts[1, 2] = (drafts[1, 2] + 1) % V
    d = torch.from_numpy(drafts).to(DEV)
    a, b = _call(llmie, logits, params, st0.clone(), d, k), _call(llmie, logits, params, st0.clone(), d, k)
    for name in a:
        _same(name, a[name], b[name])
    # every sequence alone (slot 0 of a batch of 1) against its slot in the batch of 5
    for s in range(B):
        one = State(rng, 1, V)
        for name in one.fields():
            setattr(one, name, getattr(st0, name)[s:s + 1].clone())
        solo = _call(llmie, logits[s:s + 1].contiguous(), [params[s]], one, d[s:s + 1].contiguous(), k)
        for name in solo:
            _same("%s of sequence %d" % (name, s), solo[name], a[name][s:s + 1])
    assert a["cnt"].tolist() == [k + 1, 3, k + 1, k + 1, k + 1]


def test_nan_logits(llmie):
    V, B, k = 1000, 3, 4
    rng = np.random.default_rng(41)
    lg = _logits(rng, B, k, V, torch.float16)
    lg[0, 1, ::3] = float("nan")      # a third of a row
    lg[1, 2, :] = float("nan")        # a whole row: emits end_id and finishes
    lg[2, 0, 5:900] = float("nan")
    cnt, tok = _run_case(llmie, lg, _params("truncate", B), State(rng, B, V), True, [k] * B, ext=Ext(B, k, V, top_n=5))
    assert list(cnt) == [k + 1, 3, k + 1] and tok[1, 2] == END
