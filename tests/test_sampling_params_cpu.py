"""Host side of the per-request sampler (no GPU): exports and signatures, the argument checks of llmie_sample_logits and
llmie_lm_head_sample_params (they fail before any launch), the workspace query, and api/model.hpp with a SamplingConfig
compiling for gfx950."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llm-inference-engine_amd")
NEW = ("llmie_sample_logits", "llmie_sample_logits_workspace_bytes", "llmie_lm_head_sample_params")


@pytest.fixture(scope="module")
def lib(llmie):
    return llmie.lib()


def test_symbols_exported_with_signatures(lib, llmie):
    for n in NEW:
        assert n in llmie.EXPORTS
        assert getattr(lib, n).argtypes is not None
    assert len(llmie._SIGS["llmie_sample_logits"]) == 19
    assert len(llmie._SIGS["llmie_lm_head_sample_params"]) == 25
    assert C.sizeof(llmie.SamplingParams) == 32
    assert callable(llmie.sample_logits) and callable(llmie.sampling_params)
    assert callable(llmie.Decoder.lm_head_sample_params)


FAKE = 0x1000   # never dereferenced: every call below fails its host-side checks first


def _call(lib, **kw):
    a = dict(logits=FAKE, batch=2, vocab=100, params=FAKE, history=None, stride=0, hlen=None, append=0, seq=FAKE, fin=FAKE,
             out=FAKE, lp=None, step=0, step_dev=None, end=2, ws=FAKE, ws_bytes=1 << 20, dtype=1, stream=None)
    a.update(kw)
    return lib.llmie_sample_logits(a["logits"], a["batch"], a["vocab"], a["params"], a["history"], a["stride"], a["hlen"],
                                   a["append"], a["seq"], a["fin"], a["out"], a["lp"], a["step"], a["step_dev"], a["end"],
                                   a["ws"], a["ws_bytes"], a["dtype"], a["stream"])


@pytest.mark.parametrize("kw,rc,msg", [
    (dict(logits=None), -1, "NULL"), (dict(params=None), -1, "NULL"), (dict(seq=None), -1, "NULL"),
    (dict(fin=None), -1, "NULL"), (dict(out=None), -1, "NULL"),
    (dict(batch=0), -1, "batch"), (dict(vocab=0), -1, "vocab"), (dict(vocab=-3), -1, "vocab"),
    (dict(stride=-1), -1, "history_stride"), (dict(stride=4), -1, "history"), (dict(stride=4, history=FAKE), -1, "history"),
    (dict(stride=9000, history=FAKE, hlen=FAKE), -2, "history_stride"), (dict(dtype=7), -2, "dtype"),
    (dict(ws=None), -4, "workspace"), (dict(ws_bytes=100), -4, "workspace"), (dict(ws=FAKE + 4), -4, "workspace"),
])
def test_host_checks(lib, kw, rc, msg):
    assert _call(lib, **kw) == rc
    assert msg in lib.llmie_last_error().decode()


def test_workspace_query_is_monotone(lib):
    assert lib.llmie_sample_logits_workspace_bytes(0, 100) == 0
    assert lib.llmie_sample_logits_workspace_bytes(1, 0) == 0
    prev_b = 0
    for b in (1, 2, 5, 64, 128, 1024):
        prev_v = 0
        for v in (1, 7, 1000, 32000, 32001, 128256):
            n = lib.llmie_sample_logits_workspace_bytes(b, v)
            assert n >= 4 * b * v and n % 16 == 0
            assert n >= prev_v
            prev_v = n
        assert prev_v >= prev_b
        prev_b = prev_v


def test_lm_head_sample_params_checks(lib):
    f = lib.llmie_lm_head_sample_params
    args = [None, FAKE, FAKE, FAKE, 0, FAKE, FAKE, None, 0, None, 0, FAKE, FAKE, FAKE, None, 1, 0, None, 2, None, None, 0,
            FAKE, 1 << 20, None]
    assert f(*args) == -1 and "decoder" in lib.llmie_last_error().decode()
    a = list(args)
    a[0], a[20] = FAKE, FAKE   # next_hidden without an embedding table
    assert f(*a) == -1 and "embedding" in lib.llmie_last_error().decode()
    a = list(args)
    a[0], a[21] = FAKE, 1      # advance_step without step_dev
    assert f(*a) == -1 and "step" in lib.llmie_last_error().decode()


def test_model_with_sampling_config_compiles():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "cfg.cpp")
        open(src, "w").write('''
#include "src/utils/model_utils.h"
int main() {
    BaseModel *m = llm::createDummyLLMModel<half>("x");
    LlamaModel<half> *lm = static_cast<LlamaModel<half> *>(m);
    LlamaModel<half>::SamplingConfig c;
    c.temperature = 0.7f; c.top_k = 40; c.top_p = 0.9f; c.min_p = 0.05f;
    c.repetition_penalty = 1.1f; c.presence_penalty = 0.2f; c.frequency_penalty = 0.1f; c.seed = 1234u;
    lm->sampling = c;
    bool d = LlamaModel<float>::SamplingConfig().isDefault() && !c.isDefault();
    return d ? 0 : 1;
}
''')
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", PKG, src],
                           cwd=d, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
