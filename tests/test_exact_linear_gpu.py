"""Every projection route against the exactly known answer of tests/exact_linear_cases.py: equality of bits on every element.

One case per route of llmie_linear / _w8a16 / _w4a16 / _fp8 / _packed at the smallest shape that selects it (which route a case takes is
asserted without a GPU by tests/test_exact_linear_cpu.py, together with the conditions that make the arithmetic exact).  Each integer
case runs plain (large codes: the one rounding to fp16 is exercised), with bias + separate residual, and with the residual in place
(y == residual), which must also equal the separate form; probe cases run plain.  Outputs are pre-filled with NaN, every element is
compared, no tolerance anywhere: +0 and -0 are the only two patterns taken for one another (the sign of an exact zero sum is the
summation order's to decide).  The packed fp8 cases also run llmie_linear_fp8 on the row-major codes: the two kernels and the float64
reference must agree in every bit, with and without the K split.
"""
import numpy as np
import pytest
import torch

from exact_linear_cases import CASES, PROBES, build, epilogues

pytestmark = pytest.mark.gpu
DEV, F16 = "cuda", torch.float16


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    b = t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16).copy()
    b[b == 0x8000] = 0
    return b


def _assert_bits(got, expected, what):
    g, e = _bits(got), expected.view(np.uint16).copy()
    e[e == 0x8000] = 0
    bad = g != e
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        ulps = np.abs(g.astype(np.int64) - e.astype(np.int64))[bad]
        raise AssertionError("%s: %d of %d elements differ (largest distance %d fp16 patterns); first at %s: got 0x%04x, exact 0x%04x"
                             % (what, bad.sum(), bad.size, ulps.max(), i, g[i], e[i]))


class _Runner:
    """the device operands of one built case and run(y, residual, with_bias) for its entry point"""

    def __init__(self, llmie, b):
        c = self.case = b["case"]
        self.llmie, self.fmt, self.M, self.N = llmie, c["fmt"], c["M"], c["N"]
        if c["xoff"]:   # x at `xoff` fp16 elements past a 256-byte aligned allocation
            buf = torch.zeros(b["x"].size + c["xoff"], dtype=F16, device=DEV)
            self.x = buf[c["xoff"]:].view(b["x"].shape)
            self.x.copy_(_dev(b["x"]))
        else:
            self.x = _dev(b["x"])
        self.w, self.scale, self.bias = _dev(b["w"]), _dev(b["scale"]), _dev(b["bias"])
        self.code = {"f16": llmie.W_F16, "int8": llmie.W_INT8, "int4": llmie.W_INT4, "fp8": llmie.W_FP8}[self.fmt]
        if c["entry"] == "packed":
            self.packed, pscale = llmie.pack_weight(self.code, self.w, self.scale, False)
            self.pk_scale = pscale if self.fmt == "int4" else self.scale
        if self.fmt == "fp8":
            self.fp8_ws = torch.empty(llmie.linear_fp8_workspace_bytes(c["M"], c["K"], c["N"]), dtype=torch.uint8, device=DEV)

    def fresh(self):
        return torch.full((self.M, self.N), float("nan"), dtype=F16, device=DEV)

    def run(self, y, residual=None, with_bias=False, entry=None):
        ll, c = self.llmie, self.case
        bias = self.bias if with_bias else None
        entry = entry or c["entry"]
        if entry == "packed":
            ll.linear_packed(self.code, self.x, self.packed, self.pk_scale, y, self.N, residual=residual)
        elif self.fmt == "f16":
            ll.linear(self.x, self.w, y, bias=bias, residual=residual, workspace=c["ws"])
        elif self.fmt == "int8":
            ll.linear_w8a16(self.x, self.w, self.scale, y, bias=bias, residual=residual, workspace=c["ws"])
        elif self.fmt == "int4":
            ll.linear_w4a16(self.x, self.w, self.scale, y, c["group"], bias=bias, residual=residual, workspace=c["ws"])
        else:
            ll.linear_fp8(self.x, self.w, self.scale, y, self.fp8_ws, bias=bias, residual=residual)
        torch.cuda.synchronize()
        return y

    def run_or_stop(self, *a, **kw):
        """a device error ends the session: nothing more is launched on a GPU that has faulted"""
        try:
            return self.run(*a, **kw)
        except Exception as e:
            pytest.exit("%s: %s" % (self.case["id"], e), returncode=3)


ALL = CASES + PROBES


@pytest.mark.parametrize("case", ALL, ids=[c["id"] for c in ALL])
def test_route_is_bit_exact(llmie, case):
    for epi in epilogues(case):
        b = build(case, epi, check=False)      # (the conditions are asserted for these very cases by test_exact_linear_cpu.py)
        r = _Runner(llmie, b)
        both = case["entry"] == "packed" and case["fmt"] == "fp8"    # + the row-major fp8 kernel on the same codes
        if epi == "plain":
            _assert_bits(r.run_or_stop(r.fresh()), b["expected"], "%s plain" % case["id"])
            if both:
                _assert_bits(r.run_or_stop(r.fresh(), entry="linear"), b["expected"], "%s plain, llmie_linear_fp8" % case["id"])
            continue
        res = _dev(b["residual"])
        y1 = r.run_or_stop(r.fresh(), residual=res.clone(), with_bias=True)
        _assert_bits(y1, b["expected"], "%s bias + residual" % case["id"])
        y2 = res.clone()
        r.run_or_stop(y2, residual=y2, with_bias=True)
        _assert_bits(y2, b["expected"], "%s residual in place" % case["id"])
        assert torch.equal(y1.view(torch.int16), y2.view(torch.int16)), "%s: in place differs from the separate residual" % case["id"]
        if both:
            _assert_bits(r.run_or_stop(r.fresh(), residual=res.clone(), entry="linear"), b["expected"], "%s residual, llmie_linear_fp8" % case["id"])
