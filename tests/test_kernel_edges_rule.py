"""CPU test of the comparison rule that ``test_kernel_edges_gpu.py`` holds every kernel to
(``check``: |got - ref64| <= k*E32 + u*|ref64| + tiny, same finiteness, worst element reported)."""

import pytest
import torch

from .test_kernel_edges_gpu import DTYPES, F32, U, check


def test_check_rule_selftest():
    """A reference perturbed by one output ulp passes; one perturbed by 8*E32 + 2u|ref| fails; a single
    bad or non-finite element is found and named."""
    g = torch.Generator().manual_seed(0)
    ref64 = torch.randn(64, 33, generator=g, dtype=torch.float64) * 3
    ref32 = (ref64.float() * (1 + 2.0**-22)).double()  # a plain fp32 evaluation: off by a few fp32 ulps
    e32 = max((ref32 - ref64).abs().max().item(), 2.0**-23 * ref64.abs().max().item())
    sign = torch.where(torch.rand(ref64.shape, generator=g) < 0.5, -1.0, 1.0).double()
    for dt in DTYPES:
        ulp = U[dt] if dt != F32 else 2.0**-23
        assert check(ref64 + sign * ulp * ref64.abs(), ref64, ref32, dt, None) <= 4
        with pytest.raises(pytest.fail.Exception, match="worst element"):
            check(ref64 + sign * (8 * e32 + 2 * U[dt] * ref64.abs()), ref64, ref32, dt, None)
        one = ref64.clone()
        one[17, 5] += 8 * e32 + 2 * U[dt] * one[17, 5].abs()
        with pytest.raises(pytest.fail.Exception, match=r"worst element \(17, 5\)"):
            check(one, ref64, ref32, dt, None)
        nan = ref64.clone()
        nan[3, 4] = float("nan")
        with pytest.raises(pytest.fail.Exception, match=r"finiteness differs at \(3, 4\)"):
            check(nan, ref64, ref32, dt, None)
        inf32 = ref32.clone()
        inf32[0, 0] = float("inf")  # an fp32 reference that overflowed would make E32 meaningless
        with pytest.raises(AssertionError, match="disagree"):
            check(ref64, ref64, inf32, dt, None)
