"""The crafted cohort of tests/test_gpu_call_domain.py is not vacuous: tests/call_domain_case.case asserts, from the oracle and the
inputs alone, that it has calls (with Q = 100 and with mid-range Q, below and above 2^24 reads), queued-but-not-called pairs at
RD >= 2^24, pairs the fp32 test skips, and pairs for each arm of the drain (m > 0, m == 0, m < 0).  No GPU."""
import pytest

from tests import call_domain_case


@pytest.mark.parametrize("with_rd", [False, True])
@pytest.mark.parametrize("cov", [1, 100])
def test_the_case_holds_what_it_is_meant_to_hold(cov, with_rd):
    c = call_domain_case.case(cov, with_rd)
    print(cov, with_rd, c["stats"])
    assert c["stats"]["records"] == 685 and c["exp"]["call_mask"].shape == (5, 137)
