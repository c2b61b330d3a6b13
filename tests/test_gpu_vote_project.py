"""GPU: ``ops.vote_project`` on the MI355X -- the bodies of tests/finish_cases.py, compared with numpy for equality."""
import pytest

import finish_cases as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("case", sorted(F.CASES))
def test_vote_project_case(case):
    F.CASES[case](DEV)
