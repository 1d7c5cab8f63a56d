"""The sequential restatement tests/_dkg_oracle.py alone, through the reference's scenarios (dkg_test.go,
dkg_vartime_test.go) with n = 5..10, t = 3..8: each ends in testResults' property -- any t shares of QUAL interpolate to a
secret whose commitment is Commits[0], and all nodes hold the same commits."""
import pytest

from tests import _dkg_scenarios as S


@pytest.mark.parametrize("name", sorted(S.SCENARIOS))
def test_scenario(name):
    S.run(S.OracleKit(), name)
