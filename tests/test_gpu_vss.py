"""kyber_amd.share.vss.pedersen and .rabin on the device: every scenario of the reference's two vss_test.go files
(tests/_vss_scenarios.py) run over the product with the engine behind it, against the transcript the sequential oracle
(tests/_vss_oracle.py) leaves under the same random streams -- byte for byte: encrypted deals, responses,
justifications, recovered secrets and every error string in order.  The batch entries run the whole protocol too, and
a protocol of 65 verifiers takes Dealer.EncryptedDeals() past a wave."""
import pytest

from tests import _vss_scenarios as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle_transcripts():
    K = SC.OracleKit()
    return {name: f(K) for name, f in SC.SCENARIOS.items()}


@pytest.mark.parametrize("name", list(SC.SCENARIOS))
def test_scenario_on_the_device_leaves_the_oracles_transcript(oracle_transcripts, name):
    assert SC.SCENARIOS[name](SC.ProductKit()) == oracle_transcripts[name]


@pytest.fixture(scope="module")
def rabin_transcripts():
    K = SC.OracleKit("rabin")
    return {name: f(K) for name, f in SC.RABIN_SCENARIOS.items()}


@pytest.mark.parametrize("name", list(SC.RABIN_SCENARIOS))
def test_rabin_scenario_on_the_device_leaves_the_oracles_transcript(rabin_transcripts, name):
    assert SC.RABIN_SCENARIOS[name](SC.ProductKit("rabin")) == rabin_transcripts[name]


def test_a_rabin_protocol_of_65_verifiers_through_the_batch_entries():
    """65 deals at threshold 33 under the 128-byte context: EncryptedDeals() is one seal and equals the loop;
    process_encrypted_deals is one deal_check2 with one H; the oracle is compared on the first and the last deal"""
    n = 65
    K, KO = SC.ProductKit("rabin"), SC.OracleKit("rabin")
    a, b = SC.World(K, n=n).genDealer(), SC.World(K, n=n).genDealer()
    batch = a.EncryptedDeals()
    assert [SC.t_enc(e) for e in batch] == [SC.t_enc(b.EncryptedDeal(i)) for i in range(n)]
    o = SC.World(KO, n=n).genDealer()
    for i in range(n):
        if i in (0, 64):
            assert SC.t_enc(o.EncryptedDeal(i)) == SC.t_enc(batch[i]), i
        else:
            KO.pick(o.read), KO.pick(o.read)
    w = SC.World(K, n=n)
    dealer, verifiers = w.genAll()
    resps = K.process_deals(verifiers, dealer.EncryptedDeals())
    assert all(not isinstance(r, Exception) and r.Approved for r in resps)
    assert K.process_responses(dealer, resps) == [None] * n and dealer.DealCertified()


def test_a_protocol_of_65_verifiers_through_the_batch_entries():
    """Dealer.EncryptedDeals() of 65 deals at threshold 33 is one seal; the loop over EncryptedDeal(i) gives the same
    bytes; the oracle is compared on the first, the 64th and the last deal (pure Python cannot seal 65 in seconds)"""
    n = 65
    K, KO = SC.ProductKit(), SC.OracleKit()
    a, b = SC.World(K, n=n).genDealer(), SC.World(K, n=n).genDealer()
    batch = a.EncryptedDeals()
    assert [SC.t_enc(e) for e in batch] == [SC.t_enc(b.EncryptedDeal(i)) for i in range(n)]
    o = SC.World(KO, n=n).genDealer()
    for i in range(n):  # the oracle's stream moves as the dealer's does: two draws a deal
        if i in (0, 63, 64):
            assert SC.t_enc(o.EncryptedDeal(i)) == SC.t_enc(batch[i]), i
        else:
            KO.pick(o.read), KO.pick(o.read)
    w = SC.World(K, n=n)
    dealer, verifiers = w.genAll()
    resps = K.process_deals(verifiers, dealer.EncryptedDeals())
    assert all(not isinstance(r, Exception) and r.StatusApproved for r in resps)
    assert K.process_responses(dealer, resps) == [None] * n and dealer.DealCertified()
    assert K.process_responses(verifiers[64], resps[:64]) == [None] * 64 and verifiers[64].DealCertified()
