"""kyber_amd.share.dkg_rabin without a GPU: the engine behind it replaced as in tests/test_vss_callers_host.py (the fused
share/vss calls answered by the lane programs compiled for the CPU, the standing calls by stand-ins over the oracles), every
scenario of tests/_dkg_rabin_scenarios.py -- dkg_test.go's, `fullExchange` included, 7 participants with t = 4 -- must leave
the transcript the sequential oracle (tests/_dkg_rabin_oracle.py) leaves, byte for byte, under the same random stream, the
error strings included; and the keys of a full Rabin exchange carry sign/dss (dss_test.go's genDistSecret).

Limit of the check: see tests/_dkg_rabin_oracle.py -- no bytes of the Go program are pinned; the algebra is (one set of
commitments for all, every share on them, t shares recover the secret behind Public())."""
import numpy as np
import pytest

from oracle import ed25519 as O
from tests import _dkg_oracle as DO
from tests import _dkg_rabin_scenarios as SC
from tests.test_vss_callers_host import calls as vss_calls, harness  # noqa: F401  (fixtures)


@pytest.fixture
def calls(vss_calls, monkeypatch):
    """... plus the MSM behind PubPoly.Eval"""
    from kyber_amd.group import edwards25519 as ed

    def msm(scalars, points):
        s, p = bytes(scalars), bytes(points)
        acc = O.IDENTITY
        for i in range(0, len(s), 32):
            acc = O.add(acc, O.mul_int(int.from_bytes(s[i:i + 32], "little"), O.decode(p[i:i + 32])))
        return np.frombuffer(O.encode(acc), dtype=np.uint8).copy(), np.zeros(1, dtype=np.uint8)

    monkeypatch.setattr(ed, "msm", msm)
    return vss_calls


@pytest.fixture(scope="module")
def oracle_transcripts():
    return {name: f(SC.Kit(True)) for name, f in SC.SCENARIOS.items()}


@pytest.fixture(scope="module")
def product_transcripts():
    return {}


@pytest.mark.parametrize("name", list(SC.SCENARIOS))
def test_scenario_leaves_the_oracles_transcript(calls, oracle_transcripts, product_transcripts, name):
    product_transcripts[name] = SC.SCENARIOS[name](SC.Kit(False))
    assert product_transcripts[name] == oracle_transcripts[name]


ERRORS = ("dkg: own public key not found in list of participants", "dkg: dist deal out of bounds index",
          "dkg: already received dist deal from same index", "dkg: complaint received but no deal for it",
          "dkg: Justification received but no deal for it", "dkg: can't give SecretCommits if deal not certified",
          "dkg: distributed key not certified", "dkg: secretcommits received with index out of bounds",
          "dkg: secretcommits from a non QUAL member", "dkg: secretcommits received with wrong session id",
          "schnorr: invalid signature", "dkg: protocol not finished: 0 commitments missing",
          "dkg: commitcomplaint with unknown issuer", "dkg: complaintcommit from non-qual member",
          "dkg: commitcomplaint linked to unknown verifier",
          "dkg: verifying deal: vss: share does not verify against commitments in Deal",
          "dkg: complaint about non received commitments", "dkg: invalid complaint, deal verifying",
          "dkg: commitments not invalidated by any complaints", "dkg: reconstruct commits with invalid verifier index",
          "dkg: reconstruct commits invalid session id")


def test_the_scenarios_meet_the_reference_error_strings(oracle_transcripts):
    """A pin of the ORACLE's transcripts (the parametrised test above holds the product's equal to them): every error
    string of dkg.go that a scenario can reach is in them, and the steps answer as dkg_test.go asserts"""
    flat = repr(oracle_transcripts)
    for msg in ERRORS:
        assert msg in flat, msg
    t = oracle_transcripts
    before, after = t["set_timeout"]
    assert before[1] == [[]] * 7 and before[2] == [False] * 7 and after[1] == [list(range(7))] * 7 and after[2] == [True] * 7
    pr = dict((r[0], r) for r in t["process_response"])
    assert pr["complaint"][4] is False and pr["complaint 12"][3] is False and pr["deal 2 -> 0"][3] is True
    assert pr["justification"][1] is None and pr["justification"][2:4] == (0, 1) and pr["justification 2"][1] is None and pr["justification 2"][2:4] == (2, 1)
    assert pr["response from 1"][1] == (None, None) and pr["process justification"][1] == (None, None)
    rc = dict((r[0], r) for r in t["reconstruct_commits"])
    assert rc["reconstructed already"][1:] == ((None, None), []) and rc["good"][1:] == ((None, None), [1], False) and rc["again"][2] == 1
    assert rc["recovered"][1] is True and rc["recovered"][2] == rc["recovered"][3] and rc["recovered"][4:] == (True, False)
    sc = dict((r[0], r) for r in t["secret_commits"])
    assert sc["own signature"][1] is None and sc["complaint"][1] is None and sc["complaint"][2:4] == (1, 0) and sc["good"][1:] == ((None, None), True)
    assert t["complaint_commits"][0][1] is None and t["secret_commits"][2][1] == [list(range(7))] * 7  # QUAL ascending


def _one_key(transcript):
    keys = [r for r in transcript if r[0] == "keys"][0][1]
    commits = keys[0][0]
    assert all(k[0] == commits for k in keys) and [k[1] for k in keys] == list(range(7))
    for c, i, v in keys:
        assert O.mul_base(v) == DO.pub_eval(commits, i)
    secret = DO.recover_secret([(i, int.from_bytes(v, "little")) for _, i, v in keys[2:6]], 4)
    assert DO.base_mul(secret) == commits[0]
    _, s, sb, pub = [r for r in transcript if r[0] == "secret"][0]
    assert s == DO.le(secret) and sb == pub == commits[0]  # share.RecoverSecret over all seven, as TestDistKeyShare ends


def test_the_distributed_key_is_one_key(calls, oracle_transcripts):
    """the algebra that pins the exchange -- one set of commitments, every share on them, t shares recover Public()'s secret
    -- in big integers on the bytes of the ORACLE's DistKeyShares and on those of the PRODUCT's"""
    _one_key(oracle_transcripts["dist_key_share"])
    _one_key(SC.dist_key_share(SC.Kit(False)))


def test_dss_over_the_keys_of_a_full_rabin_exchange(calls):
    """dss_test.go's fixtures: genDistSecret twice (the long-term key, the random key), then TestDSSSignature on them"""
    from kyber_amd.sign import dss
    from tests import _ed_verify_oracle as V

    kit = SC.Kit(False)
    w = SC.World(kit, b"dss over dkg")
    _, longs = SC.gen_dist_secret(kit, w)
    _, randoms = SC.gen_dist_secret(kit, w)
    nodes = [dss.NewDSS(w.S, w.secrets[i], w.pubs, longs[i], randoms[i], b"hello", SC.T, rand=w.S.RandomStream()) for i in range(SC.N)]
    pss = [d.PartialSig() for d in nodes]
    for i, d in enumerate(nodes):
        for j, ps in enumerate(pss):
            if i != j:
                d.ProcessPartialSig(ps)
    sigs = [d.Signature() for d in nodes]
    assert len(set(sigs)) == 1
    assert V.verify_with_checks(longs[0].Public().MarshalBinary(), b"hello", sigs[0]) == (True, V.OK)
    dss.Verify(longs[0].Public(), b"hello", sigs[0])
