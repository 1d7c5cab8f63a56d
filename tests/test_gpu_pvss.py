"""share/pvss end to end on the GPU (kyber_amd/share/pvss.py over the batch engine) against the oracle's restatement of
pvss.go, given the same nonce stream: every share, proof and challenge equal, corrupted shares dropped, too few shares an
error."""
import numpy as np
import pytest

from kyber_amd.util import blake2xb as X
from oracle import ed25519 as O
from tests import _pvss_oracle as PO

pytestmark = pytest.mark.gpu


def _tuple(s):
    return (s.S.I, s.S.V.MarshalBinary(), (s.P.C, s.P.R, s.P.VG, s.P.VH))


@pytest.mark.parametrize("n,t", [(10, 7), (64, 33), (1000, 501)])
def test_round_equals_the_oracle_and_recovers_the_secret(n, t):
    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.proof import dleq
    from kyber_amd.share import poly, pvss

    seed = b"pvss %d %d" % (n, t)
    keys = X.New(seed + b" keys").Read
    xs = [X.pick(keys) for _ in range(n)]
    Xs = [bytes(r) for r in ed.batch_mul_base(np.frombuffer(b"".join(xs), dtype=np.uint8).reshape(n, 32))]
    H = O.encode(O.mul_int(0xC0FFEE, O.B))
    secret = X.pick(keys)
    G = PO.BASE

    # (1) the dealer: the engine and the oracle read the same stream
    rand, orand = X.New(seed), X.New(seed).Read
    shares, pub = pvss.EncShares(H, Xs, secret, t, rand)
    o_shares, o_commits, o_coeffs = PO.enc_shares(H, Xs, secret, t, orand)
    assert [_tuple(s) for s in shares] == o_shares
    assert [c.MarshalBinary() for c in pub.Info()[1]] == o_commits
    sH = [bytes(r) for r in pvss.computeCommitments(n, pub.Info()[1])]
    assert sH == (PO.compute_commitments(n, o_commits) if n <= 64 else PO.compute_commitments(n, o_commits, o_coeffs, H))
    gc = pvss.computeGlobalChallenge(n, pub, shares)
    assert gc == PO.global_challenge(sH, o_shares) and all(s.P.C == gc for s in shares)

    # (2) anyone: verify the encrypted shares; k corrupted ones are dropped, exactly those
    K, E = pvss.VerifyEncShareBatch(H, Xs, sH, pub, shares)
    assert K == Xs and E == shares
    k = [1, n // 2, n - 1]
    spoiled = list(shares)
    spoiled[k[0]] = pvss.PubVerShare(shares[k[0]].S, dleq.Proof(shares[k[0]].P.C, PO.sc(PO.le(shares[k[0]].P.R) + 1), shares[k[0]].P.VG, shares[k[0]].P.VH))
    spoiled[k[1]] = pvss.PubVerShare(poly.PubShare(k[1], ed.Point(shares[k[1] - 1].S.V.MarshalBinary())), shares[k[1]].P)
    spoiled[k[2]] = pvss.PubVerShare(shares[k[2]].S, dleq.Proof(shares[k[2]].P.C, shares[k[2]].P.R, shares[k[2]].P.VH, shares[k[2]].P.VG))
    K2, E2 = pvss.VerifyEncShareBatch(H, Xs, sH, pub, spoiled)
    # (the global challenge hashes S.V, VG and VH, so a spoiled share moves it for every share: none verifies, as in the reference)
    assert K2 == [] and E2 == []
    ok, st = pvss._verify_enc(H, Xs, sH, gc, spoiled)
    assert list(np.flatnonzero(~ok)) == k and not st.any()
    with pytest.raises(pvss.PVSSError) as e:
        pvss.VerifyEncShare(H, Xs[k[0]], sH[k[0]], gc, spoiled[k[0]])
    assert e.value.err == pvss.ErrEncVerification and PO.verify_enc_share(H, Xs[k[0]], sH[k[0]], gc, o_shares[k[0]][:2] + (_tuple(spoiled[k[0]])[2],)) == PO.ErrEncVerification
    with pytest.raises(pvss.PVSSError) as e:
        pvss.VerifyEncShare(H, Xs[0], sH[0], PO.sc(PO.le(gc) + 1), shares[0])
    assert e.value.err == pvss.ErrGlobalChallengeVerification

    # (3) the trustees decrypt (each with its own key) and prove it; the corrupted shares are left out of K, E and D
    drand, odrand = X.New(seed + b" dec"), X.New(seed + b" dec").Read
    K, E, D = pvss.DecShares(H, Xs, sH, xs, gc, spoiled, drand)
    keep = [i for i in range(n) if i not in k]
    assert K == [Xs[i] for i in keep] and E == [shares[i] for i in keep] and [d.S.I for d in D] == keep
    o_D = []
    for i in keep:
        d, err = PO.dec_share(H, Xs[i], sH[i], xs[i], gc, o_shares[i], odrand)
        assert err is None
        o_D.append(d)
    assert [_tuple(d) for d in D] == o_D
    assert PO.dec_share(H, Xs[k[0]], sH[k[0]], xs[k[0]], gc, _tuple(spoiled[k[0]]), odrand)[1] == PO.ErrEncVerification
    one = pvss.DecShare(H, Xs[0], sH[0], xs[0], gc, shares[0], X.New(seed + b" dec"))
    assert _tuple(one) == o_D[0]
    # DecShareBatch: ONE trustee's key over shares of several sharings, each with its own expected challenge
    Kb, Eb, Db = pvss.DecShareBatch(H, [Xs[0]] * 3, [sH[0]] * 3, xs[0], [gc, PO.sc(PO.le(gc) + 1), gc], [shares[0]] * 3, X.New(seed + b" dec"))
    assert len(Db) == 2 and _tuple(Db[0]) == o_D[0] and Eb == [shares[0]] * 2

    # (4) anyone: verify the decrypted shares and recover s * G
    want = O.mul_base(secret)
    assert pvss.VerifyDecShareBatch(G, K, E, D) == D
    got = pvss.RecoverSecret(G, K, E, D, t, n)
    assert got.MarshalBinary() == want
    if n <= 64:
        assert PO.recover_secret(G, K, [_tuple(e) for e in E], o_D, t, n) == (want, None)
    # corrupted decrypted shares: nulled values (pvss_test.go:169-172), a moved response, a challenge off by one
    null = ed.Point()
    D2 = list(D)
    D2[0] = pvss.PubVerShare(poly.PubShare(D[0].S.I, null), D[0].P)
    D2[2] = pvss.PubVerShare(D[2].S, dleq.Proof(D[2].P.C, PO.sc(PO.le(D[2].P.R) + 1), D[2].P.VG, D[2].P.VH))
    D2[3] = pvss.PubVerShare(D[3].S, dleq.Proof(PO.sc(PO.le(D[3].P.C) + 1), D[3].P.R, D[3].P.VG, D[3].P.VH))
    good = pvss.VerifyDecShareBatch(G, K, E, D2)
    assert good == [d for j, d in enumerate(D2) if j not in (0, 2, 3)]
    for j, err, oerr in ((0, pvss.ErrDecVerification, PO.ErrDecVerification), (2, pvss.ErrDecVerification, PO.ErrDecVerification),
                         (3, pvss.ErrDecShareChallengeVerification, PO.ErrDecShareChallengeVerification)):
        with pytest.raises(pvss.PVSSError) as e:
            pvss.VerifyDecShare(G, K[j], E[j], D2[j])
        assert e.value.err == err and PO.verify_dec_share(G, K[j], _tuple(E[j]), _tuple(D2[j])) == oerr
    if len(keep) - 3 >= t:
        assert pvss.RecoverSecret(G, K, E, D2, t, n).MarshalBinary() == want
    # fewer than t valid shares: ErrTooFewShares
    D3 = [pvss.PubVerShare(poly.PubShare(d.S.I, null), d.P) if j <= len(D) - t else d for j, d in enumerate(D)]
    with pytest.raises(pvss.PVSSError) as e:
        pvss.RecoverSecret(G, K, E, D3, t, n)
    assert e.value.err == pvss.ErrTooFewShares
