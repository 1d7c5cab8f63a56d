"""kyber_amd.encrypt.ecies, sign/schnorr's Sign / Scheme and share.check_shares on the GPU: the package layer over the
fused calls against the sequential restatements (tests/_ecies_oracle.py, schnorr.go:56-82 in integers) and against the
composed standing calls (PubPoly.Check, per-element Decrypt)."""
import hashlib

import pytest

from kyber_amd import _lib
from kyber_amd.util import blake2xb
from oracle import ed25519 as O
from tests import _dkg_cases as DC
from tests import _ecies_oracle as EO

pytestmark = pytest.mark.gpu


def test_ecies_package_matches_the_oracle_under_the_same_random_stream():
    from kyber_amd.encrypt import ecies
    from kyber_amd.group import edwards25519 as ed

    g = ed.NewSuite()
    keys = [ed.Scalar().Pick(blake2xb.New(b"receiver %d" % i)) for i in range(5)]
    pubs = [g.Point().Mul(x, None) for x in keys]
    msgs = [hashlib.shake_256(b"m %d" % i).digest(ln) for i, ln in enumerate((0, 32, 33, 100, 1000))]
    ctx = ecies.EncryptBatch(g, pubs, msgs, rand=blake2xb.New(b"deals"))
    rand = blake2xb.New(b"deals")
    assert ctx == [EO.encrypt(ed.Scalar().Pick(rand).v, p.MarshalBinary(), m) for p, m in zip(pubs, msgs)]
    out, st = ecies.DecryptBatch(g, keys, ctx)
    assert out == msgs and not st.any()
    assert [ecies.Decrypt(g, x, c, hash=hashlib.sha256) for x, c in zip(keys, ctx)] == msgs
    # one receiver of many ciphertexts, some of them not for it, cut short or without a point in front
    one = ecies.EncryptBatch(g, pubs[0], msgs, rand=blake2xb.New(b"to one"))
    mixed = one + [ctx[1], one[2][:47], DC.UNDECODABLE + one[3][32:]]
    out, st = ecies.DecryptBatch(g, keys[0], mixed)
    assert out == msgs + [None, None, None]
    assert list(st) == [0] * 5 + [_lib.ST_ECIES_AUTH, _lib.ST_ECIES_SHORT, _lib.ST_BAD_POINT]
    for c, code in zip(mixed, st):  # the batch call is the single call, element by element
        assert EO.decrypt(keys[0].v, c)[1] == code
        if code:
            with pytest.raises(ValueError):
                ecies.Decrypt(g, keys[0], c)
    assert ecies.Decrypt(g, keys[0], ecies.Encrypt(g, pubs[0], b"os randomness")) == b"os randomness"


def test_schnorr_sign_matches_the_restatement_and_verifies():
    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.sign import schnorr

    g = ed.NewSuite()
    scheme = schnorr.NewScheme(g, rand=blake2xb.New(b"nonces"))
    x, pub = scheme.NewKeyPair(blake2xb.New(b"signer"))
    rand = blake2xb.New(b"nonces")
    for msg in (b"", b"a deal bundle's hash", bytes(300)):
        sig = scheme.Sign(x, msg)
        k = int.from_bytes(ed.Scalar().Pick(rand).v, "little")
        R = O.mul_base(DC.le(k))
        h = int.from_bytes(hashlib.sha512(R + pub.MarshalBinary() + msg).digest(), "little") % O.L
        assert sig == R + DC.le((k + int.from_bytes(x.v, "little") * h) % O.L)
        scheme.Verify(pub, msg, sig)
        for bad in (sig[:63] + bytes([sig[63] ^ 1]), bytes([sig[0] ^ 1]) + sig[1:], sig[:-1]):
            with pytest.raises(ValueError):
                scheme.Verify(pub, msg, bad)
        with pytest.raises(ValueError):
            scheme.Verify(pub, msg + b"x", sig)


def test_check_shares_equals_pubpoly_check():
    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.share import poly

    g = ed.NewSuite()
    t, n = 4, 9
    rand = blake2xb.New(b"dealers").Read
    pris = [poly.PriPoly.new(g, t, rand=rand) for _ in range(n)]
    pubs = [p.Commit() for p in pris]
    me = 6
    shares = [p.Eval(me) for p in pris]
    shares[3] = poly.PriShare(me, g.Scalar().Add(shares[3].V, g.Scalar().One()))
    shares[5] = pris[5].Eval(me + 1)
    shares[7] = poly.PriShare(me, ed.Scalar((int.from_bytes(shares[7].V.v, "little") + O.L).to_bytes(32, "little")))
    want = [True] * n
    want[3] = False
    assert poly.check_shares(pubs, shares) == want  # (shares[5] is right for its own index)
    shares[5] = poly.PriShare(me, shares[5].V)
    want[5] = False
    got = poly.check_shares(pubs, shares)
    assert got == want == [p.Check(s) for p, s in zip(pubs, shares)]
