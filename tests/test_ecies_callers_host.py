"""kyber_amd.encrypt.ecies, sign/schnorr's Sign / Scheme and share.check_shares without a GPU: the three engine calls
(and the two fixed-base multiplications of Sign) answered by host stand-ins over the oracles, as tests/test_callers_host.py
does for share/poly -- what is under test is the host logic: who is asked what, in which order the random stream is
read, which errors are raised."""
import hashlib

import numpy as np
import pytest

from kyber_amd import _lib
from kyber_amd.util import blake2xb
from oracle import ed25519 as O
from tests import _dkg_cases as DC
from tests import _ecies_oracle as EO


@pytest.fixture
def ed(monkeypatch):
    from kyber_amd.group import edwards25519 as ed

    def rows(x):
        return [bytes(x[i:i + 32]) for i in range(0, len(x), 32)]

    def seal(r, pubs, msgs):
        r, pubs = rows(r), rows(pubs)
        pubs = pubs * len(r) if len(pubs) == 1 else pubs
        out = [EO.encrypt(a, p, m) for a, p, m in zip(r, pubs, msgs)]
        st = np.array([_lib.ST_BAD_POINT if c is None else 0 for c in out], dtype=np.uint8)
        return [c if c is not None else bytes(len(m) + 48) for c, m in zip(out, msgs)], st

    def open_(privs, ctx):
        privs = rows(privs)
        privs = privs * len(ctx) if len(privs) == 1 else privs
        res = [EO.decrypt(x, c) for x, c in zip(privs, ctx)]
        return [m if m is not None else b"" for m, _ in res], np.array([s for _, s in res], dtype=np.uint8)

    def deal_check(poly, idx, shares, commits, m, t):
        shares, commits = rows(shares), rows(commits)
        assert len(commits) == m * t
        ok = [DC.expected_ok(s, commits[k * t:(k + 1) * t], i) for k, i, s in zip(poly, idx, shares)]
        return np.array(ok, dtype=np.uint8), np.zeros(m, dtype=np.uint8)

    def mul_base(scalars, vartime=False, uniform=False):
        return np.frombuffer(b"".join(O.mul_base(s) for s in rows(scalars)), dtype=np.uint8).reshape(-1, 32)

    monkeypatch.setattr(ed, "batch_ecies_seal", seal)
    monkeypatch.setattr(ed, "batch_ecies_open", open_)
    monkeypatch.setattr(ed, "batch_deal_check", deal_check)
    monkeypatch.setattr(ed, "batch_mul_base", mul_base)
    return ed


def test_encrypt_draws_in_message_order_and_decrypt_raises_the_references_errors(ed):
    from kyber_amd.encrypt import ecies

    g = ed.NewSuite()
    x = ed.Scalar().Pick(blake2xb.New(b"receiver"))
    pub = g.Point().Mul(x, None)
    msgs = [b"", b"a share", bytes(range(100))]
    ctx = ecies.EncryptBatch(g, pub, msgs, hash=hashlib.sha256, rand=blake2xb.New(b"ecies"))
    rand = blake2xb.New(b"ecies")
    rs = [ed.Scalar().Pick(rand).v for _ in msgs]
    assert ctx == [EO.encrypt(r, pub.MarshalBinary(), m) for r, m in zip(rs, msgs)]
    assert ecies.Encrypt(g, pub, msgs[1], rand=blake2xb.New(b"ecies")) == EO.encrypt(rs[0], pub.MarshalBinary(), msgs[1])
    assert [ecies.Decrypt(g, x, c) for c in ctx] == msgs
    out, st = ecies.DecryptBatch(g, x, ctx + [ctx[1][:47], ctx[2][:-1] + b"\0", DC.UNDECODABLE + ctx[1][32:]], hash="sha256")
    assert out == msgs + [None, None, None]
    assert list(st) == [0, 0, 0, _lib.ST_ECIES_SHORT, _lib.ST_ECIES_AUTH, _lib.ST_BAD_POINT]
    with pytest.raises(ValueError, match="invalid ecies cipher"):
        ecies.Decrypt(g, x, ctx[1][:40])
    with pytest.raises(ValueError, match="message authentication failed"):
        ecies.Decrypt(g, x, ctx[2][:-1] + b"\0")
    with pytest.raises(ValueError, match="curve point"):
        ecies.Decrypt(g, x, DC.UNDECODABLE + ctx[1][32:])
    for bad in (hashlib.sha512, "sha3_256", hashlib.blake2b):
        with pytest.raises(ValueError, match="SHA-256"):
            ecies.Encrypt(g, pub, b"m", hash=bad)
        with pytest.raises(ValueError, match="SHA-256"):
            ecies.Decrypt(g, x, ctx[0], hash=bad)
    assert ecies.EncryptBatch(g, pub, []) == [] and ecies.DecryptBatch(g, x, [])[0] == []


def test_schnorr_sign_is_the_references_and_verifies_as_eddsa(ed):
    from kyber_amd.sign import schnorr

    g = ed.NewSuite()
    x = ed.Scalar().Pick(blake2xb.New(b"signer"))
    msg = b"a bundle's hash"
    sig = schnorr.Sign(g, x, msg, rand=blake2xb.New(b"nonce"))
    # schnorr.go:56-82 in integers
    k = int.from_bytes(ed.Scalar().Pick(blake2xb.New(b"nonce")).v, "little")
    R, A = O.mul_base(DC.le(k)), O.mul_base(x.v)
    h = int.from_bytes(hashlib.sha512(R + A + msg).digest(), "little") % O.L
    assert sig == R + DC.le((k + int.from_bytes(x.v, "little") * h) % O.L)
    # S B = R + h A, by the oracle
    S = int.from_bytes(sig[32:], "little")
    assert O.mul_base(DC.le(S)) == O.encode(O.add(O.decode(R), O.mul_int(h, O.decode(A))))
    s = schnorr.NewScheme(g, rand=blake2xb.New(b"nonce"))
    assert s.Sign(x, msg) == sig
    priv, pub = schnorr.NewScheme(g).NewKeyPair(blake2xb.New(b"signer"))
    assert priv.v == x.v and pub.MarshalBinary() == A


def test_check_shares_asks_the_engine_once_and_falls_back_for_another_base(ed, monkeypatch):
    from kyber_amd.share import poly

    g = ed.NewSuite()
    calls = []
    real = ed.batch_deal_check
    monkeypatch.setattr(ed, "batch_deal_check", lambda *a: (calls.append(a), real(*a))[1])
    t, n = 3, 5
    coeffs = [[DC.scalar(b"cs %d %d" % (k, j)) for j in range(t)] for k in range(n)]
    pubs = [poly.PubPoly(g, None, [ed.Point(O.mul_base(DC.le(c))) for c in row]) for row in coeffs]
    shares = [poly.PriShare(3, ed.Scalar(DC.le(DC.eval_scalar(row, 3)))) for row in coeffs]
    shares[2] = poly.PriShare(3, ed.Scalar(DC.le(DC.eval_scalar(coeffs[2], 3) + 1)))
    shares[4] = poly.PriShare(4, shares[4].V)
    assert poly.check_shares(pubs, shares) == [True, True, False, True, False]
    assert len(calls) == 1 and calls[0][0] == [0, 1, 2, 3, 4] and calls[0][1] == [3, 3, 3, 3, 4] and calls[0][4:] == (n, t)
    assert poly.check_shares([], []) == []
    # another base: polynomial by polynomial through PubPoly.Check
    seen = []
    monkeypatch.setattr(poly.PubPoly, "Check", lambda self, s: (seen.append(s.I), True)[1])
    other = [poly.PubPoly(g, ed.Point(O.mul_base(DC.le(7))), p.commits) for p in pubs]
    assert poly.check_shares(other, shares) == [True] * n and seen == [3, 3, 3, 3, 4] and len(calls) == 1
