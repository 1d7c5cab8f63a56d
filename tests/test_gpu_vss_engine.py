"""kyb_ed25519_schnorr_sign, kyb_ed25519_vss_seal / _open and kyb_ed25519_deal_check2 on the GPU, host and _dev entries,
against the sequential oracle (tests/_vss_oracle.py, on the labelled cases of tests/_vss_cases.py) and against the
composed standing calls (mul_base, mul, verify): batch sizes either side of the wave and the block, every message length
of the block edges and of a real deal in one batch, an odd byte offset in front of an empty first element, every stride
at both values, rejects planted in first, middle and last place, and one batch across the piece boundary."""
import random

import numpy as np
import pytest

from kyber_amd import _lib
from oracle import ed25519 as O
from tests import _dkg_cases as DC
from tests import _oracle_c as OC
from tests import _vss_cases as VC
from tests import _vss_oracle as VO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ed():
    from kyber_amd.group import edwards25519

    return edwards25519


@pytest.fixture(scope="module")
def sch():
    from kyber_amd.sign import schnorr

    return schnorr


def _dev_msgs(msgs):
    import torch

    blob = torch.from_numpy(np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy()).cuda()
    off = torch.from_numpy(np.cumsum([0] + [len(m) for m in msgs]).astype(np.int64)).cuda()
    return blob, off


def _dev_split(blob, off, n):
    b, o = blob.cpu().numpy(), off.cpu().numpy()
    return [bytes(b[o[i]:o[i + 1]]) for i in range(n)]


# -------------------------------------------------------------------------------------------------------- schnorr.Sign
@pytest.mark.parametrize("n", VC.SIZES)
def test_sign_matches_the_oracle_and_verifies(ed, sch, n):
    k, x, m, want = VC.sign_pool()
    lo = VC.POOL - 3 - n  # (the three rows of scalars at and above 2^255 have a test of their own)
    sigs, st = ed.batch_schnorr_sign(k[lo:lo + n], x[lo:lo + n], m[lo:lo + n])
    assert not st.any() and [bytes(s) for s in sigs] == want[lo:lo + n]
    pubs = ed.batch_mul_base(x[lo:lo + n])  # the composed standing calls: A and R are mul_base's, the verdict verify's
    assert np.array_equal(np.asarray(sigs)[:, :32], ed.batch_mul_base(k[lo:lo + n]))
    assert sch.batch_verify_with_checks(pubs, m[lo:lo + n], sigs).all()
    moved = np.asarray(sigs).copy()
    moved[n // 2, 40] ^= 1
    assert list(sch.batch_verify_with_checks(pubs, m[lo:lo + n], moved)) == [0 if i == n // 2 else 1 for i in range(n)]


def test_sign_one_signer_any_scalar_and_the_device_entry(ed):
    import torch

    k, x, m, want = VC.sign_pool()
    sigs, _ = ed.batch_schnorr_sign(k[:65], x[9], m[:65])
    assert [bytes(s) for s in sigs] == [VO.schnorr_sign(bytes(k[i]), bytes(x[9]), m[i]) for i in range(65)]
    sigs, _ = ed.batch_schnorr_sign(k[-3:], x[-3:], m[-3:])
    assert [bytes(s) for s in sigs] == want[-3:]
    n = 129
    sigs, st = ed.batch_schnorr_sign(torch.from_numpy(k[:n]).cuda(), torch.from_numpy(x[:n]).cuda(), _dev_msgs(m[:n]))
    torch.cuda.synchronize()
    assert not st.any().item() and [bytes(s) for s in sigs.cpu().numpy()] == want[:n]
    sigs, _ = ed.batch_schnorr_sign(torch.from_numpy(k[:n]).cuda(), torch.from_numpy(x[4:5]).cuda(), _dev_msgs(m[:n]))
    assert bytes(sigs[n - 1].cpu().numpy()) == VO.schnorr_sign(bytes(k[n - 1]), bytes(x[4]), m[n - 1])


def test_sign_batch_draws_as_sequential_signs_do(ed, sch):
    from kyber_amd.util import blake2xb

    g = ed.NewSuite()
    privs = [g.Scalar().Pick(blake2xb.New(b"signer %d" % i)) for i in range(5)]
    msgs = [b"", b"a", bytes(47), bytes(range(48)), b"deal" * 40]
    seq_stream, batch_stream = blake2xb.New(b"nonces"), blake2xb.New(b"nonces")
    seq = [sch.Sign(g, p, m, rand=seq_stream) for p, m in zip(privs, msgs)]
    assert sch.SignBatch(g, privs, msgs, rand=batch_stream) == seq
    assert seq_stream.Read(16) == batch_stream.Read(16)  # both streams stand at the same place
    one = sch.SignBatch(g, privs[0], msgs, rand=blake2xb.New(b"one"))
    s = blake2xb.New(b"one")
    assert one == [sch.Sign(g, privs[0], m, rand=s) for m in msgs]
    assert sch.SignBatch(g, [], [], rand=batch_stream) == []
    for p, m, sig in zip(privs, msgs, seq):
        sch.Verify(g, g.Point().Mul(p, None), m, sig)


# ------------------------------------------------------------------------------------------------------ seal and open
def _check_seal(keys, sigs, ciphers, st, want, msgs):
    for i, w in enumerate(want):
        if w is None:
            assert st[i] == _lib.ST_BAD_POINT and (bytes(keys[i]), bytes(sigs[i]), ciphers[i]) == (bytes(32), bytes(64), bytes(len(msgs[i]) + 16)), i
        else:
            assert st[i] == 0 and (bytes(keys[i]), bytes(sigs[i]), ciphers[i]) == w, i


@pytest.mark.parametrize("per_element_ctx", [False, True])
@pytest.mark.parametrize("n", VC.SIZES)
def test_seal_matches_the_oracle_and_round_trips(ed, sch, n, per_element_ctx):
    dh, k, priv, pub, vpriv, vpubs, ctx, m, want = VC.seal_pool(per_element_ctx)
    s = slice(VC.POOL - n, VC.POOL)
    c = ctx[s] if per_element_ctx else ctx
    keys, sigs, ciphers, st = ed.batch_vss_seal(dh[s], k[s], priv, pub, vpubs[s], c, m[s])
    _check_seal(keys, sigs, ciphers, st, want[s], m[s])
    # the composed standing calls: DHKey is mul_base's, the signature passes verify under the dealer's key
    assert np.array_equal(np.asarray(keys)[np.asarray(st) == 0], ed.batch_mul_base(dh[s])[np.asarray(st) == 0])
    ok = sch.batch_verify_with_checks([pub] * n, [bytes(x) for x in keys], sigs)
    assert list(ok) == [0 if w is None else 1 for w in want[s]]
    # decryptDeal: verify (above), then open under the verifier's key
    back, st2 = ed.batch_vss_open(vpriv[s], keys, c, ciphers)
    for j, i in enumerate(range(VC.POOL - n, VC.POOL)):
        if want[i] is None:  # zero bytes for a key: the identity's y is 1, so y = 0 decodes or not as the oracle says
            assert (st2[j], back[j]) == (VO.open_(bytes(vpriv[i]), bytes(32), bytes(c[j] if per_element_ctx else c[0]), ciphers[j])[1], b""), i
        elif i in VC.SPECIAL:  # a key nobody here holds the scalar of
            assert st2[j] == _lib.ST_ECIES_AUTH and back[j] == b"", i
        else:
            assert st2[j] == 0 and back[j] == m[i], i


def test_a_batch_of_one_and_a_front_cut(ed):
    dh, k, priv, pub, vpriv, vpubs, ctx, m, want = VC.seal_pool(False)
    for lo, hi in ((0, 1), (1, 2), (0, 2 * len(VC.LENGTHS))):
        keys, sigs, ciphers, st = ed.batch_vss_seal(dh[lo:hi], k[lo:hi], priv, pub, vpubs[lo:hi], ctx, m[lo:hi])
        _check_seal(keys, sigs, ciphers, st, want[lo:hi], m[lo:hi])


@pytest.mark.parametrize("per_element_ctx", [False, True])
def test_open_of_the_tampered_the_short_and_the_undecodable(ed, per_element_ctx):
    dh, k, priv, pub, vpriv, vpubs, ctx, m, want = VC.seal_pool(per_element_ctx)
    i = 5
    good = [j for j in range(3, 3 + len(VC.LENGTHS)) if j not in VC.SPECIAL]
    cx = bytes(ctx[i] if per_element_ctx else ctx[0])
    keys, sigs, ciphers, st = ed.batch_vss_seal(dh[good], k[good], priv, pub, np.repeat(vpubs[i:i + 1], len(good), axis=0), cx,
                                                [m[j] for j in good])
    assert not st.any()
    sealed = [(bytes(a), bytes(b), c) for a, b, c in zip(keys, sigs, ciphers)]
    rows = VC.open_cases(bytes(vpriv[i]), cx, sealed)
    random.Random(3).shuffle(rows)
    rows = [r for r in rows if r[2] == "undecodable key"][:1] + rows + [r for r in rows if r[2] == "short"][:1]  # first and last place
    cxs = np.repeat(np.frombuffer(cx, dtype=np.uint8)[None, :], len(rows), axis=0) if per_element_ctx else cx
    back, st = ed.batch_vss_open(vpriv[i], b"".join(r[0] for r in rows), cxs, [r[1] for r in rows])
    seen = set()
    for j, (key, cipher, label) in enumerate(rows):
        msg, code = VO.open_(bytes(vpriv[i]), key, cx, cipher)
        assert st[j] == code and back[j] == (msg if msg is not None else b""), (j, label)
        seen.add(code)
    assert seen == {0, _lib.ST_BAD_POINT, _lib.ST_ECIES_SHORT, _lib.ST_ECIES_AUTH}
    # a flipped context bit fails every element; the raw slots are zero wherever the status is not 0
    flipped = bytes([cx[0]]) + bytes([cx[1] ^ 0x10]) + cx[2:]
    _, st = ed.batch_vss_open(vpriv[i], b"".join(s[0] for s in sealed), flipped, [s[2] for s in sealed])
    assert list(st) == [_lib.ST_ECIES_AUTH] * len(sealed)
    lead = 3  # an odd byte offset in front of the first element, which is empty
    blob = np.frombuffer(b"\x5a" * lead + b"".join(r[1] for r in [(None, b"")] + rows), dtype=np.uint8)
    off = np.zeros(len(rows) + 2, dtype=np.uint64)
    np.cumsum([0] + [len(r[1]) for r in rows], out=off[1:])
    off += np.uint64(lead)
    kb = np.frombuffer(b"".join([DC.IDENTITY] + [r[0] for r in rows]), dtype=np.uint8)
    out, st3 = np.full(len(blob), 0xEE, dtype=np.uint8), np.zeros(len(rows) + 1, dtype=np.uint8)
    cb, xs = np.frombuffer(cx, dtype=np.uint8), np.ascontiguousarray(vpriv[i])
    _lib.check(_lib.load().kyb_ed25519_vss_open(len(rows) + 1, xs.ctypes.data, 0, kb.ctypes.data, cb.ctypes.data, 0, 32, blob.ctypes.data,
                                                off.ctypes.data, out.ctypes.data, st3.ctypes.data), "open")
    assert st3[0] == _lib.ST_ECIES_SHORT and bytes(out[:lead]) == b"\xee" * lead
    for j, (key, cipher, _) in enumerate(rows):
        msg, _ = VO.open_(bytes(vpriv[i]), key, cx, cipher)
        assert bytes(out[int(off[j + 1]):int(off[j + 2])]) == (msg or b"") + bytes(len(cipher) - len(msg or b"")), j


def test_seal_and_open_device_entries_on_tensors(ed):
    import torch

    dh, k, priv, pub, vpriv, vpubs, ctx, m, want = VC.seal_pool(True)
    n = 129
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tb = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    keys, sigs, (cblob, coff), st = ed.batch_vss_seal(t(dh[:n]), t(k[:n]), tb(priv), tb(pub), t(vpubs[:n]), t(ctx[:n]), _dev_msgs(m[:n]))
    torch.cuda.synchronize()
    _check_seal(keys.cpu().numpy(), sigs.cpu().numpy(), _dev_split(cblob, coff, n), st.cpu().numpy(), want[:n], m[:n])
    (pblob, poff), st2 = ed.batch_vss_open(t(vpriv[:n]), keys, t(ctx[:n]), (cblob, coff))
    torch.cuda.synchronize()
    slots, st2 = _dev_split(pblob, poff, n), st2.cpu().numpy()
    for i in range(n):
        if want[i] is None or i in VC.SPECIAL:
            assert st2[i] != 0 and slots[i] == bytes(len(slots[i])), i
        else:
            assert st2[i] == 0 and slots[i] == m[i] + bytes(16), i
    # one context and one receiver (both strides 0) on the device
    d0, k0, priv0, pub0, vpriv0, vpubs0, ctx0, m0, want0 = VC.seal_pool(False)
    one = np.repeat(vpubs0[7:8], 65, axis=0)
    keys, sigs, (cblob, coff), st = ed.batch_vss_seal(t(d0[:65]), t(k0[:65]), tb(priv0), tb(pub0), t(one), t(ctx0), _dev_msgs(m0[:65]))
    (pblob, poff), st2 = ed.batch_vss_open(t(vpriv0[7:8]), keys, t(ctx0), (cblob, coff))
    torch.cuda.synchronize()
    assert not st.any().item() and not st2.any().item()
    assert [s[:len(s) - 16] for s in _dev_split(pblob, poff, 65)] == m0[:65]


def test_a_batch_across_the_piece_boundary_round_trips_on_the_device(ed, sch):
    """2^18 + 5 elements of 32 bytes: sealed, then opened, on the device; every message must come back.  The oracle is
    compared at the elements around the boundary and at 32 seeded random ones (pure Python cannot do 2^18 in seconds)."""
    import torch

    n = (1 << 18) + 5
    g = torch.Generator(device="cpu").manual_seed(17)
    dh = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
    k = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
    dh[:, 31] &= 0x0F
    k[:, 31] &= 0x0F
    msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
    x = VC.scalars(b"vss piece x", 1)
    vpub = OC.ed_mul_base(x, threads=1)
    priv = bytes(VC.scalars(b"vss piece dealer", 1)[0])
    pub, ctx = O.mul_base(priv), bytes(VC.scalars(b"vss piece ctx", 1, 0xFF)[0])
    tb = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    off = (torch.arange(n + 1, dtype=torch.int64) * 32).cuda()
    pubs = torch.from_numpy(vpub).cuda().expand(n, 32).contiguous()
    keys, sigs, (cblob, coff), st = ed.batch_vss_seal(dh.cuda(), k.cuda(), tb(priv), tb(pub), pubs, tb(ctx), (msgs.cuda().view(-1), off))
    (pblob, _), st2 = ed.batch_vss_open(torch.from_numpy(x).cuda(), keys, tb(ctx), (cblob, coff))
    torch.cuda.synchronize()
    assert not st.any().item() and not st2.any().item()
    slots = pblob.view(n, 48)
    assert torch.equal(slots[:, :32].cpu(), msgs) and not slots[:, 32:].any().item()
    sample = sorted({0, 1, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, n - 1} | set(random.Random(5).sample(range(n), 32)))
    idx = torch.tensor(sample).cuda()
    got = (keys[idx].cpu().numpy(), sigs[idx].cpu().numpy(), [bytes(c) for c in cblob.view(n, 48)[idx].cpu().numpy()])
    want = VC.seal_expected(dh.numpy()[sample], k.numpy()[sample], priv, pub, np.repeat(vpub, len(sample), axis=0), [ctx],
                            [bytes(m) for m in msgs.numpy()[sample]])
    _check_seal(got[0], got[1], got[2], np.zeros(len(sample)), want, [bytes(32)] * len(sample))
    # the signatures of the same batch, signed again on their own across the boundary
    s2, _ = ed.batch_schnorr_sign(k.cuda(), tb(priv), (keys.view(-1), off))
    torch.cuda.synchronize()
    assert bytes(s2[n - 1].cpu().numpy()) == VO.schnorr_sign(bytes(k[n - 1].numpy()), priv, bytes(keys[n - 1].cpu().numpy()))
    assert torch.equal(s2, sigs)


# ------------------------------------------------------------------------------------------------- Rabin's share check
@pytest.mark.parametrize("per_poly_h", [False, True])
def test_deal_check2_on_the_share_table_host_and_device(ed, per_poly_h):
    import torch

    poly, idx, f, g, m, t, commits, H, want_ok, want_st, labels = VC.check2_table(per_poly_h)
    ok, st = ed.batch_deal_check2(poly, idx, f, g, commits, H, m, t)
    assert list(st) == want_st and list(ok) == want_ok
    tb = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    ok, st = ed.batch_deal_check2(torch.from_numpy(poly.view(np.int32)).cuda(), torch.from_numpy(idx.view(np.int32)).cuda(), tb(f), tb(g),
                                  tb(commits), tb(H), m, t)
    torch.cuda.synchronize()
    assert list(st.cpu().numpy()) == want_st and list(ok.cpu().numpy()) == want_ok
    # the composed standing calls on the rows whose polynomial is sound: f B + g H by mul_base, mul and add
    rows = [i for i in range(len(poly)) if not want_st[poly[i]]]
    fa, ga = np.frombuffer(f, dtype=np.uint8).reshape(-1, 32)[rows], np.frombuffer(g, dtype=np.uint8).reshape(-1, 32)[rows]
    Hr = np.frombuffer(H, dtype=np.uint8).reshape(-1, 32)
    hk = Hr[poly[rows]] if per_poly_h else np.repeat(Hr, len(rows), axis=0)
    gh, sth = ed.batch_mul(ga, hk)
    left, _ = ed.batch_add(ed.batch_mul_base(fa), gh)
    cm = np.frombuffer(commits, dtype=np.uint8).reshape(m, t, 32)
    for j, i in enumerate(rows[::7]):
        v = O.encode(VO.pub_eval([O.decode(bytes(c)) for c in cm[poly[i]]], int(idx[i])))
        assert (bytes(left[7 * j]) == v) == bool(want_ok[i]), i


def test_deal_check2_at_every_threshold_and_device_rule_for_unnamed_polynomials(ed):
    import torch

    for t in range(18):
        rows, commits, H, want = VC.check2_threshold(t)
        n = len(rows)
        ok, st = ed.batch_deal_check2(np.zeros(n, dtype=np.uint32), np.array([r[0] for r in rows], dtype=np.uint32),
                                      b"".join(r[1] for r in rows), b"".join(r[2] for r in rows), commits, H, 1, t)
        assert list(ok) == want == [1, 0, 0] * 3 and list(st) == [0], t
    rows, commits, H, want = VC.check2_threshold(3)
    tb = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    poly = torch.tensor([0, 1, 0, 5, 0, 0, 2**31 - 1, 0, 0], dtype=torch.int32).cuda()  # the table holds one polynomial
    ok, st = ed.batch_deal_check2(poly, torch.tensor([r[0] for r in rows], dtype=torch.int64).cuda(), tb(b"".join(r[1] for r in rows)),
                                  tb(b"".join(r[2] for r in rows)), tb(commits), tb(H), 1, 3)
    assert list(ok.cpu().numpy()) == [w if p == 0 else 0 for w, p in zip(want, poly.cpu().numpy())] and not st.any().item()
    with pytest.raises(_lib.KyberHipError):  # the host entry refuses such a check before any device work
        ed.batch_deal_check2(np.array([1], dtype=np.uint32), np.array([0], dtype=np.uint32), rows[0][1], rows[0][2], commits, H, 1, 3)


# ----------------------------------------------------------------- rabin's context, offsets that do not start at zero
@pytest.mark.parametrize("per_element_ctx", [False, True])
def test_seal_and_open_under_rabins_128_byte_context(ed, per_element_ctx):
    import torch

    dh, k, priv, pub, vpriv, vpubs, _, m, _ = VC.seal_pool(False)
    n = 129
    rows = [i for i in range(VC.POOL) if i not in VC.SPECIAL][:n]
    ctx = VC.scalars(b"vss gpu ctx128", 4 * (n if per_element_ctx else 1), 0xFF).reshape(-1, 128)
    ms = [m[i] for i in rows]
    want = VC.seal_expected(dh[rows], k[rows], priv, pub, vpubs[rows], ctx, ms)
    assert want[5] == VO.seal(bytes(dh[rows[5]]), bytes(k[rows[5]]), priv, pub, bytes(vpubs[rows[5]]), bytes(ctx[5 if per_element_ctx else 0]), ms[5])
    keys, sigs, ciphers, st = ed.batch_vss_seal(dh[rows], k[rows], priv, pub, vpubs[rows], ctx, ms, ctx_len=128)
    _check_seal(keys, sigs, ciphers, st, want, ms)
    back, st2 = ed.batch_vss_open(vpriv[rows], keys, ctx, ciphers, ctx_len=128)
    assert not st2.any() and back == ms
    flipped = ctx.copy()
    flipped[:, 127] ^= 1  # the context's last byte: the HMAC's third block, the additional data's eighth
    back, st2 = ed.batch_vss_open(vpriv[rows], keys, flipped, ciphers, ctx_len=128)
    assert list(st2) == [_lib.ST_ECIES_AUTH] * n and back == [b""] * n
    # the device entries
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    tb = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda()
    dk, ds, (cblob, coff), dst = ed.batch_vss_seal(t(dh[rows]), t(k[rows]), tb(priv), tb(pub), t(vpubs[rows]), t(ctx), _dev_msgs(ms), ctx_len=128)
    (pblob, poff), dst2 = ed.batch_vss_open(t(vpriv[rows]), dk, t(ctx), (cblob, coff), ctx_len=128)
    torch.cuda.synchronize()
    _check_seal(dk.cpu().numpy(), ds.cpu().numpy(), _dev_split(cblob, coff, n), dst.cpu().numpy(), want, ms)
    assert not dst2.any().item() and [s[:len(s) - 16] for s in _dev_split(pblob, poff, n)] == ms
    with pytest.raises(ValueError):
        ed.batch_vss_seal(dh[rows], k[rows], priv, pub, vpubs[rows], ctx, ms, ctx_len=64)


def test_host_entries_with_an_odd_offset_in_front_of_an_empty_first_element(ed):
    """msg_off[0] = 3 and a first element of no bytes, through kyb_ed25519_schnorr_sign and kyb_ed25519_vss_seal: the
    offsets are made relative and the ciphers land at ciphers + msg_off[i] + 16 i, nothing in front of them"""
    lib = _lib.load()
    dh, k, priv, pub, vpriv, vpubs, ctx, m, want = VC.seal_pool(False)
    rows = [i for i in range(VC.POOL) if i not in VC.SPECIAL][:65]
    lead, ms = 3, [b""] + [m[i] for i in rows[1:]]
    blob = np.frombuffer(b"\x5a" * lead + b"".join(ms), dtype=np.uint8)
    off = np.zeros(len(ms) + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in ms], out=off[1:])
    off += np.uint64(lead)
    n = len(ms)
    c = lambda a: np.ascontiguousarray(a)
    d, kk, vp = c(dh[rows]), c(k[rows]), c(vpubs[rows])
    pv, pb, cx = (np.frombuffer(x, dtype=np.uint8) for x in (priv, pub, bytes(ctx[0])))
    keys, sigs = np.zeros((n, 32), dtype=np.uint8), np.zeros((n, 64), dtype=np.uint8)
    out, st = np.full(int(off[-1]) + 16 * n, 0xEE, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    _lib.check(lib.kyb_ed25519_vss_seal(n, d.ctypes.data, kk.ctypes.data, pv.ctypes.data, pb.ctypes.data, vp.ctypes.data, cx.ctypes.data, 0, 32,
                                        blob.ctypes.data, off.ctypes.data, keys.ctypes.data, sigs.ctypes.data, out.ctypes.data, st.ctypes.data), "seal")
    exp = VC.seal_expected(d, kk, priv, pub, vp, ctx, ms)
    assert bytes(out[:lead]) == b"\xee" * lead and not st.any()
    for i in range(n):
        assert (bytes(keys[i]), bytes(sigs[i]), bytes(out[int(off[i]) + 16 * i:int(off[i + 1]) + 16 * (i + 1)])) == exp[i], i
    sk, sx, smsgs, swant = VC.sign_pool()
    sm = [b""] + smsgs[1:n]
    sblob = np.frombuffer(b"\x5a" * lead + b"".join(sm), dtype=np.uint8)
    soff = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(x) for x in sm], out=soff[1:])
    soff += np.uint64(lead)
    k2, x2 = c(sk[:n]), c(sx[:n])
    s2, st2 = np.zeros((n, 64), dtype=np.uint8), np.full(n, 0xEE, dtype=np.uint8)
    _lib.check(lib.kyb_ed25519_schnorr_sign(n, k2.ctypes.data, x2.ctypes.data, 32, sblob.ctypes.data, soff.ctypes.data, s2.ctypes.data,
                                            st2.ctypes.data), "sign")
    assert not st2.any() and [bytes(s) for s in s2] == [VO.schnorr_sign(bytes(k2[i]), bytes(x2[i]), sm[i]) for i in range(n)]


def test_one_undecodable_h_for_the_batch_marks_every_polynomial(ed):
    poly, idx, f, g, m, t, commits, H, want_ok, want_st, labels = VC.check2_table(False)
    ok, st = ed.batch_deal_check2(poly[:70], idx[:70], f[:70 * 32], g[:70 * 32], commits, DC.UNDECODABLE, m, t)
    assert not np.asarray(ok).any() and list(st) == [1] * m
