"""sign/dss's engine calls without a GPU: kyber_amd/csrc/ed25519_dss.cuh compiled for the CPU (tests/dss_harness.cpp)
against the oracle (tests/_dss_oracle.py) on the labelled cases of tests/_dss_cases.py; the C ABI's argument checks.

Limit of the check: the reference's dss_test.go prints no bytes and no Go toolchain is at hand, so no transcript of the
Go program is pinned.  SHA-256 and SHA-512 are hashlib's; h is pinned by the RFC 8032 rows of tests/golden (S = r + h a
holds only for the right h); schnorr.Sign is held to the verification equation; the composition is the oracle's, written
from dss.go's text."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

from kyber_amd import _lib
from oracle import ed25519 as O
from tests import _dkg_cases as DC
from tests import _dss_cases as K
from tests import _dss_oracle as D
from tests import _ed_verify_oracle as V
from tests import _vss_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_harness():
    out = os.path.join(ROOT, "tests", "_build", "libdssharness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "dss_harness.cpp")])
    h = C.CDLL(out)
    sz, b, p, u32 = C.c_size_t, C.c_char_p, C.c_void_p, C.c_uint32
    h.dsh_session_id.argtypes = [sz, b, sz, b, b]
    h.dsh_partial_hash.argtypes = [b, u32, b, b]
    h.dsh_hash_sig.argtypes = [sz, sz, p, sz, p, p, p, p]
    h.dsh_dss_check.argtypes = [sz, sz, p, sz, p, sz, sz] + [p] * 12
    h.dsh_dss_partial.argtypes = [sz, p, u32, p, p, p, sz, p, sz, p, p, p, p, p, p]
    for f in (h.dsh_session_id, h.dsh_partial_hash, h.dsh_hash_sig):
        f.restype = None
    return h


@pytest.fixture(scope="module")
def harness():
    return build_harness()


@pytest.fixture(scope="module")
def worlds():
    return K.worlds()


def _arr(x, dtype=np.uint8):
    return np.frombuffer(x, dtype=dtype).copy() if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=dtype)


def _packed(msgs, lead: int = 0):
    """(exactly sized blob, offsets): `lead` stray bytes stand in front of the first message"""
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    off += np.uint64(lead)
    return _arr(b"\xa5" * lead + b"".join(msgs) or b"\0"), off


# the two entry points of the harness, with the shapes of kyber_amd.group.edwards25519's batch_dss_* wrappers
def check(h, participants, long_commits, rand_commits, msgs, sess, idx, Vs, sids, sigs, want_status=True, folded=False):
    n, ns, tl = len(sess), len(msgs), len(long_commits) // 32
    tr = len(rand_commits) // 32 // ns
    pk, lc, rc = _arr(participants), _arr(long_commits), _arr(rand_commits)
    blob, off = _packed(msgs, 3)
    se, ix, v, s, g = _arr(sess, np.uint32), _arr(idx, np.uint32), _arr(Vs), _arr(sids), _arr(sigs)
    ok, st, sst = np.full(n, 0xEE, dtype=np.uint8), np.full(n, 0xEE, dtype=np.uint8), np.full(ns, 0xEE, dtype=np.uint8)
    fo = np.zeros(ns * max(tl, tr) * 32, dtype=np.uint8)
    rc_ = h.dsh_dss_check(n, len(pk) // 32, pk.ctypes.data, tl, lc.ctypes.data, ns, tr, rc.ctypes.data, blob.ctypes.data, off.ctypes.data,
                          se.ctypes.data, ix.ctypes.data, v.ctypes.data, s.ctypes.data, g.ctypes.data, ok.ctypes.data,
                          st.ctypes.data if want_status else None, sst.ctypes.data if want_status else None,
                          fo.ctypes.data if folded else None)
    assert rc_ == 0
    if folded:
        return ok, st, sst, fo.tobytes()
    return ok, (st if want_status else None), (sst if want_status else None)


def partial(h, priv, index, alpha, beta, k, long_commits, rand_commits, msgs):
    ns, tl = len(msgs), len(long_commits) // 32
    tr = len(rand_commits) // 32 // ns
    x, a, b, kk, lc, rc = (_arr(t) for t in (priv, alpha, beta, k, long_commits, rand_commits))
    blob, off = _packed(msgs, 1)
    Vs, sids, sigs = (np.full((ns, w), 0xEE, dtype=np.uint8) for w in (32, 32, 64))
    assert h.dsh_dss_partial(ns, x.ctypes.data, index, a.ctypes.data, b.ctypes.data, kk.ctypes.data, tl, lc.ctypes.data, tr, rc.ctypes.data,
                             blob.ctypes.data, off.ctypes.data, Vs.ctypes.data, sids.ctypes.data, sigs.ctypes.data) == 0
    return Vs, sids, sigs


def world_args(w):
    return b"".join(w.participants), b"".join(w.long_commits), b"".join(b"".join(rc) for rc in w.rand_commits), w.msgs


def run_cases(call, w, rows, **kw):
    """the rows of one world through ONE call of `call` (the harness's check or the engine's wrapper)"""
    return call(*world_args(w), [r[1] for r in rows], [r[2] for r in rows], b"".join(r[3] for r in rows), b"".join(r[4] for r in rows),
                b"".join(r[5] for r in rows), **kw)


# ------------------------------------------------------------------------------------------------------ the yardsticks
def test_the_oracle_agrees_with_every_label(worlds):
    seen = set()
    for w in worlds:
        for label, b, i, v, sid, sig, want in K.cases(w):
            assert w.expected(b, i, v, sid, sig) == (int(want == K.OK), want), (w.name, label)
            seen.add(want)
        assert w.sess_status() == [K.BAD_POINT if (w.name == "bad session" and b == 1) else K.OK for b in range(w.ns)]
    assert seen == {K.OK, K.BAD_POINT, K.NONCANONICAL, K.SMALL_ORDER, K.INDEX, K.SIG, K.SESSION, K.PARTIAL}
    assert sorted(len(m) for w in worlds[:3] for m in w.msgs) == list(K.MSG_LENGTHS)
    assert (K.INDEX, K.SIG, K.SESSION, K.PARTIAL) == (_lib.ST_DSS_INDEX, _lib.ST_DSS_SIG, _lib.ST_DSS_SESSION, _lib.ST_DSS_PARTIAL) == (14, 15, 16, 17)


def test_the_fold_is_exact_off_the_prime_order_subgroup(worlds):
    """sum_k x^k (R_k + h A_k) = randomPoly.Eval(I) + h longPoly.Eval(I), commitments with torsion and tl != tr included"""
    for w in worlds:
        for b in range(w.ns):
            f = D.folded(w.long_commits, w.rand_commits[b], w.msgs[b])
            if f is None:
                continue
            for i in (0, 1, 6, 2**32 - 1):
                assert DC.eval_commits(f, i) == D.right_side(w.long_commits, w.rand_commits[b], w.msgs[b], i), (w.name, b, i)
    t = worlds[4]
    assert O.mul_int(O.L, O.decode(t.long_commits[-1])) != O.IDENTITY  # the torsion world has torsion


def test_h_is_pinned_by_rfc8032(harness):
    """S = r + h a: with R, A and S of an RFC 8032 signature, S B = R + h A holds only for h = SHA-512(R || A || msg) mod l"""
    rows = V.rfc8032()
    assert len(rows) >= 4
    for pub, msg, sig in rows:
        blob, off = _packed([msg], 5)
        out = np.zeros(32, dtype=np.uint8)
        lc, rc = _arr(pub), _arr(sig[:32])  # hashSig's order: the random key's commitment 0, then the long-term key's
        harness.dsh_hash_sig(1, 1, lc.ctypes.data, 1, rc.ctypes.data, blob.ctypes.data, off.ctypes.data, out.ctypes.data)
        h = int.from_bytes(out.tobytes(), "little")
        assert h == D.hash_sig(sig[:32], pub, msg) and h < O.L
        assert O.mul_base(sig[32:]) == O.encode(O.add(O.decode(sig[:32]), O.mul_int(h, O.decode(pub))))


@pytest.mark.parametrize("tl,tr", [(1, 1), (1, 2), (2, 1), (4, 4), (2, 5), (5, 2), (9, 9), (65, 65)])
def test_session_id_ends_on_and_off_a_block(harness, tl, tr):
    lc, rc = hashlib.shake_128(b"lc").digest(32 * tl), hashlib.shake_128(b"rc").digest(32 * tr)
    out = C.create_string_buffer(32)
    harness.dsh_session_id(tl, lc, tr, rc, out)
    assert out.raw == hashlib.sha256(lc + rc).digest()
    assert D.session_id([lc], [rc]) == out.raw


def test_partial_hash_is_two_nested_sha256(harness):
    for index in (0, 1, 6, 255, 256, 2**32 - 1):
        v, sid = hashlib.sha256(b"v %d" % index).digest(), hashlib.sha256(b"sid %d" % index).digest()
        out = C.create_string_buffer(32)
        harness.dsh_partial_hash(v, index, sid, out)
        assert out.raw == D.partial_hash(v, index, sid) == hashlib.sha256(hashlib.sha256(v + index.to_bytes(4, "little")).digest() + sid).digest()


# --------------------------------------------------------------------------------------------------------- the calls
def test_check_on_the_case_table(harness, worlds):
    for w in worlds:
        rows = K.cases(w)
        ok, st, sst, fo = run_cases(lambda *a, **k: check(harness, *a, **k), w, rows, folded=True)
        for r, o, s in zip(rows, ok, st):
            assert (int(o), int(s)) == (int(r[6] == K.OK), r[6]), (w.name, r[0])
        assert list(sst) == w.sess_status(), w.name
        T = max(w.tl, w.tr)
        for b in range(w.ns):
            f = D.folded(w.long_commits, w.rand_commits[b], w.msgs[b])
            if f is not None:
                assert fo[32 * T * b:32 * T * (b + 1)] == b"".join(f), (w.name, b)
        ok2, _, _ = run_cases(lambda *a, **k: check(harness, *a, **k), w, rows, want_status=False)
        assert list(ok2) == list(ok), w.name


def test_check_signature_verdicts_are_verifys(harness, worlds):
    """the signature step returns kyb_ed25519_verify's ok and status for the same (key, m, sig)"""
    w = worlds[0]
    for label, b, i, v, sid, sig, want in K.cases(w):
        if i >= K.NP:
            continue
        pub, m = w.participants[i], D.partial_hash(v, i, sid)
        vok, vst = V.verify_with_checks(pub, m, sig)[0], V.abi_status(pub, m, sig)
        if vst:
            assert want == vst, label
        elif not vok:
            assert want == K.SIG, label
        else:
            assert want not in (K.SIG, K.NONCANONICAL, K.SMALL_ORDER), label


def test_a_session_the_call_does_not_hold_reads_nothing(harness, worlds):
    w = worlds[0]
    v, sid, sig = w.honest(1, 0)
    ok, st, _ = check(harness, *world_args(w), [1, w.ns, 2**32 - 1], [0, 0, 0], v * 3, sid * 3, sig * 3)
    assert list(ok) == [1, 0, 0] and list(st) == [0, 0, 0]


def test_partial_matches_the_oracle_and_the_signatures_hold(harness, worlds):
    for w in worlds:
        if w.name == "bad session":
            continue
        for i in (0, 6, K.NP - 1):
            beta = b"".join(DC.le(w.beta(b, i)) for b in range(w.ns))
            k = b"".join(w.nonce(b, i) for b in range(w.ns))
            Vs, sids, sigs = partial(harness, DC.le(w.privs[i]), i, DC.le(w.alpha(i)), beta, k, *world_args(w)[1:])
            for b in range(w.ns):
                got = (bytes(Vs[b]), bytes(sids[b]), bytes(sigs[b]))
                assert got == w.honest(b, i), (w.name, i, b)
                m = D.partial_hash(got[0], i, got[1])
                assert got[2] == VO.schnorr_sign(w.nonce(b, i), DC.le(w.privs[i]), m)  # kyb_ed25519_schnorr_sign's bytes
                assert V.verify_with_checks(w.participants[i], m, got[2]) == (True, V.OK)
                if not w.torsion:  # (there the right side has a torsion component no honest share matches)
                    assert w.expected(b, i, *got) == (1, 0)


def test_partial_takes_any_32_bytes_of_secret_and_nonce(harness, worlds):
    w = worlds[3]
    priv, k = b"\xff" * 32, DC.le(2**255 + 12345)
    Vs, sids, sigs = partial(harness, priv, 4, b"\xfe" * 32, b"\xfd" * 32, k, *world_args(w)[1:])
    assert (bytes(Vs[0]), bytes(sids[0]), bytes(sigs[0])) == D.partial(priv, 4, b"\xfe" * 32, b"\xfd" * 32, k, w.long_commits, w.rand_commits[0], w.msgs[0])


# ------------------------------------------------------------------------------------------------- the C ABI's checks
def test_harness_argument_rules(harness):
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    assert harness.dsh_dss_check(0, 0, None, 0, None, 0, 0, *([None] * 12)) == 0
    assert harness.dsh_dss_partial(0, None, 0, None, None, None, 0, None, 0, None, None, None, None, None, None) == 0
    for tl, tr, ns in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert harness.dsh_dss_check(1, 1, p, tl, p, ns, tr, *([p] * 12)) == -1
    assert harness.dsh_dss_partial(1, p, 0, p, p, p, 0, p, 1, p, p, p, p, p, p) == -1
    assert harness.dsh_dss_partial(1, p, 0, p, p, p, 1, p, 1, p, p, p, p, None, p) == -1


def test_argument_errors_and_empty_batches_never_touch_the_device():
    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    assert lib.kyb_ed25519_dss_check(0, 0, None, 0, None, 0, 0, *([None] * 11)) == 0
    assert lib.kyb_ed25519_dss_check_dev(0, 3, p, 0, p, 0, 0, *([p] * 11), None) == 0
    assert lib.kyb_ed25519_dss_partial(0, p, 0, p, p, p, 0, p, 0, p, p, p, p, p, p) == 0
    assert lib.kyb_ed25519_dss_partial_dev(0, None, 0, None, None, None, 1, None, 1, None, None, None, None, None, None, None) == 0
    off = (C.c_uint64 * 3)(0, 40, 8)  # decreasing
    po = C.addressof(off)
    big = (C.c_uint32 * 2)(0, 2)  # names session 2 of a call of two
    pb = C.addressof(big)
    # (n, np, participants, tl, long, ns, tr, rand, msgs, off, sess, idx, V, sid, sigs, ok, status, sess_status)
    bad = [
        ("kyb_ed25519_dss_check", (2, 3, p, 0, p, 2, 1, p, p, p, p, p, p, p, p, p, p, p)),     # tl = 0
        ("kyb_ed25519_dss_check", (2, 3, p, 1, p, 2, 0, p, p, p, p, p, p, p, p, p, p, p)),     # tr = 0
        ("kyb_ed25519_dss_check", (2, 3, p, 1, p, 0, 1, p, p, p, p, p, p, p, p, p, p, p)),     # no session
        ("kyb_ed25519_dss_check", (2, 3, None, 1, p, 2, 1, p, p, p, p, p, p, p, p, p, p, p)),
        ("kyb_ed25519_dss_check", (2, 3, p, 1, p, 2, 1, p, p, p, p, p, p, p, p, None, p, p)),  # ok
        ("kyb_ed25519_dss_check", (2, 3, p, 1, p, 2, 1, p, p, po, p, p, p, p, p, p, p, p)),    # decreasing offsets
        ("kyb_ed25519_dss_check", (2, 3, p, 1, p, 2, 1, p, p, p, pb, p, p, p, p, p, p, p)),    # sess[1] >= ns
        ("kyb_ed25519_dss_check_dev", (2, 3, p, 1, p, 2, 1, p, p, p, p, p, None, p, p, p, p, p, None)),
        ("kyb_ed25519_dss_check_dev", (2, 3, p, 0, p, 2, 1, p, p, p, p, p, p, p, p, p, p, p, None)),
        ("kyb_ed25519_dss_partial", (2, p, 0, p, p, p, 0, p, 1, p, p, p, p, p, p)),
        ("kyb_ed25519_dss_partial", (2, p, 0, p, p, p, 1, p, 0, p, p, p, p, p, p)),
        ("kyb_ed25519_dss_partial", (2, p, 0, p, p, p, 1, p, 1, p, p, po, p, p, p)),
        ("kyb_ed25519_dss_partial", (2, p, 0, None, p, p, 1, p, 1, p, p, p, p, p, p)),
        ("kyb_ed25519_dss_partial_dev", (2, p, 0, p, p, p, 1, p, 1, p, p, p, p, p, None, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args)
        assert name.encode() in lib.kyb_last_error()
    # KYB_E_ALLOC: no such workspace (status and sess_status may be NULL: they are not what is refused)
    assert lib.kyb_ed25519_dss_check(1, 3, p, 1 << 40, p, 2, 1, p, p, p, p, p, p, p, p, p, None, None) == -4
    assert lib.kyb_ed25519_dss_check(1, 3, p, 2, p, 1 << 40, 1 << 40, p, p, p, p, p, p, p, p, p, None, None) == -4


def test_the_header_and_the_binding_name_the_calls():
    header = open(os.path.join(ROOT, "include", "kyber_hip.h")).read()
    for cite in ("dss.go:141-173", "dss.go:113-134", "dss.go:201-211, 235-246", "KYB_ST_DSS_INDEX 14", "KYB_ST_DSS_SIG 15",
                 "KYB_ST_DSS_SESSION 16", "KYB_ST_DSS_PARTIAL 17", "kyb_ed25519_dss_check_dev", "kyb_ed25519_dss_partial_dev"):
        assert cite in header, cite
    from kyber_amd.group import edwards25519 as ed

    assert callable(ed.batch_dss_check) and callable(ed.batch_dss_partial)
