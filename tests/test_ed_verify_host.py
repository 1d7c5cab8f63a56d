"""Ed25519 fused verification and a*P + b*Q without a GPU: the lane programs of kyber_amd/csrc/ed25519_verify.cuh
compiled for the CPU (tests/ed_verify_harness.cpp) against hashlib and the oracle, the oracle's restatement of
VerifyWithChecks against the Wycheproof verdicts, and the C ABI's argument checks."""
import collections
import ctypes as C
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import ed25519 as O
from tests import _ed_verify_oracle as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the scalar edge list of tests/test_gpu_ed25519.py
EDGE_SCALARS = [0, 1, O.L, O.L - 1, 2**255, 2**256 - 1]


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build", "libedverifyharness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "ed_verify_harness.cpp")])
    return C.CDLL(out)


def _buf(b):
    return C.create_string_buffer(bytes(b), max(len(b), 1))


def test_oracle_reproduces_the_wycheproof_verdicts_and_reason_counts():
    c = collections.Counter()
    for pub, msg, sig, valid in V.wycheproof():
        ok, why = V.verify_with_checks(pub, msg, sig)
        assert ok == valid
        c[why] += 1
    assert c == {V.OK: 88, V.S_NONCANONICAL: 17, V.LENGTH: 12, V.EQUATION: 12, V.R_NOT_A_POINT: 10, V.R_SMALL_ORDER: 7,
                 V.R_NONCANONICAL: 4}
    for i in (0, 47, 48, 175, 176, 383):
        assert V.verify_with_checks(*V.sign_input()[i]) == (True, V.OK)


def test_hash_and_reduction_match_hashlib(harness):
    out = C.create_string_buffer(32)
    for pub, msg, sig in V.sign_input():  # message lengths 0..383: every block boundary up to four blocks
        harness.edv_hram(sig[:32], pub, _buf(msg), C.c_size_t(len(msg)), out)
        want = int.from_bytes(hashlib.sha512(sig[:32] + pub + msg).digest(), "little") % O.L
        assert int.from_bytes(out.raw, "little") == want, len(msg)
    rng = random.Random(5)
    edges = [2**512 - 1, O.L - 1, O.L, 2**252, 0, 1, 2**256 - 1, 2**256, 2**256 + 1]
    edges += [O.L << k for k in (1, 4, 128, 259)] + [(O.L << k) - 1 for k in (1, 4, 128, 259)] + [(O.L << k) + 1 for k in (1, 128, 259)]
    edges += [rng.getrandbits(512) for _ in range(200)]
    for x in edges:
        assert x < 2**512
        harness.edv_reduce512(x.to_bytes(64, "little"), out)
        assert int.from_bytes(out.raw, "little") == x % O.L, hex(x)


def test_byte_checks_match_the_oracle(harness):
    encs = [c[0] for c in V.synthetic_rejects()] + [c[2][:32] for c in V.synthetic_rejects()] + [c[0] for c in V.sign_input()[:32]]
    seen = collections.Counter()
    for enc in encs:
        canon = V.point_is_canonical(enc)
        assert bool(harness.edv_point_is_canonical(enc)) == canon
        pt = O.decode(enc)
        if canon and pt is not None:
            small = V.has_small_order(pt)
            assert bool(harness.edv_point_has_small_order(enc)) == small, enc.hex()
            seen[small] += 1
        seen["canon" if canon else "noncanon"] += 1
    assert seen[True] >= 10 and seen[False] >= 32 and seen["noncanon"] >= 19


def _run_verify(harness, cases):
    pubs, msgs, off, sigs = V.pack(cases)
    n = len(cases)
    ok, st = np.zeros(n, dtype=np.uint8), np.full(n, 255, dtype=np.uint8)
    harness.edv_verify(C.c_size_t(n), pubs.ctypes.data_as(C.c_void_p), msgs.ctypes.data_as(C.c_void_p),
                       off.ctypes.data_as(C.c_void_p), sigs.ctypes.data_as(C.c_void_p), ok.ctypes.data_as(C.c_void_p),
                       st.ctypes.data_as(C.c_void_p))
    return ok, st


def test_lane_verify_program_matches_the_oracle_on_every_vector(harness):
    cases = V.all_cases()
    ok, st = _run_verify(harness, cases)
    reasons = collections.Counter()
    for i, c in enumerate(cases):
        want_ok, why = V.verify_with_checks(*c)
        reasons[why] += 1
        assert bool(ok[i]) == want_ok, (i, why)
        assert st[i] == V.abi_status(*c), (i, why, st[i])
    for why in V.REASONS:  # no class may silently go missing
        if why != V.LENGTH:  # lengths are the host's check: a signature of another length never reaches the engine
            assert reasons[why] >= 1, why
    assert reasons[V.OK] >= 384 + 5 + 88
    assert set(int(x) for x in st) == {V.ST_OK, V.ST_BAD_POINT, V.ST_SIG_NONCANONICAL, V.ST_SIG_SMALL_ORDER}


def test_flipped_bits_are_rejected_by_the_lane_program(harness):
    rows = V.sign_input()
    cases = []
    for i in range(1, 65):
        pub, msg, sig = rows[i]
        cases.append((pub, msg, bytes([sig[0] ^ 1]) + sig[1:]))            # R
        cases.append((pub, msg, sig[:32] + bytes([sig[32] ^ 1]) + sig[33:]))  # S
        cases.append((bytes([pub[0] ^ 1]) + pub[1:], msg, sig))            # A
        cases.append((pub, bytes([msg[0] ^ 1]) + msg[1:], sig))            # message
    ok, st = _run_verify(harness, cases)
    assert not ok.any()
    for i, c in enumerate(cases):
        assert st[i] == V.abi_status(*c)


def _mul2(harness, a, P, b, Q, full):
    n = len(a)
    out, st = np.zeros((n, 32), dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    harness.edv_mul2(C.c_size_t(n), b"".join(a), b"".join(P), b"".join(b), b"".join(Q), int(full), out.ctypes.data_as(C.c_void_p),
                     st.ctypes.data_as(C.c_void_p))
    return [out[i].tobytes() for i in range(n)], st


def mul2_cases(seed=11, nrandom=24):
    """(a, P, b, Q) lists: random scalars and points, the scalar edge list against itself, P = Q, P = -Q, a = b,
    a P = -b Q (identity result), identity and small-order points, an undecodable point"""
    rng = random.Random(seed)
    rs = lambda: rng.getrandbits(256).to_bytes(32, "little")
    rp = lambda: O.encode(O.mul_int(rng.getrandbits(252) + 1, O.B))
    a, P, b, Q = [], [], [], []

    def put(x, p, y, q):
        a.append(x), P.append(p), b.append(y), Q.append(q)

    for _ in range(nrandom):
        put(rs(), rp(), rs(), rp())
    for x in EDGE_SCALARS:
        for y in EDGE_SCALARS:
            put(x.to_bytes(32, "little"), rp(), y.to_bytes(32, "little"), rp())
    p = rp()
    negp = O.encode(O.neg(O.decode(p)))
    k = rng.getrandbits(250).to_bytes(32, "little")
    put(rs(), p, rs(), p)
    put(rs(), p, rs(), negp)
    put(k, rp(), k, rp())
    put(k, p, k, negp)  # a P = -b Q
    ident = O.encode(O.IDENTITY)
    small = bytes.fromhex("26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05")
    put(rs(), ident, rs(), rp())
    put(rs(), rp(), rs(), ident)
    put(rs(), small, rs(), rp())
    put(rs(), small, rs(), small)
    bad = V._not_on_curve()
    put(rs(), bad, rs(), rp())
    put(rs(), rp(), rs(), bad)
    return a, P, b, Q


def mul2_oracle(a, P, b, Q, vartime):
    x, y = O.mul(a, P, vartime), O.mul(b, Q, vartime)
    if x is None or y is None:
        return None
    return O.encode(O.add(O.decode(x), O.decode(y)))


@pytest.mark.parametrize("vartime", [False, True])
def test_straus_chain_matches_add_of_two_muls(harness, vartime):
    a, P, b, Q = mul2_cases()
    out, st = _mul2(harness, a, P, b, Q, vartime)
    idents = bads = 0
    for i in range(len(a)):
        want = mul2_oracle(a[i], P[i], b[i], Q[i], vartime)
        if want is None:
            assert st[i] == 1 and out[i] == bytes(32)
            bads += 1
        else:
            assert st[i] == 0 and out[i] == want, i
            idents += want == O.encode(O.IDENTITY)
    assert bads == 2 and idents >= 2


def test_abi_checks_arguments_without_a_device():
    from kyber_amd import _lib

    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    off = (C.c_uint64 * 5)(0, 1, 2, 3, 4)
    bad_off = (C.c_uint64 * 5)(0, 3, 2, 3, 4)
    o, b = C.addressof(off), C.addressof(bad_off)
    assert lib.kyb_ed25519_verify(0, p, p, o, p, p, p, 0) == 0
    assert lib.kyb_ed25519_verify_dev(0, p, p, o, p, p, p, 0, None) == 0
    assert lib.kyb_ed25519_mul2(0, p, p, p, p, p, p, 0) == 0
    assert lib.kyb_ed25519_mul2_dev(0, p, p, p, p, p, p, 1, None) == 0
    for name, args in (("kyb_ed25519_verify", (4, None, p, o, p, p, p, 0)), ("kyb_ed25519_verify", (4, p, p, None, p, p, p, 0)),
                       ("kyb_ed25519_verify", (4, p, p, o, None, p, p, 0)), ("kyb_ed25519_verify", (4, p, p, o, p, None, p, 0)),
                       ("kyb_ed25519_verify", (4, p, p, o, p, p, p, 1)),      # flags must be 0
                       ("kyb_ed25519_verify", (4, p, p, b, p, p, p, 0)),      # offsets that decrease
                       ("kyb_ed25519_verify", (4, p, None, o, p, p, None, 0)),  # message bytes named, no buffer
                       ("kyb_ed25519_verify_dev", (4, p, p, o, p, None, p, 0, None)), ("kyb_ed25519_verify_dev", (4, p, p, o, p, p, p, 8, None)),
                       ("kyb_ed25519_mul2", (4, p, None, p, p, p, p, 0)), ("kyb_ed25519_mul2", (4, p, p, p, p, None, p, 0)),
                       ("kyb_ed25519_mul2", (4, p, p, p, p, p, p, 8)),        # KYB_F_UNIFORM
                       ("kyb_ed25519_mul2", (4, p, p, p, p, p, p, 16)), ("kyb_ed25519_mul2_dev", (4, p, p, p, p, p, p, 8, None)),
                       ("kyb_ed25519_mul2_dev", (4, None, p, p, p, p, p, 0, None))):
        assert getattr(lib, name)(*args) == -1, (name, args)
        assert name.encode() in lib.kyb_last_error()


def test_header_cites_the_reference_and_names_the_status_codes():
    src = open(os.path.join(ROOT, "include", "kyber_hip.h")).read()
    for cite in ("eddsa.go:143-229", "schnorr.go:84-160", "dleq.go:160-172", "KYB_ST_SIG_NONCANONICAL 5", "KYB_ST_SIG_SMALL_ORDER 6",
                 "not a curve point"):
        assert cite in src, cite
    assert (V.ST_OK, V.ST_BAD_POINT, V.ST_SIG_NONCANONICAL, V.ST_SIG_SMALL_ORDER) == (0, 1, 5, 6)
