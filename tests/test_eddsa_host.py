"""sign/eddsa's two engine calls without a GPU: kyber_amd/csrc/ed25519_eddsa.cuh compiled for the CPU
(tests/eddsa_harness.cpp) against the oracle (tests/_eddsa_oracle.py), the reference's own 1 024 sign.input lines and
the RFC 8032 rows; the C ABI's argument checks.

Every byte is pinned: the fixture's columns are what eddsa.go computes (a = the clamped first half of SHA-512(seed),
r = SHA-512(prefix || msg) mod l, h = SHA-512(R || A || msg) mod l, S = r + h a mod l), and the messages are 0 to 1 023
bytes long, one of every length, so they cross every padding boundary of both hashes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from kyber_amd import _lib
from tests import _eddsa_oracle as EO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_harness():
    out = os.path.join(ROOT, "tests", "_build", "libeddsaharness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "eddsa_harness.cpp")])
    h = C.CDLL(out)
    sz, p = C.c_size_t, C.c_void_p
    h.esh_expand.argtypes = [sz, p, p, p, p]
    h.esh_sign.argtypes = [sz, p, p, p, sz, p, p, p, p, p, p]
    h.esh_expand.restype = h.esh_sign.restype = None
    return h


@pytest.fixture(scope="module")
def harness():
    return build_harness()


def _arr(x):
    return np.frombuffer(x, dtype=np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=np.uint8)


def _packed(msgs, lead: int = 0):
    """(exactly sized blob, offsets): `lead` stray bytes stand in front of the first element"""
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    off += np.uint64(lead)
    return _arr(b"\xa5" * lead + b"".join(msgs) or b"\0"), off


# the two entry points of the harness, with the shapes of kyber_amd.group.edwards25519's batch_eddsa_* wrappers
def expand(h, seeds):
    s = _arr(seeds).reshape(-1, 32)
    n = s.shape[0]
    secrets, prefixes, pubs = (np.full((n, 32), 0xEE, dtype=np.uint8) for _ in range(3))
    h.esh_expand(n, s.ctypes.data, secrets.ctypes.data, prefixes.ctypes.data, pubs.ctypes.data)
    return secrets, prefixes, pubs


def sign(h, secrets, prefixes, pubs, msgs, lead: int = 3, scalars: bool = False):
    a, p, A = (_arr(x).reshape(-1, 32) for x in (secrets, prefixes, pubs))
    n = len(msgs)
    assert a.shape == p.shape == A.shape and a.shape[0] in (1, n)
    blob, off = _packed(msgs, lead)
    sigs, st = np.full((n, 64), 0xEE, dtype=np.uint8), np.full(n, 0xEE, dtype=np.uint8)
    r, hh = np.zeros((n, 32), dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8)
    h.esh_sign(n, a.ctypes.data, p.ctypes.data, A.ctypes.data, 32 if a.shape[0] == n and n != 1 else 0, blob.ctypes.data, off.ctypes.data,
               sigs.ctypes.data, st.ctypes.data, r.ctypes.data, hh.ctypes.data)
    assert not st.any()
    return (sigs, r, hh) if scalars else sigs


# ------------------------------------------------------------------------------------------------------ the yardsticks
def test_boundary_lines_hold_the_listed_lengths_and_both_hashes_edges():
    assert set(EO.LISTED) <= set(EO.BOUNDARY)
    for head in (32, 64):
        for edge in (111, 112, 127, 0):
            hit = [n for n in EO.BOUNDARY if (head + n) % 128 == edge]
            assert len(hit) >= 7, (head, edge)  # one in each of the first eight blocks
    # 1 023 bytes behind the prefix: nine blocks; behind R || A: nine too, the padding in the last
    assert (32 + 1023 + 17 + 127) // 128 == 9 and (64 + 1023 + 17 + 127) // 128 == 9


def test_oracle_matches_every_sign_input_line():
    seeds, kat, msgs, sigs = EO.sign_input()
    secrets, prefixes, pubs = EO.sign_input_keys()
    assert np.array_equal(secrets, kat[:, 0]) and np.array_equal(pubs, kat[:, 1])
    for i in range(1024):
        a, p, A = bytes(secrets[i]), bytes(prefixes[i]), bytes(pubs[i])
        assert EO.sign(a, p, A, msgs[i]) == sigs[i], i
        assert EO.nonce(p, msgs[i]).to_bytes(32, "little") == kat[i, 2].tobytes(), i
        assert EO.challenge(sigs[i][:32], A, msgs[i]).to_bytes(32, "little") == kat[i, 4].tobytes(), i


def test_oracle_matches_rfc8032():
    rows = EO.rfc8032()
    assert len(rows) == 5
    for seed, pub, msg, sig in rows:
        a, p, A = EO.expand(seed)
        assert A == pub and EO.sign(a, p, A, msg) == sig


# ------------------------------------------------------------------------------------------------------ lane programs
def test_expand_matches_the_fixture_and_the_oracle(harness):
    seeds, kat, _, _ = EO.sign_input()
    want = EO.sign_input_keys()
    rows = list(EO.BOUNDARY)
    got = expand(harness, seeds[rows])
    for g, w in zip(got, want):
        assert np.array_equal(g, w[rows])
    assert np.array_equal(got[0], kat[rows, 0]) and np.array_equal(got[2], kat[rows, 1])
    rfc = EO.rfc8032()
    got = expand(harness, b"".join(r[0] for r in rfc))
    assert [tuple(bytes(x[i]) for x in got) for i in range(5)] == [EO.expand(r[0]) for r in rfc]
    assert [bytes(x) for x in got[2]] == [r[1] for r in rfc]


def test_sign_matches_the_fixture_on_every_boundary_length(harness):
    _, kat, msgs, sigs = EO.sign_input()
    secrets, prefixes, pubs = EO.sign_input_keys()
    rows = list(EO.BOUNDARY)
    got, r, h = sign(harness, secrets[rows], prefixes[rows], pubs[rows], [msgs[i] for i in rows], scalars=True)
    assert [bytes(s) for s in got] == [sigs[i] for i in rows]
    assert np.array_equal(r, kat[rows, 2]) and np.array_equal(h, kat[rows, 4])  # the two hashes, each on its own
    assert [bytes(s) for s in got] == [EO.sign(bytes(secrets[i]), bytes(prefixes[i]), bytes(pubs[i]), msgs[i]) for i in rows]


def test_sign_matches_rfc8032(harness):
    rfc = EO.rfc8032()
    keys = expand(harness, b"".join(r[0] for r in rfc))
    got = sign(harness, *keys, [r[2] for r in rfc])
    assert [bytes(s) for s in got] == [r[3] for r in rfc]


def test_one_key_for_the_batch_equals_the_key_repeated(harness):
    _, _, msgs, _ = EO.sign_input()
    secrets, prefixes, pubs = EO.sign_input_keys()
    rows = list(EO.LISTED)
    m = [msgs[i] for i in rows]
    one = sign(harness, secrets[5], prefixes[5], pubs[5], m)
    rep = sign(harness, *(np.repeat(x[5:6], len(rows), axis=0) for x in (secrets, prefixes, pubs)), m)
    assert np.array_equal(one, rep)
    assert [bytes(s) for s in one] == [EO.sign(bytes(secrets[5]), bytes(prefixes[5]), bytes(pubs[5]), x) for x in m]


def test_stray_bytes_in_front_and_an_empty_first_message(harness):
    _, _, msgs, sigs = EO.sign_input()
    secrets, prefixes, pubs = EO.sign_input_keys()
    rows = [0, 1, 96, 97, 223]  # line 0's message is empty
    assert msgs[0] == b""
    for lead in (0, 1, 7):
        got = sign(harness, secrets[rows], prefixes[rows], pubs[rows], [msgs[i] for i in rows], lead=lead)
        assert [bytes(s) for s in got] == [sigs[i] for i in rows], lead


def test_the_public_key_is_hashed_as_its_bytes_stand(harness):
    """eddsa.go:110-118: Sign hashes Public's bytes; a key whose pub is not secret * B signs over those bytes"""
    _, _, msgs, _ = EO.sign_input()
    secrets, prefixes, pubs = EO.sign_input_keys()
    got = sign(harness, secrets[7], prefixes[7], pubs[8], [msgs[40]])
    assert bytes(got[0]) == EO.sign(bytes(secrets[7]), bytes(prefixes[7]), bytes(pubs[8]), msgs[40])
    assert bytes(got[0]) != EO.sign(bytes(secrets[7]), bytes(prefixes[7]), bytes(pubs[7]), msgs[40])


# ------------------------------------------------------------------------------------------------- the C ABI's checks
def test_argument_errors_and_empty_batches_never_touch_the_device():
    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    assert lib.kyb_ed25519_eddsa_expand(0, p, p, p, p) == 0
    assert lib.kyb_ed25519_eddsa_expand_dev(0, p, p, p, p, None) == 0
    assert lib.kyb_ed25519_eddsa_sign(0, p, p, p, 32, p, p, p, p) == 0
    assert lib.kyb_ed25519_eddsa_sign_dev(0, p, p, p, 0, p, p, p, p, None) == 0
    assert lib.kyb_ed25519_eddsa_expand(0, None, None, None, None) == 0
    assert lib.kyb_ed25519_eddsa_sign(0, None, None, None, 0, None, None, None, None) == 0
    off = (C.c_uint64 * 3)(0, 40, 8)  # decreasing
    po = C.addressof(off)
    bad = [
        ("kyb_ed25519_eddsa_expand", (2, None, p, p, p)),
        ("kyb_ed25519_eddsa_expand", (2, p, None, p, p)),
        ("kyb_ed25519_eddsa_expand", (2, p, p, None, p)),
        ("kyb_ed25519_eddsa_expand", (2, p, p, p, None)),
        ("kyb_ed25519_eddsa_expand_dev", (2, None, p, p, p, None)),
        ("kyb_ed25519_eddsa_expand_dev", (2, p, p, p, None, None)),
        ("kyb_ed25519_eddsa_sign", (2, p, p, p, 32, p, po, p, p)),
        ("kyb_ed25519_eddsa_sign", (2, p, p, p, 16, p, p, p, p)),
        ("kyb_ed25519_eddsa_sign", (2, p, p, p, 64, p, p, p, p)),
        ("kyb_ed25519_eddsa_sign", (2, None, p, p, 32, p, p, p, p)),
        ("kyb_ed25519_eddsa_sign", (2, p, None, p, 32, p, p, p, p)),
        ("kyb_ed25519_eddsa_sign", (2, p, p, None, 0, p, p, p, p)),
        ("kyb_ed25519_eddsa_sign", (2, p, p, p, 32, p, None, p, p)),
        ("kyb_ed25519_eddsa_sign", (2, p, p, p, 32, p, p, None, p)),
        ("kyb_ed25519_eddsa_sign_dev", (2, p, p, p, 33, p, p, p, p, None)),
        ("kyb_ed25519_eddsa_sign_dev", (2, p, p, p, 0, p, p, None, p, None)),
        ("kyb_ed25519_eddsa_sign_dev", (2, p, None, p, 32, p, p, p, p, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args)
        assert name.encode() in lib.kyb_last_error()
