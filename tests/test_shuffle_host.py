"""shuffle/ without a GPU: kyber_amd/csrc/ed25519_shuffle.cuh compiled for the CPU (tests/shuffle_harness.cpp) against
the Python XOF and the big-integer oracle; the sequential restatement of pair.go, simple.go, sequences.go and hash.go
(tests/_shuffle_oracle.py) through full rounds with the tamperings of shuffle_test.go; the C ABI's argument checks.

The reference's shuffle tests print no bytes and no Go toolchain is at hand, so no transcript of the Go program is
pinned: the oracle, written from the reference's text, is the yardstick."""
import ctypes as C
import math
import os
import random
import subprocess

import pytest

from kyber_amd import _lib
from kyber_amd.util import blake2xb as X
from oracle import ed25519 as O
from tests import _shuffle_cases as SC
from tests import _shuffle_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_harness():
    out = os.path.join(ROOT, "tests", "_build", "libshuffleharness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "shuffle_harness.cpp")])
    h = C.CDLL(out)
    h.shf_window.restype = C.c_uint64
    h.shf_window.argtypes = [C.c_uint64]
    h.shf_node.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p]
    h.shf_stream.argtypes = [C.c_char_p, C.c_uint64, C.c_size_t, C.c_char_p]
    h.shf_draws.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_size_t, C.c_char_p, C.c_char_p]
    h.shf_theta.argtypes = [C.c_size_t] + [C.c_char_p] * 7 + [C.c_int, C.c_char_p, C.c_char_p]
    return h


@pytest.fixture(scope="module")
def harness():
    return build_harness()


ROOT_HASH = X.root_hash(b"shuffle host tests", b"a transcript")


def test_root_hash_by_hashlib_equals_the_parameterised_blake2b():
    for key, msg in ((b"", b""), (b"eleven byte", b"x"), (bytes(range(64)), bytes(1000)), (bytes(32), b"")):
        want = X.blake2b_param(msg, X.param_block(X.SIZE, len(key), 1, 1, 0, 0, X.UNKNOWN, 0, 0), key)
        assert X.root_hash(key, msg) == want, (len(key), len(msg))


def test_stream_nodes_match_the_python_xof(harness):
    out = C.create_string_buffer(64)
    for node in list(range(300)) + [2**31 - 1, 2**31, 2**32 - 3, 2**32 - 2, 2**32 - 1]:
        harness.shf_node(ROOT_HASH, node, out)
        assert out.raw == X.output_node(ROOT_HASH, node), node
    xof = X.New(b"stream")
    xof.Read(77)
    want = xof.Clone().Read(1000)
    buf = C.create_string_buffer(1000)
    harness.shf_stream(xof.Root(), xof.Tell(), 1000, buf)
    assert buf.raw == want


@pytest.mark.parametrize("pos", [0, 1, 8, 32, 40, 63])
def test_draws_match_pick_at_every_alignment(harness, pos):
    n = 2000
    stream = b"".join(X.output_node(ROOT_HASH, i) for i in range((pos + 32 * n) // 64 + 1))
    value, accept = C.create_string_buffer(32 * n), C.create_string_buffer(n)
    harness.shf_draws(ROOT_HASH, pos, 0, n, value, accept)
    accepted = 0
    for j in range(n):
        draw = stream[pos + 32 * j:pos + 32 * j + 32]
        want = int.from_bytes(bytes([draw[0] & 0x1F]) + draw[1:], "big")
        assert int.from_bytes(value.raw[32 * j:32 * j + 32], "little") == want, (pos, j)
        assert accept.raw[j] == (want < X.ORDER), (pos, j)
        if want < X.ORDER:
            assert X.pick_int(lambda k: draw) == (want, 1)
            accepted += 1
    assert 900 < accepted < 1150  # l / 2^253 is just above one half
    # the last whole draw before the stream's end: inside or across the last two of the 2^32 nodes
    j = (2**38 - 32 - pos) // 32
    at = pos + 32 * j - (2**32 - 2) * 64
    draw = (X.output_node(ROOT_HASH, 2**32 - 2) + X.output_node(ROOT_HASH, 2**32 - 1))[at:at + 32]
    harness.shf_draws(ROOT_HASH, pos, j, 1, value, accept)
    assert int.from_bytes(value.raw[:32], "little") == int.from_bytes(bytes([draw[0] & 0x1F]) + draw[1:], "big")


def test_window_is_the_formula_and_leaves_sixteen_root_n_of_slack(harness):
    for n in (1, 2, 64, 4099, 2**16, 2**20):
        w = harness.shf_window(n)
        root = math.isqrt(n - 1) + 1  # ceil(sqrt n) for n >= 1
        assert root * root >= n > (root - 1) * (root - 1)
        assert w == 2 * n + 16 * root + 256
        assert w - 2 * n >= 16 * math.sqrt(n)


def _run_theta(harness, u, w, rows, vartime):
    n = len(rows)
    col = lambda i: b"".join(r[i] for r in rows)
    ok, st = C.create_string_buffer(n), C.create_string_buffer(n)
    harness.shf_theta(n, col(1), col(2), u, col(3), col(4), w, col(5), int(vartime), ok, st)
    return list(ok.raw), list(st.raw)


@pytest.mark.parametrize("vartime", [False, True])
def test_theta_lane_program_matches_the_oracle_on_the_labelled_table(harness, vartime):
    differs_from_point_negation = labels = 0
    seen = set()
    for name, u, w, rows in SC.batches():
        ok, st = _run_theta(harness, u, w, rows, vartime)
        for (label, a, A, b, B, T, must), got_ok, got_st in zip(rows, ok, st):
            want_ok, want_st = SC.expect(a, A, u, b, B, w, T, vartime)
            assert (got_ok, got_st) == (want_ok, want_st), (name, label)
            if must is not None:
                assert want_ok == must, (name, label)
            if "undecodable" in label or label == "and A too":
                assert want_st == SC.ST_BAD_POINT and want_ok == 0
            if label == "T off the curve":
                assert (want_ok, want_st) == (0, 0)
            if want_st == 0 and SC.expect(a, A, u, b, B, w, T, vartime, point_negation=True)[0] != want_ok:
                differs_from_point_negation += 1
            seen.add(label)
            labels += 1
    assert differs_from_point_negation >= 2  # Neg(b) is a scalar: rows whose verdict point negation would flip
    assert {"a tampered", "b tampered", "A tampered", "B tampered", "T tampered", "U tampered", "W tampered", "as y + p",
            "as -0", "Xhat identity", "Yhat identity", "torsion in A and B", "a = scalar 4", "b = scalar 4"} <= seen
    assert labels >= 100


def test_scalar_negation_is_the_reduced_residue(harness):
    out = C.create_string_buffer(32)
    for v in (0, 1, O.L - 1, O.L, O.L + 5, 2**255, 2**255 + 7, 2**256 - 1, 16 * O.L - 1, 16 * O.L):
        if v < 2**256:
            harness.shf_neg(v.to_bytes(32, "little"), out)
            assert int.from_bytes(out.raw, "little") == -v % O.L, v


# ------------------------------------------------------------------------------------------------ oracle round trips
def _pairs(k: int, seed: bytes, H):
    """k ElGamal encryptions of random points under the key H (shuffle_test.go:60-80)"""
    rng = X.New(seed).Read
    X_, Y_ = [], []
    for _ in range(k):
        c = SO.sc(SO.pick(rng))
        r = SO.sc(SO.pick(rng))
        X_.append(SO.pmul(r, None))
        Y_.append(SO.padd(SO.pmul(r, H), SO.pmul(c, None)))
    return X_, Y_


def _oracle_round(k: int, given_g: bool):
    h = SO.sc(SO.pick(X.New(b"key").Read))
    H = SO.pmul(h, None)
    G = SO.pmul(SO.sc(7), None) if given_g else None
    if given_g:
        H = SO.pmul(h, G)
    Xs, Ys = _pairs(k, b"pairs %d" % k, H)
    rand = X.New(b"rand %d" % k)
    Xbar, Ybar, prover = SO.shuffle(G, H, Xs, Ys, rand.Read)
    proof = SO.hash_prove(b"PairShuffle", prover, rand.Read)
    return G, H, Xs, Ys, Xbar, Ybar, proof


@pytest.mark.parametrize("given_g", [False, True])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_oracle_round_trip_and_the_references_tamperings(k, given_g):
    G, H, Xs, Ys, Xbar, Ybar, proof = _oracle_round(k, given_g)
    assert len(proof) == 32 * (9 * k + 3 + k + 1 + 2 * k - 1)
    assert SO.hash_verify(b"PairShuffle", SO.verifier(G, H, Xs, Ys, Xbar, Ybar), proof) is None
    assert sorted(Xbar) != sorted(Xs)  # re-randomised
    # Xbar[0] and Xbar[1] swapped (shuffle_test.go:97-115)
    swapped = [Xbar[1], Xbar[0]] + Xbar[2:]
    assert SO.hash_verify(b"PairShuffle", SO.verifier(G, H, Xs, Ys, swapped, Ybar), proof) == SO.ERR_PAIR
    # a truncated proof fails, trailing bytes pass, another protocol name fails
    assert SO.hash_verify(b"PairShuffle", SO.verifier(G, H, Xs, Ys, Xbar, Ybar), proof[:-1]) == SO.ERR_SHORT
    assert SO.hash_verify(b"PairShuffle", SO.verifier(G, H, Xs, Ys, Xbar, Ybar), proof + b"trailing") is None
    assert SO.hash_verify(b"pairShuffle", SO.verifier(G, H, Xs, Ys, Xbar, Ybar), proof) == SO.ERR_SIMPLE
    # an undecodable transcript point decides before any equation
    bad = SC._off_curve(random.Random(1))
    assert SO.hash_verify(b"PairShuffle", SO.verifier(G, H, Xs, Ys, Xbar, Ybar), proof[:32] + bad + proof[64:]) == SO.ERR_POINT


def test_oracle_sequences_round_trip_and_a_corrupted_input():
    NQ, k = 6, 3
    h = SO.sc(SO.pick(X.New(b"key").Read))
    H = SO.pmul(h, None)
    cols = [_pairs(k, b"seq %d" % j, H) for j in range(NQ)]
    Xs, Ys = [c[0] for c in cols], [c[1] for c in cols]
    rand = X.New(b"sequences")
    xbar, ybar, get_prover = SO.sequences_shuffle(None, H, Xs, Ys, rand.Read)
    e = [SO.pick(rand.Read) for _ in range(NQ)]
    proof = SO.hash_prove(b"PairShuffle", get_prover(e), rand.Read)
    ew = [SO.sc(v) for v in e]
    up = SO.get_sequence_verifiable(Xs, Ys, xbar, ybar, ew)
    assert SO.hash_verify(b"PairShuffle", SO.verifier(None, H, *up), proof) is None
    # a corrupted sequence input (shuffle_test.go:192-221)
    Xs[1][0] = SO.pmul(SO.sc(12345), None)
    up = SO.get_sequence_verifiable(Xs, Ys, xbar, ybar, ew)
    assert SO.hash_verify(b"PairShuffle", SO.verifier(None, H, *up), proof) == SO.ERR_PAIR


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_checks_arguments_without_a_device():
    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    used = C.c_uint64(77)
    up = C.addressof(used)
    assert lib.kyb_ed25519_xof_pick(0, p, 0, p, up) == 0 and used.value == 0
    assert lib.kyb_ed25519_xof_pick_dev(0, p, 0, p, up, None) == 0
    assert lib.kyb_ed25519_theta_check(0, p, p, None, p, p, None, p, p, None, 0) == 0
    assert lib.kyb_ed25519_theta_check_dev(0, p, p, p, p, p, p, p, p, p, 1, None) == 0
    limit = 2**38  # 2^32 output nodes of 64 bytes
    w4 = 2 * 4 + 16 * 2 + 256
    bad = [
        ("kyb_ed25519_xof_pick", (4, None, 0, p, up)),
        ("kyb_ed25519_xof_pick", (4, p, 0, None, up)),
        ("kyb_ed25519_xof_pick", (4, p, 0, p, None)),
        ("kyb_ed25519_xof_pick", (4, p, limit - 32 * w4 + 1, p, up)),  # the window's last byte would lie in node 2^32
        ("kyb_ed25519_xof_pick", (4, p, 2**64 - 1, p, up)),
        ("kyb_ed25519_xof_pick", (2**31 + 1, p, 0, p, up)),
        ("kyb_ed25519_xof_pick_dev", (4, p, limit, p, up, None)),
        ("kyb_ed25519_xof_pick_dev", (4, None, 0, p, up, None)),
        ("kyb_ed25519_theta_check", (4, None, p, p, p, p, p, p, p, p, 0)),
        ("kyb_ed25519_theta_check", (4, p, p, None, p, p, None, None, p, p, 0)),
        ("kyb_ed25519_theta_check", (4, p, p, None, p, p, None, p, None, p, 0)),
        ("kyb_ed25519_theta_check", (4, p, p, p, p, p, p, p, p, p, _lib.KYB_F_UNIFORM)),
        ("kyb_ed25519_theta_check", (4, p, p, p, p, p, p, p, p, p, 2)),
        ("kyb_ed25519_theta_check_dev", (4, p, p, p, p, p, p, p, p, p, _lib.KYB_F_UNIFORM | 1, None)),
        ("kyb_ed25519_theta_check_dev", (4, p, None, p, p, p, p, p, p, p, 0, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args)
        assert name.encode() + b":" in lib.kyb_last_error(), (name, lib.kyb_last_error())


def test_header_cites_the_reference_lines():
    src = open(os.path.join(ROOT, "include", "kyber_hip.h")).read()
    for cite in ("simple.go:178-183", "pair.go:295-309", "hash.go:111-142", "blake.go:55-74", "rand.go:19-46"):
        assert cite in src, cite
    assert "KYB_E_EXHAUSTED" in src and _lib.E_EXHAUSTED == -5
