"""kyb_ed25519_lincomb and kyb_ed25519_fs_challenge without a GPU: kyber_amd/csrc/ed25519_proof.cuh compiled for the CPU
(tests/proof_harness.cpp) against the big-integer oracle (tests/_proof_cases.py) and the Python XOF
(kyber_amd/util/blake2xb.py), and the C ABI's argument checks through the built library."""
import ctypes as C
import os
import random
import subprocess

import pytest

from kyber_amd import _lib
from kyber_amd.util import blake2xb as X
from tests import _proof_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_harness():
    out = os.path.join(ROOT, "tests", "_build", "libproofharness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "proof_harness.cpp")])
    h = C.CDLL(out)
    h.prf_lincomb.argtypes = [C.c_size_t] * 3 + [C.c_char_p] * 3 + [C.c_uint32, C.c_char_p, C.c_int] + [C.c_char_p] * 3
    h.prf_lincomb.restype = None
    h.prf_fs_challenge.argtypes = [C.c_size_t, C.c_char_p, C.c_void_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p]
    h.prf_fs_challenge.restype = None
    return h


@pytest.fixture(scope="module")
def harness():
    return build_harness()


def run_lincomb(harness, ko, ks, nil_mask, shared, rows, expect, vartime, want_out=True, want_ok=True):
    n = len(rows)
    scalars = b"".join(b"".join(r[1]) for r in rows)
    own = b"".join(b"".join(r[2]) for r in rows) if ko else None
    out, ok, st = C.create_string_buffer(32 * n), C.create_string_buffer(n), C.create_string_buffer(n)
    harness.prf_lincomb(n, ko, ks, scalars, own, b"".join(shared) if ks else None, nil_mask, b"".join(expect) if want_ok else None,
                        int(vartime), out if want_out else None, ok if want_ok else None, st)
    return [out.raw[32 * i:32 * i + 32] for i in range(n)], list(ok.raw), list(st.raw)


@pytest.mark.parametrize("vartime", [False, True])
@pytest.mark.parametrize("ko,ks,nil_mask", PC.shapes())
def test_lane_program_matches_the_oracle_on_the_labelled_table(harness, ko, ks, nil_mask, vartime):
    for name, shared, rows in PC.batches(ko, ks, nil_mask):
        vals = [PC.value(ko, ks, nil_mask, shared, r[1], r[2], vartime) for r in rows]
        expect = [PC.expect_bytes(r[3], v) for r, v in zip(rows, vals)]
        out, ok, st = run_lincomb(harness, ko, ks, nil_mask, shared, rows, expect, vartime)
        for i, (row, v, e) in enumerate(zip(rows, vals, expect)):
            want_ok, want_st = PC.verdict(v, e)
            assert out[i] == (v if v is not None else bytes(32)), (name, row[0])
            assert (ok[i], st[i]) == (want_ok, want_st), (name, row[0], PC.kind_checked(row[3], v))
        # the parts alone give the same answers
        assert run_lincomb(harness, ko, ks, nil_mask, shared, rows, expect, vartime, want_ok=False)[0] == out
        assert run_lincomb(harness, ko, ks, nil_mask, shared, rows, expect, vartime, want_out=False)[1:] == (ok, st)


def test_the_table_holds_what_it_promises():
    """every kind of row, both verdicts of every expect kind, and the flag-dependent values"""
    labels, verdicts, flag_dependent = set(), set(), 0
    for ko, ks, nil_mask in ((1, 2, 1), (2, 2, 1), (4, 4, 5)):
        assert (ko, ks, nil_mask) in PC.FULL_GRID
        for name, shared, rows in PC.batches(ko, ks, nil_mask):
            for label, s, o, kind in rows:
                labels.add(label)
                v = PC.value(ko, ks, nil_mask, shared, s, o, False)
                verdicts.add((PC.kind_checked(kind, v), PC.verdict(v, PC.expect_bytes(kind, v))))
                flag_dependent += v != PC.value(ko, ks, nil_mask, shared, s, o, True)
                if v is not None and "cancel" in label or label == "zero scalars":
                    assert v == PC.IDENT and PC.expect_bytes(kind, v) == (PC.O.P + 1).to_bytes(32, "little"), label
    for kind, want in (("equal", (1, 0)), ("equal", (0, 1)), ("noncanonical", (1, 0)), ("sign", (0, 0)), ("off curve", (0, 0))):
        assert (kind, want) in verdicts, (kind, want)
    assert flag_dependent >= 10  # scalars at or above 2^255 in own and shared slots; nil slots do not depend on the flag
    for part in ("zero scalars", "every term on one point", "terms 0 and 1 cancel", "own 0 undecodable", "own 1 identity as y + p",
                 "shared 1 undecodable", "shared 1 identity as y + p", "own 0 order 8", "every scalar 2^256 - 1"):
        assert any(part in l for l in labels), part
    # a nil term is checked against mul_base's value, which the flag does not change
    s = [PC.raw(2**255 + 2**252 + 9)]  # top digit 9: dropped by the constant-structure ladder
    assert PC.value(0, 1, 1, [bytes(32)], s, [], True) == PC.value(0, 1, 1, [bytes(32)], s, [], False) == PC.O.mul_base(s[0])
    assert PC.value(0, 1, 0, [PC.BASE], s, [], True) != PC.value(0, 1, 0, [PC.BASE], s, [], False)
    assert len(PC.shapes()) == 5 * (1 + 2 + 4 + 3 + 3) - 1 and {(a, b) for a, b, _ in PC.shapes()} == \
        {(a, b) for a in range(5) for b in range(5)} - {(0, 0)}


NAME_LENS = (0, 1, 63, 64, 65, 128, 129)
DATA_LENS = (0, 32, 96, 2048)


def fs_challenge(name: bytes, data: bytes) -> bytes:
    """hashVerifier.PubRand's pick by the Python XOF (hash.go:111-142)"""
    x = X.New(name)
    if data:
        x.Reseed()
        x.Write(data)
    return X.pick(x)


@pytest.mark.parametrize("data_len", DATA_LENS)
@pytest.mark.parametrize("name_len", NAME_LENS)
def test_challenge_lane_matches_the_python_xof(harness, name_len, data_len):
    rng = random.Random(name_len * 4096 + data_len)
    n = 5
    data = rng.randbytes(n * data_len)
    c, st = C.create_string_buffer(32 * n), C.create_string_buffer(n)
    # one name for the batch
    name = rng.randbytes(name_len)
    harness.prf_fs_challenge(n, name, None, name_len, data, data_len, c, st)
    for i in range(n):
        assert c.raw[32 * i:32 * i + 32] == fs_challenge(name, data[i * data_len:(i + 1) * data_len]), i
    assert st.raw == bytes(n)
    # a name per proof: this length, its neighbours and an empty one, at offsets of every alignment
    lens = [name_len, 0, name_len + 1, max(name_len - 1, 0), name_len]
    names = [rng.randbytes(k) for k in lens]
    off = (C.c_uint64 * (n + 1))(*[3 + sum(lens[:i]) for i in range(n + 1)])
    harness.prf_fs_challenge(n, b"pad" + b"".join(names), off, 7777, data, data_len, c, st)
    for i in range(n):
        assert c.raw[32 * i:32 * i + 32] == fs_challenge(names[i], data[i * data_len:(i + 1) * data_len]), i
    assert st.raw == bytes(n)


def test_challenge_reproduces_the_printed_proof_of_hash_prove_1():
    """Example_hashProve1 (hash_test.go:14-57): Rep("X", "x", "B") under the name "Hello World!"; the proof's 64 bytes are
    the commitment V and the response r = v - c x, and V == c X + r B with the challenge the lane derives from V"""
    import json
    from oracle import ed25519 as O
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "proof_examples.json")))
    proof = bytes.fromhex(gold["hashProve1"]["proof"])
    name = gold["hashProve1"]["name"].encode()
    c = fs_challenge(name, proof[:32])
    h = build_harness()
    cb, st = C.create_string_buffer(32), C.create_string_buffer(1)
    h.prf_fs_challenge(1, name, None, len(name), proof[:32], 32, cb, st)
    assert cb.raw == c and st.raw == b"\0"
    # X = x B with x the first pick of blake2xb.New("example") (hash_test.go:27-29)
    x = X.pick(X.New(b"example"))
    Xp = O.mul_base(x)
    assert PC.value(1, 1, 1, [bytes(32)], [c, proof[32:64]], [Xp], False) == proof[:32]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_checks_arguments_without_a_device():
    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    V = _lib.KYB_F_VARTIME
    # n = 0 is KYB_OK and touches no device
    assert lib.kyb_ed25519_lincomb(0, 1, 2, p, p, p, 2, p, p, p, p, V) == 0
    assert lib.kyb_ed25519_lincomb_dev(0, 0, 1, p, None, p, 1, None, p, None, None, 0, None) == 0
    assert lib.kyb_ed25519_fs_challenge(0, p, None, 5, p, 32, p, p) == 0
    assert lib.kyb_ed25519_fs_challenge_dev(0, None, None, 0, None, 0, None, None, None) == 0
    # n, ko, ks, scalars, own, shared, nil_mask, expect, out, ok, status, flags
    bad = [
        (4, 1, 2, p, p, p, 0, p, p, p, p, _lib.KYB_F_UNIFORM),
        (4, 1, 2, p, p, p, 0, p, p, p, p, _lib.KYB_F_UNIFORM | V),
        (4, 1, 2, p, p, p, 0, p, p, p, p, 2),
        (4, 1, 2, p, p, p, 0, p, p, p, p, _lib.KYB_F_DLEQ_FS),
        (4, 1, 2, p, p, p, 4, p, p, p, p, 0),  # nil_mask bits at or above ks
        (4, 1, 0, p, p, None, 1, p, p, p, p, 0),
        (4, 1, 4, p, p, p, 16, p, p, p, p, 0),
        (4, 1, 2, p, p, p, 0, p, p, None, p, 0),  # expect without ok
        (4, 1, 2, p, p, p, 0, None, p, p, p, 0),  # ok without expect
        (4, 1, 2, p, p, p, 0, None, None, None, p, 0),  # neither out nor ok
        (4, 1, 2, p, None, p, 0, p, p, p, p, 0),  # pointers that contradict ko / ks
        (4, 0, 2, p, p, p, 0, p, p, p, p, 0),
        (4, 1, 2, p, p, None, 0, p, p, p, p, 0),
        (4, 1, 0, p, p, p, 0, p, p, p, p, 0),
        (4, 0, 0, p, None, None, 0, p, p, p, p, 0),  # limits
        (4, 5, 0, p, p, None, 0, p, p, p, p, 0),
        (4, 0, 5, p, None, p, 0, p, p, p, p, 0),
        (4, 1, 2, None, p, p, 0, p, p, p, p, 0),
    ]
    for args in bad:
        for name, extra in (("kyb_ed25519_lincomb", ()), ("kyb_ed25519_lincomb_dev", (None,))):
            assert getattr(lib, name)(*args, *extra) == -1, (name, args)
            assert name.encode() + b":" in lib.kyb_last_error(), (name, lib.kyb_last_error())
        if args[3] is not None:  # the shape of a call is wrong whatever n is
            assert lib.kyb_ed25519_lincomb(0, *args[1:]) == -1, args
    off = (C.c_uint64 * 5)(0, 3, 2, 5, 9)
    bad = [
        ("kyb_ed25519_fs_challenge", (4, p, None, 5, p, 33, p, p)),  # data_len is a multiple of 32
        ("kyb_ed25519_fs_challenge", (4, p, None, 5, p, 32, None, p)),
        ("kyb_ed25519_fs_challenge", (4, p, None, 5, None, 32, p, p)),
        ("kyb_ed25519_fs_challenge", (4, None, None, 5, p, 32, p, p)),
        ("kyb_ed25519_fs_challenge", (4, None, C.addressof(off), 0, p, 32, p, p)),
        ("kyb_ed25519_fs_challenge", (4, p, C.addressof(off), 0, p, 32, p, p)),  # offsets that decrease
        ("kyb_ed25519_fs_challenge_dev", (4, p, None, 5, p, 16, p, p, None)),
        ("kyb_ed25519_fs_challenge_dev", (4, p, None, 5, p, 32, None, p, None)),
        ("kyb_ed25519_fs_challenge_dev", (4, None, None, 5, p, 32, p, p, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args)
        assert name.encode() + b":" in lib.kyb_last_error(), (name, lib.kyb_last_error())


def test_header_cites_the_reference_lines_and_the_current_device():
    src = open(os.path.join(ROOT, "include", "kyber_hip.h")).read()
    item = src[src.index("int kyb_ed25519_theta_check_dev"):src.index("int kyb_ed25519_fs_challenge_dev")]
    for cite in ("proof.go:203-237", "proof.go:298-322", "point.go:243", "biffle_test.go:41", "hash.go:111-142", "blake.go:19-41, 55-74",
                 "hash.go:46-65"):
        assert cite in item, cite
    assert item.count("runs on the current device") == 2
    hip = open(os.path.join(ROOT, "kyber_amd", "csrc", "ed25519_proof.hip")).read()
    assert "md_active(" not in hip and "current device" in hip[:hip.index("#include")]
