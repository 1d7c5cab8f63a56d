"""sign/anon Encrypt / Decrypt without a GPU: the oracle (tests/_anon_enc_oracle.py) pinned to the two ciphertexts the
reference prints (tests/golden/anon_enc_examples.json: ExampleEncrypt_one and ExampleEncrypt_anonSet of enc_test.go, keys
rebuilt from blake2xb.New(nil) in the examples' order), and kyber_amd/csrc/ed25519_anonenc.cuh compiled for the CPU
(tests/anon_enc_harness.cpp) against the oracle on the labelled cases of tests/_anon_enc_cases.py; the C ABI's argument
checks; the Python mirror's key generation.

Limit of the check: the two printed ciphertexts pin the composition (key generation, the reduced master secret, the slot
and body streams, the MAC) byte for byte; every other case -- lengths, rejects, precedence -- is the oracle's, written
from enc.go's text."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from kyber_amd import _lib
from kyber_amd.util import blake2xb
from tests import _anon_enc_cases as AC
from tests import _anon_enc_oracle as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "anon_enc_examples.json")))["examples"]


# ------------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("ex", GOLDEN, ids=[g["name"] for g in GOLDEN])
def test_the_oracle_reproduces_the_printed_ciphertexts(ex):
    keys, mine, x, rand = E.golden_keys(ex["name"])
    assert len(keys) == ex["ring"] and mine == ex["mine"]
    msg, want = ex["message"].encode(), bytes.fromhex(ex["ciphertext"])
    assert E.encrypt(msg, keys, rand) == want
    assert E.decrypt(want, keys, mine, x) == msg == E.GOLDEN_MESSAGE


def test_the_goldens_need_the_reduced_master_secret():
    """with the clamped bytes in the slots instead of x mod l the printed ciphertext does not come out"""
    keys, _, _, rand = E.golden_keys("ExampleEncrypt_one")
    x = E.new_key(rand)
    assert x != E.reduced(x)
    wrong = E.slot(x, keys[0], x)
    assert wrong != bytes.fromhex(GOLDEN[0]["ciphertext"])[32:64] == E.slot(x, keys[0], E.reduced(x))


# ----------------------------------------------------------------------------------------------------- the harness
def build_harness():
    out = os.path.join(ROOT, "tests", "_build", "libanonencharness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "anon_enc_harness.cpp")])
    h = C.CDLL(out)
    sz, b, p = C.c_size_t, C.c_char_p, C.c_void_p
    h.aeh_stream32.argtypes = [b, b]
    h.aeh_xor_stream.argtypes = [b, b, sz, b]
    h.aeh_mac.argtypes = [b, sz, b]
    h.aeh_reduce.argtypes = [b, b]
    h.aeh_anon_seal.argtypes = [sz, sz, p, sz, p, p, p, p, p]
    h.aeh_anon_open.argtypes = [sz, sz, p, sz, p, p, sz, p, p, p, p]
    for f in (h.aeh_stream32, h.aeh_xor_stream, h.aeh_mac, h.aeh_reduce, h.aeh_anon_seal, h.aeh_anon_open):
        f.restype = None
    return h


@pytest.fixture(scope="module")
def harness():
    return build_harness()


def _arr(x, dtype=np.uint8):
    return np.frombuffer(x, dtype=dtype) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=dtype)


def _packed(msgs, lead: int):
    """(exactly sized blob, offsets): `lead` stray bytes stand in front of the first element"""
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    np.cumsum([len(m) for m in msgs], out=off[1:])
    off += np.uint64(lead)
    return _arr(b"\xa5" * lead + b"".join(msgs) or b"\0"), off


def _keys(sets, n):
    """(rows, stride) of one set or one per element"""
    shared = not isinstance(sets[0], (list, tuple))
    ring = len(sets) if shared else len(sets[0])
    rows = _arr(b"".join(sets) if shared else b"".join(b"".join(s) for s in sets))
    assert rows.size == 32 * ring * (1 if shared else n)
    return rows, 0 if shared else 32 * ring


def seal(h, ring, sets, xs, msgs, lead: int = 3):
    n = len(msgs)
    keys, stride = _keys(sets, n)
    x = _arr(b"".join(xs))
    blob, off = _packed(msgs, lead)
    over = 48 + 32 * ring
    out = np.full(int(off[-1]) + over * n, 0xEE, dtype=np.uint8)  # exactly sized: the last ciphertext ends it
    st = np.full(n, 0xEE, dtype=np.uint8)
    h.aeh_anon_seal(n, ring, keys.ctypes.data, stride, x.ctypes.data, blob.ctypes.data, off.ctypes.data, out.ctypes.data, st.ctypes.data)
    assert bytes(out[:lead]) == b"\xee" * lead  # nothing in front of the first slot
    raw = out.tobytes()
    return [raw[int(off[i]) + over * i:int(off[i + 1]) + over * (i + 1)] for i in range(n)], [int(s) for s in st]


def open_(h, ring, sets, mine, privs, cts, lead: int = 1):
    n = len(cts)
    keys, stride = _keys(sets, n)
    one = not isinstance(privs, (list, tuple))
    p = _arr(privs if one else b"".join(privs))
    blob, off = _packed(cts, lead)
    out = np.full(int(off[-1]), 0xEE, dtype=np.uint8)
    st = np.full(n, 0xEE, dtype=np.uint8)
    m = _arr(mine, np.uint32)
    h.aeh_anon_open(n, ring, keys.ctypes.data, stride, m.ctypes.data, p.ctypes.data, 0 if one else 32, blob.ctypes.data, off.ctypes.data,
                    out.ctypes.data, st.ctypes.data)
    assert bytes(out[:lead]) == b"\xee" * lead
    raw = out.tobytes()
    return [raw[int(off[i]):int(off[i + 1])] for i in range(n)], [int(s) for s in st]


def check_open(b, slots, sts):
    """every element of an open against the batch's oracle answer: the plaintext and zeros behind it, or an all-zero slot"""
    assert sts == b["open_status"], [(l, s, w) for l, s, w in zip(b["labels"], sts, b["open_status"]) if s != w]
    for label, slot, want, ct in zip(b["labels"], slots, b["opened"], b["cts"]):
        assert len(slot) == len(ct)
        assert slot == (want or b"").ljust(len(ct), b"\0"), label


def test_the_hash_parts_match_the_host_xof(harness):
    for n in AC.LENGTHS:
        data = blake2xb.New(b"parts%d" % n).Read(n)
        mac = C.create_string_buffer(16)
        harness.aeh_mac(data, n, mac)
        assert mac.raw == blake2xb.New(data).Read(16), n
        key = blake2xb.New(b"key%d" % n).Read(32)
        out = C.create_string_buffer(n or 1)
        harness.aeh_xor_stream(out, data, n, key)
        assert out.raw[:n] == blake2xb.New(key).XORKeyStream(data), n
    ks = C.create_string_buffer(32)
    harness.aeh_stream32(bytes(range(32)), ks)
    assert ks.raw == blake2xb.New(bytes(range(32))).Read(32)
    for x in (bytes(32), E.X_IS_L, bytes([0xFF]) * 32, (E.L - 1).to_bytes(32, "little"), (2 * E.L + 5).to_bytes(32, "little")):
        r = C.create_string_buffer(32)
        harness.aeh_reduce(x, r)
        assert r.raw == E.reduced(x)


@pytest.mark.parametrize("ex", GOLDEN, ids=[g["name"] for g in GOLDEN])
def test_the_harness_reproduces_the_printed_ciphertexts(harness, ex):
    keys, mine, x, rand = E.golden_keys(ex["name"])
    want = bytes.fromhex(ex["ciphertext"])
    cts, st = seal(harness, len(keys), keys, [E.new_key(rand)], [ex["message"].encode()])
    assert st == [0] and cts[0] == want
    slots, st = open_(harness, len(keys), keys, [mine], x, [want])
    assert st == [0] and slots[0] == ex["message"].encode().ljust(len(want), b"\0")


def test_every_message_length(harness):
    b = AC.lengths_batch()
    cts, st = seal(harness, b["ring"], b["sets"], b["x"], b["msgs"])
    assert st == b["seal_status"] and cts == b["sealed"]
    check_open(b, *open_(harness, b["ring"], b["sets"], b["mine"], b["privs"], b["cts"]))


@pytest.mark.parametrize("n,ring,per_element,one", [(5, 1, False, False), (5, 3, True, False), (5, 3, False, True), (5, 27, False, False),
                                                   (3, 27, True, True)])
def test_shapes(harness, n, ring, per_element, one):
    b = AC.shape_batch(n, ring, per_element, one)
    cts, st = seal(harness, ring, b["sets"], b["x"], b["msgs"])
    assert st == b["seal_status"] == [0] * n and cts == b["sealed"]
    check_open(b, *open_(harness, ring, b["sets"], b["mine"], b["privs"], b["cts"]))
    assert all(m is not None for m in b["opened"])


def test_rejects_between_valid_neighbours(harness):
    b = AC.rejects_batch()
    check_open(b, *open_(harness, b["ring"], b["sets"], b["mine"], b["privs"], b["cts"]))


def test_seal_edges_and_the_scalar_reduction(harness):
    b = AC.seal_edge_batch()
    cts, st = seal(harness, b["ring"], b["sets"], b["x"], b["msgs"])
    assert st == b["seal_status"] and cts == b["sealed"]
    assert cts[1] == bytes(len(cts[1]))  # the member that is no point: an all-zero slot
    i = b["labels"].index("x + l")
    xb = E.reduced(b["x"][i])
    assert xb == E.reduced(b["x"][0]) != b["x"][i]
    assert cts[i][32:64] == E.slot(b["x"][i], b["sets"][i][0], xb)  # the slots carry x mod l, the product uses x as given


def test_a_shared_set_with_a_member_that_is_no_point(harness):
    ring, K, xs, msgs, cts, mem = AC.shared_bad_set()
    out, st = seal(harness, ring, K, xs, msgs)
    assert st == [1, 1, 1] and all(c == bytes(len(c)) for c in out)
    slots, st = open_(harness, ring, K, [0, 0, 2, 0], [mem[0][0], mem[0][0], mem[2][0], mem[0][0]], cts + [cts[0][:40]])
    assert st == [1, 1, 1, 11] and all(s == bytes(len(s)) for s in slots)  # the short one: its length is checked first


# ------------------------------------------------------------------------------------------------- the Python mirror
def test_new_key_and_the_key_pair_helper():
    from kyber_amd.group import edwards25519 as ed

    suite = ed.NewSuite()
    r1, r2 = blake2xb.New(b"pair"), blake2xb.New(b"pair")
    x = suite.NewKey(r1)
    assert x.v == E.new_key(r2) and x.v[0] & 7 == 0 and x.v[31] & 0xC0 == 0x40
    assert x.MarshalBinary() == E.reduced(x.v) != x.v  # stored unreduced, marshalled reduced
    secret, buf, rest = suite.NewKeyAndSeed(blake2xb.New(b"pair"))
    assert secret.v == x.v and buf == blake2xb.New(b"pair").Read(32) and len(rest) == 32


# ------------------------------------------------------------------------------------------------- the C ABI's checks
def test_argument_errors_and_empty_batches_never_touch_the_device():
    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    assert lib.kyb_ed25519_anon_seal(0, 3, p, 0, p, p, p, p, p) == 0
    assert lib.kyb_ed25519_anon_seal_dev(0, 3, p, 96, p, p, p, p, p, None) == 0
    assert lib.kyb_ed25519_anon_open(0, 1, p, 0, p, p, 32, p, p, p, p) == 0
    assert lib.kyb_ed25519_anon_open_dev(0, 1, p, 32, p, p, 0, p, p, p, p, None) == 0
    off = (C.c_uint64 * 3)(0, 40, 8)  # decreasing
    po = C.addressof(off)
    mine = (C.c_uint32 * 2)(0, 3)  # names position 3 of a set of three
    bad = [
        ("kyb_ed25519_anon_seal", (2, 0, p, 0, p, p, p, p, p)),  # an empty set
        ("kyb_ed25519_anon_seal", (2, _lib.ANON_MAX_RING + 1, p, 0, p, p, p, p, p)),
        ("kyb_ed25519_anon_seal", (2, 3, p, 32, p, p, p, p, p)),  # a stride that is not the set's length
        ("kyb_ed25519_anon_seal", (2, 3, p, 0, p, p, po, p, p)),
        ("kyb_ed25519_anon_seal", (2, 3, None, 0, p, p, p, p, p)),
        ("kyb_ed25519_anon_seal", (2, 3, p, 0, p, p, p, None, p)),
        ("kyb_ed25519_anon_seal_dev", (2, 0, p, 0, p, p, p, p, p, None)),
        ("kyb_ed25519_anon_seal_dev", (2, 3, p, 64, p, p, p, p, p, None)),
        ("kyb_ed25519_anon_seal_dev", (2, 3, p, 96, None, p, p, p, p, None)),
        ("kyb_ed25519_anon_open", (2, 0, p, 0, p, p, 0, p, p, p, p)),
        ("kyb_ed25519_anon_open", (2, _lib.ANON_MAX_RING + 1, p, 0, p, p, 0, p, p, p, p)),
        ("kyb_ed25519_anon_open", (2, 3, p, 0, p, p, 8, p, p, p, p)),  # a key stride that is neither 0 nor 32
        ("kyb_ed25519_anon_open", (2, 3, p, 33, p, p, 0, p, p, p, p)),
        ("kyb_ed25519_anon_open", (2, 3, p, 0, p, p, 0, p, po, p, p)),
        ("kyb_ed25519_anon_open", (2, 3, p, 0, C.addressof(mine), p, 0, p, p, p, p)),  # mine out of range
        ("kyb_ed25519_anon_open", (2, 3, p, 0, None, p, 0, p, p, p, p)),
        ("kyb_ed25519_anon_open_dev", (2, 3, p, 0, p, p, 16, p, p, p, p, None)),
        ("kyb_ed25519_anon_open_dev", (2, 3, p, 0, p, None, 0, p, p, p, p, None)),
    ]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args)
        assert name.encode() in lib.kyb_last_error()
