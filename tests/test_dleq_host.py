"""proof/dleq and share/pvss without a GPU: kyber_amd/csrc/blake2xb.cuh and ed25519_dleq.cuh compiled for the CPU
(tests/dleq_harness.cpp) against hashlib, the Python XOF and the oracle; the oracle's restatement of pvss.go through a
full round with the tamperings of pvss_test.go; the C ABI's argument checks."""
import collections
import ctypes as C
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

from kyber_amd.util import blake2xb as X
from oracle import ed25519 as O
from tests import _dleq_cases as DC
from tests import _ed_verify_oracle as V
from tests import _pvss_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# SHA-256(i as four little-endian bytes), i < 2000, as XOF seeds; found on the CPU with the Python XOF: the indices whose
# pick needs exactly 1, 2, 3, 4 draws and one that needs at least 6
PICK_SEEDS = 2000
FIRST_BY_DRAWS = {1: 0, 2: 1, 3: 45, 4: 22}  # and 6 draws at i = 17, 16 at i = 1943, 17 at i = 994


def _seed(i: int) -> bytes:
    return hashlib.sha256(i.to_bytes(4, "little")).digest()


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build", "libdleqharness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "dleq_harness.cpp")])
    return C.CDLL(out)


def test_compression_matches_hashlib_on_every_length_and_key(harness):
    rng = random.Random(1)
    out = C.create_string_buffer(64)
    for key in (b"", bytes(rng.getrandbits(8) for _ in range(32)), bytes(rng.getrandbits(8) for _ in range(64))):
        for n in range(258):
            msg = bytes(rng.getrandbits(8) for _ in range(n))
            harness.dlq_blake2b(key, C.c_size_t(len(key)), msg, C.c_size_t(n), out)
            assert out.raw == hashlib.blake2b(msg, key=key).digest(), (len(key), n)


def test_scalar_pick_matches_the_python_xof_and_its_rejection_loop(harness):
    out = C.create_string_buffer(32)
    hist = collections.Counter()
    for i in range(PICK_SEEDS):
        want, draws = X.pick_int(X.New(_seed(i)).Read)
        got = harness.dlq_pick(_seed(i), out)
        assert got == draws and int.from_bytes(out.raw, "little") == want, i
        hist[draws] += 1
    assert all(hist[k] for k in (1, 2, 3, 4)) and any(hist[k] for k in hist if k >= 6), hist
    assert 800 < hist[1] < 1250  # about half of all draws are rejected: l is just above 2^252 of 2^253


def test_pick_seed_list_is_fixed():
    """the first seed of the list for each draw count (a change of the derivation would move them)"""
    first = {}
    for i in range(PICK_SEEDS):
        d = X.pick_int(X.New(_seed(i)).Read)[1]
        first.setdefault(d, i)
    assert {k: first[k] for k in (1, 2, 3, 4)} == FIRST_BY_DRAWS and first[6] == 17 and first[17] == 994


def test_canonical_bytes_rule_is_encode_of_decode(harness):
    misc = V._misc()
    encs = [bytes.fromhex(h) for h in misc["small_order"]]
    encs += [s[:31] + bytes([s[31] | 0x80]) for s in encs]
    for y in (0, 1, O.P - 1, O.P, O.P + 1, 2**255 - 1):
        encs += [y.to_bytes(32, "little"), (y | 1 << 255).to_bytes(32, "little")]
    rng = random.Random(2)
    encs += [(O.P + k | s << 255).to_bytes(32, "little") for k in range(19) for s in (0, 1)]  # every y + p that fits
    encs += [O.encode(O.mul_int(rng.getrandbits(252) + 1, O.B)) for _ in range(64)]
    encs += [rng.getrandbits(256).to_bytes(32, "little") for _ in range(256)]
    out = C.create_string_buffer(32)
    decoded = noncanon = 0
    for e in encs:
        harness.dlq_canon(e, out)
        assert out.raw == PO.canon_bytes_rule(e)
        want = PO.canon(e)
        if want is not None:
            assert out.raw == want, e.hex()
            decoded += 1
            noncanon += want != e
    assert decoded >= 64 + 16 + 100 and noncanon >= 6
    assert PO.canon((1 | 1 << 255).to_bytes(32, "little")) == (1).to_bytes(32, "little")  # "-0" decodes, sign 0 comes back


def test_challenge_matches_hashlib_and_the_python_xof(harness):
    out = C.create_string_buffer(32)
    rows = [r[2:4] + r[6:8] for r in DC.cases(fs=True)[0] if all(PO.canon(p) is not None for p in r[2:4] + r[6:8])]
    assert len(rows) >= 40
    for xG, xH, vG, vH in rows:
        assert harness.dlq_challenge(xG, xH, vG, vH, out) >= 1
        assert out.raw == PO.dleq_challenge(xG, xH, vG, vH)
    draws = collections.Counter()
    for row in DC.challenge_inputs(600):
        draws[harness.dlq_challenge(*row, out)] += 1
        assert out.raw == PO.device_challenge(*row)
    assert max(draws) >= 6 and min(draws) == 1


def _verify(harness, rows, gs=32, hs=32, expect=None, fs=False, vartime=False):
    n = len(rows)
    a = DC.pack(rows)
    ok, st = np.zeros(n, dtype=np.uint8), np.full(n, 255, dtype=np.uint8)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    harness.dlq_verify(C.c_size_t(n), p(a[0]), C.c_size_t(gs), p(a[1]), C.c_size_t(hs), *[p(x) for x in a[2:]], expect,
                       int(fs), int(vartime), p(ok), p(st))
    return ok.astype(bool), st


@pytest.mark.parametrize("vartime", [False, True])
def test_lane_program_matches_the_oracle(harness, vartime):
    rows, labels = DC.cases()
    rows = rows + [DC.commitments_from_equations(r, vartime) for r, l in zip(rows, labels) if l == "edge-scalars"]
    labels = labels + ["edge-valid"] * (len(rows) - len(labels))
    ok, st = _verify(harness, rows, vartime=vartime)
    want = DC.oracle_ok(rows, vartime)
    for i, r in enumerate(rows):
        assert ok[i] == want[i], (i, labels[i])
        assert st[i] == PO.abi_status(*r[:5]), (i, labels[i])
    by = collections.defaultdict(list)
    for l, o in zip(labels, ok):
        by[l].append(bool(o))
    assert all(by["valid"]) and all(by["edge-valid"]) and all(by["vG-plus-p"]) and all(by["vH-plus-p"]) and all(by["vG-minus-zero"])
    assert all(by["both-minus-zero-noncanonical"])
    assert not any(by["vG-plus-p-wrong"]) and not any(by["vH-wrong-x0-point"])
    assert not any(o for l, v in by.items() if l.startswith(("tampered", "undecodable")) for o in v)


def test_lane_program_challenge_checks_strides_and_precedence(harness):
    rows, labels = DC.cases(seed=4, fs=True)
    ok, st = _verify(harness, rows, fs=True)
    want = DC.oracle_ok(rows)
    for i, r in enumerate(rows):
        s = PO.abi_status(*r[:5], fs_with=r[6:8])
        assert st[i] == s and ok[i] == (want[i] and s == 0), (i, labels[i])
    assert all(o for o, l in zip(ok, labels) if l == "valid")
    # a tampered xG, xH, VG or VH moves the derived challenge: the status says so before any equation
    assert {int(st[i]) for i, l in enumerate(labels) if l.split("-")[-1] in ("xG", "xH", "VG", "VH") and l.startswith("tampered")} == {7}
    assert {int(st[i]) for i, l in enumerate(labels) if l in ("C-plus-l", "tampered-C")} == {7}  # raw bytes, not residues
    # precedence: a wrong challenge AND an undecodable G report the challenge
    both = [list(rows[0])]
    both[0][0], both[0][4] = V._not_on_curve(), bytes(32)
    assert _verify(harness, both, fs=True)[1][0] == 7 and _verify(harness, both)[1][0] == 1
    # expect_c: right and wrong
    rng = random.Random(8)
    rows2 = [DC.valid_proof(rng) for _ in range(4)]
    for r in rows2:
        r[:] = DC.commitments_from_equations(r[:4] + [rows2[0][4]] + r[5:], False)
    ok, st = _verify(harness, rows2, expect=rows2[0][4])
    assert ok.all() and not st.any()
    ok, st = _verify(harness, rows2, expect=bytes(31) + b"\x01")
    assert not ok.any() and set(st) == {7}
    # stride 0 against the same base replicated
    for r in rows2:
        r[:] = DC.commitments_from_equations([rows2[0][0], rows2[1][1]] + r[2:], False)
    rows2[3][6] = rows2[2][6]
    a = _verify(harness, rows2)
    b = _verify(harness, rows2, gs=0, hs=0)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and list(a[0]) == [True, True, True, False]


def test_oracle_round_at_10_7_and_the_tamperings_of_pvss_test():
    n, t = 10, 7
    rand = X.New(b"pvss oracle").Read
    H = O.encode(O.mul_int(0xC0FFEE, O.B))
    xs = [X.pick(rand) for _ in range(n)]
    Xs = [O.mul_base(x) for x in xs]
    secret = X.pick(rand)
    shares, commits, coeffs = PO.enc_shares(H, Xs, secret, t, rand)
    sH = PO.compute_commitments(n, commits)
    assert sH == PO.compute_commitments(n, commits, coeffs, H)  # the Horner loop yields the points of PubPoly.Eval
    gc = PO.global_challenge(sH, shares)
    assert all(s[2][0] == gc for s in shares)
    assert all(PO.verify_enc_share(H, Xs[i], sH[i], gc, shares[i]) is None for i in range(n))
    decs = []
    for i in range(n):
        d, err = PO.dec_share(H, Xs[i], sH[i], xs[i], gc, shares[i], rand)
        assert err is None and PO.verify_dec_share(PO.BASE, Xs[i], shares[i], d) is None
        decs.append(d)
    want = O.mul_base(secret)
    assert PO.recover_secret(PO.BASE, Xs, shares, decs, t, n) == (want, None)
    # pvss_test.go:153-195: three decrypted shares nulled still recover, four do not
    null = O.encode(O.IDENTITY)
    bad = [(d[0], null, d[2]) if i < 3 else d for i, d in enumerate(decs)]
    assert [PO.verify_dec_share(PO.BASE, Xs[i], shares[i], bad[i]) for i in range(4)] == [PO.ErrDecVerification] * 3 + [None]
    assert PO.recover_secret(PO.BASE, Xs, shares, bad, t, n) == (want, None)
    bad[3] = (decs[3][0], null, decs[3][2])
    assert PO.recover_secret(PO.BASE, Xs, shares, bad, t, n) == (None, PO.ErrTooFewShares)
    # the other ways a share fails, each under its own error
    assert PO.verify_enc_share(H, Xs[0], sH[0], X.pick(rand), shares[0]) == PO.ErrGlobalChallengeVerification
    assert PO.verify_enc_share(H, Xs[0], sH[1], gc, shares[0]) == PO.ErrEncVerification
    assert PO.verify_enc_share(H, Xs[1], sH[0], gc, shares[0]) == PO.ErrEncVerification
    c, r, vg, vh = decs[0][2]
    assert PO.verify_dec_share(PO.BASE, Xs[0], shares[0], (0, decs[0][1], (PO.sc(PO.le(c) + 1), r, vg, vh))) == PO.ErrDecShareChallengeVerification
    assert PO.verify_dec_share(PO.BASE, Xs[0], shares[0], (0, decs[0][1], (c, PO.sc(PO.le(r) + 1), vg, vh))) == PO.ErrDecVerification
    assert PO.dec_share(H, Xs[0], sH[0], xs[0], bytes(32), shares[0], rand) == (None, PO.ErrGlobalChallengeVerification)


def test_abi_checks_arguments_without_a_device():
    from kyber_amd import _lib

    lib = _lib.load()
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    V_, FS, UNI = _lib.KYB_F_VARTIME, _lib.KYB_F_DLEQ_FS, _lib.KYB_F_UNIFORM
    assert lib.kyb_ed25519_dleq_challenge(0, p, p, p, p, p, p) == 0
    assert lib.kyb_ed25519_dleq_challenge_dev(0, p, p, p, p, p, p, None) == 0
    assert lib.kyb_ed25519_dleq_verify(0, p, 32, p, 0, p, p, p, p, p, p, None, p, p, V_ | FS) == 0
    assert lib.kyb_ed25519_dleq_verify_dev(0, p, 0, p, 32, p, p, p, p, p, p, p, p, None, 0, None) == 0
    ver = lambda **kw: tuple({**dict(n=4, G=p, gs=32, H=p, hs=32, xG=p, xH=p, C=p, R=p, VG=p, VH=p, e=None, ok=p, st=p, f=0), **kw}.values())
    bad = [("kyb_ed25519_dleq_challenge", (4, None, p, p, p, p, p)), ("kyb_ed25519_dleq_challenge", (4, p, p, p, p, None, p)),
           ("kyb_ed25519_dleq_challenge_dev", (4, p, p, None, p, p, p, None)),
           ("kyb_ed25519_dleq_verify", ver(f=UNI)), ("kyb_ed25519_dleq_verify", ver(f=32)), ("kyb_ed25519_dleq_verify", ver(f=2)),
           ("kyb_ed25519_dleq_verify", ver(gs=31)), ("kyb_ed25519_dleq_verify", ver(hs=64)), ("kyb_ed25519_dleq_verify", ver(gs=1)),
           ("kyb_ed25519_dleq_verify", ver(f=FS, e=p)), ("kyb_ed25519_dleq_verify", ver(n=0, f=FS, e=p)),
           ("kyb_ed25519_dleq_verify", ver(n=0, gs=8))]
    bad += [("kyb_ed25519_dleq_verify", ver(**{k: None})) for k in ("G", "H", "xG", "xH", "C", "R", "VG", "VH", "ok")]
    bad += [("kyb_ed25519_dleq_verify_dev", ver(f=UNI | V_) + (None,)), ("kyb_ed25519_dleq_verify_dev", ver(hs=33) + (None,)),
            ("kyb_ed25519_dleq_verify_dev", ver(VG=None) + (None,)), ("kyb_ed25519_dleq_verify_dev", ver(f=FS | V_, e=p) + (None,))]
    for name, args in bad:
        assert getattr(lib, name)(*args) == -1, (name, args)
        assert name.encode() in lib.kyb_last_error()


def test_header_cites_the_reference_and_names_the_new_codes():
    src = open(os.path.join(ROOT, "include", "kyber_hip.h")).read()
    for cite in ("dleq.go:57-79", "pvss.go:154-157", "pvss.go:250-270", "blake.go:19-41", "rand.go:19-46", "scalar.go:180-184",
                 "KYB_ST_DLEQ_CHALLENGE 7", "KYB_ST_PICK_EXHAUSTED 8", "KYB_F_DLEQ_FS 16u"):
        assert cite in src, cite
