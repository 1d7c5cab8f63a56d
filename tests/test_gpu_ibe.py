"""encrypt/ibe (ibe.go:51-232) on the engine: kyb_bls12381_ibe_encrypt/decrypt_g1/g2 bit-exact against the oracle
(tests/_ibe_oracle.py, tests/_oracle_c.py), rejections with their statuses, batch shapes, the device-pointer entry
points and the Python caller layer (kyber_amd/encrypt/ibe.py)."""
import hashlib
import random

import numpy as np
import pytest

from oracle import bls12381 as O
from tests import _ibe_oracle as IBE

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 16, 31, 32)
IDENT = b"tlock round 4242"
SECRET = 0x7E57C0DE1234 % O.R


@pytest.fixture(scope="module")
def bls():
    import torch

    assert torch.cuda.is_available()
    from kyber_amd.pairing import bls12381 as bls

    return bls


@pytest.fixture(scope="module")
def keys():
    return {g2: IBE.keys(g2, SECRET, IDENT) for g2 in (False, True)}


@pytest.fixture(scope="module")
def gids(keys):
    return {g2: IBE.gid(g2, keys[g2][0], IDENT) for g2 in (False, True)}


def _rb(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def _arr(items, width):
    return np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), width) if items else np.zeros((0, width), np.uint8)


def _enc(bls, on_g2):
    return bls.batch_ibe_encrypt_g2 if on_g2 else bls.batch_ibe_encrypt_g1


def _dec(bls, on_g2):
    return bls.batch_ibe_decrypt_g2 if on_g2 else bls.batch_ibe_decrypt_g1


@pytest.mark.parametrize("on_g2", [False, True])
def test_decrypt_matches_the_oracle(bls, keys, gids, on_g2):
    master, private = keys[on_g2]
    rng = random.Random(11 + on_g2)
    for ln in LENGTHS:
        msgs = [_rb(rng, ln) for _ in range(3)]
        cts = [IBE.encrypt(on_g2, master, IDENT, m, _rb(rng, ln), g=gids[on_g2]) for m in msgs]
        U, V, W = [c[0] for c in cts], _arr([c[1] for c in cts], ln), _arr([c[2] for c in cts], ln)
        for priv in (private, [private] * len(cts)):  # one shared key (private_stride 0), then one key per element
            out, st = _dec(bls, on_g2)(priv, U, V, W)
            assert not st.any(), (ln, st)
            assert [bytes(x) for x in out] == msgs


@pytest.mark.parametrize("on_g2", [False, True])
def test_encrypt_matches_the_oracle_byte_for_byte(bls, keys, gids, on_g2):
    master, _ = keys[on_g2]
    rng = random.Random(21 + on_g2)
    n = 32
    for ln in (0, 16, 32) if not on_g2 else (1, 31):
        msgs, sigmas = [_rb(rng, ln) for _ in range(n)], [_rb(rng, ln) for _ in range(n)]
        U, V, W, st = _enc(bls, on_g2)(master, IDENT, _arr(msgs, ln), sigmas=_arr(sigmas, ln))
        assert not st.any()
        for i in range(0, n, 4 if ln else 8):
            want = IBE.encrypt(on_g2, master, IDENT, msgs[i], sigmas[i], g=gids[on_g2])
            assert (bytes(U[i]), bytes(V[i]), bytes(W[i])) == want, (ln, i)


def _oracle_c_decrypt(on_g2, private, U, V, W):
    """DecryptCCA of every ciphertext by the C oracle (pairing, G1 / G2 multiplication) + hashlib"""
    from tests import _oracle_c as OC

    n = len(U)
    privs = np.frombuffer(private * n, dtype=np.uint8).reshape(n, -1)
    gt, st = OC.bls12381_pair_compressed(privs, U) if on_g2 else OC.bls12381_pair_compressed(U, privs)
    assert not st.any()
    msgs, rs = [], []
    for i in range(n):
        sigma, msg = IBE._ibe_decrypt(bytes(gt[i]), bytes(V[i]), bytes(W[i]), IBE.TAGS)
        msgs.append(msg)
        rs.append(IBE.h3(sigma, msg).to_bytes(32, "big"))
    base = O.g2_compress(O.G2_GEN) if on_g2 else O.g1_compress(O.G1_GEN)
    rp, st = (OC.bls12381_g2_mul if on_g2 else OC.bls12381_g1_mul)(_arr(rs, 32), np.frombuffer(base * n, dtype=np.uint8))
    assert not st.any()
    return msgs, rp


@pytest.mark.parametrize("on_g2", [False, True])
def test_encrypt_at_scale_decrypts_on_the_c_oracle_and_the_engine(bls, keys, on_g2):
    master, private = keys[on_g2]
    n, ln = 1 << 14, 32
    raw = hashlib.shake_256(b"ibe scale %d" % on_g2).digest(2 * n * ln)
    msgs, sigmas = np.frombuffer(raw[:n * ln], dtype=np.uint8).reshape(n, ln), np.frombuffer(raw[n * ln:], dtype=np.uint8).reshape(n, ln)
    U, V, W, st = _enc(bls, on_g2)(master, IDENT, msgs, sigmas=sigmas)
    assert not st.any()
    want, rp = _oracle_c_decrypt(on_g2, private, U, V, W)
    assert [bytes(m) for m in msgs] == want
    assert np.array_equal(rp, U)  # the CCA check passes on the oracle
    out, st = _dec(bls, on_g2)(private, U, V, W)
    assert not st.any() and np.array_equal(out, msgs)


def _off_subgroup(g2):
    """a point of the curve (G2: of the twist) outside the order-r subgroup"""
    k = 1
    while True:
        if g2:
            x = (k, 1)
            y = O.f2_sqrt(O.f2_add(O.f2_mul(O.f2_sqr(x), x), O._Fp2.b))
            if y is not None and not O.g2_in_subgroup((x, y)):
                return (x, y)
        else:
            y = O.fp_sqrt((k ** 3 + 4) % O.P)
            if y is not None and not O.g1_in_subgroup((k, y)):
                return (k, y)
        k += 1


@pytest.mark.parametrize("on_g2", [False, True])
def test_rejections_give_their_status_and_zero_bytes(bls, keys, gids, on_g2):
    master, private = keys[on_g2]
    rng = random.Random(31 + on_g2)
    ln = 16
    msg, sigma = _rb(rng, ln), _rb(rng, ln)
    U, V, W = IBE.encrypt(on_g2, master, IDENT, msg, sigma, g=gids[on_g2])
    u_plus_base = O.g2_compress(O.g2_add(O.g2_decompress(U), O.G2_GEN)) if on_g2 else O.g1_compress(O.g1_add(O.g1_decompress(U), O.G1_GEN))
    usz = len(U)
    inf = bytes([0xC0]) + bytes(usz - 1)
    bad_u = bytes([0x80 | 0x1F]) + b"\xff" * (usz - 1)  # x >= p: not a point
    off_u = O.g2_compress(_off_subgroup(True)) if on_g2 else O.g1_compress(_off_subgroup(False))
    cases = [
        (U, V, bytes([W[0] ^ 1]) + W[1:], 3),
        (U, bytes([V[0] ^ 0x80]) + V[1:], W, 3),
        (u_plus_base, V, W, 3),
        (inf, V, W, 3),
        (bad_u, V, W, 1),
        (off_u, V, W, 2),
        (U, V, W, 0),
    ]
    out, st = _dec(bls, on_g2)(private, [c[0] for c in cases], _arr([c[1] for c in cases], ln), _arr([c[2] for c in cases], ln))
    assert list(st) == [c[3] for c in cases]
    assert not out[:-1].any() and bytes(out[-1]) == msg
    # the decode verdicts agree with UnmarshalBinary on the engine
    _, ust = (bls.g2_batch_unmarshal if on_g2 else bls.g1_batch_unmarshal)(bad_u + off_u)
    assert list(ust) == [1, 2]
    # a private key that does not decode fails every element with its own status, ahead of U's
    bad_key = bytes([0x9F]) + b"\xff" * (len(private) - 1)
    out, st = _dec(bls, on_g2)(bad_key, [c[0] for c in cases], _arr([c[1] for c in cases], ln), _arr([c[2] for c in cases], ln))
    assert list(st) == [1] * len(cases) and not out.any()
    # a master key that does not decode: every element gets its status and zero bytes
    U2, V2, W2, st = _enc(bls, on_g2)(bytes([0x9F]) + b"\xff" * (len(master) - 1), IDENT, _arr([msg] * 3, ln), sigmas=_arr([sigma] * 3, ln))
    assert list(st) == [1] * 3 and not U2.any() and not V2.any() and not W2.any()
    # a master key at infinity encrypts as the oracle does, with Gid = 1
    minf = bytes([0xC0]) + bytes(len(master) - 1)
    U3, V3, W3, st = _enc(bls, on_g2)(minf, IDENT, _arr([msg], ln), sigmas=_arr([sigma], ln))
    assert not st.any()
    assert (bytes(U3[0]), bytes(V3[0]), bytes(W3[0])) == IBE.encrypt(on_g2, minf, IDENT, msg, sigma, g=O.F12_ONE)


def test_golden_vector_fails_the_rp_check_on_the_engine(bls, golden_dir):
    import json
    import os

    v = json.load(open(os.path.join(golden_dir, "bls12381_ibe.json")))
    out, st = bls.batch_ibe_decrypt_g1(bytes.fromhex(v["beacon_g2"]), [bytes.fromhex(v["U_g1"])], _arr([bytes.fromhex(v["V"])], 16),
                                       _arr([bytes.fromhex(v["W"])], 16))
    assert list(st) == [3] and not out.any()


@pytest.mark.parametrize("n", [1, 63, 65, 4097])
def test_shapes_and_mixed_batches(bls, keys, n):
    on_g2 = n % 2 == 1 and n > 1
    master, private = keys[on_g2]
    ln = 24
    raw = hashlib.shake_256(b"shape %d" % n).digest(2 * n * ln)
    msgs, sigmas = np.frombuffer(raw[:n * ln], dtype=np.uint8).reshape(n, ln), np.frombuffer(raw[n * ln:], dtype=np.uint8).reshape(n, ln)
    U, V, W, st = _enc(bls, on_g2)(master, IDENT, msgs, sigmas=sigmas)
    assert not st.any()
    W = W.copy()
    bad = list(range(0, n, 7))
    W[bad, 0] ^= 1
    out, st = _dec(bls, on_g2)(private, U, V, W)
    good = np.ones(n, dtype=bool)
    good[bad] = False
    assert (st[good] == 0).all() and (st[~good] == 3).all()
    assert np.array_equal(out[good], msgs[good]) and not out[~good].any()


def test_sharded_host_call_and_dev_entry_points_agree(bls, keys):
    import torch

    from kyber_amd import devices

    n, ln = 4096, 32
    for on_g2 in (False, True):
        master, private = keys[on_g2]
        raw = hashlib.shake_256(b"dev %d" % on_g2).digest(2 * n * ln)
        msgs, sigmas = np.frombuffer(raw[:n * ln], dtype=np.uint8).reshape(n, ln), np.frombuffer(raw[n * ln:], dtype=np.uint8).reshape(n, ln)
        ref = _enc(bls, on_g2)(master, IDENT, msgs, sigmas=sigmas)
        d = _enc(bls, on_g2)(torch.from_numpy(np.frombuffer(master, dtype=np.uint8).copy()).cuda(), IDENT, torch.from_numpy(msgs.copy()).cuda(),
                             sigmas=torch.from_numpy(sigmas.copy()).cuda())
        torch.cuda.synchronize()
        for a, b in zip(ref, d):
            assert np.array_equal(a, b.cpu().numpy())
        out_d, st_d = _dec(bls, on_g2)(torch.from_numpy(np.frombuffer(private, dtype=np.uint8).copy()).cuda(),
                                      *(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in ref[:3]))
        torch.cuda.synchronize()
        assert not st_d.cpu().numpy().any() and np.array_equal(out_d.cpu().numpy(), msgs)
        # one GPU listed twice: the host calls shard, every shard recomputes Gid; the bytes are the same
        devices.set_devices([0, 0])
        devices.set_shard_threshold(1024)
        try:
            two = _enc(bls, on_g2)(master, IDENT, msgs, sigmas=sigmas)
            out2, st2 = _dec(bls, on_g2)(private, *ref[:3])
        finally:
            devices.set_devices([])
            devices.set_shard_threshold(16384)
        for a, b in zip(ref, two):
            assert np.array_equal(a, b)
        assert not st2.any() and np.array_equal(out2, msgs)


def test_python_caller_layer(bls, keys):
    from kyber_amd.encrypt import ibe

    rng = random.Random(51)
    for on_g2 in (False, True):
        master, private = keys[on_g2]
        enc = ibe.encrypt_cca_on_g2 if on_g2 else ibe.encrypt_cca_on_g1
        dec = ibe.decrypt_cca_on_g2 if on_g2 else ibe.decrypt_cca_on_g1
        c = enc(master, IDENT, b"hello tlock")
        assert dec(private, c) == b"hello tlock"
        with pytest.raises(ValueError, match="rP check"):
            dec(private, ibe.Ciphertext(c.U, c.V, bytes([c.W[0] ^ 1]) + c.W[1:]))
        with pytest.raises(ValueError):
            enc(master, IDENT, bytes(33))
        msgs = [_rb(rng, ln) for ln in (5, 0, 32, 5, 17, 32)]
        cts = (ibe.batch_encrypt_cca_on_g2 if on_g2 else ibe.batch_encrypt_cca_on_g1)(master, IDENT, msgs)
        cts.append(ibe.Ciphertext(cts[0].U, cts[0].V + b"x", cts[0].W))  # len(V) != len(W): never reaches the device
        got, st = (ibe.batch_decrypt_cca_on_g2 if on_g2 else ibe.batch_decrypt_cca_on_g1)(private, cts)
        assert got[:-1] == msgs and got[-1] is None
        assert list(st) == [0] * len(msgs) + [ibe.ST_MALFORMED]
