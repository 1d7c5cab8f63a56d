"""The rest of encrypt/ibe's C ABI contract (include/kyber_hip.h, kyb_bls12381_ibe_*), each case against the oracles
(tests/_ibe_oracle.py, tests/_oracle_c.py), never against the engine itself:

- batches that cross bls12381_ibe.hip's piece of 2^16 elements, on encrypt and on decrypt with one key per element
  (private_stride = the key's size), with rejections planted on both sides of the boundary;
- the flags: KYB_F_UNCOMPRESSED (master key, or private keys and U), KYB_F_UNCOMPRESSED_OUT (U out), KYB_F_TRUSTED(0/1);
- identities at the block edges of expand_message_xmd and DSTs of 1 to 255 bytes (256 is an argument error);
- drand's own keys and DSTs (tests/golden/bls12381_drand.json);
- the per-stream fixed-base table and its hint, shared with g1/g2_commit;
- a host call sharded over one GPU listed twice, each shard crossing a piece."""
import hashlib
import json
import os
import random
import time

import numpy as np
import pytest

from oracle import bls12381 as O
from tests import _ibe_oracle as IBE
from tests import _oracle_c as OC
from tests.test_gpu_ibe import _arr, _dec, _enc, _off_subgroup

pytestmark = pytest.mark.gpu

PIECE = 1 << 16  # bls12381_ibe.hip ibe::PIECE
N = PIECE + 37
IDENT = b"tlock contract round 77"
SECRET = 0x1BEC0DE5EED % O.R
F_UNC, F_UNC_OUT = 2, 4  # KYB_F_UNCOMPRESSED, KYB_F_UNCOMPRESSED_OUT


def F_TRUSTED(i):
    return 0x100 << i


def _ser(g2, pt):
    return O.g2_serialize_unc(pt) if g2 else O.g1_serialize_unc(pt)


def _cmp(g2, pt):
    return O.g2_compress(pt) if g2 else O.g1_compress(pt)


def _dcmp(g2, b):
    return O.g2_decompress(b) if g2 else O.g1_decompress(b)


def _unc(g2, b):
    """the uncompressed encoding of a compressed point"""
    return _ser(g2, _dcmp(g2, b))


def _seeded(seed: bytes, n: int, ln: int):
    raw = hashlib.shake_256(seed).digest(2 * n * ln) if ln else b""
    a = np.frombuffer(raw, dtype=np.uint8).reshape(2, n, ln) if ln else np.zeros((2, n, 0), np.uint8)
    return a[0].copy(), a[1].copy()


def _ident(rnd: int) -> bytes:
    return hashlib.sha256(rnd.to_bytes(8, "big")).digest()


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


@pytest.fixture(scope="module")
def big(bls, keys):
    """one engine encrypt of N > PIECE seeded elements per orientation (msg_len 32 on G1, 17 on G2), made once"""
    cache = {}

    def get(on_g2):
        if on_g2 not in cache:
            ln = 17 if on_g2 else 32
            msgs, sigmas = _seeded(b"ibe contract big %d" % on_g2, N, ln)
            U, V, W, st = _enc(bls, on_g2)(keys[on_g2][0], IDENT, msgs, sigmas=sigmas)
            assert not st.any()
            cache[on_g2] = (msgs, sigmas, U, V, W)
        return cache[on_g2]

    return get


def _oracle_c_open(on_g2, private, U, V, W, idx):
    """DecryptCCA of the elements idx by the C oracle (pairing, r * Base) + hashlib: (messages, r * Base == U)"""
    n, th = len(idx), OC.host_threads()
    U, V, W = U[idx], V[idx], W[idx]
    privs = np.frombuffer(private * n, dtype=np.uint8).reshape(n, -1)
    gt, st = OC.bls12381_pair_compressed(privs, U, th) if on_g2 else OC.bls12381_pair_compressed(U, privs, th)
    assert not st.any()
    msgs, rs = [], []
    for i in range(n):
        sigma, msg = IBE._ibe_decrypt(bytes(gt[i]), bytes(V[i]), bytes(W[i]), IBE.TAGS)
        msgs.append(msg)
        rs.append(IBE.h3(sigma, msg).to_bytes(32, "big"))
    base = O.g2_compress(O.G2_GEN) if on_g2 else O.g1_compress(O.G1_GEN)
    rp, st = (OC.bls12381_g2_mul if on_g2 else OC.bls12381_g1_mul)(_arr(rs, 32), np.frombuffer(base * n, dtype=np.uint8), th)
    assert not st.any()
    return msgs, np.array_equal(rp, U)


# ---- 1. encrypt across the piece boundary

@pytest.mark.parametrize("on_g2", [False, True])
def test_encrypt_across_the_piece_boundary(bls, keys, gids, big, on_g2):
    master, private = keys[on_g2]
    msgs, sigmas, U, V, W = big(on_g2)
    rng = random.Random(101 + on_g2)
    windows = list(range(32)) + list(range(PIECE - 48, min(PIECE + 48, N))) + list(range(N - 32, N))
    for i in windows + rng.sample(range(N), 64):
        want = IBE.encrypt(on_g2, master, IDENT, bytes(msgs[i]), bytes(sigmas[i]), g=gids[on_g2])
        assert (bytes(U[i]), bytes(V[i]), bytes(W[i])) == want, i
    out, st = _dec(bls, on_g2)(private, U, V, W)  # one shared key (private_stride 0) over both pieces
    assert not st.any() and np.array_equal(out, msgs)
    t0 = time.perf_counter()
    got, rp_ok = _oracle_c_open(on_g2, private, U, V, W, np.arange(N))
    print(f"C oracle DecryptCCA of {N} elements: {time.perf_counter() - t0:.1f} s")
    assert rp_ok and got == [bytes(m) for m in msgs]


# ---- 2. decrypt across pieces with one key per element

K = 5


def _triples(on_g2):
    """K (master, identity, private) triples with distinct secrets, identity k = sha256(BE64(round_k))"""
    out = []
    for k in range(K):
        ident = _ident(1000 + 17 * k)
        master, private = IBE.keys(on_g2, (SECRET * (k + 3) + 11) % O.R, ident)
        out.append((master, ident, private))
    return out


@pytest.mark.parametrize("on_g2", [False, True])
def test_decrypt_across_pieces_with_one_key_per_element(bls, on_g2):
    ln = 29
    tr = _triples(on_g2)
    j = np.arange(N)
    t = (j + j // K) % K  # the key changes from every element to the next
    assert (t[1:] != t[:-1]).all()
    msgs, sigmas = _seeded(b"ibe contract per key %d" % on_g2, N, ln)
    usz = 96 if on_g2 else 48
    U, V, W = np.zeros((N, usz), np.uint8), np.zeros((N, ln), np.uint8), np.zeros((N, ln), np.uint8)
    for k, (master, ident, private) in enumerate(tr):
        rows = np.nonzero(t == k)[0]
        u, v, w, st = _enc(bls, on_g2)(master, ident, msgs[rows], sigmas=sigmas[rows])  # one encrypt call per triple
        assert not st.any()
        U[rows], V[rows], W[rows] = u, v, w
        g = IBE.gid(on_g2, master, ident)
        for i in (rows[0], rows[len(rows) // 2], rows[-1]):
            assert (bytes(U[i]), bytes(V[i]), bytes(W[i])) == IBE.encrypt(on_g2, master, ident, bytes(msgs[i]), bytes(sigmas[i]), g=g), (k, i)
    privs = np.stack([np.frombuffer(p, dtype=np.uint8) for _, _, p in tr])[t]
    want_st = np.zeros(N, np.uint8)
    for i in (PIECE - 1, PIECE, N - 1):
        W[i, 3] ^= 0x10
        want_st[i] = 3
    privs[PIECE + 1] = np.frombuffer(tr[(t[PIECE + 1] + 1) % K][2], dtype=np.uint8)  # a valid key of another identity
    want_st[PIECE + 1] = 3
    privs[PIECE - 2] = np.frombuffer(bytes([0x9F]) + b"\xff" * (privs.shape[1] - 1), dtype=np.uint8)  # x >= p: no point
    want_st[PIECE - 2] = 1
    privs[PIECE + 2] = np.frombuffer(_cmp(not on_g2, _off_subgroup(not on_g2)), dtype=np.uint8)  # G2 keys: the Miller-loop rule
    want_st[PIECE + 2] = 2
    out, st = _dec(bls, on_g2)(privs, U, V, W)
    assert np.array_equal(st, want_st), np.nonzero(st != want_st)[0][:16]
    good = want_st == 0
    assert np.array_equal(out[good], msgs[good]) and not out[~good].any()
    # the same batch under ONE key (private_stride 0): triple 0's elements open, every other one fails the rP check
    out, st = _dec(bls, on_g2)(tr[0][2], U, V, W)
    opens = t == 0
    opens[[PIECE - 1, PIECE, N - 1]] = False  # the flipped W bits
    assert np.array_equal(st, np.where(opens, 0, 3).astype(np.uint8))
    assert np.array_equal(out[opens], msgs[opens]) and not out[~opens].any()


# ---- 3. flags

FLAG_SETS = [0, F_UNC, F_UNC_OUT, F_TRUSTED(0), F_UNC | F_UNC_OUT, F_UNC | F_TRUSTED(0), F_UNC_OUT | F_TRUSTED(0),
             F_UNC | F_UNC_OUT | F_TRUSTED(0)]


@pytest.fixture(scope="module")
def small(keys, gids):
    """6 oracle ciphertexts per orientation, msg_len 20"""
    out = {}
    for on_g2 in (False, True):
        msgs, sigmas = _seeded(b"ibe contract flags %d" % on_g2, 6, 20)
        cts = [IBE.encrypt(on_g2, keys[on_g2][0], IDENT, bytes(m), bytes(s), g=gids[on_g2]) for m, s in zip(msgs, sigmas)]
        out[on_g2] = (msgs, sigmas, cts)
    return out


@pytest.mark.parametrize("on_g2", [False, True])
def test_encrypt_flags_byte_exact(bls, keys, small, on_g2):
    master, _ = keys[on_g2]
    msgs, sigmas, cts = small[on_g2]
    for fl in FLAG_SETS:
        mk = _unc(on_g2, master) if fl & F_UNC else master
        U, V, W, st = _enc(bls, on_g2)(mk, IDENT, msgs, sigmas=sigmas, flags=fl)
        assert not st.any(), fl
        for i, (u, v, w) in enumerate(cts):
            assert bytes(U[i]) == (_unc(on_g2, u) if fl & F_UNC_OUT else u), (fl, i)
            assert (bytes(V[i]), bytes(W[i])) == (v, w), (fl, i)


@pytest.mark.parametrize("on_g2", [False, True])
def test_decrypt_flags_byte_exact(bls, keys, small, on_g2):
    _, private = keys[on_g2]
    msgs, _, cts = small[on_g2]
    V, W = _arr([c[1] for c in cts], 20), _arr([c[2] for c in cts], 20)
    for fl in (0, F_UNC, F_TRUSTED(0), F_TRUSTED(1), F_TRUSTED(0) | F_TRUSTED(1), F_UNC | F_TRUSTED(0), F_UNC | F_TRUSTED(1)):
        key = _unc(not on_g2, private) if fl & F_UNC else private
        U = [_unc(on_g2, c[0]) if fl & F_UNC else c[0] for c in cts]
        for priv in (key, [key] * len(cts)):  # private_stride 0, then the key's size (96 / 192 B, 48 / 96 B)
            out, st = _dec(bls, on_g2)(priv, U, V, W, flags=fl)
            assert not st.any() and np.array_equal(out, msgs), (fl, isinstance(priv, list))


@pytest.mark.parametrize("on_g2", [False, True])
def test_uncompressed_rejections(bls, keys, small, on_g2):
    _, private = keys[on_g2]
    msgs, _, cts = small[on_g2]
    key = _unc(not on_g2, private)
    u_ok = [_unc(on_g2, c[0]) for c in cts]
    not_on_curve = u_ok[1][:-1] + bytes([u_ok[1][-1] ^ 1])  # y + or - 1
    with pytest.raises(ValueError):
        (O.g2_deserialize_unc if on_g2 else O.g1_deserialize_unc)(not_on_curve)
    inf = bytes([0x40]) + bytes(len(u_ok[0]) - 1)  # the uncompressed encoding of infinity
    assert inf == _ser(on_g2, None)
    U = [u_ok[0], not_on_curve, _ser(on_g2, _off_subgroup(on_g2)), inf, u_ok[4], u_ok[5]]
    off_key = _ser(not on_g2, _off_subgroup(not on_g2))
    privs = [key, key, key, key, off_key, key]
    V, W = _arr([c[1] for c in cts], 20), _arr([c[2] for c in cts], 20)
    out, st = _dec(bls, on_g2)(privs, U, V, W, flags=F_UNC)
    assert list(st) == [0, 1, 2, 3, 2, 0]
    assert np.array_equal(out[[0, 5]], msgs[[0, 5]]) and not out[1:5].any()
    # vouched-for garbage has no contract: only the elements whose vouched-for operands are valid are asserted
    out, st = _dec(bls, on_g2)(privs, U, V, W, flags=F_UNC | F_TRUSTED(1))
    assert list(st[[0, 4, 5]]) == [0, 2, 0] and np.array_equal(out[[0, 5]], msgs[[0, 5]])
    out, st = _dec(bls, on_g2)(privs, U, V, W, flags=F_UNC | F_TRUSTED(0))
    assert list(st[[0, 1, 2, 3, 5]]) == [0, 1, 2, 3, 0] and np.array_equal(out[[0, 5]], msgs[[0, 5]])


@pytest.mark.parametrize("on_g2", [False, True])
def test_master_key_off_the_subgroup_fails_every_element(bls, small, on_g2):
    msgs, sigmas, _ = small[on_g2]
    off = _off_subgroup(on_g2)
    for mk, fl in ((_cmp(on_g2, off), 0), (_ser(on_g2, off), F_UNC), (_cmp(on_g2, off), F_UNC_OUT)):
        U, V, W, st = _enc(bls, on_g2)(mk, IDENT, msgs, sigmas=sigmas, flags=fl)
        assert list(st) == [2] * len(msgs), fl
        assert not U.any() and not V.any() and not W.any(), fl


# ---- 4. identities and DSTs

@pytest.mark.parametrize("on_g2", [False, True])
def test_identity_lengths_at_the_hash_block_edges(bls, keys, on_g2):
    master, _ = keys[on_g2]
    msgs, sigmas = _seeded(b"ibe contract ids %d" % on_g2, 2, 11)
    for ln in (0, 1, 8, 32, 55, 56, 64, 65, 119, 120, 1000):
        ident = hashlib.shake_256(b"id %d" % ln).digest(ln) if ln else b""
        U, V, W, st = _enc(bls, on_g2)(master, ident, msgs, sigmas=sigmas)
        assert not st.any()
        g = IBE.gid(on_g2, master, ident)
        for i in range(2):
            assert (bytes(U[i]), bytes(V[i]), bytes(W[i])) == IBE.encrypt(on_g2, master, ident, bytes(msgs[i]), bytes(sigmas[i]), g=g), (ln, i)


@pytest.mark.parametrize("on_g2", [False, True])
def test_dst_lengths(bls, on_g2):
    msgs, sigmas = _seeded(b"ibe contract dst %d" % on_g2, 3, 32)
    for dl in (1, 43, 200, 255):
        dst = hashlib.shake_256(b"dst %d %d" % (on_g2, dl)).digest(dl)
        master, private = IBE.keys(on_g2, (SECRET + dl) % O.R, IDENT, dst=dst)
        U, V, W, st = _enc(bls, on_g2)(master, IDENT, msgs, sigmas=sigmas, dst=dst)
        assert not st.any()
        g = IBE.gid(on_g2, master, IDENT, dst=dst)
        for i in range(3):
            assert (bytes(U[i]), bytes(V[i]), bytes(W[i])) == IBE.encrypt(on_g2, master, IDENT, bytes(msgs[i]), bytes(sigmas[i]), g=g), (dl, i)
        out, st = _dec(bls, on_g2)(private, U, V, W)
        assert not st.any() and np.array_equal(out, msgs), dl
    with pytest.raises(ValueError):
        _enc(bls, on_g2)(master, IDENT, msgs, sigmas=sigmas, dst=bytes(256))


# ---- 5. drand's keys

def test_drand_keys_open_their_rounds(bls, golden_dir):
    v = json.load(open(os.path.join(golden_dir, "bls12381_drand.json")))
    msgs, sigmas = _seeded(b"ibe contract drand", 4, 32)
    a = v["sig_on_g1"]  # keys on G2, signatures on G1 under the G2 DST (drand's bls-unchained-on-g1)
    pk, sig, ident = bytes.fromhex(a["pk_g2"]), bytes.fromhex(a["sig_g1"]), _ident(a["round"])
    dst = v["dst_g2"].encode()
    U, V, W, st = bls.batch_ibe_encrypt_g2(pk, ident, msgs, sigmas=sigmas, dst=dst)
    assert not st.any()
    assert (bytes(U[0]), bytes(V[0]), bytes(W[0])) == IBE.encrypt(True, pk, ident, bytes(msgs[0]), bytes(sigmas[0]), dst=dst)
    out, st = bls.batch_ibe_decrypt_g2(sig, U, V, W)
    assert not st.any() and np.array_equal(out, msgs)
    U, V, W, st = bls.batch_ibe_encrypt_g2(pk, ident, msgs, sigmas=sigmas)  # the default (G1) DST: another identity point
    assert not st.any()
    out, st = bls.batch_ibe_decrypt_g2(sig, U, V, W)
    assert list(st) == [3] * 4 and not out.any()
    b = v["sig_on_g2"]  # keys on G1, chained signatures on G2
    pk, sig = bytes.fromhex(b["pk_g1"]), bytes.fromhex(b["sig_g2"])
    ident = hashlib.sha256(bytes.fromhex(b["prev_sig"]) + b["round"].to_bytes(8, "big")).digest()
    U, V, W, st = bls.batch_ibe_encrypt_g1(pk, ident, msgs, sigmas=sigmas)
    assert not st.any()
    assert (bytes(U[1]), bytes(V[1]), bytes(W[1])) == IBE.encrypt(False, pk, ident, bytes(msgs[1]), bytes(sigmas[1]))
    out, st = bls.batch_ibe_decrypt_g1(sig, U, V, W)
    assert not st.any() and np.array_equal(out, msgs)


# ---- 6. the fixed-base table and its hint, shared with g1/g2_commit

@pytest.mark.parametrize("group", [1, 2])
def test_commit_ibe_commit_on_one_stream(bls, keys, gids, group):
    """host calls of one thread run on the same pool stream: a large commit of B leaves B's table and the hint that it is
    there (small commits of B take the table), IBE replaces the table with the generator's and must drop the hint"""
    on_g2 = group == 2
    mul = O.g2_mul if on_g2 else O.g1_mul
    commit = bls.g2_commit if on_g2 else bls.g1_commit
    rng = random.Random(61 + group)
    gen = O.G2_GEN if on_g2 else O.G1_GEN
    bp, cp = mul(rng.randrange(1, O.R), gen), mul(rng.randrange(1, O.R), gen)
    B, C = _cmp(on_g2, bp), _cmp(on_g2, cp)

    def check_commit(ks, base, base_pt, idx):
        out, st = commit(np.frombuffer(b"".join(k.to_bytes(32, "big") for k in ks), dtype=np.uint8).reshape(-1, 32), base)
        assert not np.asarray(st).any()
        out = np.asarray(out)
        for i in idx:
            assert bytes(out[i]) == _cmp(on_g2, mul(ks[i], base_pt)), (base == B, i)

    big_ks = [rng.randrange(O.R) for _ in range(1 << 17)]  # from 2^17 scalars a table of an unknown base is built
    check_commit(big_ks, B, bp, (0, 1, (1 << 17) - 1))
    small_ks = [rng.randrange(O.R) for _ in range(96)]  # >= 64: the table path when the hint names B
    check_commit(small_ks, B, bp, range(0, 96, 19))
    master, private = keys[on_g2]
    msgs, sigmas = _seeded(b"ibe contract table %d" % group, 80, 16)
    U, V, W, st = _enc(bls, on_g2)(master, IDENT, msgs, sigmas=sigmas)
    assert not st.any()
    for i in (0, 79):
        assert (bytes(U[i]), bytes(V[i]), bytes(W[i])) == IBE.encrypt(on_g2, master, IDENT, bytes(msgs[i]), bytes(sigmas[i]), g=gids[on_g2])
    out, st = _dec(bls, on_g2)(private, U, V, W)
    assert not st.any() and np.array_equal(out, msgs)
    check_commit(small_ks, B, bp, range(0, 96, 19))
    check_commit(small_ks[::-1], C, cp, range(3, 96, 23))


# ---- 8. sharding

@pytest.mark.parametrize("on_g2", [False, True])
def test_sharded_calls_cross_pieces_and_match_one_device(bls, keys, big, on_g2):
    """one GPU listed twice: a batch of 2 N splits into two shards of N > PIECE elements; the first is item 1's batch, the
    second a fixed permutation of it, so every byte is that of the single-device call"""
    from kyber_amd import devices

    master, private = keys[on_g2]
    msgs, sigmas, U, V, W = big(on_g2)
    perm = np.random.default_rng(8 + on_g2).permutation(N)
    assert devices.shard_range(2 * N, 0, 2) == (0, N)
    devices.set_devices([0, 0])
    devices.set_shard_threshold(1024)
    try:
        two = _enc(bls, on_g2)(master, IDENT, np.concatenate([msgs, msgs[perm]]), sigmas=np.concatenate([sigmas, sigmas[perm]]))
        out, st = _dec(bls, on_g2)(private, *(np.concatenate([x, x[perm]]) for x in (U, V, W)))
    finally:
        devices.set_devices([])
        devices.set_shard_threshold(16384)
    for a, b in zip(two[:3], (U, V, W)):
        assert np.array_equal(a, np.concatenate([b, b[perm]]))
    assert not two[3].any()
    assert not st.any() and np.array_equal(out, np.concatenate([msgs, msgs[perm]]))
