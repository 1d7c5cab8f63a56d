"""Device hash-to-curve at every padding boundary, DST length and launch path, against the oracles.

One implementation of expand_message_xmd is reached through many launches (the per-lane hash kernels, the two-wave
kernels of large batches, the operand lanes of the fused verifications, the host-buffer twins of all of them), and the
hashes under it (sha256.cuh, keccak256.cuh, sha512.cuh) index their block with a run-time position.  A mistake there
shows only at particular lengths, and a fused verification that hashes wrongly just answers ok = 0.  tests/_hash_cases.py
holds (msg_len, dst_len) tables that put the finish of both hashes of the construction on every position around the
padding switch and the block end, with empty, one-byte, small, one-block and multi-block messages
(tests/test_hash_cases.py checks that claim); this file runs them through every entry point that hashes.

The oracles (oracle/*.py: hashlib + big integers) run in worker processes that never open the GPU."""
import ctypes
import hashlib
import os
import re
import time

import numpy as np
import pytest

from tests import _hash_cases as HC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 67  # one full wave plus a ragged one
KYB_E_ARG = -1
ORACLE_SECONDS = [0.0]


@pytest.fixture(scope="module")
def torch_():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def pool():
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor

    workers = max(1, min(12, int(os.environ.get("OMP_NUM_THREADS") or 0) or (os.cpu_count() or 2)))
    with ProcessPoolExecutor(max_workers=workers, mp_context=mp.get_context("spawn")) as ex:
        yield ex
    print(f"\n[hash lengths] oracle wall time {ORACLE_SECONDS[0]:.1f} s on {workers} workers")


def _map(pool, fn, jobs):
    t0 = time.time()
    jobs = list(jobs)
    out = list(pool.map(fn, jobs, chunksize=max(1, len(jobs) // 96)))
    ORACLE_SECONDS[0] += time.time() - t0
    return out


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _sweep(pool, torch, kind, table, hash_fn, width, lanes_of, has_status=True):
    """every pair of `table` through hash_fn(msgs, dst) from host buffers and from device tensors; the lanes lanes_of(pair)
    names against the oracle, every lane host against device.  Returns the number of oracle values compared."""
    calls = []
    for m, d in table:
        msgs, dst = HC.messages(b"hash-lengths/" + kind.encode(), N, m), HC.dst_bytes(d)
        outs = []
        for arg in (msgs, torch.from_numpy(msgs).cuda()):
            r = hash_fn(arg, dst)
            out, st = r if has_status else (r, None)
            out = _np(out)
            assert out.shape == (N, width) and (st is None or not _np(st).any()), (kind, m, d)
            outs.append(out)
        calls.append((m, d, msgs, dst, outs))
    jobs = [(kind, bytes(msgs[i]), dst) for m, d, msgs, dst, _ in calls for i in lanes_of((m, d))]
    want = iter(_map(pool, HC.oracle_hash, jobs))
    bad = []
    for m, d, msgs, dst, (host, dev) in calls:
        if not (host == dev).all():
            bad.append((m, d, "host != device", np.flatnonzero((host != dev).any(axis=1)).tolist()))
        wrong = [i for i in lanes_of((m, d)) if bytes(host[i]) != next(want)]
        if wrong:
            bad.append((m, d, "oracle", wrong))
    assert not bad, f"{kind}: (msg_len, dst_len, against, lanes) {bad}"
    return len(jobs)


ALL = lambda pair: range(N)


# ------------------------------------------------------------------ 2. plain hashing against the oracle
def test_bls12381_hash_g1_every_pair_every_lane(pool, torch_):
    """111 (msg_len, dst_len) pairs x 67 messages = 7 437 outputs of batch_hash_g1, each against
    g1_compress(hash_to_g1(..)); host buffers and device tensors (equal bytes in all 67 lanes)."""
    from kyber_amd.pairing import bls12381 as B

    assert _sweep(pool, torch_, "bls_g1", HC.SHA256_CASES, B.batch_hash_g1, 48, ALL) == len(HC.SHA256_CASES) * N == 7437


def test_bls12381_hash_g2_every_pair(pool, torch_):
    """111 pairs x 67 messages through batch_hash_g2; the oracle (about 80 ms a hash) checks lanes 0, 63 and 66 of every
    pair and all 67 of the six pairs that sit on the boundaries (HC.boundary_pairs): 105 x 3 + 6 x 67 = 717 outputs.
    Host buffers against device tensors in every lane of every pair."""
    from kyber_amd.pairing import bls12381 as B

    full = set(HC.boundary_pairs(HC.SHA256_CASES, HC.SHA256))
    n = _sweep(pool, torch_, "bls_g2", HC.SHA256_CASES, B.batch_hash_g2, 96, lambda pair: range(N) if pair in full else (0, 63, 66))
    assert n == (len(HC.SHA256_CASES) - 6) * 3 + 6 * N == 717


def test_bn254_hash_g1_every_pair_every_lane(pool, torch_):
    """114 pairs of the Keccak-256 table (rate 136) x 67 messages through bn254.batch_hash_g1, every output against the
    oracle: the first DST sweep of this entry point."""
    from kyber_amd.pairing import bn254 as B4

    assert _sweep(pool, torch_, "bn254", HC.KECCAK256_CASES, B4.batch_hash_g1, 64, ALL) == 114 * N


def test_bn256_hash_g1_svdw_every_pair_every_lane(pool, torch_):
    """157 pairs (the SHA-256 table plus the pairs that put HKDF's own hashes on the boundaries) x 67 messages through
    bn256.batch_hash_g1_svdw, every output against the oracle."""
    from kyber_amd.pairing import bn256 as BN

    assert _sweep(pool, torch_, "bn256_svdw", HC.SVDW_CASES, BN.batch_hash_g1_svdw, 64, ALL) == 157 * N


def test_bn256_hash_g1_every_length_every_lane(pool, torch_):
    """pointG1.Hash has no DST: 36 message lengths that put the one-shot SHA-256 on every required position (len mod 64)
    below one block, within the second and past 1000 bytes, x 67 messages, every output against the oracle."""
    from kyber_amd.pairing import bn256 as BN

    lens = HC.oneshot_lengths(64)
    assert _sweep(pool, torch_, "bn256", [(m, 0) for m in lens], lambda msgs, dst: BN.batch_hash_g1(msgs), 64, ALL) == 36 * N


def test_ed25519_hash_every_pair_every_lane(pool, torch_):
    """167 pairs of the SHA-512 table (block 128, finish threshold 112) x 67 messages through ed25519.batch_hash, every
    output against the oracle; an empty DST is refused from host buffers and device tensors, as the reference refuses it
    (point.go:365) and as the oracle does."""
    from kyber_amd._lib import KyberHipError
    from kyber_amd.group import edwards25519 as ED
    from oracle import ed25519 as O

    assert _sweep(pool, torch_, "ed25519", HC.SHA512_CASES, ED.batch_hash, 32, ALL, has_status=False) == 167 * N
    msgs = HC.messages(b"hash-lengths/ed-empty-dst", N, 32)
    with pytest.raises(ValueError):
        O.hash_to_curve(bytes(msgs[0]), b"")
    with pytest.raises(KyberHipError):
        ED.batch_hash(msgs, b"")
    with pytest.raises(KyberHipError):
        ED.batch_hash(torch_.from_numpy(msgs).cuda(), b"")


# ------------------------------------------------------------------ argument edges on every entry that hashes
def _entries(torch):
    """(name, kind, call(n, msgs, msg_len, dst, dst_len) -> (rc, out bytes, extra bytes), default DST) for every kyb_*_hash_*
    entry: outputs and statuses start as 0xA5 so that an untouched buffer is recognisable"""
    from kyber_amd._lib import load

    lib = load()
    out = []

    def host(fn, width, has_dst, has_st):
        def call(n, msgs, msg_len, dst, dst_len):
            o, s = np.full(max(n, N) * width, 0xA5, dtype=np.uint8), np.full(max(n, N), 0xA5, dtype=np.uint8)
            args = [n, msgs.ctypes.data if msgs is not None else None, msg_len] + ([dst, dst_len] if has_dst else []) + \
                [o.ctypes.data] + ([s.ctypes.data] if has_st else [])
            return fn(*args), o, s
        return call

    def dev(fn, width, has_dst, has_st):
        def call(n, msgs, msg_len, dst, dst_len):
            o = torch.full((max(n, N) * width,), 0xA5, dtype=torch.uint8, device="cuda")
            s = torch.full((max(n, N),), 0xA5, dtype=torch.uint8, device="cuda")
            m = torch.from_numpy(msgs).cuda() if msgs is not None else None
            args = [n, m.data_ptr() if m is not None else None, msg_len] + ([dst, dst_len] if has_dst else []) + \
                [o.data_ptr()] + ([s.data_ptr()] if has_st else []) + [None]
            rc = fn(*args)
            torch.cuda.synchronize()
            return rc, o.cpu().numpy(), s.cpu().numpy()
        return call

    for name, kind, width, has_dst, has_st in (("kyb_bls12381_hash_g1", "bls_g1", 48, True, True), ("kyb_bls12381_hash_g2", "bls_g2", 96, True, True),
                                               ("kyb_bn254_hash_g1", "bn254", 64, True, True), ("kyb_bn256_hash_g1_svdw", "bn256_svdw", 64, True, True),
                                               ("kyb_bn256_hash_g1", "bn256", 64, False, True), ("kyb_ed25519_hash", "ed25519", 32, True, False)):
        out.append((name, kind, width, has_dst, host(getattr(lib, name), width, has_dst, has_st)))
        out.append((name + "_dev", kind, width, has_dst, dev(getattr(lib, name + "_dev"), width, has_dst, has_st)))
    return out


def test_hash_entries_argument_edges(pool, torch_):
    """every kyb_*_hash_* entry, host and _dev: a 256-byte DST is KYB_E_ARG with outputs untouched; a DST length with a NULL
    DST pointer is an error; n = 0 is OK; msg_len = 0 with a NULL message pointer gives the hash of the empty message in
    all 67 lanes"""
    dst = HC.dst_bytes(43)
    long_dst = ctypes.create_string_buffer(bytes(range(256)), 256)
    good = ctypes.create_string_buffer(dst, len(dst))
    msgs = HC.messages(b"hash-lengths/edges", N, 32)
    for name, kind, width, has_dst, call in _entries(torch_):
        if has_dst:
            rc, o, s = call(N, msgs, 32, ctypes.cast(long_dst, ctypes.c_void_p), 256)
            assert rc == KYB_E_ARG and (o == 0xA5).all() and (s == 0xA5).all(), (name, rc)
            rc, o, s = call(N, msgs, 32, None, 5)
            assert rc == KYB_E_ARG and (o == 0xA5).all() and (s == 0xA5).all(), (name, rc)
        rc, o, s = call(0, None, 32, ctypes.cast(good, ctypes.c_void_p), len(dst))
        assert rc == 0 and (o == 0xA5).all(), (name, rc)
        rc, o, s = call(0, msgs, 0, ctypes.cast(good, ctypes.c_void_p), len(dst))
        assert rc == 0 and (o == 0xA5).all(), (name, rc)
        rc, o, s = call(N, None, 0, ctypes.cast(good, ctypes.c_void_p), len(dst))
        want = _map(pool, HC.oracle_hash, [(kind, b"", dst)])[0]
        assert rc == 0 and o[:N * width].tobytes() == want * N, (name, rc)
        rc, o, s = call(N, None, 32, ctypes.cast(good, ctypes.c_void_p), len(dst))  # a NULL pointer to 32-byte messages
        assert rc == KYB_E_ARG and (o == 0xA5).all(), (name, rc)


# ------------------------------------------------------------------ 3. the large-batch kernels at lengths other than 32
def _w2_threshold(torch):
    """the batch size from which kyb_bls12381_hash_g*_dev launches the two-wave kernels, read from the source: two waves
    per SIMD on every CU (bls12381_h2c.hip hash_w2)"""
    src = open(os.path.join(ROOT, "kyber_amd", "csrc", "bls12381_h2c.hip")).read()
    m = re.search(r"n >= \(size_t\)ctx->num_cu \* (\d+) \* (\d+) \* (\d+);", src)
    assert m, "hash_w2's threshold is no longer where this test reads it"
    return torch.cuda.get_device_properties(0).multi_processor_count * int(m[1]) * int(m[2]) * int(m[3])


def _large(pool, torch, kind, hash_fn, n, seam, m, dst, width):
    msgs = HC.messages(b"hash-lengths/large/" + kind.encode(), n, m)
    d_msgs = torch.from_numpy(msgs).cuda()
    out, st = hash_fn(d_msgs, dst)
    assert not st.any().item()
    step = seam // 2 - 3  # slices below the threshold, their seams off the wave grid
    parts = [hash_fn(d_msgs[lo:lo + step], dst) for lo in range(0, n, step)]
    assert all(p[0].shape[0] < seam and not p[1].any().item() for p in parts)
    sliced = torch.cat([p[0] for p in parts])
    got, got_sliced = out.cpu().numpy(), sliced.cpu().numpy()
    assert got.shape == got_sliced.shape == (n, width)
    assert hashlib.sha256(got.tobytes()).digest() == hashlib.sha256(got_sliced.tobytes()).digest(), \
        (kind, m, len(dst), "large-batch kernel != per-lane kernel at lanes", np.flatnonzero((got != got_sliced).any(axis=1))[:8].tolist())
    lanes = sorted(set(range(0, n, n // 64)) | {0, 63, 64, step - 1, step, seam - 1, seam, n - 1})
    want = _map(pool, HC.oracle_hash, [(kind, bytes(msgs[i]), dst) for i in lanes])
    wrong = [i for i, w in zip(lanes, want) if bytes(got[i]) != w]
    assert not wrong, (kind, m, len(dst), wrong)
    return len(lanes)


def test_bls12381_two_wave_hash_kernels_on_the_boundaries(pool, torch_):
    """threshold + 5 messages (the threshold read from bls12381_h2c.hip: 2^17 on 256 CUs) on G1 and G2 at three table entries:
    b_0 finishing at 56, a 22-byte DST (b_i finishing at 56), and a message of more than 200 bytes.  About 70 lanes of each
    (64 strided, first, wave / slice / threshold seams, last) against the oracle, and the whole output against the per-lane
    kernels' for the same messages hashed in slices below the threshold."""
    from kyber_amd.pairing import bls12381 as B

    thr = _w2_threshold(torch_)
    assert thr >= 1 << 12
    x = HC.SHA256
    table = HC.SHA256_CASES
    e1 = next(c for c in table if HC.b0_position(*c, x.block, x.zpad) == 56 and 2 <= c[0] < 64)
    e2 = next(c for c in table if c[1] == 22 and c[0] >= 2)
    e3 = next(c for c in table if 200 <= c[0] < 1000 and HC.b0_position(*c, x.block, x.zpad) == 55 and c not in (e1, e2))
    assert len({e1, e2, e3}) == 3
    for m, d in (e1, e2, e3):
        dst = HC.dst_bytes(d)
        assert _large(pool, torch_, "bls_g1", B.batch_hash_g1, thr + 5, thr, m, dst, 48) >= 67
        assert _large(pool, torch_, "bls_g2", B.batch_hash_g2, thr + 5, thr, m, dst, 96) >= 67


def test_bn256_queued_hash_kernel_lengths(pool, torch_):
    """bn256's queued pointG1.Hash kernel (from 2^17 messages, bn256.hip) at message lengths 0, 55, 56 and 200: strided lanes
    against the oracle, the whole output against the per-lane kernel's for the same messages in slices below 2^17"""
    from kyber_amd.pairing import bn256 as BN

    src = open(os.path.join(ROOT, "kyber_amd", "csrc", "bn256.hip")).read()
    assert "hash_queue_on() && n >= (size_t(1) << 17)" in src, "the queued kernel's threshold is no longer where this test reads it"
    for m in (0, 55, 56, 200):
        _large(pool, torch_, "bn256", lambda msgs, dst: BN.batch_hash_g1(msgs, m), (1 << 17) + 9, 1 << 17, m, b"", 64)


# ------------------------------------------------------------------ 4. fused verifications hold valid signatures
ORACLE_LANES = (0, 3, 65, 66)
VERIFY_CASES = HC.cover(HC.SHA256_CASES, HC.SHA256)


def _scalars(label: bytes, n: int):
    from oracle import bls12381 as O

    raw = hashlib.shake_256(label).digest(n * 48)
    xs = [int.from_bytes(raw[48 * i:48 * i + 48], "big") % (O.R - 1) + 1 for i in range(n)]
    return xs, np.frombuffer(b"".join(x.to_bytes(32, "big") for x in xs), dtype=np.uint8).reshape(n, 32).copy()


def _signatures(pool, B, group, xs, xb, msgs, dst):
    """sig_i = x_i H(m_i): lanes ORACLE_LANES by the oracle alone, the rest by the engine's hash (tied to the oracle at the
    same lengths by the tests above) and its scalar multiplication"""
    h, st = (B.batch_hash_g1 if group == 1 else B.batch_hash_g2)(msgs, dst)
    assert not st.any()
    sigs, st = (B.g1_batch_mul if group == 1 else B.g2_batch_mul)(xb, h)
    assert not np.asarray(st).any()
    sigs = np.asarray(sigs).copy()
    made = _map(pool, HC.oracle_sign, [(group, xs[i], bytes(msgs[i]), dst) for i in ORACLE_LANES])
    for i, s in zip(ORACLE_LANES, made):
        assert bytes(sigs[i]) == s, (group, msgs.shape, len(dst), i)  # (engine and oracle agree; the oracle's bytes go in)
        sigs[i] = np.frombuffer(s, dtype=np.uint8)
    return sigs


def _expect(verify, torch, args, want, what):
    """verify(*args) from host buffers and from device tensors: status zero, ok == want"""
    for on_dev in (False, True):
        a = [torch.from_numpy(np.ascontiguousarray(x)).cuda() if on_dev and isinstance(x, np.ndarray) else x for x in args]
        ok, st = verify(*a)
        ok, st = _np(ok), _np(st)
        assert not st.any(), (what, on_dev, st.tolist())
        assert ok.tolist() == want, (what, "device tensors" if on_dev else "host buffers", np.flatnonzero(ok != np.array(want)).tolist())


def _flipped(msgs):
    bad = msgs.copy()
    bad[3, -1] ^= 0x01   # the byte next to the padding
    bad[65, -1] ^= 0x80
    return bad


def _swapped(sigs):
    bad = sigs.copy()
    bad[[3, 65]] = bad[[65, 3]]
    return bad


TWO_FALSE = [0 if i in (3, 65) else 1 for i in range(N)]


@pytest.mark.parametrize("entry", ["verify_g1", "verify_g2", "verify_g1_same_key"])
def test_fused_verify_accepts_valid_signatures_at_every_boundary(pool, torch_, entry):
    """for the entries of HC.cover (every required finish position of b_0 and of b_i, an empty message, an empty and a
    255-byte DST, a message of more than 1000 bytes): 67 valid signatures, four of them made by the oracle alone, verify
    with ok all ones and status zero from host buffers and device tensors; with the last byte of messages 3 and 65
    flipped exactly those two fail (empty messages: with signatures 3 and 65 exchanged)."""
    from kyber_amd.pairing import bls12381 as B

    group = 2 if entry == "verify_g2" else 1
    xs, xb = _scalars(b"hash-lengths/keys/" + entry.encode(), N)
    if entry == "verify_g1_same_key":
        x_other, xb_other = xs[1], xb[1:2]
        xs, xb = [xs[0]] * N, np.repeat(xb[:1], N, axis=0)
    keys, st = (B.g2_commit if group == 1 else B.g1_commit)(xb)
    keys = np.asarray(keys)
    assert not np.asarray(st).any()
    assert len(VERIFY_CASES) >= 12
    for m, d in VERIFY_CASES:
        msgs, dst = HC.messages(b"hash-lengths/" + entry.encode(), N, m), HC.dst_bytes(d)
        sigs = _signatures(pool, B, group, xs, xb, msgs, dst)
        if entry == "verify_g1_same_key":
            key = keys[0].copy()
            verify = lambda k, mm, ss: B.batch_verify_g1_same_key(k, mm, ss, dst)
        else:
            key = keys
            verify = lambda k, mm, ss: (B.batch_verify_g1 if group == 1 else B.batch_verify_g2)(k, mm, ss, dst)
        _expect(verify, torch_, (key, msgs, sigs), [1] * N, (entry, m, d, "valid"))
        if m:
            _expect(verify, torch_, (key, _flipped(msgs), sigs), TWO_FALSE, (entry, m, d, "flipped"))
        elif entry != "verify_g1_same_key":  # (under one key and one empty message every signature is the same)
            _expect(verify, torch_, (key, msgs, _swapped(sigs)), TWO_FALSE, (entry, m, d, "swapped"))
        else:
            other = _signatures(pool, B, 1, [x_other] * N, np.repeat(xb_other, N, axis=0), msgs, dst)
            wrong = sigs.copy()
            wrong[[3, 65]] = other[[3, 65]]
            _expect(verify, torch_, (key, msgs, wrong), TWO_FALSE, (entry, m, d, "other key"))


def test_fused_verify_same_msg_at_every_boundary(pool, torch_):
    """batch_verify_g1_same_msg (one lane of workgroup 0 hashes the message) for the same entries: 67 keys, 67 valid
    signatures over ONE message (four made by the oracle alone) verify; with signatures 3 and 65 exchanged exactly those
    two fail, with the message's last byte flipped all fail.  The empty message from a device pointer and a host pointer."""
    from kyber_amd.pairing import bls12381 as B

    xs, xb = _scalars(b"hash-lengths/keys/same_msg", N)
    keys, st = B.g2_commit(xb)
    keys = np.asarray(keys)
    assert not np.asarray(st).any()
    assert any(m == 0 for m, _ in VERIFY_CASES)
    for m, d in VERIFY_CASES:
        msg, dst = bytes(HC.messages(b"hash-lengths/same_msg", 1, m)[0]), HC.dst_bytes(d)
        msgs = np.repeat(np.frombuffer(msg, dtype=np.uint8).reshape(1, m), N, axis=0)
        sigs = _signatures(pool, B, 1, xs, xb, msgs, dst)
        for on_dev in (False, True):
            put = (lambda x: torch_.from_numpy(np.ascontiguousarray(x)).cuda()) if on_dev else (lambda x: x)
            one = torch_.from_numpy(np.frombuffer(msg, dtype=np.uint8).copy()).cuda() if on_dev else msg
            ok, st = B.batch_verify_g1_same_msg(put(keys), one, put(sigs), dst)
            assert not _np(st).any() and _np(ok).tolist() == [1] * N, ("same_msg", m, d, on_dev, _np(ok).tolist())
            ok, st = B.batch_verify_g1_same_msg(put(keys), one, put(_swapped(sigs)), dst)
            assert not _np(st).any() and _np(ok).tolist() == TWO_FALSE, ("same_msg swapped", m, d, on_dev, _np(ok).tolist())
            if m:
                bad = msg[:-1] + bytes([msg[-1] ^ 1])
                one = torch_.from_numpy(np.frombuffer(bad, dtype=np.uint8).copy()).cuda() if on_dev else bad
                ok, st = B.batch_verify_g1_same_msg(put(keys), one, put(sigs), dst)
                assert not _np(st).any() and not _np(ok).any(), ("same_msg flipped", m, d, on_dev)


def test_verify_entries_argument_edges(pool, torch_):
    """every kyb_bls12381_verify_* entry, host and _dev: a 256-byte DST is KYB_E_ARG with ok / status untouched; a DST length
    with a NULL DST pointer is an error; n = 0 is OK; msg_len = 0 with a NULL message pointer verifies 67 valid signatures
    over the empty message"""
    from kyber_amd._lib import load
    from kyber_amd.pairing import bls12381 as B

    lib = load()
    dst = HC.dst_bytes(43)
    good = ctypes.cast(ctypes.create_string_buffer(dst, len(dst)), ctypes.c_void_p)
    long_buf = ctypes.create_string_buffer(bytes(range(256)), 256)
    long_dst = ctypes.cast(long_buf, ctypes.c_void_p)
    xs, xb = _scalars(b"hash-lengths/keys/edges", N)
    empty = np.zeros((N, 0), dtype=np.uint8)
    some = HC.messages(b"hash-lengths/verify-edges", N, 32)
    for name in ("verify_g1", "verify_g2", "verify_g1_same_key", "verify_g1_same_msg"):
        group = 2 if name == "verify_g2" else 1
        x_, xb_ = ([xs[0]] * N, np.repeat(xb[:1], N, axis=0)) if name.endswith("same_key") else (xs, xb)
        keys = np.asarray((B.g2_commit if group == 1 else B.g1_commit)(xb_)[0])
        if name.endswith("same_key"):
            keys = keys[:1]
        keys = np.ascontiguousarray(keys)
        sigs = np.ascontiguousarray(_signatures(pool, B, group, x_, xb_, empty, dst))
        for on_dev in (False, True):
            fn = getattr(lib, "kyb_bls12381_" + name + ("_dev" if on_dev else ""))

            def call(n, msgs, msg_len, dptr, dlen):
                if on_dev:
                    k, s = torch_.from_numpy(keys).cuda(), torch_.from_numpy(sigs).cuda()
                    mm = torch_.from_numpy(msgs).cuda() if msgs is not None else None
                    ok = torch_.full((N,), 0xA5, dtype=torch_.uint8, device="cuda")
                    st = torch_.full((N,), 0xA5, dtype=torch_.uint8, device="cuda")
                    rc = fn(n, k.data_ptr(), mm.data_ptr() if mm is not None else None, msg_len, dptr, dlen, s.data_ptr(),
                            ok.data_ptr(), st.data_ptr(), 0, None)
                    torch_.cuda.synchronize()
                    return rc, ok.cpu().numpy(), st.cpu().numpy()
                ok, st = np.full(N, 0xA5, dtype=np.uint8), np.full(N, 0xA5, dtype=np.uint8)
                rc = fn(n, keys.ctypes.data, msgs.ctypes.data if msgs is not None else None, msg_len, dptr, dlen, sigs.ctypes.data,
                        ok.ctypes.data, st.ctypes.data, 0)
                return rc, ok, st

            what = (name, "dev" if on_dev else "host")
            rc, ok, st = call(N, some, 32, long_dst, 256)
            assert rc == KYB_E_ARG and (ok == 0xA5).all() and (st == 0xA5).all(), (what, rc)
            rc, ok, st = call(N, some, 32, None, 5)
            assert rc == KYB_E_ARG and (ok == 0xA5).all() and (st == 0xA5).all(), (what, rc)
            rc, ok, st = call(0, some, 32, good, len(dst))
            assert rc == 0 and (ok == 0xA5).all() and (st == 0xA5).all(), (what, rc)
            rc, ok, st = call(N, None, 32, good, len(dst))
            assert rc == KYB_E_ARG and (ok == 0xA5).all() and (st == 0xA5).all(), (what, rc)
            rc, ok, st = call(N, None, 0, good, len(dst))
            assert rc == 0 and not st.any() and ok.tolist() == [1] * N, (what, rc, ok.tolist(), st.tolist())
