"""What every batch wrapper hands to the C ABI, for host buffers and for device tensors, without the library: `load` is
replaced by a stub that records each call.  Checked per call: the symbol, every integer, which pointers are NULL, that
each input pointer is the address of the caller's own contiguous array (no hidden copy), that each returned array lives
where the call was told to write, and that the device call ends with the stream.

The device space is driven with CPU tensors: `_on_device` is patched to "is a torch tensor" and the stream getter to a
constant, so no GPU is needed and addresses stay comparable.
"""
import ctypes

import numpy as np
import pytest
import torch

from kyber_amd import _buf, _lib
from kyber_amd.group import edwards25519 as ed
from kyber_amd.pairing import bls12381 as bls, bn254, bn256
from kyber_amd.pairing._engine import F_TRUSTED, F_UNCOMPRESSED, F_UNCOMPRESSED_OUT

STREAM = 0x5EED0
SPACES = ("host", "device")
NS = (0, 1, 3)


def _baddr(b: bytes) -> int:
    return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p).value


class Stub:
    """stands in for the loaded library: every attribute is a callable that checks the argument count against
    _lib.SIGNATURES, records (name, args) and returns 0"""

    def __init__(self):
        self.calls, self.on_call = [], None

    def __getattr__(self, name):
        def fn(*args):
            assert len(args) == len(_lib.SIGNATURES[name]), (name, len(args))
            args = tuple(_baddr(a) if isinstance(a, bytes) else a for a in args)  # (a bytes object passes as its buffer)
            self.calls.append((name, args))
            if self.on_call:
                self.on_call(name, args)
            return 0

        return fn


@pytest.fixture
def stub(monkeypatch):
    s = Stub()
    monkeypatch.setattr(_buf, "load", lambda: s)
    monkeypatch.setattr(_buf, "_on_device", _buf._is_torch)
    monkeypatch.setattr(_buf, "_stream", lambda: STREAM)
    return s


def arr(n, width, seed=0):
    return np.random.default_rng(seed + 7 * n + width).integers(0, 256, size=(n, width), dtype=np.uint8)


def give(space, a):
    """the caller's array as this space takes it; the tensor shares the array's memory"""
    return a if space == "host" or a is None else torch.from_numpy(a)


def addr(x):
    """where x lives, None when that cannot be compared (an empty tensor has no storage)"""
    if isinstance(x, bytes):
        return _baddr(x)
    if isinstance(x, np.ndarray):
        return x.ctypes.data
    if x.untyped_storage().nbytes() == 0:
        return None
    return x.untyped_storage().data_ptr() + x.storage_offset() * x.element_size()


class Out:
    """the pointer at this position is where result[i] lives"""

    def __init__(self, i):
        self.i = i


class Dst:
    def __init__(self, b):
        self.b = b


PTR = object()  # some non-NULL pointer of the wrapper's own (a dummy byte, packed messages)


def expect(stub, space, name, pattern, result):
    """the one recorded call is `name` (`name`_dev with the stream appended on the device) with these arguments"""
    assert len(stub.calls) == 1, [c[0] for c in stub.calls]
    got, args = stub.calls.pop()
    if space == "device":
        name, pattern = name + "_dev", tuple(pattern) + (STREAM,)
    assert got == name
    assert len(args) == len(pattern), (len(args), len(pattern))
    if not isinstance(result, tuple):
        result = (result,)
    for k, (a, p) in enumerate(zip(args, pattern)):
        if p is None:
            assert a is None, (name, k)
        elif p is PTR:
            assert a, (name, k)
        elif isinstance(p, Dst):
            assert ctypes.string_at(a, len(p.b)) == p.b, (name, k)
        elif isinstance(p, Out):
            r = result[p.i]
            assert (r.dtype == np.uint8 if isinstance(r, np.ndarray) else r.dtype == torch.uint8), (name, k)
            if addr(r) is not None:
                assert a == addr(r), (name, k, "output")
        else:
            assert not isinstance(a, bool) and int(a) == p, (name, k, a, p)


def inp(space, a):
    """(argument, expected pointer): an empty tensor has no address to compare"""
    x = give(space, a)
    return x, (addr(x) if addr(x) is not None else PTR if space == "host" else 0)


def same_type(space, *results):
    for r in results:
        assert isinstance(r, np.ndarray if space == "host" else torch.Tensor)


# ------------------------------------------------------------------ Ed25519
@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("n", NS)
def test_ed25519_plain_calls(stub, space, n):
    (s, ps), (p, pp), (b, pb), (q, pq) = (inp(space, arr(n, 32, k)) for k in range(4))
    r = ed.batch_mul_base(s, uniform=True)
    expect(stub, space, "kyb_ed25519_mul_base", (n, ps, Out(0), _lib.KYB_F_UNIFORM), r)
    assert tuple(r.shape) == (n, 32)
    r = ed.batch_mul(s, p, vartime=True)
    expect(stub, space, "kyb_ed25519_mul", (n, ps, pp, Out(0), Out(1), _lib.KYB_F_VARTIME), r)
    assert tuple(r[0].shape) == (n, 32) and tuple(r[1].shape) == (n,)
    r = ed.batch_mul2(s, p, b, q, vartime=True)
    expect(stub, space, "kyb_ed25519_mul2", (n, ps, pp, pb, pq, Out(0), Out(1), _lib.KYB_F_VARTIME), r)
    r = ed.batch_mul2(s, p, b, q)
    expect(stub, space, "kyb_ed25519_mul2", (n, ps, pp, pb, pq, Out(0), Out(1), 0), r)
    r = ed.batch_dleq_challenge(s, p, b, q)
    expect(stub, space, "kyb_ed25519_dleq_challenge", (n, ps, pp, pb, pq, Out(0), Out(1)), r)
    assert tuple(r[0].shape) == (n, 32) and tuple(r[1].shape) == (n,)
    r = ed.batch_add(s, p)
    expect(stub, space, "kyb_ed25519_add", (n, ps, pp, Out(0), Out(1)), r)
    r = ed.batch_unmarshal(p)
    expect(stub, space, "kyb_ed25519_unmarshal", (n, pp, Out(0), Out(1)), r)
    assert tuple(r[0].shape) == (n, 32) and tuple(r[1].shape) == (n,)
    r = ed.msm(s, p)
    expect(stub, space, "kyb_ed25519_msm", (n, ps, pp, Out(0), Out(1)), r)
    assert tuple(r[0].shape) == (32,) and tuple(r[1].shape) == (n,)
    same_type(space, *r)


@pytest.mark.parametrize("n", NS)
def test_ed25519_host_only_calls(stub, n):
    s, p = arr(n, 32), arr(n, 32, 1)
    r = ed.msm(s, p, scalar_bits=64)
    expect(stub, "host", "kyb_ed25519_msm_flags", (n, addr(s), addr(p), Out(0), Out(1), 64 << 16), r)
    base = bytes(range(32))
    r = ed.commit(s, base, uniform=True)
    expect(stub, "host", "kyb_ed25519_mul_same_base", (n, addr(s), addr(base), Out(0), PTR, _lib.KYB_F_UNIFORM), r)
    idx = np.arange(5, dtype=np.uint32)
    r = ed.poly_eval(p, idx)
    expect(stub, "host", "kyb_ed25519_poly_eval", (5, addr(idx), n, addr(p), Out(0), Out(1)), r)
    assert r[0].shape == (5, 32) and r[1].shape == (n,)
    r = ed.scalar_poly_eval(s, idx)
    expect(stub, "host", "kyb_ed25519_scalar_poly_eval", (5, addr(idx), n, addr(s), Out(0)), r)
    msgs = [b"x" * (i + 1) for i in range(n)]
    sigs = arr(n, 64, 2)
    for want in (True, False):
        r = ed.batch_verify(p, msgs, sigs, want_status=want)
        expect(stub, "host", "kyb_ed25519_verify", (n, addr(p), PTR, PTR, addr(sigs), Out(0), Out(1) if want else None, 0), r)
        assert (r[1] is None) == (not want) and r[0].shape == (n,)


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("shared", (False, True))
def test_ed25519_dleq_verify(stub, space, n, shared):
    six = [inp(space, arr(n, 32, k)) for k in range(6)]
    nb = 1 if shared else n
    (G, pG), (H, pH) = inp(space, arr(nb, 32, 8)), inp(space, arr(nb, 32, 9))
    stride = 0 if shared and n != 1 else 32  # one base for ONE element counts as one per element: stride 32
    (e, pe) = inp(space, arr(1, 32, 10))
    for expect_c, fs, vt in ((None, False, False), (e, True, True)):
        r = ed.batch_dleq_verify(G, H, *[x for x, _ in six], expect_c=expect_c, fiat_shamir=fs, vartime=vt)
        flags = (_lib.KYB_F_VARTIME if vt else 0) | (_lib.KYB_F_DLEQ_FS if fs else 0)
        expect(stub, space, "kyb_ed25519_dleq_verify",
               (n, pG, stride, pH, stride, *[p for _, p in six], None if expect_c is None else pe, Out(0), Out(1), flags), r)
        assert tuple(r[0].shape) == (n,) and tuple(r[1].shape) == (n,)
        same_type(space, *r)


def _msgs(space, msgs):
    """host: the list itself; device: (blob, offsets) as batch_ring_chain takes them"""
    if space == "host":
        return msgs, PTR, PTR
    blob = torch.from_numpy(np.frombuffer(b"".join(msgs), dtype=np.uint8).copy())
    off = torch.from_numpy(np.cumsum([0] + [len(m) for m in msgs]).astype(np.int64))
    return (blob, off), (addr(blob) if blob.numel() else PTR), addr(off)


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("one_ring", (False, True))
@pytest.mark.parametrize("linked", (False, True))
def test_ed25519_ring_chain_and_challenge(stub, space, n, one_ring, linked):
    ring = 3
    slots = ring + (2 if linked else 1)
    keys, pk = inp(space, arr(1 if one_ring else n, 32 * ring, 1))
    sigs, psg = inp(space, arr(n, 32 * slots, 2))
    lb, plb = inp(space, arr(1, 32, 3)) if linked else (None, None)
    for msgs, scope in (([b"m" * (5 + i) for i in range(n)], b"scope"), ([b""] * n, b"")):  # all-empty: a dummy blob
        scope = scope if linked else None
        m, pm, po = _msgs(space, msgs)
        start, pst = inp(space, np.arange(n, dtype=np.uint32 if space == "host" else np.int32))
        for st_arg, steps, vt in ((None, None, False), (start, ring - 1, True)):
            r = ed.batch_ring_chain(keys, m, scope, lb, sigs, ring, start=st_arg, steps=steps, vartime=vt)
            expect(stub, space, "kyb_ed25519_ring_chain",
                   (n, ring, pk, 0 if one_ring or n == 1 else 32 * ring, pm, po,  # (one row is one ring, whatever n)
                    PTR if linked else None, len(scope or b""), plb, psg,
                    32 * slots, None if st_arg is None else pst, ring if steps is None else steps, Out(0), Out(1), Out(2), Out(3),
                    _lib.KYB_F_VARTIME if vt else 0), r)
            assert [tuple(x.shape) for x in r] == [(n, 32), (n, 32), (n,), (n,)]
            same_type(space, *r)
        (pg, ppg), (ph, pph), (tg, ptg) = (inp(space, arr(n, 32, 4 + k)) for k in range(3))
        if not linked:
            ph = tg = pph = ptg = None
        r = ed.batch_ring_challenge(m, scope, tg, pg, ph)
        expect(stub, space, "kyb_ed25519_ring_challenge",
               (n, pm, po, PTR if linked else None, len(scope or b""), ptg, ppg, pph, Out(0), Out(1)), r)
        assert [tuple(x.shape) for x in r] == [(n, 32), (n,)]


def test_ed25519_ring_host_lists_join(stub):
    """the host space takes keys and signatures as lists of byte strings"""
    keys, sigs = [bytes([i]) * 32 for i in range(3)], [bytes([9]) * 128, bytes([8]) * 128]
    r = ed.batch_ring_chain(keys, [b"a", b"bc"], None, None, sigs, 3)
    expect(stub, "host", "kyb_ed25519_ring_chain",
           (2, 3, PTR, 0, PTR, PTR, None, 0, None, PTR, 128, None, 3, Out(0), Out(1), Out(2), Out(3), 0), r)


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("n", NS)
def test_hash_wrappers(stub, space, n):
    m, pm = inp(space, arr(n, 11))
    if n == 0 and space == "host":
        pm = PTR  # an empty host buffer is replaced by one dummy byte
    dst = b"QUUX-V01-CS02"
    r = ed.batch_hash(m, dst)
    expect(stub, space, "kyb_ed25519_hash", (n, pm, 11, Dst(dst), len(dst), Out(0)), r)
    assert tuple(r.shape) == (n, 32)
    for fn, name, w, d in ((bls.batch_hash_g1, "kyb_bls12381_hash_g1", 48, dst), (bls.batch_hash_g2, "kyb_bls12381_hash_g2", 96, dst),
                           (bls.batch_hash_g1, "kyb_bls12381_hash_g1", 48, b""), (bn254.batch_hash_g1, "kyb_bn254_hash_g1", 64, dst),
                           (bn256.batch_hash_g1_svdw, "kyb_bn256_hash_g1_svdw", 64, dst),
                           (bn256.batch_hash_g1_svdw, "kyb_bn256_hash_g1_svdw", 64, b"")):
        r = fn(m, d)
        expect(stub, space, name, (n, pm, 11, Dst(d) if d else None, len(d), Out(0), Out(1)), r)  # an empty DST is NULL, 0
        assert tuple(r[0].shape) == (n, w) and tuple(r[1].shape) == (n,)
        same_type(space, *r)
    r = bn256.batch_hash_g1(m)
    expect(stub, space, "kyb_bn256_hash_g1", (n, pm, 11, Out(0), Out(1)), r)
    assert bls.DOMAIN_G1 != bls.DOMAIN_G2
    r = bls.batch_hash_g2(m)
    expect(stub, space, "kyb_bls12381_hash_g2", (n, pm, 11, Dst(bls.DOMAIN_G2), len(bls.DOMAIN_G2), Out(0), Out(1)), r)


def test_hash_wrappers_take_lists_and_refuse_unequal_lengths(stub):
    r = ed.batch_hash([b"abc", b"def"], b"D")
    expect(stub, "host", "kyb_ed25519_hash", (2, PTR, 3, Dst(b"D"), 1, Out(0)), r)
    r = ed.batch_hash([b"", b""], b"D")  # all-empty messages: one dummy byte, never NULL
    expect(stub, "host", "kyb_ed25519_hash", (2, PTR, 0, Dst(b"D"), 1, Out(0)), r)
    for fn, what in ((lambda m: ed.batch_hash(m, b"D"), "batch_hash"), (bls.batch_hash_g1, "batch hash"),
                     (bn256.batch_hash_g1, "batch_hash_g1"), (bn256.batch_hash_g1_svdw, "batch_hash_g1_svdw"),
                     (bn254.batch_hash_g1, "batch_hash_g1"), (lambda m: bls.batch_verify_g1([], m, []), "batch_verify"),
                     (lambda m: bls.batch_verify_g1_same_key(b"", m, []), "batch_verify_same_key")):
        with pytest.raises(ValueError, match=f"^{what}: messages must have equal length$"):
            fn([b"abc", b"de"])
    assert not stub.calls


# ------------------------------------------------------------------ pairing suites
@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("mod", (bls, bn256), ids=("bls12381", "bn256"))
def test_engine_calls(stub, space, n, mod):
    eng, sym = mod.ENGINE, "kyb_" + mod.ENGINE.prefix + "_"
    w = {1: eng.G1_LEN, 2: eng.G2_LEN}
    s, ps = inp(space, arr(n, 32))
    for g in (1, 2):
        p, pp = inp(space, arr(n, w[g], g))
        q, pq = inp(space, arr(n, w[g], g + 2))
        r = eng.mul(g, s, p, False, F_TRUSTED(0))
        stride = (w[g],) if space == "device" else ()
        expect(stub, space, f"{sym}g{g}_mul", (n, ps, pp, *stride, Out(0), Out(1), F_TRUSTED(0)), r)
        assert tuple(r[0].shape) == (n, w[g]) and tuple(r[1].shape) == (n,)
        base, pb = inp(space, arr(1, w[g], 5))
        r = eng.mul(g, s, base, True)  # one base for the batch: a name of its own on the host, stride 0 on the device
        expect(stub, space, f"{sym}g{g}_mul" + ("_same_base" if space == "host" else ""),
               (n, ps, pb, *((0,) if space == "device" else ()), Out(0), Out(1), 0), r)
        r = (eng.g1_commit if g == 1 else eng.g2_commit)(s)  # the default base is bytes: uploaded on the device
        expect(stub, space, f"{sym}g{g}_mul" + ("_same_base" if space == "host" else ""),
               (n, ps, PTR, *((0,) if space == "device" else ()), Out(0), Out(1), F_TRUSTED(0)), r)
        r = eng.add(g, p, q)
        expect(stub, space, f"{sym}g{g}_add", (n, pp, pq, Out(0), Out(1)), r)
        assert tuple(r[0].shape) == (n, w[g]) and tuple(r[1].shape) == (n,)
        r = eng.batch_unmarshal(g, p)
        expect(stub, space, f"{sym}g{g}_unmarshal", (n, pp, Out(0), Out(1), 0), r)
        r = eng.msm(g, s, p, F_TRUSTED(0))
        expect(stub, space, f"{sym}g{g}_msm", (n, ps, pp, Out(0), Out(1), F_TRUSTED(0)), r)
        assert tuple(r[0].shape) == (w[g],) and tuple(r[1].shape) == (n,)
        same_type(space, *r)
        if space == "host":
            idx = np.arange(4, dtype=np.uint32)
            r = eng.poly_eval(g, p, idx, F_TRUSTED(0))
            expect(stub, "host", f"{sym}g{g}_poly_eval", (4, addr(idx), n, pp, Out(0), Out(1), F_TRUSTED(0)), r)
            assert r[0].shape == (4, w[g]) and r[1].shape == (n,)
            r = eng.scalar_poly_eval(s, idx)
            expect(stub, "host", f"{sym}scalar_poly_eval", (4, addr(idx), n, ps, Out(0)), r)
    (a, pa), (b, pb), (c, pc), (d, pd) = (inp(space, arr(n, w[1 + k % 2], 6 + k)) for k in range(4))
    r = eng.batch_pair(a, b, F_TRUSTED(1))
    expect(stub, space, f"{sym}pair", (n, pa, pb, Out(0), Out(1), F_TRUSTED(1)), r)
    assert tuple(r[0].shape) == (n, eng.GT_LEN) and tuple(r[1].shape) == (n,)
    r = eng.batch_validate_pairing(a, b, c, d, F_TRUSTED(3))
    expect(stub, space, f"{sym}pair_check", (n, pa, pb, pc, pd, Out(0), Out(1), F_TRUSTED(3)), r)
    assert tuple(r[0].shape) == (n,) and tuple(r[1].shape) == (n,)
    gt, pgt = inp(space, arr(n, eng.GT_LEN, 11))
    r = eng.gt_batch_mul(s, gt)
    expect(stub, space, f"{sym}gt_mul", (n, ps, pgt, Out(0), Out(1)), r)
    assert tuple(r[0].shape) == (n, eng.GT_LEN)
    same_type(space, *r)


@pytest.mark.parametrize("space", SPACES)
def test_bls12381_uncompressed_widths(stub, space):
    n, eng = 3, bls.ENGINE
    s, ps = inp(space, arr(n, 32))
    p, pp = inp(space, arr(n, 96))  # G1, uncompressed affine
    r = eng.mul(1, s, p, False, F_UNCOMPRESSED | F_UNCOMPRESSED_OUT)
    expect(stub, space, "kyb_bls12381_g1_mul", (n, ps, pp, *((96,) if space == "device" else ()), Out(0), Out(1), 6), r)
    assert tuple(r[0].shape) == (n, 96)
    r = eng.batch_unmarshal(2, inp(space, arr(n, 96, 1))[0], F_UNCOMPRESSED_OUT)
    assert tuple(r[0].shape) == (n, 192)
    expect(stub, space, "kyb_bls12381_g2_unmarshal", (n, PTR, Out(0), Out(1), F_UNCOMPRESSED_OUT), r)
    q, pq = inp(space, arr(n, 192, 2))
    r = eng.batch_pair(p, q, F_UNCOMPRESSED)
    expect(stub, space, "kyb_bls12381_pair", (n, pp, pq, Out(0), Out(1), F_UNCOMPRESSED), r)
    r = eng.msm(2, s, q, F_UNCOMPRESSED)
    expect(stub, space, "kyb_bls12381_g2_msm", (n, ps, pq, Out(0), Out(1), F_UNCOMPRESSED), r)
    assert tuple(r[0].shape) == (96,)
    m, pm = inp(space, arr(n, 7, 3))
    r = bls.batch_verify_g1(q, m, p, flags=F_UNCOMPRESSED)  # keys 192, signatures 96
    d = bls.DOMAIN_G1
    expect(stub, space, "kyb_bls12381_verify_g1", (n, pq, pm, 7, Dst(d), len(d), pp, Out(0), Out(1), F_UNCOMPRESSED), r)


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("n", NS)
def test_bls12381_verify_calls(stub, space, n):
    m, pm = inp(space, arr(n, 9))
    if n == 0 and space == "host":
        pm = PTR
    (k2, pk2), (s1, ps1), (k1, pk1), (s2, ps2) = (inp(space, arr(n, w, i)) for i, w in enumerate((96, 48, 48, 96)))
    d1, d2 = bls.DOMAIN_G1, bls.DOMAIN_G2
    r = bls.batch_verify_g1(k2, m, s1, flags=F_TRUSTED(0))
    expect(stub, space, "kyb_bls12381_verify_g1", (n, pk2, pm, 9, Dst(d1), len(d1), ps1, Out(0), Out(1), F_TRUSTED(0)), r)
    r = bls.batch_verify_g2(k1, m, s2, dst=b"")
    expect(stub, space, "kyb_bls12381_verify_g2", (n, pk1, pm, 9, None, 0, ps2, Out(0), Out(1), 0), r)
    assert tuple(r[0].shape) == (n,) and tuple(r[1].shape) == (n,)
    key = bytes(range(96))
    r = bls.batch_verify_g1_same_key(key, m, s1)  # one key as bytes: in place on the host, uploaded on the device
    expect(stub, space, "kyb_bls12381_verify_g1_same_key",
           (n, addr(key) if space == "host" else PTR, pm, 9, Dst(d1), len(d1), ps1, Out(0), Out(1), 0), r)
    if space == "device":
        kt = torch.from_numpy(arr(1, 96, 5))
        r = bls.batch_verify_g1_same_key(kt, m, s1)
        expect(stub, space, "kyb_bls12381_verify_g1_same_key", (n, addr(kt), pm, 9, Dst(d1), len(d1), ps1, Out(0), Out(1), 0), r)
    msg = b"one message"
    r = bls.batch_verify_g1_same_msg(k2, msg, s1)
    expect(stub, space, "kyb_bls12381_verify_g1_same_msg",
           (n, pk2, addr(msg) if space == "host" else PTR, len(msg), Dst(d1), len(d1), ps1, Out(0), Out(1), 0), r)
    r = bls.batch_verify_g1_same_msg(k2, b"", s1)  # the empty message: NULL on the host, a dummy byte on the device
    expect(stub, space, "kyb_bls12381_verify_g1_same_msg",
           (n, pk2, None if space == "host" else PTR, 0, Dst(d1), len(d1), ps1, Out(0), Out(1), 0), r)
    same_type(space, *r)


def test_bls12381_wrong_length_elements_fail_alone(stub):
    """a list with one signature of the wrong length: that lane is ok = 0 / status = 1, its neighbours keep what the
    native call wrote, and nothing shifts"""
    def native(name, args):  # every lane verifies; the blanked lane comes back as "not in the subgroup"
        ctypes.memset(args[7], 1, 3)
        ctypes.memmove(args[8], bytes([0, 2, 0]), 3)

    stub.on_call = native
    keys = [bytes([i + 1]) * 96 for i in range(3)]
    sigs = [bytes([7]) * 48, bytes([8]) * 47, bytes([9]) * 48]
    msgs = [b"abc"] * 3
    # batch_verify reports the lane as BAD_POINT whatever the native call said; the same-key and same-msg calls keep a
    # native verdict that says more (the header's precedence)
    for r, status in ((bls.batch_verify_g1(keys, msgs, sigs), 1), (bls.batch_verify_g1_same_key(keys[0], msgs, sigs), 2),
                      (bls.batch_verify_g1_same_msg(keys, b"abc", sigs), 2)):
        name, args = stub.calls.pop()
        packed = ctypes.string_at(args[6], 3 * 48)
        assert packed == sigs[0] + bytes(48) + sigs[2]
        assert list(r[0]) == [1, 0, 1] and list(r[1]) == [0, status, 0]
    stub.on_call = lambda name, args: (ctypes.memset(args[7], 1, 3), ctypes.memset(args[8], 0, 3))  # native status 0: BAD_POINT
    for r in (bls.batch_verify_g1_same_key(keys[0], msgs, sigs), bls.batch_verify_g1_same_msg(keys, b"abc", sigs)):
        stub.calls.pop()
        assert list(r[0]) == [1, 0, 1] and list(r[1]) == [0, 1, 0]
    stub.on_call = None
    # a key of the wrong length fails every element without a call (host space)
    ok, st = bls.batch_verify_g1_same_key(bytes(95), msgs, [s if len(s) == 48 else bytes(48) for s in sigs])
    assert not stub.calls and list(ok) == [0, 0, 0] and list(st) == [1, 1, 1]


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("on_g2", (False, True))
def test_bls12381_ibe_calls(stub, space, n, on_g2):
    enc, dec = (bls.batch_ibe_encrypt_g2, bls.batch_ibe_decrypt_g2) if on_g2 else (bls.batch_ibe_encrypt_g1, bls.batch_ibe_decrypt_g1)
    g, wm, wk = ("g2", 96, 48) if on_g2 else ("g1", 48, 96)
    master, ident = bytes(range(wm)), b"round 7"
    (m, pm), (sg, psg) = inp(space, arr(n, 16)), inp(space, arr(n, 16, 1))
    dst = bls.DOMAIN_G1 if on_g2 else bls.DOMAIN_G2
    host = space == "host"
    r = enc(master, ident, m, sg)
    expect(stub, space, f"kyb_bls12381_ibe_encrypt_{g}",
           (n, addr(master) if host else PTR, addr(ident) if host else PTR, len(ident), Dst(dst), len(dst), psg, pm, 16,
            Out(0), Out(1), Out(2), Out(3), 0), r)
    assert [tuple(x.shape) for x in r] == [(n, wm), (n, 16), (n, 16), (n,)]
    r = enc(master + master, b"", m, None, b"", F_UNCOMPRESSED | F_UNCOMPRESSED_OUT)  # fresh sigmas, empty identity and DST
    expect(stub, space, f"kyb_bls12381_ibe_encrypt_{g}",
           (n, PTR, PTR, 0, None, 0, PTR if n or host else 0, pm, 16, Out(0), Out(1), Out(2), Out(3), 6), r)  # (no sigmas for no messages)
    assert tuple(r[0].shape) == (n, 2 * wm)
    (u, pu), (v, pv), (w, pw) = inp(space, arr(n, wm, 2)), inp(space, arr(n, 16, 3)), inp(space, arr(n, 16, 4))
    if n == 0 and host:  # nothing to take a width from: V and W are the wrapper's own empty arrays
        pv = pw = PTR
    key = bytes(range(wk))
    ln = 0 if n == 0 and host else 16
    r = dec(key, u, v, w)  # ONE private key: stride 0
    expect(stub, space, f"kyb_bls12381_ibe_decrypt_{g}", (n, addr(key) if host else PTR, 0, pu, pv, pw, ln, Out(0), Out(1), 0), r)
    assert [tuple(x.shape) for x in r] == [(n, ln), (n,)]
    if n > 1:  # (one key for one ciphertext is the shared key on the device)
        ks, pks = inp(space, arr(n, wk, 5))
        r = dec(ks, u, v, w)
        expect(stub, space, f"kyb_bls12381_ibe_decrypt_{g}", (n, pks, wk, pu, pv, pw, 16, Out(0), Out(1), 0), r)
    same_type(space, *r)


def test_bn256_hash_takes_a_flat_device_tensor_with_msg_len(stub):
    """a flat tensor is n x msg_len bytes: n is the number of messages, not of bytes"""
    flat = torch.from_numpy(arr(3, 11).reshape(-1))
    r = bn256.batch_hash_g1(flat, msg_len=11)
    expect(stub, "device", "kyb_bn256_hash_g1", (3, addr(flat), 11, Out(0), Out(1)), r)
    assert tuple(r[0].shape) == (3, 64) and tuple(r[1].shape) == (3,)
    with pytest.raises(ValueError, match="^batch_hash_g1: a flat tensor needs msg_len$"):
        bn256.batch_hash_g1(flat)


def test_ed25519_ring_device_start_and_link_base_shapes(stub):
    """on the device `start` is any tensor of n positions (a column too); link_base is exactly one point"""
    keys, sigs = torch.from_numpy(arr(1, 96)), torch.from_numpy(arr(2, 160))
    m = _msgs("device", [b"a", b"bc"])[0]
    lb, start = torch.from_numpy(arr(1, 32)), torch.from_numpy(np.array([[1], [2]], dtype=np.int32))
    r = ed.batch_ring_chain(keys, m, b"s", lb.view(32), sigs, 3, start=start, steps=2)
    name, args = stub.calls.pop()
    assert name == "kyb_ed25519_ring_chain_dev" and args[8] == addr(lb) and args[11] == addr(start) and args[12] == 2
    with pytest.raises(ValueError, match="^link_base: one 32-byte point$"):
        ed.batch_ring_chain(keys, m, b"s", torch.from_numpy(arr(2, 32)), sigs, 3)
    with pytest.raises(ValueError, match="^expect_c: one 32-byte scalar$"):
        ed.batch_dleq_verify(*[torch.from_numpy(arr(2, 32, k)) for k in range(8)], expect_c=torch.from_numpy(arr(2, 32)))
    assert not stub.calls


# ------------------------------------------------------------------ the memory space and the errors
def test_cpu_tensors_are_host_buffers(monkeypatch):
    """a tensor that is not on a device is a host buffer everywhere: it reaches the host entry point with its own address"""
    s = Stub()
    monkeypatch.setattr(_buf, "load", lambda: s)  # (_on_device is the real one here)
    a, b = torch.from_numpy(arr(3, 32)), torch.from_numpy(arr(3, 32, 1))
    out, st = ed.batch_mul(a, b)
    expect(s, "host", "kyb_ed25519_mul", (3, addr(a), addr(b), Out(0), Out(1), 0), (out, st))
    same_type("host", out, st)
    c, d = torch.from_numpy(arr(3, 48)), torch.from_numpy(arr(3, 48, 1))
    r = bls.ENGINE.add(1, c, d)
    expect(s, "host", "kyb_bls12381_g1_add", (3, addr(c), addr(d), Out(0), Out(1)), r)
    r = bls.batch_hash_g1(torch.from_numpy(arr(3, 5)), b"D")
    assert s.calls.pop()[0] == "kyb_bls12381_hash_g1"


@pytest.mark.parametrize("space", SPACES)
def test_non_contiguous_input_is_copied_once_and_status_is_sliced(stub, space):
    wide = arr(3, 64)
    a, b = give(space, wide)[:, :32], give(space, arr(3, 32, 1))
    seen = []
    stub.on_call = lambda name, args: seen.append(ctypes.string_at(args[1], 96))  # (the copy lives as long as the call)
    out, st = ed.batch_add(a, b)
    name, args = stub.calls.pop()
    assert args[1] != addr(a) and seen == [wide[:, :32].tobytes()] and args[2] == addr(b)
    stub.on_call = None
    out, st = ed.batch_add(give(space, arr(0, 32)), give(space, arr(0, 32)))
    name, args = stub.calls.pop()
    assert args[4] and tuple(st.shape) == (0,)  # one byte behind an empty status: never a NULL status pointer


@pytest.mark.parametrize("space", SPACES)
def test_argument_errors_keep_their_wording(stub, space):
    t = lambda n, w=32, k=0: give(space, arr(n, w, k))
    E = bls.ENGINE
    msgs = _msgs(space, [b"a", b"b"])[0]
    cases = [
        (lambda: ed.batch_mul(t(2), t(3)), "scalars/points length mismatch"),
        (lambda: ed.msm(t(2), t(3)), "scalars/points length mismatch"),
        (lambda: ed.batch_mul_base(t(2), vartime=True, uniform=True), "vartime and uniform are exclusive"),
        (lambda: ed.batch_add(t(2), t(3)), "length mismatch"),
        (lambda: ed.batch_mul2(t(2), t(2), t(3), t(2)), "length mismatch"),
        (lambda: ed.batch_dleq_challenge(t(2), t(2), t(2), t(1)), "length mismatch"),
        (lambda: ed.batch_dleq_verify(t(1), t(1), *[t(3)] * 5, t(2)), "length mismatch"),
        (lambda: ed.batch_dleq_verify(t(2), t(1), *[t(3)] * 6), "G: one base or one per element"),
        (lambda: ed.batch_dleq_verify(t(1), t(2), *[t(3)] * 6), "H: one base or one per element"),
        (lambda: ed.batch_ring_chain(t(1, 96), msgs, b"s", None, t(2, 160), 3), "a link scope and its base go together"),
        (lambda: ed.batch_ring_chain(t(1, 96), msgs, None, t(1), t(2, 128), 3), "a link scope and its base go together"),
        (lambda: ed.batch_ring_chain(t(1, 96), msgs, None, None, t(2, 128), 0), "empty ring"),
        (lambda: ed.batch_ring_chain(t(3, 96), msgs, None, None, t(2, 128), 3), "keys: one ring or one per signature"),
        (lambda: ed.batch_ring_chain(t(1, 96), msgs, None, None, t(2, 128), 3, start=give(space, np.zeros(3, dtype=np.int32))),
         "start: one position per signature"),
        (lambda: ed.batch_ring_challenge(msgs, b"s", None, t(2), t(2)), "scope, tags and PH go together"),
        (lambda: ed.batch_ring_challenge(msgs, None, None, t(2), t(2)), "scope, tags and PH go together"),
        (lambda: ed.batch_ring_challenge(msgs, b"s", t(3), t(2), t(2)), "length mismatch"),
        (lambda: E.mul(1, t(2), t(3, 48), False), "scalars/points length mismatch"),
        (lambda: E.msm(2, t(2), t(3, 96)), "scalars/points length mismatch"),
        (lambda: E.add(1, t(2, 48), t(3, 48)), "length mismatch"),
        (lambda: E.batch_pair(t(2, 48), t(3, 96)), "g1/g2 length mismatch"),
        (lambda: E.gt_batch_mul(t(2), t(3, 576)), "length mismatch"),
        (lambda: E.batch_validate_pairing(t(2, 48), t(2, 96), t(3, 48), t(2, 96)), "length mismatch"),
        (lambda: bls.batch_verify_g1(t(2, 96), t(3, 5), t(3, 48)), "batch_verify: 3 messages, 2 public keys, 3 signatures"),
        (lambda: bls.batch_verify_g1_same_msg(t(3, 96), b"m", t(2, 48)), "batch_verify_same_msg: 3 public keys, 2 signatures"),
        (lambda: bls.batch_verify_g1_same_key(bytes(96), t(3, 5), t(2, 48)),
         "batch_verify_same_key: " + ("" if space == "host" else "key of 96 bytes, ") + "3 messages, 2 signatures"),
    ]
    if space == "host":
        cases += [(lambda: ed.batch_ring_chain(t(1, 96), [b"a"], None, None, t(2, 128), 3), "msgs/sigs length mismatch"),
                  (lambda: ed.batch_ring_challenge([b"a"], None, None, t(2), None), "length mismatch"),
                  (lambda: ed.batch_verify(t(2), [b"a"], t(2, 64)), "pubs/msgs/sigs length mismatch")]
    else:
        bad = (msgs[0], msgs[1][:2])
        cases += [(lambda: ed.batch_ring_chain(t(1, 96), bad, None, None, t(2, 128), 3), "msgs: (blob, n + 1 64-bit offsets)"),
                  (lambda: bls.batch_verify_g1_same_key(bytes(95), t(3, 5), t(3, 48)),
                   "batch_verify_same_key: key of 95 bytes, 3 messages, 3 signatures")]
    for fn, wording in cases:
        with pytest.raises(ValueError) as e:
            fn()
        assert str(e.value) == wording
    assert not stub.calls


def test_failures_name_the_symbol(monkeypatch):
    """a non-zero return raises KyberHipError naming the full symbol, _dev included"""
    class Failing:
        def __getattr__(self, name):
            return (lambda *a: None) if name == "kyb_last_error" else (lambda *a: -1)

    monkeypatch.setattr(_buf, "load", Failing)
    monkeypatch.setattr(_lib, "load", Failing)
    monkeypatch.setattr(_buf, "_stream", lambda: STREAM)
    with pytest.raises(_lib.KyberHipError, match="^kyb_bls12381_hash_g1 failed rc=-1"):
        bls.batch_hash_g1(arr(2, 5))
    monkeypatch.setattr(_buf, "_on_device", _buf._is_torch)
    with pytest.raises(_lib.KyberHipError, match="^kyb_bls12381_hash_g2_dev failed rc=-1"):
        bls.batch_hash_g2(torch.from_numpy(arr(2, 5)))
