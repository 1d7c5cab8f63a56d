"""The two memory spaces of the batch wrappers agree on the device: every wrapper is called once with host buffers and
once with CUDA tensors on a side stream, one input given as a non-contiguous slice, and outputs and statuses must be
byte-identical.  Batches of 1 and of 65 (one wave plus one lane); inputs are valid points made by the engine from small
scalars, and one undecodable point so that a non-zero status is compared too."""
import numpy as np
import pytest
import torch

from kyber_amd.group import edwards25519 as ed
from kyber_amd.pairing import bls12381 as bls, bn256

pytestmark = pytest.mark.gpu

# (batch size, lane of the undecodable point)
CASES = [(1, None), (1, 0), (65, 7)]


class Msgs:
    """messages of any lengths: a list of byte strings for the host space, (blob, offsets) tensors for the device"""

    def __init__(self, msgs):
        self.msgs = msgs


def _to_dev(a, slice_it):
    if isinstance(a, Msgs):
        blob = np.frombuffer(b"".join(a.msgs), dtype=np.uint8).copy()
        off = np.cumsum([0] + [len(m) for m in a.msgs]).astype(np.int64)
        return torch.from_numpy(blob).cuda(), torch.from_numpy(off).cuda()
    if not isinstance(a, np.ndarray):
        return a
    t = torch.from_numpy(a).cuda()
    if slice_it:  # the left half of a buffer twice as wide: rows are not adjacent
        t = torch.cat([t, t], dim=1)[:, :a.shape[1]]
        assert a.shape[0] == 1 or not t.is_contiguous()
    return t


def both(fn, *args, sliced=0, **kw):
    """fn on host buffers and on device tensors (argument `sliced` non-contiguous) on a side stream: identical bytes"""
    host = fn(*[a.msgs if isinstance(a, Msgs) else a for a in args], **kw)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev = fn(*[_to_dev(a, i == sliced) for i, a in enumerate(args)], **{k: _to_dev(v, False) for k, v in kw.items()})
    stream.synchronize()
    host, dev = (host, dev) if isinstance(host, tuple) else ((host,), (dev,))
    assert len(host) == len(dev)
    for k, (h, d) in enumerate(zip(host, dev)):
        assert isinstance(h, np.ndarray) and d.is_cuda
        d = d.cpu().numpy()
        assert h.shape == d.shape and h.dtype == d.dtype == np.uint8, (fn, k, h.shape, d.shape)
        assert np.array_equal(h, d), (fn, k, np.nonzero((h != d).reshape(len(h), -1).any(axis=1))[0][:8])
    return host


def _scalars(n, seed, big_endian=False):
    s = np.zeros((n, 32), dtype=np.uint8)
    v = np.random.default_rng(seed).integers(1, 1 << 16, size=n)
    lo, hi = (31, 30) if big_endian else (0, 1)
    s[:, lo], s[:, hi] = v & 0xFF, v >> 8
    return s


@pytest.fixture(scope="module")
def ed_bad():
    """an encoding that UnmarshalBinary rejects (no x for this y)"""
    cand = np.zeros((64, 32), dtype=np.uint8)
    cand[:, 0] = np.arange(2, 66)
    _, st = ed.batch_unmarshal(cand)
    return cand[np.nonzero(st)[0][0]].copy()


@pytest.mark.parametrize("n,bad", CASES)
def test_ed25519_spaces_agree(n, bad, ed_bad):
    s, t = _scalars(n, 1), _scalars(n, 2)
    P, Q = ed.batch_mul_base(s), ed.batch_mul_base(t)
    Pb = P.copy()
    if bad is not None:
        Pb[bad] = ed_bad
    both(ed.batch_mul_base, s)
    _, st = both(ed.batch_mul, s, Pb, sliced=1)
    assert [i for i in range(n) if st[i]] == ([] if bad is None else [bad])
    both(ed.batch_mul, s, Pb, vartime=True)
    both(ed.batch_mul2, s, Pb, t, Q, sliced=3)
    _, st = both(ed.batch_add, Pb, Q)
    assert bool(st.any()) == (bad is not None)
    both(ed.batch_unmarshal, Pb)
    both(ed.msm, s, Pb, sliced=1)
    msgs = np.random.default_rng(3).integers(0, 256, size=(n, 37), dtype=np.uint8)
    both(ed.batch_hash, msgs, b"QUUX-V01-CS02-with-edwards25519_XMD:SHA-512_ELL2_RO_")
    both(ed.batch_dleq_challenge, P, Q, Pb, s, sliced=2)
    for G, H in ((P, Q), (P[:1], Q[:1])):  # one base per element, one base for the batch
        _, st = both(ed.batch_dleq_verify, G, H, Pb, Q, s, t, P, Q, sliced=2)
        assert bool(st.any()) == (bad is not None)
    both(ed.batch_dleq_verify, P[:1], Q[:1], Pb, Q, s, t, P, Q, expect_c=s[:1].copy(), vartime=True)
    both(ed.batch_dleq_verify, P, Q, Pb, Q, s, t, P, Q, fiat_shamir=True)


@pytest.mark.parametrize("linked", (False, True))
@pytest.mark.parametrize("n,bad", CASES)
def test_ed25519_ring_spaces_agree(n, bad, linked, ed_bad):
    ring = 3
    keys = ed.batch_mul_base(_scalars(ring * n, 4)).reshape(n, ring * 32)
    if bad is not None:
        keys[bad, 32:64] = ed_bad
    cols = [_scalars(n, 5 + k) for k in range(1 + ring)]  # c_0, s_0 .. s_2
    scope = link_base = tags = PH = None
    if linked:
        scope, link_base = b"a link scope", ed.batch_mul_base(_scalars(1, 9))
        tags = PH = ed.batch_mul_base(_scalars(n, 10))
        cols.append(tags)
    sigs = np.ascontiguousarray(np.concatenate(cols, axis=1))
    msgs = Msgs([b"message %d" % i * (i % 3) for i in range(n)])  # lengths differ, some are empty
    start = (np.arange(n) % ring).astype(np.int32)
    for k, kw in ((keys, {}), (keys[:1].copy(), {"start": start, "steps": ring - 1, "vartime": True})):  # n rings, one ring
        r = both(ed.batch_ring_chain, k, msgs, scope, link_base, sigs, ring, sliced=4, **kw)
        if k is keys:
            assert bool(r[3].any()) == (bad is not None)
    both(ed.batch_ring_challenge, msgs, scope, tags, keys[:, :32].copy(), PH, sliced=3)


def _suite_inputs(mod, n, bad):
    eng = mod.ENGINE
    s, t = _scalars(n, 11, True), _scalars(n, 12, True)
    (p1, _), (q1, _), (p2, _), (q2, _) = eng.g1_commit(s), eng.g1_commit(t), eng.g2_commit(s), eng.g2_commit(t)
    b1, b2 = p1.copy(), p2.copy()
    if bad is not None:
        b1[bad], b2[bad] = 0xFF, 0xFF  # a coordinate above the modulus (BLS12-381) / a point off the curve (bn256)
    return s, t, p1, q1, p2, q2, b1, b2


@pytest.mark.parametrize("mod", (bls, bn256), ids=("bls12381", "bn256"))
@pytest.mark.parametrize("n,bad", CASES)
def test_pairing_suite_spaces_agree(mod, n, bad):
    eng = mod.ENGINE
    s, t, p1, q1, p2, q2, b1, b2 = _suite_inputs(mod, n, bad)
    for g, p, q, b in ((1, p1, q1, b1), (2, p2, q2, b2)):
        _, st = both(eng.mul, g, s, b, False, sliced=2)
        assert [i for i in range(n) if st[i]] == ([] if bad is None else [bad])
        both(eng.mul, g, s, p[0].tobytes(), True, sliced=1)  # one base for the batch, as bytes
        both(eng.mul, g, s, p[:1].copy(), True)
        both(eng.add, g, b, q, sliced=2)
        both(eng.batch_unmarshal, g, b, sliced=1)
        both(eng.msm, g, s, b, sliced=2)
    gt, st = both(eng.batch_pair, b1, q2)
    assert bool(st.any()) == (bad is not None)
    both(eng.gt_batch_mul, t, gt, sliced=1)
    # e(s G1, t G2) == e(t G1, s G2); the undecodable lane fails with a status
    ok, st = both(eng.batch_validate_pairing, b1, q2, q1, p2, sliced=2)
    assert [int(x) for x in ok] == [0 if i == bad else 1 for i in range(n)] and bool(st.any()) == (bad is not None)
    msgs = np.random.default_rng(13).integers(0, 256, size=(n, 29), dtype=np.uint8)
    if mod is bls:
        both(bls.batch_hash_g1, msgs)
        both(bls.batch_hash_g2, msgs, b"another tag")
    else:
        both(bn256.batch_hash_g1, msgs)
        both(bn256.batch_hash_g1_svdw, msgs, b"a tag")
        both(bn256.batch_hash_g1_svdw, msgs)
