"""kyb_ed25519_ecies_seal / _open on the GPU against the sequential restatement tests/_ecies_oracle.py (points by the
oracle's C restatement, AES-GCM and HKDF in Python): every plaintext length of the block edges mixed in one batch, batch
sizes either side of the wave and the block, one recipient or one per element, recipients that are the identity, of order
8, written non-canonically or no point at all; opens of the sealed, the tampered and the short; the device entries on
tensors; one batch across the piece boundary."""
import hashlib
import random

import numpy as np
import pytest

from kyber_amd import _lib
from tests import _dkg_cases as DC
from tests import _ecies_oracle as EO
from tests import _oracle_c as OC

pytestmark = pytest.mark.gpu

POOL = 300
SIZES = (1, 63, 64, 65, 127, 128, 129, 300)


@pytest.fixture(scope="module")
def ed():
    from kyber_amd.group import edwards25519

    return edwards25519


def _scalars(tag: bytes, n: int) -> np.ndarray:
    raw = hashlib.shake_256(tag).digest(32 * n)
    s = np.frombuffer(raw, dtype=np.uint8).reshape(n, 32).copy()
    s[:, 31] &= 0x0F
    return s


def _seal_expected(r, pubs, msgs):
    """EO.encrypt for a batch, its two scalar multiplications by the oracle's C restatement"""
    R = OC.ed_mul_base(r, threads=4)
    dh, st = OC.ed_mul(r, pubs, threads=4)
    out = []
    for i, m in enumerate(msgs):
        if st[i]:
            out.append(None)
            continue
        key, nonce = EO.derive(bytes(dh[i]))
        out.append(bytes(R[i]) + EO.gcm_seal(key, nonce, m))
    return out


def _msgs(n: int, tag: bytes):
    return [hashlib.shake_256(tag + b" %d" % i).digest(EO.LENGTHS[i % len(EO.LENGTHS)]) for i in range(n)]


@pytest.fixture(scope="module")
def pool():
    """POOL elements, each with its own recipient and a length cycling through LENGTHS; four special recipients planted"""
    r = _scalars(b"ecies gpu r", POOL)
    x = _scalars(b"ecies gpu x", POOL)
    pubs = OC.ed_mul_base(x, threads=4)
    special = {POOL - 2: DC.IDENTITY, POOL - 7: DC.ORDER8, POOL - 40: DC.NONCANONICAL, POOL - 66: DC.UNDECODABLE, 3: DC.UNDECODABLE}
    for i, p in special.items():
        pubs[i] = np.frombuffer(p, dtype=np.uint8)
    msgs = _msgs(POOL, b"ecies gpu msg")
    want = _seal_expected(r, pubs, msgs)
    assert [i for i, w in enumerate(want) if w is None] == [3, POOL - 66]
    assert want[0] == EO.encrypt(bytes(r[0]), bytes(pubs[0]), msgs[0])  # the batch helper is the oracle's Encrypt
    return r, x, pubs, msgs, want, special


@pytest.fixture(scope="module")
def pool_one():
    """POOL elements for ONE recipient"""
    r = _scalars(b"ecies gpu r one", POOL)
    x = _scalars(b"ecies gpu x one", 1)
    pub = OC.ed_mul_base(x, threads=1)
    msgs = _msgs(POOL, b"ecies gpu one")
    want = _seal_expected(r, np.repeat(pub, POOL, axis=0), msgs)
    return r, x, pub, msgs, want


def _check_seal(ctx, st, want, msgs):
    for i, w in enumerate(want):
        if w is None:
            assert st[i] == _lib.ST_BAD_POINT and ctx[i] == bytes(len(msgs[i]) + 48), i
        else:
            assert st[i] == 0 and ctx[i] == w, i


@pytest.mark.parametrize("n", SIZES)
def test_seal_and_open_per_recipient_match_the_oracle(ed, pool, n):
    r, x, pubs, msgs, want, _ = pool
    ctx, st = ed.batch_ecies_seal(r[-n:], pubs[-n:], msgs[-n:])
    _check_seal(ctx, st, want[-n:], msgs[-n:])
    back, st2 = ed.batch_ecies_open(x[-n:], [w if w is not None else bytes(len(m) + 48) for w, m in zip(want[-n:], msgs[-n:])])
    for k in range(n):
        i = POOL - n + k
        if want[i] is None:  # zero bytes: an R that decodes, so the oracle says the tag fails
            assert (st2[k], back[k]) == (EO.decrypt(bytes(x[i]), bytes(len(msgs[i]) + 48))[1], b"") and st2[k] == _lib.ST_ECIES_AUTH, i
        elif i in pool[5]:
            # a special recipient has no private key here: its ciphertext opens only to a failure under x[i]
            assert (st2[k], back[k]) == (EO.decrypt(bytes(x[i]), want[i])[1], b""), i
        else:
            assert st2[k] == 0 and back[k] == msgs[i], i


@pytest.mark.parametrize("n", SIZES)
def test_seal_and_open_for_one_recipient_match_the_oracle(ed, pool_one, n):
    r, x, pub, msgs, want = pool_one
    ctx, st = ed.batch_ecies_seal(r[:n], pub, msgs[:n])
    _check_seal(ctx, st, want[:n], msgs[:n])
    back, st2 = ed.batch_ecies_open(x, want[:n])
    assert not np.asarray(st2).any() and back == msgs[:n]


def test_open_of_tampered_and_short_elements_matches_the_oracle(ed, pool_one):
    r, x, pub, msgs, want = pool_one
    rng = random.Random(7)
    cases = []
    for i in range(2 * len(EO.LENGTHS)):  # every length twice over
        c = want[i]
        ats = [32, len(c) - 17, len(c) - 1] if len(msgs[i]) else [len(c) - 1]
        for at in ats:  # first / last ciphertext byte, last tag byte
            b = bytearray(c)
            b[at] ^= 1 << rng.randrange(8)
            cases.append(bytes(b))
        b = bytearray(c)
        b[0] ^= 1 << rng.randrange(8)  # R: another point, or none
        cases.append(bytes(b))
        cases.append(c)  # an untouched one in between
    cases += [want[40][:k] for k in (0, 31, 32, 47)] + [DC.UNDECODABLE + want[5][32:], want[0]]
    rng.shuffle(cases)
    back, st = ed.batch_ecies_open(x, cases)
    seen = set()
    for i, c in enumerate(cases):
        msg, code = EO.decrypt(bytes(x[0]), c)
        assert st[i] == code and back[i] == (msg if msg is not None else b""), (i, len(c))
        seen.add(code)
    assert seen == {0, _lib.ST_BAD_POINT, _lib.ST_ECIES_SHORT, _lib.ST_ECIES_AUTH}
    # the raw slots: zero bytes wherever the status is not 0 (the wrapper above would hide a stray byte)
    blob = np.frombuffer(b"".join(cases), dtype=np.uint8)
    off = np.zeros(len(cases) + 1, dtype=np.uint64)
    np.cumsum([len(c) for c in cases], out=off[1:])
    out, st3 = np.full(len(blob), 0xEE, dtype=np.uint8), np.zeros(len(cases), dtype=np.uint8)
    lib = _lib.load()
    xs = np.ascontiguousarray(x)
    _lib.check(lib.kyb_ed25519_ecies_open(len(cases), xs.ctypes.data, 0, blob.ctypes.data, off.ctypes.data, out.ctypes.data,
                                          st3.ctypes.data), "open")
    for i, c in enumerate(cases):
        msg, _ = EO.decrypt(bytes(x[0]), c)
        slot = bytes(out[int(off[i]):int(off[i + 1])])
        assert slot == (msg or b"") + bytes(len(c) - len(msg or b"")), i


def test_device_entries_on_tensors(ed, pool, pool_one):
    import torch

    r, x, pubs, msgs, want, _ = pool
    n = 129
    blob = torch.from_numpy(np.frombuffer(b"".join(msgs[:n]), dtype=np.uint8).copy()).cuda()
    off = torch.from_numpy(np.cumsum([0] + [len(m) for m in msgs[:n]]).astype(np.int64)).cuda()
    (cblob, coff), st = ed.batch_ecies_seal(torch.from_numpy(r[:n]).cuda(), torch.from_numpy(pubs[:n]).cuda(), (blob, off))
    torch.cuda.synchronize()
    cb, co, st = cblob.cpu().numpy(), coff.cpu().numpy(), st.cpu().numpy()
    ctx = [bytes(cb[co[i]:co[i + 1]]) for i in range(n)]
    _check_seal(ctx, st, want[:n], msgs[:n])
    (pblob, poff), st2 = ed.batch_ecies_open(torch.from_numpy(x[:n]).cuda(), (cblob, coff))
    torch.cuda.synchronize()
    pb, st2 = pblob.cpu().numpy(), st2.cpu().numpy()
    for i in range(n):
        slot = bytes(pb[co[i]:co[i + 1]])
        if want[i] is None or i in pool[5]:  # the zeroed slot of a refused seal, or a key nobody here holds
            assert st2[i] == EO.decrypt(bytes(x[i]), ctx[i])[1] != 0 and slot == bytes(len(slot)), i
        else:
            assert st2[i] == 0 and slot == msgs[i] + bytes(48), i
    # one receiver (stride 0) on the device
    r1, x1, pub1, msgs1, want1 = pool_one
    cb1 = torch.from_numpy(np.frombuffer(b"".join(want1[:65]), dtype=np.uint8).copy()).cuda()
    co1 = torch.from_numpy(np.cumsum([0] + [len(c) for c in want1[:65]]).astype(np.int64)).cuda()
    (pb1, _), st3 = ed.batch_ecies_open(torch.from_numpy(x1).cuda(), (cb1, co1))
    torch.cuda.synchronize()
    pb1, co1 = pb1.cpu().numpy(), co1.cpu().numpy()
    assert not st3.cpu().numpy().any()
    assert [bytes(pb1[co1[i]:co1[i + 1] - 48]) for i in range(65)] == msgs1[:65]


def test_a_batch_across_the_piece_boundary_round_trips_on_the_device(ed):
    """2^18 + 5 elements of 32 bytes: sealed, then opened, on the device; every message must come back.  The oracle is
    compared at the elements around the boundary and at 64 seeded random ones (pure Python cannot do 2^18 in seconds)."""
    import torch

    n = (1 << 18) + 5
    g = torch.Generator(device="cpu").manual_seed(11)
    r = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
    r[:, 31] &= 0x0F
    msgs = torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g)
    x = _scalars(b"ecies gpu piece x", 1)
    pub = OC.ed_mul_base(x, threads=1)
    off = (torch.arange(n + 1, dtype=torch.int64) * 32).cuda()
    (cblob, coff), st = ed.batch_ecies_seal(r.cuda(), torch.from_numpy(pub).cuda(), (msgs.cuda().view(-1), off))
    (pblob, _), st2 = ed.batch_ecies_open(torch.from_numpy(x).cuda(), (cblob, coff))
    torch.cuda.synchronize()
    assert not st.any().item() and not st2.any().item()
    slots = pblob.view(n, 80)
    assert torch.equal(slots[:, :32].cpu(), msgs) and not slots[:, 32:].any().item()
    sample = sorted({0, 1, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, n - 1} | set(random.Random(5).sample(range(n), 64)))
    ctx = cblob.view(n, 80)[torch.tensor(sample).cuda()].cpu().numpy()
    rs, ms = r.numpy()[sample], msgs.numpy()[sample]
    want = _seal_expected(rs, np.repeat(pub, len(sample), axis=0), [bytes(m) for m in ms])
    for k, i in enumerate(sample):
        assert bytes(ctx[k]) == want[k], i
