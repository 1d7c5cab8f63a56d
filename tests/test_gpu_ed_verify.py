"""Ed25519 fused verification (kyb_ed25519_verify), a*P + b*Q (kyb_ed25519_mul2) and their callers on the MI355X, through
the C ABI: the reference's vectors and the synthetic rejects against the oracle's restatement of VerifyWithChecks, the
composed path as a second opinion, batch sizes across the encoder's chunk and the slab's piece boundary."""
import collections
import ctypes as C
import hashlib
import random
import threading

import numpy as np
import pytest

from oracle import ed25519 as O
from tests import _ed_verify_oracle as V
from tests.test_ed_verify_host import mul2_cases, mul2_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ed():
    from kyber_amd.group import edwards25519

    return edwards25519


def _verify_host(cases, want_status=True):
    from kyber_amd import _lib

    lib = _lib.load()
    pubs, msgs, off, sigs = V.pack(cases)
    n = len(cases)
    ok, st = np.full(n, 7, dtype=np.uint8), np.full(n, 255, dtype=np.uint8)
    _lib.check(lib.kyb_ed25519_verify(n, pubs.ctypes.data, msgs.ctypes.data, off.ctypes.data, sigs.ctypes.data, ok.ctypes.data,
                                      st.ctypes.data if want_status else None, 0), "kyb_ed25519_verify")
    return ok, st


def _verify_dev(cases, want_status=True):
    import torch

    from kyber_amd import _lib

    lib = _lib.load()
    pubs, msgs, off, sigs = V.pack(cases)
    n = len(cases)
    d = [torch.from_numpy(x).cuda() for x in (pubs, msgs, off.view(np.int64), sigs)]
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 255, dtype=torch.uint8, device="cuda")
    _lib.check(lib.kyb_ed25519_verify_dev(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), ok.data_ptr(),
                                          st.data_ptr() if want_status else None, 0, torch.cuda.current_stream().cuda_stream),
               "kyb_ed25519_verify_dev")
    torch.cuda.synchronize()
    return ok.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("run", [_verify_host, _verify_dev])
@pytest.mark.parametrize("want_status", [True, False])
def test_vectors_and_synthetic_rejects_against_the_oracle(run, want_status):
    cases = V.all_cases()
    ok, st = run(cases, want_status)
    reasons = collections.Counter()
    for i, c in enumerate(cases):
        want_ok, why = V.verify_with_checks(*c)
        reasons[why] += 1
        assert ok[i] == int(want_ok), (i, why, ok[i])
        if want_status:
            assert st[i] == V.abi_status(*c), (i, why, st[i])
    for why in V.REASONS:
        if why != V.LENGTH:
            assert reasons[why] >= 1, why
    if not want_status:
        assert (st == 255).all()  # a NULL status is not written through some other pointer


def _mixed_batch(n, seed=3):
    """valid rows, each followed by copies with one flipped bit in R, S, A or the message, plus the rejects"""
    rng = random.Random(seed)
    rows = V.sign_input()
    cases = list(V.synthetic_rejects()) + [(p, m, s) for p, m, s, _ in V.wycheproof() if len(s) == 64]
    while len(cases) < n:
        pub, msg, sig = rows[rng.randrange(1, len(rows))]
        cases.append((pub, msg, sig))
        bit = rng.randrange(256)
        flip = lambda b, k: b[:k >> 3] + bytes([b[k >> 3] ^ (1 << (k & 7))]) + b[(k >> 3) + 1:]
        which = rng.randrange(4)
        if which == 0:
            cases.append((pub, msg, flip(sig, bit)))
        elif which == 1:
            cases.append((pub, msg, flip(sig, 256 + bit)))
        elif which == 2:
            cases.append((flip(pub, bit), msg, sig))
        else:
            cases.append((pub, flip(msg, rng.randrange(8 * len(msg))), sig))
    return cases[:n]


def test_callers_agree_with_the_composed_path_and_the_oracle_on_a_mixed_batch():
    from kyber_amd.sign import eddsa, schnorr

    cases = _mixed_batch(4096 + 333)  # crosses ENC_DEFER_MIN of the composed path's kernels
    cases += [(p, m, s) for p, m, s, _ in V.wycheproof() if len(s) != 64]  # lengths: the host's check
    pubs, msgs, sigs = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    fused = eddsa.batch_verify_with_checks(pubs, msgs, sigs)
    composed = eddsa._batch_verify_composed(pubs, msgs, sigs)
    want = np.array([V.verify_with_checks(*c)[0] for c in cases])
    reasons = collections.Counter(V.verify_with_checks(*c)[1] for c in cases)
    for why in V.REASONS:
        assert reasons[why] >= 1, why
    assert 1000 < want.sum() < len(cases) - 1000
    assert (fused == want).all(), np.nonzero(fused != want)[0][:10]
    assert (composed == want).all(), np.nonzero(composed != want)[0][:10]
    assert (schnorr.batch_verify_with_checks(pubs, msgs, sigs) == want).all()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096])
def test_batch_sizes(n):
    cases = _mixed_batch(n, seed=n)
    want = [int(V.verify_with_checks(*c)[0]) for c in cases]
    for run in (_verify_host, _verify_dev):
        ok, st = run(cases)
        assert list(ok) == want
        assert list(st) == [V.abi_status(*c) for c in cases]


def test_two_pieces_of_the_slab_against_the_composed_path():
    """2^18 + 77 signatures: more than one piece (ED_PIECE = 2^18 lanes).  Every 7th row has a flipped bit."""
    from kyber_amd.sign import eddsa

    rows = V.sign_input()
    n = (1 << 18) + 77
    rng = random.Random(9)
    pubs, msgs, sigs = [], [], []
    for i in range(n):
        pub, msg, sig = rows[1 + i % 383]
        if i % 7 == 3:
            k = rng.randrange(512)
            sig = sig[:k >> 3] + bytes([sig[k >> 3] ^ (1 << (k & 7))]) + sig[(k >> 3) + 1:]
        pubs.append(pub), msgs.append(msg), sigs.append(sig)
    fused = eddsa.batch_verify_with_checks(pubs, msgs, sigs)
    composed = eddsa._batch_verify_composed(pubs, msgs, sigs)
    assert hashlib.sha256(fused.astype(np.uint8).tobytes()).hexdigest() == hashlib.sha256(composed.astype(np.uint8).tobytes()).hexdigest()
    good = np.array([i % 7 != 3 for i in range(n)])
    assert fused[good].all() and not fused[~good].any()


@pytest.mark.parametrize("vartime", [False, True])
def test_mul2_equals_add_of_two_muls_and_the_oracle(ed, vartime):
    a, P, b, Q = mul2_cases()
    out, st = ed.batch_mul2(b"".join(a), b"".join(P), b"".join(b), b"".join(Q), vartime)
    x, sx = ed.batch_mul(b"".join(a), b"".join(P), vartime)
    y, sy = ed.batch_mul(b"".join(b), b"".join(Q), vartime)
    s, _ = ed.batch_add(x, y)
    bads = 0
    for i in range(len(a)):
        want = mul2_oracle(a[i], P[i], b[i], Q[i], vartime)
        if want is None:
            assert st[i] == 1 and bytes(out[i]) == bytes(32) and (sx[i] or sy[i])
            bads += 1
        else:
            assert st[i] == 0 and bytes(out[i]) == want == bytes(s[i]), i
    assert bads == 2


@pytest.mark.parametrize("vartime", [False, True])
def test_mul2_across_the_piece_boundary_host_and_device(ed, vartime):
    import torch

    n = (1 << 18) + 130
    rng = np.random.default_rng(21)
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    b = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    if vartime:
        a[::3, 16:] = 0  # short scalars: waves that start their chain lower
        b[::3, 20:] = 0
    P = ed.batch_mul_base(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))
    Q = ed.batch_mul_base(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))
    out, st = ed.batch_mul2(a, P, b, Q, vartime)
    x, _ = ed.batch_mul(a, P, vartime)
    y, _ = ed.batch_mul(b, Q, vartime)
    s, _ = ed.batch_add(x, y)
    assert not st.any() and (out == s).all()
    d = [torch.from_numpy(v).cuda() for v in (a, P, b, Q)]
    dout, dst = ed.batch_mul2(*d, vartime)
    torch.cuda.synchronize()
    assert not dst.any().item() and (dout.cpu().numpy() == s).all()
    for i in (0, 1, (1 << 18) - 1, 1 << 18, n - 1):
        assert bytes(out[i]) == mul2_oracle(bytes(a[i]), bytes(P[i]), bytes(b[i]), bytes(Q[i]), vartime)


def test_dleq_batch_verify():
    """Proofs made with the oracle: vG = v G, vH = v H, r = v - c x for any challenge c (Verify does not recompute it)."""
    from kyber_amd.proof import dleq

    rng = random.Random(17)
    n = 40
    enc = lambda k, pt=O.B: O.encode(O.mul_int(k % O.L, pt))
    cols = {k: [] for k in ("G", "H", "xG", "xH", "C", "R", "VG", "VH")}
    for _ in range(n):
        g, h, x, v, c = (rng.getrandbits(252) for _ in range(5))
        G, H = O.mul_int(g + 1, O.B), O.mul_int(h + 1, O.B)
        r = (v - c * x) % O.L
        row = {"G": O.encode(G), "H": O.encode(H), "xG": enc(x, G), "xH": enc(x, H), "C": (c % O.L).to_bytes(32, "little"),
               "R": r.to_bytes(32, "little"), "VG": enc(v, G), "VH": enc(v, H)}
        for k in cols:
            cols[k].append(row[k])
    join = lambda c: {k: b"".join(v) for k, v in c.items()}
    assert dleq.batch_verify(**join(cols)).all()
    for k in ("C", "R", "VG", "VH", "xG", "xH"):
        bad = {q: list(v) for q, v in cols.items()}
        for i in range(n):  # another valid scalar / point in its place
            bad[k][i] = (5 + i).to_bytes(32, "little") if k in "CR" else enc(1000 + i)
        assert not dleq.batch_verify(**join(bad)).any(), k
    # a non-canonical encoding of the right point is accepted (Equal compares re-encodings): y = 1 as p + 1 needs the
    # identity as vG, i.e. v = 0
    ident_nc = (O.P + 1).to_bytes(32, "little")
    G, H, x, c = O.mul_int(7, O.B), O.mul_int(9, O.B), 12345, 999
    one = {"G": O.encode(G), "H": O.encode(H), "xG": enc(x, G), "xH": enc(x, H), "C": c.to_bytes(32, "little"),
           "R": ((-c * x) % O.L).to_bytes(32, "little"), "VG": ident_nc, "VH": O.encode(O.IDENTITY)}
    assert dleq.batch_verify(**one).all()
    one["G"] = V._not_on_curve()  # an undecodable point: invalid
    assert not dleq.batch_verify(**one).any()


def test_two_host_threads_verify_at_once():
    cases_a, cases_b = _mixed_batch(6000, seed=1), _mixed_batch(5000, seed=2)
    alone = [_verify_host(cases_a), _verify_host(cases_b)]
    res = [None, None]

    def run(k, cases):
        res[k] = _verify_host(cases)

    for _ in range(3):
        ts = [threading.Thread(target=run, args=(0, cases_a), daemon=True), threading.Thread(target=run, args=(1, cases_b), daemon=True)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(120)
        assert not any(t.is_alive() for t in ts)
        for k in range(2):
            assert (res[k][0] == alone[k][0]).all() and (res[k][1] == alone[k][1]).all()
