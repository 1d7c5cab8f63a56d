"""kyb_ed25519_xof_pick, kyb_ed25519_theta_check and the shuffle package on the GPU: the picks against the CPU build of
the same stream (tests/shuffle_harness.cpp) and a vectorised numpy Pick, the theta kernel against the oracle and the
composed device path it replaces, the protocol layer against the sequential restatement tests/_shuffle_oracle.py."""
import ctypes as C
import random

import numpy as np
import pytest

from kyber_amd.util import blake2xb as X
from oracle import ed25519 as O
from tests import _oracle_c as OC
from tests import _shuffle_cases as SC
from tests import _shuffle_oracle as SO
from tests.test_shuffle_host import build_harness

pytestmark = pytest.mark.gpu

ROOT_HASH = X.root_hash(b"shuffle gpu tests", b"transcript bytes")
L_BE = np.frombuffer(X.ORDER.to_bytes(32, "big"), dtype=np.uint8)


@pytest.fixture(scope="module")
def ed():
    from kyber_amd.group import edwards25519

    return edwards25519


@pytest.fixture(scope="module")
def harness():
    return build_harness()


def _window(n: int) -> int:
    import math

    return 2 * n + 16 * (math.isqrt(n - 1) + 1) + 256


def _expected_picks(harness, pos: int, n: int):
    """(scalars, draws_used) of n sequential Picks from byte pos: every draw of the window, compared with l as big-endian
    byte strings, the first n accepted ones kept in order"""
    w = _window(n)
    buf = C.create_string_buffer(32 * w)
    harness.shf_stream(ROOT_HASH, pos, 32 * w, buf)
    d = np.frombuffer(buf.raw, dtype=np.uint8).reshape(w, 32).copy()
    d[:, 0] &= 0x1F
    diff = d != L_BE
    first = diff.argmax(axis=1)
    less = diff.any(axis=1) & (d[np.arange(w), first] < L_BE[first])
    idx = np.nonzero(less)[0]
    assert len(idx) >= n
    return d[idx[:n], ::-1].copy(), int(idx[n - 1]) + 1


def _sizes():
    """1, 2 and the edges of a wave of 64 draws; n whose window (always even) ends two draws below, at and two above a
    whole number of 64-draw blocks; n whose window is one block below, at and above the 256 x 64 draws after which each lane of the scan
    workgroup owns two block totals instead of one (and the same at four); 2^18 + 5"""
    sizes = {1, 2, 63, 64, 65, (1 << 18) + 5}
    for rem in (62, 0, 2):
        sizes.add(next(n for n in range(66, 4000) if _window(n) % 64 == rem))
    for blocks in (256, 1024):
        edge = max(m for m in range(1, 40000) if _window(m) <= blocks * 64)
        sizes |= {edge - 1, edge, edge + 1}
    return sorted(sizes)


SIZES = _sizes()
POSITIONS = [0, 8, 128, 40 + 64 * 7]


def test_the_pick_sizes_cover_the_block_and_scan_edges():
    assert len(SIZES) >= 15
    assert any(_window(n) <= 256 * 64 < _window(n + 1) for n in SIZES)
    assert {_window(n) % 64 for n in SIZES} >= {62, 0, 2}


@pytest.mark.parametrize("pos", POSITIONS)
def test_xof_pick_matches_sequential_picks_host_and_device(ed, harness, pos):
    import torch

    root = np.frombuffer(ROOT_HASH, dtype=np.uint8).copy()
    d_root = torch.from_numpy(root).cuda()
    for n in SIZES:
        want, used = _expected_picks(harness, pos, n)
        got, got_used = ed.batch_xof_pick(root, pos, n)
        assert got_used == used, (pos, n)
        assert (got == want).all(), (pos, n)
        d_got, d_used = ed.batch_xof_pick(d_root, pos, n)
        assert int(d_used.item()) == used, (pos, n)
        assert (d_got.cpu().numpy() == want).all(), (pos, n)
    # the first picks against the Python XOF itself
    xof = X.New(b"pick gpu")
    xof.Read(pos)
    got, used = ed.batch_xof_pick(xof.Root(), xof.Tell(), 40)
    clone = xof.Clone()
    assert b"".join(X.pick(clone.Read) for _ in range(40)) == got.tobytes() and clone.Tell() == xof.Tell() + 32 * used


def test_xof_pick_continued_across_two_calls_equals_one_call(ed):
    pos, n1, n2 = 24, 1000, 777
    one, used = ed.batch_xof_pick(ROOT_HASH, pos, n1 + n2)
    a, used_a = ed.batch_xof_pick(ROOT_HASH, pos, n1)
    b, used_b = ed.batch_xof_pick(ROOT_HASH, pos + 32 * used_a, n2)
    assert (np.concatenate([a, b]) == one).all() and used_a + used_b == used
    empty, zero = ed.batch_xof_pick(ROOT_HASH, pos, 0)
    assert empty.shape == (0, 32) and zero == 0


# ------------------------------------------------------------------------------------------------------ theta_check
def _cols(rows):
    return [np.frombuffer(b"".join(r[i] for r in rows), dtype=np.uint8).reshape(len(rows), 32).copy() for i in range(1, 6)]


@pytest.mark.parametrize("vartime", [False, True])
def test_theta_check_on_the_labelled_table_host_and_device(ed, vartime):
    import torch

    for name, u, w, rows in SC.batches():
        a, A, b, B, T = _cols(rows)
        want = [SC.expect(r[1], r[2], u, r[3], r[4], w, r[5], vartime) for r in rows]
        ok, st = ed.batch_theta_check(a, A, u, b, B, w, T, vartime=vartime)
        assert [(int(x), int(y)) for x, y in zip(ok, st)] == want, name
        dev = lambda x: None if x is None else torch.from_numpy(np.frombuffer(x, dtype=np.uint8).copy() if isinstance(x, bytes) else x).cuda()
        ok, st = ed.batch_theta_check(dev(a), dev(A), dev(u), dev(b), dev(B), dev(w), dev(T), vartime=vartime)
        assert [(int(x), int(y)) for x, y in zip(ok.cpu().numpy(), st.cpu().numpy())] == want, name


@pytest.fixture(scope="module")
def theta_pool():
    """4 099 elements with the oracle's verdicts, computed once: products by the oracle's C restatement (itself held to
    the big-integer oracle by tests/test_oracle_ed25519_c.py), sums and encodings by the big-integer oracle.  Two in
    three are valid; the rest carry a T moved by the base point."""
    n = 4099
    rng = np.random.default_rng(11)
    threads = OC.host_threads()
    sc = lambda: rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a, b = sc(), sc()
    a[:, 31] &= 0x7F  # below 2^255: one value under both flags
    a[::5, 31] &= 0x0F
    ka, kb = sc(), sc()
    ka[:, 31] &= 0x0F
    kb[:, 31] &= 0x0F
    A, B = OC.ed_mul_base(ka, threads), OC.ed_mul_base(kb, threads)
    U, W = SC._pt(0xABCDEF0123), SC._pt(0x9876543210FF)
    add = lambda p, q: O.encode(O.add(O.decode(bytes(p)), O.decode(bytes(q))))
    xhat = np.frombuffer(b"".join(add(p, U) for p in A), dtype=np.uint8).reshape(n, 32)
    yhat = np.frombuffer(b"".join(add(p, W) for p in B), dtype=np.uint8).reshape(n, 32)
    nb = np.frombuffer(b"".join(SC.sc(-int.from_bytes(bytes(x), "little")) for x in b), dtype=np.uint8).reshape(n, 32)
    P, st1 = OC.ed_mul(a, xhat, False, threads)
    Q, st2 = OC.ed_mul(nb, yhat, False, threads)
    assert not st1.any() and not st2.any()
    one = SC._pt(1)
    T, want = [], []
    for i in range(n):
        t = add(P[i], Q[i])
        valid = i % 3 != 2
        T.append(t if valid else add(t, one))
        want.append(int(valid))
    T = np.frombuffer(b"".join(T), dtype=np.uint8).reshape(n, 32).copy()
    for i in (0, 1, 2, 2048, n - 1):  # and the big-integer oracle's own word on a few
        assert SC.expect(bytes(a[i]), bytes(A[i]), U, bytes(b[i]), bytes(B[i]), W, bytes(T[i]), False) == (want[i], 0)
    return a, A, U, b, B, W, T, np.array(want, dtype=np.uint8)


@pytest.mark.parametrize("n", [1, 2, 127, 128, 129, 4099])
def test_theta_check_matches_the_oracle_at_block_edges(ed, theta_pool, n):
    a, A, U, b, B, W, T, want = theta_pool
    for vartime in (False, True):
        ok, st = ed.batch_theta_check(a[-n:], A[-n:], U, b[-n:], B[-n:], W, T[-n:], vartime=vartime)
        assert not st.any() and (ok == want[-n:]).all(), (n, vartime)


def test_theta_check_across_pieces_matches_the_composed_device_path(ed, theta_pool):
    """2^18 + 5 lanes: add, add, mul2 and a byte comparison on the device -- calls the oracle tests hold on their own"""
    import torch

    a, A, U, b, B, W, T, want = theta_pool
    n = (1 << 18) + 5
    reps = -(-n // len(a))
    tile = lambda x: torch.from_numpy(np.tile(x, (reps, 1))[:n].copy()).cuda()
    rng = np.random.default_rng(3)
    d_a = torch.from_numpy(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)).cuda()  # any 32 bytes: unreduced, >= 2^255
    d_b = torch.from_numpy(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)).cuda()
    d_A, d_B, d_T = tile(A), tile(B), tile(T)
    d_U = torch.from_numpy(np.frombuffer(U, dtype=np.uint8).copy()).cuda()
    d_W = torch.from_numpy(np.frombuffer(W, dtype=np.uint8).copy()).cuda()
    nb = np.frombuffer(b"".join(SC.sc(-int.from_bytes(x.tobytes(), "little")) for x in d_b.cpu().numpy()), dtype=np.uint8).reshape(n, 32)
    d_nb = torch.from_numpy(nb.copy()).cuda()
    for vartime in (False, True):
        xhat, s1 = ed.batch_add(d_A, d_U.expand(n, 32).contiguous())
        yhat, s2 = ed.batch_add(d_B, d_W.expand(n, 32).contiguous())
        lhs, s3 = ed.batch_mul2(d_a, xhat, d_nb, yhat, vartime=vartime)
        assert not (s1.any() or s2.any() or s3.any()).item()
        T2 = d_T.clone()
        T2[::2] = lhs[::2]  # every other element valid under this flag
        want2 = (lhs == T2).all(dim=1).to(torch.uint8)
        ok, st = ed.batch_theta_check(d_a, d_A, d_U, d_b, d_B, d_W, T2, vartime=vartime)
        assert not st.any().item() and (ok == want2).all().item(), vartime
        assert want2[::2].all().item() and int(want2.sum().item()) < n
        for i in (0, (1 << 18) - 1, 1 << 18, n - 1):
            assert int(ok[i].item()) == int(want2[i].item())


def test_theta_check_without_shared_points_is_mul2_with_the_negated_scalar(ed, theta_pool):
    a, A, _, b, B, _, _, _ = theta_pool
    n = 1000
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    nb = np.frombuffer(b"".join(SC.sc(-int.from_bytes(bytes(x), "little")) for x in b[:n]), dtype=np.uint8).reshape(n, 32)
    for vartime in (False, True):
        T, st = ed.batch_mul2(a, A[:n], nb, B[:n], vartime=vartime)
        assert not st.any()
        T = T.copy()
        T[1::4, 0] ^= 1
        ok, st = ed.batch_theta_check(a, A[:n], None, b[:n], B[:n], None, T, vartime=vartime)
        want = np.ones(n, dtype=np.uint8)
        want[1::4] = 0
        assert not st.any() and (ok == want).all(), vartime


# ------------------------------------------------------------------------------------------------------ end to end
def _pairs(k: int, H):
    """k ElGamal pairs under H, by the oracle's C restatement (any points would do: the proof is about the shuffle)"""
    rng = np.random.default_rng(k)
    r = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
    r[:, 31] &= 0x0F
    m = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
    m[:, 31] &= 0x0F
    threads = OC.host_threads()
    Xs = OC.ed_mul_base(r, threads)
    rH, _ = OC.ed_mul(r, np.tile(np.frombuffer(H, dtype=np.uint8), (k, 1)), False, threads)
    M = OC.ed_mul_base(m, threads)
    Ys = np.frombuffer(b"".join(SO.padd(p, q) for p, q in zip(rH, M)), dtype=np.uint8).reshape(k, 32)
    return Xs, Ys


def _rows(x):
    return [bytes(r) for r in x]


def _products(scalars, points):
    """the oracle verifier's products of one loop in one batch, by the oracle's C restatement (tests/_oracle_c.py)"""
    base = np.frombuffer(O.encode(O.B), dtype=np.uint8)
    s = np.frombuffer(b"".join(scalars), dtype=np.uint8).reshape(-1, 32)
    p = np.stack([base if q is None else np.frombuffer(q, dtype=np.uint8) for q in points])
    out, st = OC.ed_mul(s, p, False, OC.host_threads())
    assert not st.any()
    return _rows(out)


@pytest.mark.parametrize("k,given_g", [(2, False), (2, True), (3, False), (3, True), (5, False), (5, True), (130, True)])
def test_shuffle_prove_verify_equal_the_oracle_byte_for_byte(k, given_g):
    """At k = 130 the oracle still proves element by element in Python integers; its verifications take their products
    in batches, and only the reference's own tampering is replayed."""
    from kyber_amd import shuffle
    from kyber_amd.proof import hash as PH

    G = SO.pmul(SO.sc(7), None) if given_g else None
    H = SO.pmul(SO.sc(0x1234567), G)
    Xs, Ys = _pairs(k, H)
    seed = b"e2e %d" % k
    # the engine: Shuffle -> HashProve -> Verifier -> HashVerify
    rand = X.New(seed)
    suite = PH.NewBlakeSHA256Ed25519WithRand(rand)
    Xbar, Ybar, prover = shuffle.Shuffle(suite, G, H, Xs, Ys, rand)
    proof = PH.HashProve(suite, "PairShuffle", prover)
    PH.HashVerify(suite, "PairShuffle", shuffle.Verifier(suite, G, H, Xs, Ys, Xbar, Ybar), proof)
    # the oracle on the same streams: the same pairs, the same proof bytes
    orand = X.New(seed)
    oXbar, oYbar, oprover = SO.shuffle(G, H, _rows(Xs), _rows(Ys), orand.Read)
    oproof = SO.hash_prove(b"PairShuffle", oprover, orand.Read)
    assert _rows(Xbar) == oXbar and _rows(Ybar) == oYbar
    assert proof == oproof
    with SO.many_products(_products if k > 5 else SO._pmul_each):
        assert SO.hash_verify(b"PairShuffle", SO.verifier(G, H, _rows(Xs), _rows(Ys), oXbar, oYbar), proof) is None
    # the reference's tampering (shuffle_test.go:97-115) and the transcript's: same verdicts, same messages
    swapped = np.concatenate([Xbar[1:2], Xbar[0:1], Xbar[2:]])
    bad = SC._off_curve(random.Random(k))
    scalar_at = 32 * (5 * k + 3)  # sigma_0: a moved scalar leaves every point decodable
    cases = {
        "swapped": (swapped, proof, "PairShuffle"),
        "truncated": (Xbar, proof[:-1], "PairShuffle"),
        "trailing": (Xbar, proof + b"xyz", "PairShuffle"),
        "protocol": (Xbar, proof, "pairShuffle"),
        "bad point": (Xbar, proof[:32 * 5] + bad + proof[32 * 6:], "PairShuffle"),
        "bad point and truncated": (Xbar, (proof[:32 * 5] + bad + proof[32 * 6:])[:32 * 40 + 7], "PairShuffle"),
        "sigma moved": (Xbar, proof[:scalar_at] + bytes([proof[scalar_at] ^ 1]) + proof[scalar_at + 1:], "PairShuffle"),
        "alpha moved": (Xbar, proof[:-32] + bytes([proof[-32] ^ 1]) + proof[-31:], "PairShuffle"),
    }
    if k > 5:
        cases = {"swapped": cases["swapped"]}
    seen = {None}
    for name, (xb, pf, proto) in cases.items():
        with SO.many_products(_products if k > 5 else SO._pmul_each):
            want = SO.hash_verify(proto.encode(), SO.verifier(G, H, _rows(Xs), _rows(Ys), _rows(xb), oYbar), pf)
        try:
            PH.HashVerify(suite, proto, shuffle.Verifier(suite, G, H, Xs, Ys, xb, Ybar), pf)
            got = None
        except PH.ProofError as e:
            got = str(e)
        assert got == want, (name, got, want)
        seen.add(want)
    assert SO.ERR_PAIR in seen and (k > 5 or {None, SO.ERR_SIMPLE, SO.ERR_POINT, SO.ERR_SHORT} <= seen)


def test_sequences_shuffle_matches_the_oracle_and_rejects_a_corrupted_input():
    from kyber_amd import shuffle
    from kyber_amd.proof import hash as PH

    NQ, k = 6, 5
    H = SO.pmul(SO.sc(0x7654321), None)
    cols = [_pairs(k + j, H) for j in range(NQ)]
    Xs = np.stack([c[0][:k] for c in cols])
    Ys = np.stack([c[1][:k] for c in cols])
    rand = X.New(b"sequences gpu")
    suite = PH.NewBlakeSHA256Ed25519WithRand(rand)
    xbar, ybar, get_prover = shuffle.SequencesShuffle(suite, None, H, Xs, Ys, rand)
    e = PH.picks(rand, NQ)
    proof = PH.HashProve(suite, "PairShuffle", get_prover(e))
    up = shuffle.GetSequenceVerifiable(suite, Xs, Ys, xbar, ybar, e)
    PH.HashVerify(suite, "PairShuffle", shuffle.Verifier(suite, None, H, *up), proof)
    # the oracle, same stream
    grid = lambda M: [_rows(r) for r in M]
    orand = X.New(b"sequences gpu")
    oxbar, oybar, oget = SO.sequences_shuffle(None, H, grid(Xs), grid(Ys), orand.Read)
    oe = [SO.pick(orand.Read) for _ in range(NQ)]
    assert grid(xbar) == oxbar and grid(ybar) == oybar and [SO.sc(v) for v in oe] == _rows(e)
    assert SO.hash_prove(b"PairShuffle", oget(oe), orand.Read) == proof
    oup = SO.get_sequence_verifiable(grid(Xs), grid(Ys), oxbar, oybar, _rows(e))
    assert [_rows(v) for v in up] == list(oup)
    # a corrupted sequence input (shuffle_test.go:192-221)
    Xs[1, 0] = np.frombuffer(SO.pmul(SO.sc(12345), None), dtype=np.uint8)
    up = shuffle.GetSequenceVerifiable(suite, Xs, Ys, xbar, ybar, e)
    with pytest.raises(PH.ProofError, match=SO.ERR_PAIR):
        PH.HashVerify(suite, "PairShuffle", shuffle.Verifier(suite, None, H, *up), proof)


def test_round_trip_at_4099_pairs_with_the_oracles_verdict_on_the_engines_proof():
    from kyber_amd import shuffle
    from kyber_amd.proof import hash as PH

    k = 4099
    H = SO.pmul(SO.sc(0x1234567), None)
    Xs, Ys = _pairs(k, H)
    rand = X.New(b"e2e 4099")
    suite = PH.NewBlakeSHA256Ed25519WithRand(rand)
    Xbar, Ybar, prover = shuffle.Shuffle(suite, None, H, Xs, Ys, rand)
    proof = PH.HashProve(suite, "PairShuffle", prover)
    assert len(proof) == 32 * (12 * k + 3)
    PH.HashVerify(suite, "PairShuffle", shuffle.Verifier(suite, None, H, Xs, Ys, Xbar, Ybar), proof)
    swapped = np.concatenate([Xbar[1:2], Xbar[0:1], Xbar[2:]])
    with pytest.raises(PH.ProofError, match=SO.ERR_PAIR):
        PH.HashVerify(suite, "PairShuffle", shuffle.Verifier(suite, None, H, Xs, Ys, swapped, Ybar), proof)
    at = 32 * (5 * k + 3 + 7)  # sigma_7: hashed into the simple k-shuffle's challenges, so that proof fails first
    with pytest.raises(PH.ProofError, match=SO.ERR_SIMPLE):
        PH.HashVerify(suite, "PairShuffle", shuffle.Verifier(suite, None, H, Xs, Ys, Xbar, Ybar),
                      proof[:at] + bytes([proof[at] ^ 1]) + proof[at + 1:])
    # the oracle's verdict on the proof the engine produced; its products in batches by the oracle's C restatement
    with SO.many_products(_products):
        assert SO.hash_verify(b"PairShuffle", SO.verifier(None, H, _rows(Xs), _rows(Ys), _rows(Xbar), _rows(Ybar)), proof) is None
