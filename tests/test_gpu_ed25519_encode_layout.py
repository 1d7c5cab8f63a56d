"""The shared-inversion encoder (ed25519_dev.cuh ed_encode_chunk) hands a block's parked points to its lanes interleaved:
a block of ED_ENC_BLOCK lanes owns S = ED_ENC_BLOCK * ENC_CHUNK consecutive points and lane t takes base + t + j * block.
Montgomery's trick gives the same canonical bytes whatever the grouping, so every batch size at an edge of that
geometry -- a block's last and first point, a lane with one point more than its neighbour, lanes of the last block with
no point at all -- is held byte for byte, status included, against the C oracle.  Deferred encoding starts at 4 096
elements; the sizes below it run the same rows through the kernels that encode in place.

One table of rows serves every size (the first n rows): its oracle results are computed once.  The fused callers that
reach the same helper (verify, a P + b Q, DLEQ: two points per record) run once each on more than one block of their
existing case tables; the ring chain, which encodes inside its own kernel, runs one group for the record."""
import os
import re

import numpy as np
import pytest

from oracle import ed25519 as O
from tests import _oracle_c as OC

# The geometry this file is written for.  Pinned here, and held against the two constants in the sources by a test that
# needs no GPU: a change of either constant must come with the sizes below worked out again.
ENC_BLOCK, ENC_CHUNK = 64, 16
S = ENC_BLOCK * ENC_CHUNK
DEFER_MIN = 4096  # ed25519.hip ENC_DEFER_MIN
K = -(-DEFER_MIN // S)  # the smallest k with k * S >= 4 096
SIZES = sorted({DEFER_MIN, DEFER_MIN + 1, S - 1, S, S + 1, K * S + ENC_CHUNK - 1, K * S + ENC_CHUNK + 1,
                K * S + ENC_BLOCK + 5,   # last block: lanes 0 .. 4 hold two points, the others one
                K * S + S - 1,           # last block: its last lane is one point short
                K * S + 3})              # last block: lanes 3 .. 63 hold nothing
NMAX = max(SIZES)
THREADS = min(16, os.cpu_count() or 1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _le(v):
    return np.frombuffer((v % 2**256).to_bytes(32, "little"), dtype=np.uint8)


def _not_on_curve():
    for y in range(2, 100):
        if O.decode(y.to_bytes(32, "little")) is None:
            return np.frombuffer(y.to_bytes(32, "little"), dtype=np.uint8)
    raise AssertionError("no undecodable y found")


BAD = _not_on_curve()
# a chunk's first, middle and last position: the lane's points are j * ENC_BLOCK apart, lane 5 of block 0 here
BAD_ROWS = [5 + j * ENC_BLOCK for j in (0, ENC_CHUNK // 2, ENC_CHUNK - 1)]


def _table():
    """scalars and points of NMAX rows, in the order the issue lists them: 0 and l, 1, the undecodable points at the
    three positions of one lane's chunk, the rest from a labelled SHAKE stream"""
    import hashlib

    stream = np.frombuffer(hashlib.shake_256(b"kyberhip/test_gpu_ed25519_encode_layout/v1").digest(64 * NMAX), dtype=np.uint8)
    s = stream[:32 * NMAX].reshape(NMAX, 32).copy()
    k = stream[32 * NMAX:].reshape(NMAX, 32).copy()
    k[:, 31] &= 0x0F
    p = OC.ed_mul_base(k, threads=THREADS)
    s[0], s[1], s[2] = _le(0), _le(O.L), _le(1)
    for r in BAD_ROWS:
        p[r] = BAD
    return s, p


_CACHE = {}


def _ref(vartime=False):
    """(scalars, points, fixed-base bytes, variable-base bytes, variable-base status) of the whole table, once"""
    if "table" not in _CACHE:
        _CACHE["table"] = _table()
    s, p = _CACHE["table"]
    if vartime not in _CACHE:
        if vartime:  # geScalarMultVartime on the standard base: the reference of KYB_F_VARTIME's fixed-base path
            fix, fst = OC.ed_mul(s, np.tile(np.frombuffer(O.encode(O.B), dtype=np.uint8), (NMAX, 1)), vartime=True, threads=THREADS)
            assert not fst.any()
        else:
            fix = OC.ed_mul_base(s, threads=THREADS)
        var, st = OC.ed_mul(s, p, vartime=vartime, threads=THREADS)
        _CACHE[vartime] = (fix, var, st)
    return (s, p) + _CACHE[vartime]


def test_pinned_geometry_is_the_library_s_and_the_table_holds_its_rows():
    dev = open(os.path.join(ROOT, "kyber_amd", "csrc", "ed25519_dev.cuh")).read()
    launch = open(os.path.join(ROOT, "kyber_amd", "csrc", "ed25519_launch.h")).read()
    assert int(re.search(r"constexpr int ENC_CHUNK = (\d+);", dev).group(1)) == ENC_CHUNK
    assert int(re.search(r"constexpr unsigned ED_ENC_BLOCK = (\d+);", launch).group(1)) == ENC_BLOCK
    assert K * S >= DEFER_MIN > (K - 1) * S and min(SIZES) == S - 1
    # a last block with empty lanes, one with lanes of different counts, one short by a single point
    assert any(0 < n - K * S < ENC_BLOCK for n in SIZES) and any(ENC_BLOCK < n - K * S < 2 * ENC_BLOCK for n in SIZES)
    s, p, fix, var, st = _ref()
    assert bytes(fix[0]) == bytes(fix[1]) == O.encode(O.IDENTITY) and bytes(fix[2]) == O.encode(O.B)
    assert bytes(var[0]) == bytes(var[1]) == O.encode(O.IDENTITY) and bytes(var[2]) == bytes(p[2])
    assert sorted(np.nonzero(st)[0].tolist()) == BAD_ROWS and (st[BAD_ROWS] == 1).all() and not var[BAD_ROWS].any()
    assert max(BAD_ROWS) < min(SIZES) and len({r % ENC_BLOCK for r in BAD_ROWS}) == 1  # one lane's chunk, at every size
    for i in (3, 4, S, NMAX - 1):
        assert bytes(fix[i]) == O.mul_base(bytes(s[i])) and bytes(var[i]) == O.mul(bytes(s[i]), bytes(p[i])), i


@pytest.fixture(scope="module")
def ed():
    import torch

    assert torch.cuda.is_available()
    from kyber_amd.group import edwards25519 as ed

    return ed


def _run(ed, n, vartime=False, uniform=False):
    import torch

    s, p, fix, var, st = _ref(vartime)
    d_s = torch.from_numpy(np.ascontiguousarray(s[:n])).cuda()
    got_fix = ed.batch_mul_base(d_s, vartime=vartime, uniform=uniform).cpu().numpy()
    got_var, got_st = ed.batch_mul(d_s, torch.from_numpy(np.ascontiguousarray(p[:n])).cuda(), vartime=vartime, uniform=uniform)
    got_var, got_st = got_var.cpu().numpy(), got_st.cpu().numpy()
    bad = np.nonzero((got_fix != fix[:n]).any(axis=1))[0]
    assert not len(bad), ("fixed-base", n, bad[:8].tolist())
    assert (got_st == st[:n]).all(), ("status", n, np.nonzero(got_st != st[:n])[0][:8].tolist())
    bad = np.nonzero((got_var != var[:n]).any(axis=1))[0]
    assert not len(bad), ("variable-base", n, bad[:8].tolist())
    assert (got_st[BAD_ROWS] == 1).all() and not got_var[BAD_ROWS].any()  # KYB_ST_BAD_POINT, 32 zero bytes


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_every_edge_of_the_geometry_matches_the_oracle(ed, n):
    _run(ed, n)


@pytest.mark.gpu
@pytest.mark.parametrize("flag", ["vartime", "uniform"])
def test_flags_at_4097(ed, flag):
    _run(ed, DEFER_MIN + 1, vartime=flag == "vartime", uniform=flag == "uniform")


@pytest.mark.gpu
def test_verify_through_the_shared_helper_on_two_blocks():
    from tests import _ed_verify_oracle as V
    from tests.test_gpu_ed_verify import _mixed_batch, _verify_dev

    cases = _mixed_batch(S + ENC_BLOCK + 1, seed=11)  # a second block whose lane 0 holds two points, the others one
    ok, st = _verify_dev(cases)
    for i, c in enumerate(cases):
        assert ok[i] == int(V.verify_with_checks(*c)[0]) and st[i] == V.abi_status(*c), i
    assert 0 < ok.sum() < len(cases)


@pytest.mark.gpu
def test_mul2_through_the_shared_helper(ed):
    from tests.test_ed_verify_host import mul2_cases, mul2_oracle

    a, P, b, Q = mul2_cases()
    reps = -(-(S + 3) // len(a))  # the table repeated past one block
    a, P, b, Q = a * reps, P * reps, b * reps, Q * reps
    out, st = ed.batch_mul2(b"".join(a), b"".join(P), b"".join(b), b"".join(Q), False)
    want = {}
    for i in range(len(a)):
        k = i % (len(a) // reps)
        if k not in want:
            want[k] = mul2_oracle(a[i], P[i], b[i], Q[i], False)
        if want[k] is None:
            assert st[i] == 1 and bytes(out[i]) == bytes(32), i
        else:
            assert st[i] == 0 and bytes(out[i]) == want[k], i


@pytest.mark.gpu
def test_dleq_records_of_two_points_on_two_blocks(ed):
    from tests import _dleq_cases as DC
    from tests import _pvss_oracle as PO

    rows, labels = DC.cases()
    want = DC.oracle_ok(rows)
    reps = -(-(S // 2 + ENC_BLOCK + 1) // len(rows))  # a block holds S / 2 proofs: past it, into lanes of different counts
    ok, st = ed.batch_dleq_verify(*DC.pack(rows * reps))
    for i in range(len(rows) * reps):
        k = i % len(rows)
        assert bool(ok[i]) == want[k] and st[i] == PO.abi_status(*rows[k][:5]), (i, labels[k])
    assert want.any() and not want.all()


@pytest.mark.gpu
def test_ring_chain_one_group(ed):
    from tests import _ring_cases as RC
    from tests.test_gpu_anon import _chain

    exp = RC.expected(False)
    (ring, linkable), idx = sorted(RC.groups().items())[0]
    got = _chain(ed, [RC.rows()[i] for i in idx], RC.SCOPE if linkable else None, False, False)
    for i, g in zip(idx, got):
        assert g == exp[i], (ring, linkable, RC.rows()[i].label)
