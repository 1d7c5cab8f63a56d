"""The variable-base ladder on nine-limb field elements (kyber_amd/csrc/fe29.cuh), all four instances of
ed25519_mul_kernel: outputs and status bytes against oracle/ed25519_ref.c byte for byte at flags 0, KYB_F_VARTIME and
KYB_F_UNIFORM.  Sizes 1 and 129 run the scratch-table instances (one lane; two blocks, the second ragged), 4096 is the
smallest batch on the slab table and the deferred encoder, 4096 + 129 ends that path on a ragged block.  The first rows
of the pool are every special scalar against every special point."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import ed25519 as O
from tests import _oracle_c as OC

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
N = 4096 + 129
ELL = O.L
SCALARS = [0, 1, 8, ELL - 1, ELL, 2**252 - 1, 2**252, 2**255 - 1, 2**256 - 1, int("8" * 64, 16), int("7" * 64, 16)]
ST_BAD_POINT = 1


@pytest.fixture(scope="module")
def ed():
    import torch

    assert torch.cuda.is_available()
    from kyber_amd.group import edwards25519 as ed

    return ed


def _special_points():
    """(encodings that decode, encodings with no square root)"""
    misc = json.load(open(os.path.join(G, "ed25519_misc.json")))
    le = lambda v: v.to_bytes(32, "little")
    good = [O.encode(O.B), le(1), le(O.P - 1)]  # the base point, the identity, (0, -1)
    good += [bytes.fromhex(h) for h in misc["small_order"]]
    good += [le(O.P + 1), le(O.P), le(2**255 - 1)]  # y >= p: read as y - p
    good += [le(1 | 1 << 255), le((O.P - 1) | 1 << 255)]  # x = 0 with the sign bit set
    assert all(O.decode(g) is not None for g in good)
    bad, y = [], 2
    while len(bad) < 2:
        if O.decode(le(y)) is None:
            bad += [le(y), le(y | 1 << 255)][: 2 - len(bad)]
        y += 1
    return good, bad


@pytest.fixture(scope="module")
def pool(ed):
    """N rows of (scalar, point), the expected (out, status) for both scalar semantics, and the number of leading rows
    that hold the cross of special scalars (and two random ones) with special points"""
    good, bad = _special_points()
    raw = hashlib.shake_256(b"fe29-gpu").digest(32 * 2 * N)
    rnd = np.frombuffer(raw, dtype=np.uint8).reshape(2 * N, 32)
    scalars = [s.to_bytes(32, "little") for s in SCALARS] + [bytes(rnd[0]), bytes(rnd[1])]
    rows = [(s, p) for p in good + bad for s in scalars]
    cross = len(rows)
    assert cross < 4096 - 1024
    s = np.array(rnd[:N])
    s[:cross] = np.frombuffer(b"".join(r[0] for r in rows), dtype=np.uint8).reshape(-1, 32)
    p = np.asarray(ed.batch_mul_base(np.ascontiguousarray(rnd[N:]))).copy()  # random points
    p[:cross] = np.frombuffer(b"".join(r[1] for r in rows), dtype=np.uint8).reshape(-1, 32)
    p[cross + 7::97] = np.frombuffer(bad[0], dtype=np.uint8)  # undecodable encodings among the random rows too
    want = {vt: OC.ed_mul(s, p, vartime=vt) for vt in (False, True)}
    st = want[False][1]
    assert (st == want[True][1]).all() and set(st.tolist()) == {0, ST_BAD_POINT}
    assert not want[False][0][st != 0].any()
    return s, p, want, cross, len(scalars)


FLAGS = [dict(), dict(vartime=True), dict(uniform=True)]


def _check(ed, pool, lo, n, kw):
    s, p, want, _, _ = pool
    out, st = ed.batch_mul(np.ascontiguousarray(s[lo:lo + n]), np.ascontiguousarray(p[lo:lo + n]), **kw)
    exp_out, exp_st = want[bool(kw.get("vartime"))]
    out, st = np.asarray(out), np.asarray(st)
    assert out.shape == (n, 32) and st.shape == (n,)
    assert (st == exp_st[lo:lo + n]).all(), (kw, lo, np.nonzero(st != exp_st[lo:lo + n])[0][:8])
    bad = np.nonzero((out != exp_out[lo:lo + n]).any(axis=1))[0]
    assert bad.size == 0, (kw, lo, bad[:8])


@pytest.mark.parametrize("kw", FLAGS, ids=["const", "vartime", "uniform"])
def test_one_lane_every_special_point(ed, pool, kw):
    _, _, _, cross, per_point = pool
    # one launch per special point, each with another of the scalars
    for k, lo in enumerate(range(0, cross, per_point)):
        _check(ed, pool, lo + k % per_point, 1, kw)


@pytest.mark.parametrize("kw", FLAGS, ids=["const", "vartime", "uniform"])
def test_two_blocks_scratch_table_every_special_pair(ed, pool, kw):
    _, _, _, cross, _ = pool
    for lo in range(0, cross, 129):  # windows of 129 rows over the whole cross (the last reaches into the random rows)
        _check(ed, pool, lo, 129, kw)


@pytest.mark.parametrize("n", [4096, N])
@pytest.mark.parametrize("kw", FLAGS, ids=["const", "vartime", "uniform"])
def test_slab_table_and_deferred_encoder(ed, pool, kw, n):
    _check(ed, pool, 0, n, kw)
