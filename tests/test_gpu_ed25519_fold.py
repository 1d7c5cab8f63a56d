"""The variable-base ladder on the word-folded nine-limb product (kyber_amd/csrc/fe29.cuh: each high column folded by
two multiply-adds) on the device: rows of random scalars against random points, an undecodable encoding in every 97th
row, outputs and status bytes against oracle/ed25519_ref.c byte for byte at flags 0, KYB_F_VARTIME and KYB_F_UNIFORM.
n = 129 runs the scratch-table instances (two blocks, the second ragged), n = 4096 + 129 the slab table and the deferred
encoder with a ragged end; the first 129 rows give the same bytes on both paths."""
import hashlib

import numpy as np
import pytest

from oracle import ed25519 as O
from tests import _oracle_c as OC

pytestmark = pytest.mark.gpu

SMALL, N = 129, 4096 + 129
ST_BAD_POINT = 1
FLAGS = [dict(), dict(vartime=True), dict(uniform=True)]
IDS = ["const", "vartime", "uniform"]


@pytest.fixture(scope="module")
def ed():
    import torch

    assert torch.cuda.is_available()
    from kyber_amd.group import edwards25519 as ed

    return ed


@pytest.fixture(scope="module")
def pool(ed):
    """N rows of (scalar, point) and the expected (out, status) for both scalar semantics"""
    raw = hashlib.shake_256(b"fe29-word-fold-gpu").digest(32 * 2 * N)
    rnd = np.frombuffer(raw, dtype=np.uint8).reshape(2 * N, 32)
    s = np.array(rnd[:N])
    p = np.asarray(ed.batch_mul_base(np.ascontiguousarray(rnd[N:]))).copy()
    y = 2
    while O.decode(y.to_bytes(32, "little")) is not None:
        y += 1
    p[5::97] = np.frombuffer(y.to_bytes(32, "little"), dtype=np.uint8)  # no square root
    want = {vt: OC.ed_mul(s, p, vartime=vt) for vt in (False, True)}
    st = want[False][1]
    assert (st == want[True][1]).all() and (st[5::97] == ST_BAD_POINT).all() and int((st != 0).sum()) == len(st[5::97])
    assert (st[:SMALL] != 0).sum() == 2 and (st[4096:] != 0).sum() == 1  # both paths and the ragged end meet some
    return s, p, want


def _run(ed, pool, n, kw):
    s, p, _ = pool
    out, st = ed.batch_mul(np.ascontiguousarray(s[:n]), np.ascontiguousarray(p[:n]), **kw)
    out, st = np.asarray(out), np.asarray(st)
    assert out.shape == (n, 32) and st.shape == (n,)
    return out, st


@pytest.mark.parametrize("kw", FLAGS, ids=IDS)
def test_both_table_paths_match_the_oracle_and_each_other(ed, pool, kw):
    exp_out, exp_st = pool[2][bool(kw.get("vartime"))]
    got = {}
    for n in (SMALL, N):
        out, st = got[n] = _run(ed, pool, n, kw)
        assert (st == exp_st[:n]).all(), (kw, n, np.nonzero(st != exp_st[:n])[0][:8])
        bad = np.nonzero((out != exp_out[:n]).any(axis=1))[0]
        assert bad.size == 0, (kw, n, bad[:8])
    assert (got[SMALL][0] == got[N][0][:SMALL]).all() and (got[SMALL][1] == got[N][1][:SMALL]).all()
