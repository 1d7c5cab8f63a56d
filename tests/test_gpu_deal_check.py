"""kyb_ed25519_deal_check on the GPU against the big-integer oracle (tests/_dkg_cases.py over oracle/ed25519.py) and
against the composed standing calls it replaces (batch_mul_base bytes equal to poly_eval bytes): thresholds 0 to 17,
tables of 1 to 65 polynomials, batches either side of the block of 64, several checks per polynomial and polynomials
nobody names, the indices up to 2^32 - 1, the share table, commitments off the subgroup or written non-canonically, one
undecodable commitment, the device entry on tensors, the argument error of the host entry."""
import random

import numpy as np
import pytest

from kyber_amd import _lib
from tests import _dkg_cases as DC
from tests import _oracle_c as OC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ed():
    from kyber_amd.group import edwards25519

    return edwards25519


def _table(m: int, t: int, seed: int):
    """m polynomials of t coefficients: (secret coefficients or None where a commitment is special, commitments)"""
    rng = random.Random(seed)
    coeffs = [[rng.randrange(DC.L) for _ in range(t)] for _ in range(m)]
    flat = np.frombuffer(b"".join(DC.le(c) for row in coeffs for c in row), dtype=np.uint8).reshape(-1, 32)
    commits = OC.ed_mul_base(flat, threads=4).reshape(m, t, 32).copy() if m * t else np.zeros((m, t, 32), dtype=np.uint8)
    known = [True] * m
    if t >= 2 and m >= 2:  # polynomial 1: a commitment with an order-8 component, one written non-canonically
        commits[1, t - 1] = np.frombuffer(DC.ORDER8, dtype=np.uint8)
        commits[1, 0] = np.frombuffer(DC.NONCANONICAL, dtype=np.uint8)
        known[1] = False
    if t >= 1 and m >= 3:  # polynomial 2: all identities, the share 0
        commits[2, :] = np.frombuffer(DC.IDENTITY, dtype=np.uint8)
        coeffs[2] = [0] * t
    return coeffs, known, commits


def _checks(n: int, m: int, t: int, coeffs, known, seed: int):
    """n checks: polynomials drawn with repeats from all but the last (nobody names it when m > 1), the indices and the
    share table cycled"""
    rng = random.Random(seed)
    named = list(range(m - 1)) if m > 1 else [0]
    poly, idx, shares, labels = [], [], [], []
    for i in range(n):
        k = named[i % len(named)] if i < 2 * len(named) else rng.choice(named)
        ix = DC.INDICES[(i // 2) % len(DC.INDICES)]
        rows = DC.share_table(coeffs[k], ix)
        label, share = rows[(i * 7 + i // 5) % len(rows)]
        poly.append(k)
        idx.append(ix)
        shares.append(share)
        labels.append(label if known[k] else "special")
    return poly, idx, shares, labels


def _expected(poly, idx, shares, commits):
    evals = {}
    want = []
    for k, ix, s in zip(poly, idx, shares):
        if (k, ix) not in evals:
            evals[(k, ix)] = DC.eval_commits([bytes(c) for c in commits[k]], ix)
        v = evals[(k, ix)]
        want.append(int(v is not None and bytes(OC.ed_mul_base(np.frombuffer(s, dtype=np.uint8), threads=1)[0]) == v))
    return want, evals


SHAPES = [(0, 1, 1), (0, 2, 65), (1, 1, 63), (1, 2, 64), (2, 2, 65), (2, 65, 129), (3, 1, 129), (3, 65, 64), (17, 2, 63),
          (17, 65, 129), (17, 1, 1)]


@pytest.mark.parametrize("t,m,n", SHAPES)
def test_deal_check_matches_the_oracle_and_the_composed_calls(ed, t, m, n):
    coeffs, known, commits = _table(m, t, 100 * t + m)
    poly, idx, shares, labels = _checks(n, m, t, coeffs, known, n)
    want, evals = _expected(poly, idx, shares, commits)
    ok, st = ed.batch_deal_check(poly, idx, b"".join(shares), commits.reshape(-1, 32), m, t)
    assert not np.asarray(st).any() and len(st) == m
    assert list(ok) == want
    for i, label in enumerate(labels):  # what the table promises, whatever the oracle computed
        if label in ("right", "right + l"):
            assert ok[i] == 1, (i, label)
        if label == "right + 1":
            assert ok[i] == 0, i
    if n > 8:
        assert 0 in want and 1 in want
    # the composed standing calls: mul_base bytes against poly_eval bytes
    left = ed.batch_mul_base(b"".join(shares))
    for k in sorted(set(poly)):
        rows = [i for i in range(n) if poly[i] == k]
        right, pst = ed.poly_eval(commits[k].reshape(-1, 32) if t else b"", [idx[i] for i in rows])
        assert not np.asarray(pst).any()
        for j, i in enumerate(rows):
            assert bytes(right[j]) == evals[(k, idx[i])]
            assert int(bytes(left[i]) == bytes(right[j])) == ok[i], (k, i)


def test_one_undecodable_commitment_fails_its_polynomial_only(ed):
    t, m, n = 3, 65, 129
    coeffs, known, commits = _table(m, t, 9)
    poly, idx, shares, _ = _checks(n, m, t, coeffs, known, 9)
    good, _ = ed.batch_deal_check(poly, idx, b"".join(shares), commits.reshape(-1, 32), m, t)
    k = next(p for p, g in zip(poly, good) if g and p > 2)  # a polynomial with a check that passes so far
    commits[k, 1] = np.frombuffer(DC.UNDECODABLE, dtype=np.uint8)
    ok, st = ed.batch_deal_check(poly, idx, b"".join(shares), commits.reshape(-1, 32), m, t)
    assert list(st) == [_lib.ST_BAD_POINT if j == k else 0 for j in range(m)]
    assert list(ok) == [0 if p == k else g for p, g in zip(poly, good)]


def test_device_entry_on_tensors_and_a_polynomial_index_off_the_table(ed):
    import torch

    t, m, n = 3, 2, 65
    coeffs, known, commits = _table(m, t, 21)
    poly, idx, shares, _ = _checks(n, m, t, coeffs, known, 21)
    want, _ = _expected(poly, idx, shares, commits)
    poly[7], want[7] = m, 0  # off the table: ok = 0, nothing read
    poly[9], want[9] = 2**32 - 1, 0
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ok, st = ed.batch_deal_check(dev(np.asarray(poly, dtype=np.uint32).view(np.int32)), dev(np.asarray(idx, dtype=np.uint32).view(np.int32)),
                                 dev(np.frombuffer(b"".join(shares), dtype=np.uint8).copy()), dev(commits.reshape(-1, 32)), m, t)
    torch.cuda.synchronize()
    assert list(ok.cpu().numpy()) == want and not st.cpu().numpy().any()
    # the host entry refuses the same before any device work
    with pytest.raises(_lib.KyberHipError, match="rc=-1"):
        ed.batch_deal_check(poly, idx, b"".join(shares), commits.reshape(-1, 32), m, t)
