"""The fixed-base kernels read their comb digits from a shifted pack of nibbles (ed25519_dev.cuh EdCombDigits), the
last positions -- which hold e[63] and e[64] -- by constant index, and the variable-base kernel builds its window
table by mixed additions (ge_window_table<AFFINE>).  Every position, the tail positions, the top digit that does not
fit a nibble (e[63] = 8) and the carry digit e[64] are held byte for byte against the C oracle, under flags 0,
KYB_F_VARTIME and KYB_F_UNIFORM, with the standard base (G = 4 comb, G = 1 scan) and a shared base (G = 2).

One set of 242 scalars serves every test; its oracle results are computed once per (base, semantics) and indexed."""
import os

import numpy as np
import pytest

from oracle import ed25519 as O
from tests import _oracle_c as OC

THREADS = min(16, os.cpu_count() or 1)
B_ENC = np.frombuffer(O.encode(O.B), dtype=np.uint8)
FLAGS = [(False, False), (True, False), (False, True)]  # (vartime, uniform): 0, KYB_F_VARTIME, KYB_F_UNIFORM
FLAG_IDS = ["ct", "vartime", "uniform"]


def _le(v):
    return list((v % 2**256).to_bytes(32, "little"))


def _scalar_set():
    vals = [0, 1, O.L - 1, O.L, 2**252 - 1]
    vals.append(int("88" * 32, 16))  # every digit -8 with a carry into the next; under KYB_F_VARTIME e[64] = 1
    vals.append(int("77" * 32, 16))
    vals += [int("ff" * 32, 16), 2**255 + 1]  # >= 2^255: e[63] = 8 + ... on the constant path, dropped when > 8
    vals.append(2**255)  # e[63] = 8 exactly: the digit that does not fit a nibble, kept by the reference
    # one position of the G = 4 comb at a time (16 positions have nibbles of their own; position 16 holds only the
    # carry digit e[64], which 0x8888 at position 15, 0x88.. and 0xff.. produce under KYB_F_VARTIME)
    vals += [0x8888 << (16 * k) for k in range(16)] + [0x0001 << (16 * k) for k in range(16)]
    rows = [_le(v) for v in vals]
    rnd = np.random.default_rng(0xD161).integers(0, 256, size=(200, 32), dtype=np.uint8)  # all 256 bits random
    return np.concatenate([np.array(rows, dtype=np.uint8), rnd])


SET = _scalar_set()


def _order8_point():
    """An encoded point of order 8: l * Q for the first decodable y whose l-multiple has full 8-torsion order."""
    for y in range(2, 200):
        q = O.decode(y.to_bytes(32, "little"))
        if q is None:
            continue
        t = O.mul_int(O.L, q)
        if O.mul_int(4, t) != O.IDENTITY:
            assert O.mul_int(8, t) == O.IDENTITY
            return np.frombuffer(O.encode(t), dtype=np.uint8)
    raise AssertionError("no point of order 8 found")


ORDER8 = _order8_point()
SHARED_BASE = OC.ed_mul_base(np.array([_le(0x1234567)], dtype=np.uint8))[0]  # a non-standard base in the prime subgroup


def _points(n, seed):
    """identity, a point of order 8, then random points of the prime-order subgroup"""
    k = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    k[:, 31] &= 0x0F
    p = OC.ed_mul_base(k, threads=THREADS)
    p[0] = np.frombuffer(O.encode(O.IDENTITY), dtype=np.uint8)
    p[1] = ORDER8
    p[n // 2] = ORDER8
    p[n - 1] = p[0]
    return p


_REF = {}


def _ref(base, vartime):
    """oracle results of SET on `base` (None: geScalarMultBase), computed once"""
    key = (None if base is None else bytes(base), vartime)
    if key not in _REF:
        if base is None and not vartime:
            _REF[key] = OC.ed_mul_base(SET, threads=THREADS)
        else:
            b = B_ENC if base is None else base
            out, st = OC.ed_mul(SET, np.tile(b, (len(SET), 1)), vartime=vartime, threads=THREADS)
            assert not st.any()
            _REF[key] = out
    return _REF[key]


def _index(n, seed):
    """n indices into SET: every scalar when n allows it, shuffled so that a wave holds mixed digits"""
    rng = np.random.default_rng(seed)
    idx = np.concatenate([rng.permutation(len(SET)) for _ in range(-(-n // len(SET)))])[:n]
    return idx


def test_inputs_are_accepted_by_the_reference():
    # no GPU: every scalar is 32 bytes the oracle multiplies by, every point decodes, the references agree where the
    # two semantics multiply by the same integer (scalars below 2^252), and the set holds what it says it holds
    assert SET.shape == (242, 32)
    ct, vt = _ref(None, False), _ref(None, True)
    small = SET[:, 31] < 0x10
    assert small.sum() > 10 and (ct[small] == vt[small]).all()
    assert bytes(ct[0]) == O.encode(O.IDENTITY) and bytes(ct[1]) == O.encode(O.B)
    for i in (2, 6, 9, 10, 25, 41, 100):
        assert bytes(ct[i]) == O.mul_base(bytes(SET[i])), i
    digits = [O.recode_radix16(bytes(s)) for s in SET[:10]]
    assert any(d[63] == 8 for d in digits), "no scalar with the top digit at 8"
    assert digits[5][0] == -8 and all(x == -7 for x in digits[5][1:63])  # 0x88..: a carry out of every nibble
    for n in (64, 4097):
        p = _points(n, 7)
        _, st = OC.ed_mul(SET[_index(n, 8)], p, threads=THREADS)
        assert not st.any()
    assert O.decode(bytes(SHARED_BASE)) is not None and not O.is_small_order(O.decode(bytes(SHARED_BASE)))
    assert O.mul_int(8, O.decode(bytes(ORDER8))) == O.IDENTITY and O.mul_int(4, O.decode(bytes(ORDER8))) != O.IDENTITY


@pytest.fixture(scope="module")
def ed():
    import torch

    assert torch.cuda.is_available()
    from kyber_amd.group import edwards25519 as ed

    return ed


def _fixed(ed, s, vartime, uniform):
    import torch

    return ed.batch_mul_base(torch.from_numpy(np.ascontiguousarray(s)).cuda(), vartime=vartime, uniform=uniform).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("n", [1, 63, 65])
def test_fixed_base_small_batches_cover_the_set(ed, n, flags):
    # the set cut in consecutive batches of n (the last one wraps): every scalar runs at this batch size
    vartime, uniform = flags
    exp = _ref(None, vartime)
    for lo in range(0, len(SET), n):
        idx = np.arange(lo, lo + n) % len(SET)
        out = _fixed(ed, SET[idx], vartime, uniform)
        bad = np.nonzero((out != exp[idx]).any(axis=1))[0]
        assert not len(bad), (n, lo, [int(idx[b]) for b in bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("n", [4095, 4097])  # encoded in the kernel / parked for the encode kernel
def test_fixed_base_mixed_waves(ed, n, flags):
    vartime, uniform = flags
    idx = _index(n, 100 + n)
    assert len(set(idx.tolist())) == len(SET)
    out = _fixed(ed, SET[idx], vartime, uniform)
    bad = np.nonzero((out != _ref(None, vartime)[idx]).any(axis=1))[0]
    assert not len(bad), (n, [int(idx[b]) for b in bad[:8]])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 4097])
def test_fixed_base_vartime_skips_positions_zero_in_every_lane(ed, n):
    # positions 2, 3, 9 and 15 of the G = 4 comb are zero in EVERY lane (the nibble below each is < 8, so no carry
    # arrives), and position 16 has nothing either: the ballot skip runs, in the loop and at the tail positions
    s = np.random.default_rng(0x5C1F).integers(0, 256, size=(n, 32), dtype=np.uint8)
    for k in (2, 3, 9, 15):
        s[:, 2 * k] = 0
        s[:, 2 * k + 1] = 0
        s[:, 2 * k - 1] &= 0x7F
    exp, st = OC.ed_mul(s, np.tile(B_ENC, (n, 1)), vartime=True, threads=THREADS)
    assert not st.any()
    assert (exp == OC.ed_mul_base(s, threads=THREADS)).all()  # below 2^252: the same integer on both paths
    assert (_fixed(ed, s, True, False) == exp).all()
    assert (_fixed(ed, s, False, False) == exp).all()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
def test_shared_base_radix256_comb(ed, flags):
    # kyb_ed25519_mul_same_base at 16 384 coefficients: the base gets a radix-256 table and the G = 2 instance of the
    # comb kernel (the scan under KYB_F_UNIFORM); the reference is geScalarMult on the tiled base
    vartime, uniform = flags
    n = 16384
    idx = _index(n, 300)
    out = ed.commit(SET[idx], SHARED_BASE, vartime=vartime, uniform=uniform)
    bad = np.nonzero((out != _ref(SHARED_BASE, vartime)[idx]).any(axis=1))[0]
    assert not len(bad), [int(idx[b]) for b in bad[:8]]


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS, ids=FLAG_IDS)
@pytest.mark.parametrize("n", [64, 4097])  # table in scratch, encoded in the kernel / table in the slab, parked
def test_var_base_affine_window_table(ed, n, flags):
    import torch

    vartime, uniform = flags
    idx = _index(n, 400 + n)
    s, p = SET[idx], _points(n, 7)
    exp, est = OC.ed_mul(s, p, vartime=vartime, threads=THREADS)
    assert not est.any()
    out, st = ed.batch_mul(torch.from_numpy(np.ascontiguousarray(s)).cuda(), torch.from_numpy(p).cuda(),
                           vartime=vartime, uniform=uniform)
    assert not st.cpu().numpy().any()
    out = out.cpu().numpy()
    bad = np.nonzero((out != exp).any(axis=1))[0]
    assert not len(bad), (n, [(int(b), int(idx[b])) for b in bad[:8]])
