"""How the two Ed25519 walks start, on the device: the variable-base ladder from its top digit's table entry and the
fixed-base comb from position 0's row (ed25519_dev.cuh), through batch_mul, batch_mul_base and the same-base path, at a
size on either side of the deferred encoding (the slab table / the scratch table with the in-kernel encode), under flags
0, KYB_F_VARTIME and KYB_F_UNIFORM.  The inputs are the lists of tests/_ed_walk_start_cases.py -- every top digit, every
position-0 digit, the edges of both scalar semantics, points of every small order -- with one wave of all-zero scalars
(KYB_F_VARTIME: a walk of no window), one of scalars below 16 (one window) and one of scalars below 2^64 (a short walk).
Every output and status byte must be the C oracle's."""
import numpy as np
import pytest

from oracle import ed25519 as O
from tests import _ed_walk_start_cases as cases
from tests import _oracle_c

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

N_DEFER = 4096 + 64 + 1  # deferred encoding, window tables in the slab
N_SMALL = 65             # in-kernel encoding, window tables in scratch
N_SAME = 16384 + 1       # the same-base path builds the shared base's radix-256 table from here on
FLAGS = {"plain": {}, "vartime": {"vartime": True}, "uniform": {"uniform": True}}


def _bad_point():
    y = 2
    while O.decode(y.to_bytes(32, "little")) is not None:
        y += 1
    return y.to_bytes(32, "little")


def _batch(n, stride):
    """n (scalar, point) rows: the case lists' pairs taken `stride` apart, then three special waves"""
    S, Pts = cases.scalars(), cases.points() + [_bad_point()]
    pairs = [(s, p) for s in S for p in Pts]
    rows = [pairs[(i * stride) % len(pairs)] for i in range(n)]
    s = np.frombuffer(b"".join(r[0] for r in rows), dtype=np.uint8).reshape(n, 32).copy()
    p = np.frombuffer(b"".join(r[1] for r in rows), dtype=np.uint8).reshape(n, 32).copy()
    short = [2**64 - 1, 1, 2**64 - 3, 8, 0, 2**63, 16**15 * 9, 7]
    for w, pick in enumerate((lambda i: 0, lambda i: i % 16, lambda i: short[i % len(short)])):
        lo = 64 * w if n <= 4 * 64 else 64 * (w + 1)  # whole waves: 64 rows from a multiple of 64
        if lo + 64 > n:
            break
        for i in range(64):
            s[lo + i] = np.frombuffer(pick(i).to_bytes(32, "little"), dtype=np.uint8)
    return s, p


@pytest.fixture(scope="module")
def batches():
    """{name: (scalars, points, {vartime: (out, status)}, {vartime: fixed-base out})}; the small size once per special wave"""
    out = {}
    todo = {"defer": _batch(N_DEFER, 1)}
    s, p = _batch(3 * 64 + 1, 37)
    for w, name in enumerate(("small-zero", "small-one-window", "small-short")):
        rows = list(range(64 * w, 64 * w + 64)) + [3 * 64]
        todo[name] = (s[rows].copy(), p[rows].copy())
    todo["small-mixed"] = tuple(x[:N_SMALL].copy() for x in _batch(N_DEFER, 53))
    base = np.frombuffer(O.encode(O.B), dtype=np.uint8)
    for name, (s, p) in todo.items():
        assert len(s) in (N_DEFER, N_SMALL)
        mul = {vt: _oracle_c.ed_mul(s, p, vartime=vt) for vt in (False, True)}
        fixed = {False: _oracle_c.ed_mul_base(s), True: _oracle_c.ed_mul(s, np.tile(base, (len(s), 1)), vartime=True)[0]}
        assert mul[False][1].any() and not mul[False][1].all()
        out[name] = (s, p, mul, fixed)
    return out


BATCHES = ("defer", "small-zero", "small-one-window", "small-short", "small-mixed")


@pytest.mark.parametrize("flags", sorted(FLAGS))
@pytest.mark.parametrize("name", BATCHES)
def test_batch_mul_starts_from_the_top_entry(batches, name, flags):
    from kyber_amd.group import edwards25519 as ed

    s, p, mul, _ = batches[name]
    want, want_st = mul[flags == "vartime"]
    out, st = ed.batch_mul(torch.from_numpy(s).cuda(), torch.from_numpy(p).cuda(), **FLAGS[flags])
    torch.cuda.synchronize()
    out, st = out.cpu().numpy(), st.cpu().numpy()
    assert (st == want_st).all(), np.nonzero(st != want_st)[0][:8]
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], bytes(s[bad[0]]).hex(), bytes(p[bad[0]]).hex())


@pytest.mark.parametrize("flags", sorted(FLAGS))
@pytest.mark.parametrize("name", BATCHES)
def test_batch_mul_base_starts_from_position_zero(batches, name, flags):
    from kyber_amd.group import edwards25519 as ed

    s, _, _, fixed = batches[name]
    want = fixed[flags == "vartime"]
    out = ed.batch_mul_base(torch.from_numpy(s).cuda(), **FLAGS[flags])
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], bytes(s[bad[0]]).hex())


@pytest.mark.parametrize("flags", sorted(FLAGS))
def test_the_same_base_path_starts_from_position_zero(flags):
    from kyber_amd.group import edwards25519 as ed

    s, _ = _batch(N_SAME, 1)
    base = cases.points()[-1]  # one of the SHAKE-derived points
    want, st = _oracle_c.ed_mul(s, np.tile(np.frombuffer(base, dtype=np.uint8), (N_SAME, 1)), vartime=flags == "vartime")
    assert not st.any()
    out = np.asarray(ed.commit(s, base=base, **FLAGS[flags]))
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:8], bytes(s[bad[0]]).hex())
