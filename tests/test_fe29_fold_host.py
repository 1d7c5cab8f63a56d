"""The word fold of the nine-limb product (kyber_amd/csrc/fe29.cuh) without a GPU.  A high column H_k, k = 9 .. 16, is
folded as a 64-bit word: 1216 * (its low word, unsigned) into low column k - 9 and 9728 * (its high word, signed) into
low column k - 8.  tests/fe29_harness.cpp, as it is, is built in the two builds of tests/test_fe29_host.py (-O2 with the
bound audit, -O1 under -fsanitize=undefined,signed-integer-overflow; programs of their own, nothing preloaded) and sent
mul, sq and sq2 requests aimed at what that fold can get wrong: one product alone in each high column at the word
boundaries of H (a low word read as signed, a high word read as unsigned, column 16's high word missing from column
8), the same columns through the squaring, and dense operands with 13 < m_f m_g <= 14, the largest columns there are.
Every answer is held against Python integers mod p = 2^255 - 19 and against the carried range; a sanitizer report ends
the program with an error, which fails the test.  The generator drops no request: it asserts the stated bound of each
one it emits, and the number of requests is asserted exactly."""
import math
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "fe29_harness.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")
P = 2**255 - 19
MASK = (1 << 29) - 1
U = 1 << 28  # the unit of a limb bound m
# fe29.cuh: FE29_MUL_LIMIT (m_f m_g of a product, doubled for 2 f^2) and FE29_SQ_LIMIT (m_f of a squaring), as exact
# integers: |a| |b| <= 14 * 2^56, |a| <= 3.99 * 2^28, 2 a^2 <= 14 * 2^56
MUL_LIMIT = 14 * U * U
SQ_BOUND = 399 * U // 100
SQ2_BOUND = math.isqrt(MUL_LIMIT // 2)
SAN = ["-fsanitize=undefined,signed-integer-overflow", "-fno-sanitize-recover=all"]
N_ALONE = 17 * 36             # word-boundary products x ordered limb pairs (i, j) with 9 <= i + j <= 16
N_SQUARED = 2 * (16 * 13 + 4 * 7)  # sq and sq2: limb pairs i < j x operand pairs, and single limbs 5 .. 8
N_DENSE = 2000


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.check_call(["g++", "-std=c++17", "-fno-strict-aliasing", *extra, "-o", out, SRC])
    return out


@pytest.fixture(scope="module")
def programs():
    return _build("fe29_fold_harness", ["-O2", "-DKYB_FE_AUDIT"]), _build("fe29_fold_harness_ubsan", ["-O1", *SAN])


def _answers(prog, lines, tmp_path):
    req = tmp_path / "req.txt"
    req.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(req)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])  # a sanitizer report is fatal in the second build
    out = [[int(x) for x in l.split()] for l in r.stdout.strip().split("\n")]
    assert len(out) == len(lines)
    return out


def _val(limbs):
    return sum(v << (29 * i) for i, v in enumerate(limbs))


def _carried(limbs):
    # a carried result: limbs in [-2^28, 2^28), limb 1 with the last carry (below 2^17) on top
    return all(-U <= v < U for i, v in enumerate(limbs) if i != 1) and abs(limbs[1]) < U + (1 << 17)


def _mag(limbs):
    return max(abs(v) for v in limbs)


def _unit(i, a, j=None, b=0):
    f = [0] * 9
    f[i] = a
    if j is not None:
        f[j] = b
    return f


def _line(op, *args):
    for a in args:
        assert len(a) == 9 and all(-(1 << 31) <= v < (1 << 31) for v in a), a
    return op + " " + " ".join(str(x) for a in args for x in a)


def _emit_mul(out, f, g):
    assert _mag(f) * _mag(g) <= MUL_LIMIT, (f, g)
    out.append((_line("mul", f, g), _val(f) * _val(g)))


def _emit_sq(out, f):
    assert _mag(f) <= SQ_BOUND, f
    out.append((_line("sq", f), _val(f) ** 2))


def _emit_sq2(out, f):
    assert 2 * _mag(f) ** 2 <= MUL_LIMIT, f
    out.append((_line("sq2", f), 2 * _val(f) ** 2))


# (a, b): the one product a b of a high column, at the word boundaries of the 64-bit column
_T = 3 * U - 1
_WORD_EDGES = [
    (1, 1), (-1, 1),                                    # +-1: hi = 0 / hi = -1 with lo = 0xffffffff
    ((1 << 31) - 1, 1),                                 # 2^31 - 1: the largest low word a signed reading leaves alone
    (1 << 16, 1 << 15), (-(1 << 16), 1 << 15),          # +-2^31: lo = 0x80000000 with hi = 0 and hi = -1
    (65535, 65537),                                     # 2^32 - 1: lo all ones, hi = 0
    (1 << 16, 1 << 16), (-(1 << 16), 1 << 16),          # +-2^32: lo = 0, hi = +-1
    (641, 6700417),                                     # 2^32 + 1
    (-3 << 15, 1 << 16), (-((1 << 20) + 1) << 5, 1 << 26),  # odd multiples of -2^31: lo = 0x80000000, hi < 0
    (_T, _T), (-_T, _T),                                # +-(3 * 2^28 - 1)^2: the ladder's largest product
    (7 * U // 2, 4 * U - 1), (-7 * U // 2, 4 * U - 1), (7 * U // 2, 1 - 4 * U), (-7 * U // 2, 1 - 4 * U),
]


def _alone_requests():
    out = []
    for a, b in _WORD_EDGES:
        H = a * b
        assert -(1 << 63) <= H < (1 << 63)
        for k in range(9, 17):
            for i in range(k - 8, 9):  # every (i, j) with i + j = k: both orders, and (8, 8) for k = 16
                _emit_mul(out, _unit(i, a), _unit(k - i, b))
    lo_hi = {((a * b) & 0xFFFFFFFF, (a * b) >> 32) for a, b in _WORD_EDGES}
    assert any(lo == 0x80000000 and hi < -1 for lo, hi in lo_hi) and (0xFFFFFFFF, 0) in lo_hi and (0, -1) in lo_hi
    return out


def _squared_requests():
    """f = a e_i + b e_j: 2 a b (4 a b for 2 f^2) alone in high column i + j, a^2 and b^2 on the diagonals; and
    f = a e_i, a^2 alone in column 2 i, which is the only way into column 16"""
    out = []
    for emit, L in ((_emit_sq, SQ_BOUND), (_emit_sq2, SQ2_BOUND)):
        pairs = [(1, 1), (-1, 1), (1 << 15, 1 << 15), (-(1 << 15), 1 << 15), (1 << 16, 1 << 15), (1 << 16, -(1 << 15)),
                 (L, L), (L, -L), (-L, -L), (-L, L - 1), (L, 1), (-1, L), (3 * U // 2, -L)]
        for k in range(9, 17):
            for i in range(k - 8, 9):
                if i < k - i:
                    for a, b in pairs:
                        emit(out, _unit(i, a, k - i, b))
        for i in range(5, 9):
            for a in (1, -1, 1 << 16, 46341, L, -L, L - 1):  # 46341^2 = 2^31 + 4633: just past the signed low word
                emit(out, _unit(i, a))
    return out


def _dense_requests():
    """2 000 pairs with 13 < m_f m_g <= 14: every limb at its bound in one sign, in alternating signs and in random
    signs, and random signs with magnitudes inside the last 4 % under the bound"""
    rng = random.Random(0x29F01D)
    out = []
    for t in range(N_DENSE):
        bf = rng.randrange(18 * U // 10, 77 * U // 10)   # m_f in [1.8, 7.7): m_g = 14 / m_f stays below 8
        bg = MUL_LIMIT // bf - rng.randrange(0, U // 64)
        assert 13 * U * U < bf * bg <= MUL_LIMIT and bg < (1 << 31)
        mode = t % 4
        if mode == 0:
            sf, sg = ((1, 1), (1, -1), (-1, 1), (-1, -1))[(t // 4) % 4]
            f, g = [sf * bf] * 9, [sg * bg] * 9
        elif mode == 1:
            s = 1 if (t // 4) % 2 else -1
            f = [s * bf * (-1) ** i for i in range(9)]
            g = [bg * (-1) ** (i + (t // 8) % 2) for i in range(9)]
        else:
            f = [rng.choice((-1, 1)) * (bf if mode == 2 else rng.randrange(bf - bf // 25, bf + 1)) for _ in range(9)]
            g = [rng.choice((-1, 1)) * (bg if mode == 2 else rng.randrange(bg - bg // 25, bg + 1)) for _ in range(9)]
            f[rng.randrange(9)] = rng.choice((-1, 1)) * bf
            g[rng.randrange(9)] = rng.choice((-1, 1)) * bg
        assert 13 * U * U < _mag(f) * _mag(g)
        _emit_mul(out, f, g)
    return out


@pytest.mark.parametrize("make, count", [(_alone_requests, N_ALONE), (_squared_requests, N_SQUARED), (_dense_requests, N_DENSE)],
                         ids=["one_product_alone_in_a_high_column", "high_columns_through_the_squaring", "dense_operands_at_the_bound"])
def test_word_fold_against_python_integers(programs, tmp_path, make, count):
    reqs = make()
    assert len(reqs) == count
    lines = [r[0] for r in reqs]
    for prog in programs:
        for (line, expect), ans in zip(reqs, _answers(prog, lines, tmp_path)):
            assert len(ans) == 9 and _val(ans) % P == expect % P, line
            assert _carried(ans), (line, ans)
