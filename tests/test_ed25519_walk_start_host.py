"""How the two Ed25519 walks start, without a GPU: tests/ed_walk_start_harness.cpp is a program of its own over
kyber_amd/csrc/ed25519_dev.cuh, built for the CPU and run on a file of requests.  The variable-base ladder on fe29 starts
from its top digit's table entry (doubled as it is read, or handed on as it is when the walk has no window) and leaves a
completed point; the fixed-base comb starts from position 0's row.  Both are held against oracle/ed25519_ref.c on every
top digit, every position-0 digit, the edges of both scalar semantics and points of every small order -- once plain,
with the bound audit (KYB_FE_AUDIT) recording the largest product it meets, and once under
-fsanitize=undefined,signed-integer-overflow, where a wrapped column or a shift out of range is fatal."""
import os
import subprocess

import numpy as np
import pytest

from oracle import ed25519 as O
from tests import _ed_walk_start_cases as cases
from tests import _oracle_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ed_walk_start_harness.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")
# fe29.cuh: FE29_MUL_LIMIT and FE29_SQ_LIMIT; fe25519.cuh: 2^13 / 124.5 and 2^31 / (19 * 2^25)
MUL29_LIMIT, SQ29_LIMIT, MUL_LIMIT, MUL19_LIMIT = 14.0, 3.99, 65.8, 3.36
SAN = ["-fsanitize=undefined,signed-integer-overflow", "-fno-sanitize-recover=all"]
COMB_G = 4  # ED_COMB_G


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.check_call(["g++", "-std=c++17", "-fno-strict-aliasing", *extra, "-o", out, SRC])
    return out


@pytest.fixture(scope="module")
def programs():
    return _build("ed_walk_start_harness", ["-O2", "-DKYB_FE_AUDIT"]), _build("ed_walk_start_harness_ubsan", ["-O1", *SAN])


def _answers(prog, lines, tmp_path):
    req = tmp_path / "req.txt"
    req.write_text("\n".join(lines) + "\n")
    r = subprocess.run([prog, str(req)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = [[int(x) for x in l.split()] for l in r.stdout.strip().split("\n")]
    assert len(out) == len(lines)
    return out


def _words(b):
    return [int.from_bytes(bytes(b[4 * i:4 * i + 4]), "little") for i in range(8)]


def _fmt(op, *args):
    return op + " " + " ".join(str(x) for a in args for x in a)


def test_the_case_list_reaches_every_start():
    S = cases.scalars()
    assert {cases.top_digit(s) for s in S if cases.top_digit(s) <= 8} == set(range(9))
    assert any(cases.top_digit(s) > 8 for s in S)  # dropped on the constant-structure path, carried under KYB_F_VARTIME
    E = [O.recode_radix16(s) for s in S]
    low = {e[0] + 16 * e[1] for e in E if not any(e[2:63]) and e[63] in (0, 16)}
    assert low >= set(range(-8, 9))  # comb position 0 alone (8 is recoded -8 + 16: one position from G = 2 on)
    assert sum(int.from_bytes(s, "little") < 16 for s in S) >= 9  # KYB_F_VARTIME: no window, or one
    assert len(cases.points()) == 26


def test_the_variable_base_walk_from_its_top_entry_matches_the_oracle_inside_the_bound(programs, tmp_path):
    S, Pts = cases.scalars(), cases.points()
    pairs = [(s, p) for s in S for p in Pts]
    s = np.frombuffer(b"".join(c[0] for c in pairs), dtype=np.uint8).reshape(-1, 32)
    p = np.frombuffer(b"".join(c[1] for c in pairs), dtype=np.uint8).reshape(-1, 32)
    want = {vt: _oracle_c.ed_mul(s, p, vartime=bool(vt)) for vt in (0, 1)}
    assert not want[0][1].any()
    req, exp = ["audit"], [None]
    # the slab table under both scalar semantics on every pair; the scratch table and the uniform scan (constant-structure
    # values) take the same start: every scalar on three of the points
    for flags, gtab in ((0, 1), (1, 1), (0, 0), (1, 0), (8, 0), (8, 1)):
        out, st = want[flags & 1]
        for i, (sc, pt) in enumerate(pairs):
            si, pi = divmod(i, len(Pts))
            if (flags, gtab) not in ((0, 1), (1, 1)) and (pi - si) % 9:
                continue
            req.append(_fmt("walk", [flags, gtab], _words(sc), _words(pt)))
            exp.append([int(st[i])] + _words(out[i]))
        req.append("audit")
        exp.append(None)
    assert len(req) > 3000
    seen = []
    for prog in programs:
        for line, ans, e in zip(req, _answers(prog, req, tmp_path), exp):
            if e is None:
                seen.append(ans)
            else:
                assert ans == e, line
    audits = [a for a in seen if a[0] >= 0][1:]  # the audited build's, after each batch of walks
    assert len(audits) == 6
    for mm, msq, _, _ in audits:
        print("fe29: largest m_f m_g %.3f, largest squared operand %.3f" % (mm / 1e6, msq / 1e6))
        assert 0 < mm / 1e6 < MUL29_LIMIT and 0 < msq / 1e6 < SQ29_LIMIT


def test_the_fixed_base_walk_from_position_zero_matches_the_oracle_inside_the_bound(programs, tmp_path):
    S = cases.scalars()
    s = np.frombuffer(b"".join(S), dtype=np.uint8).reshape(-1, 32)
    base = np.frombuffer(O.encode(O.B) * len(S), dtype=np.uint8).reshape(-1, 32)
    full, st = _oracle_c.ed_mul(s, base, vartime=True)
    assert not st.any()
    want = {0: _oracle_c.ed_mul_base(s), 1: full}
    req, exp = ["audit"], [None]
    for g in (2, COMB_G):
        for vt in (0, 1):
            for i, sc in enumerate(S):
                req.append(_fmt("base", [g, vt], _words(sc)))
                exp.append(_words(want[vt][i]))
            req.append("audit")
            exp.append(None)
    seen = []
    for prog in programs:
        for line, ans, e in zip(req, _answers(prog, req, tmp_path), exp):
            if e is None:
                seen.append(ans)
            else:
                assert ans == e, line
    audits = [a for a in seen if a[0] >= 0][1:]
    assert len(audits) == 4
    for _, _, mm, m19 in audits:
        print("fe: largest m_f m_g %.3f, largest 19-fold operand %.3f" % (mm / 1e6, m19 / 1e6))
        assert 0 < mm / 1e6 < MUL_LIMIT and 0 < m19 / 1e6 < MUL19_LIMIT
