"""The nine-limb field type of the variable-base ladder (kyber_amd/csrc/fe29.cuh) without a GPU: tests/fe29_harness.cpp
is a program of its own over the device headers, built for the CPU and run on a file of requests.  Every operation is
held against Python integers mod p = 2^255 - 19 -- the value of the result's limbs, and the limb range a carried result
promises -- on random elements, limbs at the stated bound in both and in mixed signs, 0, 1, p - 1 and non-canonical
representatives up to 2^261.  The variable-base walk of ed25519_mul_kernel (decode, window table in both table
layouts, ladder, both scalar semantics and the uniform scan) is replayed on the golden keys against
oracle/ed25519_ref.c, with the bound audit (KYB_FE_AUDIT) recording the largest m_f m_g it meets.  The same requests
run once more through a build under -fsanitize=undefined,signed-integer-overflow, where a wrapped column is fatal."""
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import ed25519 as O
from tests import _oracle_c

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "fe29_harness.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")
P = 2**255 - 19
MASK = (1 << 29) - 1
# fe29.cuh: a product needs m_f m_g <= 14.2 (FE29_MUL_LIMIT holds the ladder to 14), a squaring m_f < 4
MUL_LIMIT, SQ_LIMIT = 14.0, 3.99
SAN = ["-fsanitize=undefined,signed-integer-overflow", "-fno-sanitize-recover=all"]


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.check_call(["g++", "-std=c++17", "-fno-strict-aliasing", *extra, "-o", out, SRC])
    return out


@pytest.fixture(scope="module")
def programs():
    return _build("fe29_harness", ["-O2", "-DKYB_FE_AUDIT"]), _build("fe29_harness_ubsan", ["-O1", *SAN])


def _run(prog, lines, tmp_path, name="req.txt"):
    req = tmp_path / name
    req.write_text("\n".join(lines) + "\n")
    return subprocess.run([prog, str(req)], capture_output=True, text=True)


def _answers(prog, lines, tmp_path):
    r = _run(prog, lines, tmp_path)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = [[int(x) for x in l.split()] for l in r.stdout.strip().split("\n")]
    assert len(out) == len(lines)
    return out


def _val(limbs):
    return sum(v << (29 * i) for i, v in enumerate(limbs))


def _limbs_canonical(x):
    return [(x >> (29 * i)) & MASK for i in range(9)]


def _limbs_signed(x):
    """the carried form of x: limbs in [-2^28, 2^28)"""
    out = []
    for _ in range(8):
        r = ((x + (1 << 28)) & MASK) - (1 << 28)
        out.append(r)
        x = (x - r) >> 29
    out.append(x)
    return out


def _elements():
    rng = random.Random(29)
    E = [_limbs_canonical(v) for v in (0, 1, P - 1, 2, 19, P - 19, (P - 1) // 2)]
    E += [_limbs_canonical(rng.randrange(P)) for _ in range(6)]
    E += [_limbs_signed(rng.randrange(P)) for _ in range(4)]
    # non-canonical representatives: p, 2^255, 2^256 - 1, up to 2^261 - 1, and their negatives in signed limbs
    for v in (P, P + 1, 2**255, 2**256 - 1, 2**260 + 12345, 2**261 - 1):
        E.append(_limbs_canonical(v))
        E.append(_limbs_signed(-v))
    # limbs at a bound of m * 2^28 in both signs and in mixed signs
    for m in (1, 2, 3, 7):
        b = m * (1 << 28)
        E += [[b - 1] * 9, [-b] * 9, [(b - 1) if i & 1 else -b for i in range(9)], [-b if i & 1 else (b - 1) for i in range(9)]]
        E.append([rng.choice((-b, b - 1)) for _ in range(9)])
    return E


def _mag(limbs):
    return max(abs(v) for v in limbs) / (1 << 28)


def _fmt(op, *args):
    return op + " " + " ".join(str(x) for a in args for x in a)


def _carried(limbs):
    # a carried result: limbs in [-2^28, 2^28), limb 1 with the last carry (below 2^17) on top
    return all(-(1 << 28) <= v < (1 << 28) for i, v in enumerate(limbs) if i != 1) and abs(limbs[1]) < (1 << 28) + (1 << 17)


def _field_requests():
    E = _elements()
    req, chk = [], []

    def add(line, check):
        req.append(line)
        chk.append(check)

    def value_is(expect, carried=False):
        def check(ans):
            assert len(ans) == 9 and _val(ans) % P == expect % P
            assert not carried or _carried(ans), ans
        return check

    for f in E:
        vf = _val(f)
        add(_fmt("neg", f), value_is(-vf))
        add(_fmt("towords", f), lambda ans, vf=vf: ans == [(vf % P >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [vf % P & 1, int(vf % P != 0)] or pytest.fail(str(ans)))
        add(_fmt("tofe", f), lambda ans, vf=vf: sum(v << o for v, o in zip(ans, (0, 26, 51, 77, 102, 128, 153, 179, 204, 230))) % P == vf % P or pytest.fail(str(ans)))
        if _mag(f) <= SQ_LIMIT:
            add(_fmt("sq", f), value_is(vf * vf, True))
        if 2 * _mag(f) ** 2 <= MUL_LIMIT:
            add(_fmt("sq2", f), value_is(2 * vf * vf, True))
        for g in E:
            vg = _val(g)
            if _mag(f) + _mag(g) < 7.9:  # 32-bit sums
                add(_fmt("add", f, g), value_is(vf + vg))
                add(_fmt("sub", f, g), value_is(vf - vg))
            if _mag(f) * _mag(g) <= MUL_LIMIT:
                add(_fmt("mul", f, g), value_is(vf * vg, True))
    for f, g in zip(E[:8], E[5:13]):
        add(_fmt("cmov0", f, g), lambda ans, f=f: ans == f or pytest.fail(str(ans)))
        add(_fmt("cmov1", f, g), lambda ans, g=g: ans == g or pytest.fail(str(ans)))
        add(_fmt("cswap0", f, g), lambda ans, f=f, g=g: ans == f + g or pytest.fail(str(ans)))
        add(_fmt("cswap1", f, g), lambda ans, f=f, g=g: ans == g + f or pytest.fail(str(ans)))
    for f in E[:14]:
        vf = _val(f)
        add(_fmt("invert", f), value_is(pow(vf, P - 2, P), True))
        add(_fmt("pow22523", f), value_is(pow(vf, (P - 5) // 8, P), True))
    rng = random.Random(30)
    for x in (0, 1, P - 1, P, 2**255 - 1, 2**255, 2**256 - 1, rng.randrange(2**256), rng.randrange(2**256)):
        w = [(x >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
        add(_fmt("fromwords", w), lambda ans, x=x: ans == _limbs_canonical(x & (2**255 - 1)) or pytest.fail(str(ans)))
    for x in (0, 1, P - 1, rng.randrange(P), rng.randrange(P)):
        # ten limbs: canonical fields, and a signed representative
        offs, t = (0, 26, 51, 77, 102, 128, 153, 179, 204, 230), []
        for i, o in enumerate(offs):
            t.append((x >> o) & ((1 << (25 if i & 1 else 26)) - 1))
        add(_fmt("fromfe", t), value_is(x))
        t[0] -= 1 << 26
        t[1] += 1
        add(_fmt("fromfe", t), value_is(x))
    d = -121665 * pow(121666, P - 2, P) % P
    add("const", lambda ans: ans == _limbs_canonical(d) + _limbs_canonical(2 * d % P) + _limbs_canonical(pow(2, (P - 1) // 4, P)) or pytest.fail(str(ans)))
    return req, chk


def test_every_operation_against_python_integers(programs, tmp_path):
    req, chk = _field_requests()
    assert len(req) > 2000
    for prog in programs:  # the second build: no signed overflow, no out-of-range shift anywhere in these
        for ans, check in zip(_answers(prog, req, tmp_path), chk):
            check(ans)


def _walk_cases(golden_dir):
    misc = json.load(open(os.path.join(golden_dir, "ed25519_misc.json")))
    pts = [bytes.fromhex(k["pub"]) for k in misc["rfc8032"]] + [bytes.fromhex(h) for h in misc["small_order"]]
    pts += [O.encode(O.B), (P + 1).to_bytes(32, "little"), (1 | 1 << 255).to_bytes(32, "little")]  # y >= p; x = 0 with the sign bit
    y = 2
    while O.decode(y.to_bytes(32, "little")) is not None:
        y += 1
    pts.append(y.to_bytes(32, "little"))  # no square root
    raw = hashlib.shake_256(b"fe29-walk").digest(32 * len(pts))
    ell = 2**252 + 27742317777372353535851937790883648493
    fixed = [0, 1, 8, ell - 1, ell, 2**252 - 1, 2**252, 2**255 - 1, 2**256 - 1, int("8" * 64, 16), int("7" * 64, 16)]
    cases = []
    for i, p in enumerate(pts):
        scalars = [raw[32 * i:32 * i + 32], fixed[i % len(fixed)].to_bytes(32, "little"), fixed[(i + 5) % len(fixed)].to_bytes(32, "little")]
        for s in scalars:
            cases.append((s, p))
    return cases


def _words(b):
    return [int.from_bytes(b[4 * i:4 * i + 4], "little") for i in range(8)]


def test_the_ladder_walk_on_the_golden_keys_matches_the_oracle_inside_the_bound(programs, golden_dir, tmp_path):
    cases = _walk_cases(golden_dir)
    s = np.frombuffer(b"".join(c[0] for c in cases), dtype=np.uint8).reshape(-1, 32)
    p = np.frombuffer(b"".join(c[1] for c in cases), dtype=np.uint8).reshape(-1, 32)
    want = {vt: _oracle_c.ed_mul(s, p, vartime=bool(vt)) for vt in (0, 1)}
    assert (want[0][1] != 0).any() and (want[0][1] == 0).sum() > 30
    req, exp = ["audit"], [None]
    for flags in (0, 1, 8):  # constant-structure, KYB_F_VARTIME, KYB_F_UNIFORM (the scan: constant-structure values)
        out, st = want[flags & 1]
        for gtab in (0, 1):
            for i, (sc, pt) in enumerate(cases):
                req.append(_fmt("walk", [flags, gtab], _words(sc), _words(pt)))
                exp.append([int(st[i])] + _words(bytes(out[i])))
            req.append("audit")
            exp.append(None)
    seen = []
    for prog in programs:
        for line, ans, e in zip(req, _answers(prog, req, tmp_path), exp):
            if e is None:
                seen.append(ans)
            else:
                assert ans == e, line
    audits = [a for a in seen if a[0] >= 0][1:]  # the audited build's, after each batch of walks
    assert len(audits) == 6
    for mm, msq in audits:
        print("largest m_f m_g %.3f, largest squared operand %.3f" % (mm / 1e6, msq / 1e6))
        assert 0 < mm / 1e6 < MUL_LIMIT and 0 < msq / 1e6 < SQ_LIMIT


def test_a_wrapped_column_is_fatal_in_the_sanitizer_build(programs, tmp_path):
    # limbs of 8 * 2^28: nine products of 2^62 in column 8 -- far outside the bound, and outside 64 bits
    f = [(1 << 31) - 1] * 9
    r = _run(programs[1], [_fmt("mul", f, f)], tmp_path)
    assert r.returncode != 0 and "signed integer overflow" in r.stderr, (r.returncode, r.stderr[-500:])
