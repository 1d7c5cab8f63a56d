"""The host batch of variable-length elements the Ed25519 host entries share (kyber_amd/csrc/ed_spans.h) without a GPU:
tests/ed_spans_harness.cpp is a program of its own over the header, built for the CPU twice -- plainly, and with
-fsanitize=address,undefined, run directly with nothing preloaded -- and run once per case.  What the type refuses is what
every entry's offsets check refused: a decreasing pair anywhere, or bytes named where the caller gave no buffer.  What it
builds is held against Python integers: the rebased offsets, the total, off[0], and the displacements of the staged
input and of an output that lies at the same offsets; where the buffer is real the harness reads every element through
both views, in a heap block of exactly off[n] bytes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ed_spans_harness.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
BIG = 2**63


def _build(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", *extra, "-o", out, SRC])
    return out


@pytest.fixture(scope="module", params=["plain", "asan_ubsan"])
def program(request):
    if request.param == "plain":
        return _build("ed_spans_harness", ["-O2"])
    return _build("ed_spans_harness_san", ["-O1", "-g", *SAN])


def run(program, off, null=False):
    r = subprocess.run([program, "null" if null else "buf", *map(str, off)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (off, null, r.returncode, r.stderr[-2000:])
    line = r.stdout.strip()
    if line == "refused":
        return None
    return dict(kv.split("=") for kv in line.split())


def check_accepted(program, off, null=False):
    got = run(program, off, null)
    assert got is not None, (off, null)
    n = len(off) - 1
    assert int(got["lead"]) == off[0]
    assert int(got["total"]) == off[n] - off[0]
    assert [int(x) for x in got["rel"].split(",")] == [o - off[0] for o in off]
    assert int(got["offsets_bytes"]) == 8 * (n + 1)
    assert got["base"] == ("null" if null else str(off[0]))  # the staged input starts at the first element
    assert int(got["at"]) == off[0] and got["at_null"] == "1"  # an output at the same offsets; none asked for, none given
    assert got["same"] == "1"


# off[0] = 0, 3 and just below 2^63, where the elements' own offsets run past 2^63 (a pointer cannot be displaced by more
# than that: off[0] itself stays below); n = 1 and n = 3; an empty element first, in the middle (equal neighbours
# between two full ones) and last
LEADS = (0, 3, BIG - 5)
SHAPES = ((4,), (0,), (5, 0, 7), (0, 6, 1), (2, 9, 0), (1, 1, 1))


@pytest.mark.parametrize("lead", LEADS)
def test_rebased_offsets_total_and_displacements_are_exact(program, lead):
    for lens in SHAPES:
        off = [lead]
        for length in lens:
            off.append(off[-1] + length)
        check_accepted(program, off)


@pytest.mark.parametrize("n", (1, 3))
def test_all_elements_empty_need_no_buffer(program, n):
    for lead in LEADS:
        check_accepted(program, [lead] * (n + 1), null=True)
        check_accepted(program, [lead] * (n + 1))


@pytest.mark.parametrize("n", (1, 3))
def test_one_byte_named_without_a_buffer_is_refused(program, n):
    for lead in LEADS:
        for at in range(n):  # the one byte in the first, a middle, the last element
            off = [lead] * (at + 1) + [lead + 1] * (n - at)
            assert run(program, off, null=True) is None, off
            check_accepted(program, off)  # the same offsets over a buffer are fine


def test_a_decreasing_pair_is_refused_wherever_it_lies(program):
    for lead in LEADS:
        assert run(program, [lead + 1, lead]) is None  # n = 1: the only pair
        good = [lead + 2, lead + 4, lead + 6, lead + 8]
        for at in range(3):  # first, middle, last pair of n = 3
            off = list(good)
            off[at + 1] = off[at] - 1
            if at < 2:
                off[at + 2:] = [off[at + 1] + 2 * (k + 1) for k in range(2 - at)]  # only this pair decreases
            assert all(off[k + 1] >= off[k] for k in range(3) if k != at) and off[at + 1] < off[at]
            assert run(program, off) is None, off
            assert run(program, off, null=True) is None, off
    # a pair that decreases back to its start hides from a first-against-last comparison
    assert run(program, [3, 9, 3, 9]) is None and run(program, [0, 5, 0], null=True) is None
