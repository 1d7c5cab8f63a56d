"""The shared-inversion encoder without a GPU: ed25519_dev.cuh's ed_encode_chunk compiled for the CPU
(tests/ed_encode_harness.cpp) and run lane by lane over whole launches.  Montgomery's trick must give the bytes of one
inversion per point whatever the grouping: interleaved ownership, records of one point and of two (the DLEQ
encoder's), prefixes in the lane's own array and in the block's [j][limb][lane] array, last blocks whose lanes hold
different numbers of points or none.  Every point is emitted exactly once, and the second point of a record before
the first."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness():
    out = os.path.join(ROOT, "tests", "_build", "libedencodeharness.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fno-strict-aliasing", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tests", "ed_encode_harness.cpp")])
    lib = C.CDLL(out)
    lib.ede_launch.restype = C.c_long
    return lib


def _triples(points, seed):
    """random field elements as reduced limbs (26 / 25 bits, signed): the encoder does not ask for points of the curve"""
    rng = np.random.default_rng(seed)
    lim = np.tile(np.array([1 << 25, 1 << 24] * 5, dtype=np.int64), 3)
    return rng.integers(-lim, lim, size=(points, 30)).astype(np.int32)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _launch(lib, records, group, block, lds, proj):
    points = records * group
    out = np.zeros((points, 32), dtype=np.uint8)
    emitted = np.zeros(points, dtype=np.int32)
    order = np.full(points, -1, dtype=np.int32)
    blocks = lib.ede_launch(C.c_size_t(records), group, block, lds, _p(proj), _p(out), _p(emitted), _p(order))
    assert blocks >= 0
    return out, emitted, order, blocks


@pytest.mark.parametrize("lds", [0, 1])
@pytest.mark.parametrize("group", [1, 2])
def test_interleaved_grouping_gives_the_bytes_of_one_inversion_per_point(harness, group, lds):
    chunk = harness.ede_chunk()
    block = 64
    S = block * chunk
    # 3 S + 5 points (+ 1 for whole records of two); a last block with empty lanes; one with lanes of unequal counts;
    # full blocks only; a single point
    for points in (3 * S + 5 + (group - 1), S + 3 * group, S + block + 2 * group, 2 * S, group):
        proj = _triples(points, 100 * group + lds + points)
        want = np.zeros((points, 32), dtype=np.uint8)
        harness.ede_reference(C.c_size_t(points), _p(proj), _p(want))
        out, emitted, order, blocks = _launch(harness, points // group, group, block, lds, proj)
        assert blocks == -(-points // S)
        assert (emitted == 1).all(), np.nonzero(emitted != 1)[0][:8]
        assert (out == want).all(), np.nonzero((out != want).any(axis=1))[0][:8]
        assert len({bytes(r) for r in want}) == points
        if group == 2:
            assert (order[1::2] + 1 == order[0::2]).all()  # b just before a, in the same lane


def test_other_block_sizes_agree(harness):
    chunk = harness.ede_chunk()
    points = 3 * 256 * chunk + 5
    proj = _triples(points, 7)
    want = np.zeros((points, 32), dtype=np.uint8)
    harness.ede_reference(C.c_size_t(points), _p(proj), _p(want))
    for block in (128, 256):
        out, emitted, _, _ = _launch(harness, points, 1, block, 0, proj)
        assert (emitted == 1).all() and (out == want).all(), block
