"""Every sharded host entry of the C ABI (tests/_shard_cases.py: one row per public call behind an `md_active(` site,
with its strides, flags and optional arrays) run with a device set on the one GPU there is: device 0 listed three or
eight times, so every slice runs the single-device path on a host thread of its own behind the entry's per-operand
offsets.  Two assertions a row, both on bytes: every output array equals that of the same call with the device set
cleared, and at every boundary row of every shard and every planted row the outputs are the table's oracle expectation
(statuses and verdicts at every row), so a defect common to both paths does not hide."""
import numpy as np
import pytest

from tests import _shard_cases as T

pytestmark = pytest.mark.gpu

CANARY = 0xA5
ALL = sorted(T.ROWS)
ED = [r for r in ALL if r.startswith("ed25519/")]
CHEAP = [r for r in ALL if T.ROWS[r].cheap]  # one row per source file with a site
EIGHT = ED + ["bls12381/pair_check/uncompressed", "bn256/g2_mul", "bn254/pair"]


def _call(case):
    from kyber_amd import _lib
    from kyber_amd._buf import dst_arg

    outs = {o.name: np.full(o.shape, CANARY, dtype=np.uint8) for o in case.outs()}
    argv, keep = [], []
    for a in case.args:
        if isinstance(a, T.Out):
            argv.append(None if a.null else outs[a.name].ctypes.data)
        elif isinstance(a, T.Dst):
            keep.append(dst_arg(a.tag))
            argv.append(keep[-1])
        elif isinstance(a, np.ndarray):
            assert a.flags.c_contiguous and a.dtype in (np.uint8, np.uint32, np.uint64)
            argv.append(a.ctypes.data)
        else:
            argv.append(a)
    _lib.check(getattr(_lib.load(), case.entry)(*argv), case.entry)
    return outs


def _both(case, devs, threshold=1):
    """(outputs with the device set cleared, outputs with it active); the set is cleared again whatever happens"""
    from kyber_amd import devices
    from kyber_amd.pairing import bls12381 as bls

    devices.set_devices([])
    if case.fill is not None:
        case.fill(bls)
    ref = _call(case)
    devices.set_devices(devs)
    devices.set_shard_threshold(threshold)
    try:
        assert devices.get_devices() == devs
        return ref, _call(case)
    finally:
        devices.set_devices([])
        devices.set_shard_threshold(16384)


def _against_the_table(case, got, what):
    n = case.n
    for o in case.outs():
        if o.null:
            assert (got[o.name] == CANARY).all(), (what, o.name, "a NULL output was written through another pointer")
    if case.status is not None:
        bad = np.nonzero(got["status"] != case.status)[0]
        assert not len(bad), (what, "status", bad[:8], got["status"][bad[:8]], case.status[bad[:8]])
    if case.ok is not None:
        bad = np.nonzero(got["ok"] != case.ok)[0]
        assert not len(bad), (what, "ok", bad[:8], got["ok"][bad[:8]], case.ok[bad[:8]])
    for name, rows in case.expect.items():
        arr = got[name].reshape(n, -1)
        for i, want in rows.items():
            assert bytes(arr[i]) == want, (what, name, i, case.planted.get(i))
    for name, want in case.whole.items():
        assert bytes(got[name]) == want, (what, name)


def _check(name, n, devs, threshold=1):
    case = T.build(name, n, len(devs))
    ref, got = _both(case, devs, threshold)
    for o in case.outs():  # 1. the sharded call is the single-device call, byte for byte, on every output array
        bad = np.nonzero((ref[o.name].reshape(-1) != got[o.name].reshape(-1)))[0]
        assert not len(bad), (name, o.name, "differs from the single-device call from byte", int(bad[0]), "of", ref[o.name].size)
    _against_the_table(case, got, name)  # 2. and it is what the oracles say, at every row the table knows


def _size(name, world):
    """the smallest sizes at which the slices are uneven: n = 1 (mod 3), n = 3 (mod 8)"""
    if world == 8:
        return 99 if name.startswith("ed25519/") else 67
    if "same_key" in name:
        return 97
    if name.split("/")[1] in ("verify", "mul", "mul_base", "mul2"):
        return 1000  # 334 + 333 + 333
    return 100 if name.startswith("ed25519/") else 67


@pytest.mark.parametrize("name", ALL)
def test_three_uneven_shards(name):
    _check(name, _size(name, 3), [0, 0, 0])


@pytest.mark.parametrize("name", EIGHT)
def test_eight_uneven_shards(name):
    _check(name, _size(name, 8), [0] * 8)


@pytest.mark.parametrize("name", CHEAP)
def test_one_element_a_shard_and_one_too_few(name):
    _check(name, 8, [0] * 8)  # n == world: every slice is one element
    _check(name, 7, [0] * 8)  # n == world - 1: the call stays on one device


@pytest.mark.parametrize("name", CHEAP)
def test_either_side_of_the_threshold(name):
    _check(name, 63, [0, 0, 0], threshold=64)  # below: one device
    _check(name, 64, [0, 0, 0], threshold=64)  # at it: 22 + 21 + 21


def test_same_key_shards_build_and_hit_the_key_cache_under_alternating_keys():
    """three shard threads on one device meet in one per-stream key-line cache: two keys in alternating calls make them
    build, replace and hit its entry; every call must still be its own table"""
    from kyber_amd import devices
    from kyber_amd.pairing import bls12381 as bls

    cases = [T.build("bls12381/verify_g1_same_key/key " + k, 97, 3) for k in ("a", "b")]
    devices.set_devices([])
    for c in cases:
        c.fill(bls)
    single = [_call(c) for c in cases]
    devices.set_devices([0, 0, 0])
    devices.set_shard_threshold(1)
    try:
        for turn in range(6):
            k = turn % 2 if turn < 4 else 1  # a, b, a, b, b, b: a changed key every call, then the same one again
            got = _call(cases[k])
            assert bytes(got["ok"]) == bytes(single[k]["ok"]) and bytes(got["status"]) == bytes(single[k]["status"]), turn
            _against_the_table(cases[k], got, turn)
    finally:
        devices.set_devices([])
        devices.set_shard_threshold(16384)
    assert cases[0].ok.sum() == 97 - len(cases[0].planted)
