"""kyb_ed25519_mask_aggregate on the GPU: the labelled table of tests/_cosi_cases.py through the host and the device
entry, byte for byte against the oracle and against the engine's own MSM with 0/1 scalars; at the wave and block edges,
on each side of the width rule for every roster size (asked from kyb_ed25519_cosi_group_width; up to four keys there is
one width only), at mask_stride = L and L + 64, with count and status present and NULL."""
import ctypes as C

import numpy as np
import pytest

from tests import _cosi_cases as CC
from tests import _cosi_oracle as CO

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 127, 128, 129, 257)  # the wave edge and the 128-lane block edge


@pytest.fixture(scope="module")
def ed():
    from kyber_amd.group import edwards25519

    return edwards25519


def width_edges(ed, m):
    """the largest n that still takes width 4 and the next one, where the rule has two sides for m keys"""
    if ed.cosi_group_width(1 << 20, m) == 4:
        return ()
    lo, hi = 1, 1 << 20  # width(lo) == 4 (one element never pays for 256 entries), width(hi) == 8
    assert ed.cosi_group_width(lo, m) == 4
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if ed.cosi_group_width(mid, m) == 4 else (lo, mid)
    return (lo, hi)


def want_of(name, n):
    rs, ex = CC.take(name, n)
    out = np.frombuffer(b"".join(e[1] for e in ex), dtype=np.uint8).reshape(n, 32)
    return rs, out, np.array([e[2] for e in ex], dtype=np.uint32), np.array([e[3] for e in ex], dtype=np.uint8)


def raw_call(name, rs, stride, device, want_count=True, want_status=True):
    """the C ABI itself, so that count and status can be NULL and the mask buffer ends with the last mask"""
    from kyber_amd import _lib

    lib = _lib.load()
    m, n = len(CC.keys_of(name)), len(rs)
    roster = CC.pack_roster(name)
    masks = CC.pack_masks(rs, m, stride).reshape(-1)[:(n - 1) * stride + CO.mask_len(m)].copy()
    if device:
        import torch

        d_r, d_m = torch.from_numpy(roster).cuda(), torch.from_numpy(masks).cuda()
        out = torch.full((n, 32), 0xEE, dtype=torch.uint8, device="cuda")
        cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        rc = lib.kyb_ed25519_mask_aggregate_dev(n, m, d_r.data_ptr(), d_m.data_ptr(), stride, out.data_ptr(),
                                                cnt.data_ptr() if want_count else None, st.data_ptr() if want_status else None, 0,
                                                torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out, cnt, st = out.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), st.cpu().numpy()
    else:
        out, cnt, st = np.full((n, 32), 0xEE, np.uint8), np.full(n, 0xFFFFFFFF, np.uint32), np.full(n, 0xEE, np.uint8)
        rc = lib.kyb_ed25519_mask_aggregate(n, m, roster.ctypes.data, masks.ctypes.data, stride, out.ctypes.data,
                                            cnt.ctypes.data if want_count else None, st.ctypes.data if want_status else None, 0)
    assert rc == 0, lib.kyb_last_error()
    return out, cnt, st


def check(name, n, stride_slack, device, want_count=True, want_status=True):
    rs, w_out, w_cnt, w_st = want_of(name, n)
    m = len(CC.keys_of(name))
    out, cnt, st = raw_call(name, rs, CO.mask_len(m) + stride_slack, device, want_count, want_status)
    bad = np.nonzero((out != w_out).any(axis=1))[0]
    assert not len(bad), (name, n, device, [rs[i].label for i in bad[:5]])
    if want_count:
        assert (cnt == w_cnt).all(), (name, n, device)
    else:
        assert (cnt == 0xFFFFFFFF).all()  # nobody wrote where NULL was passed
    if want_status:
        assert (st == w_st).all(), (name, n, device)
    else:
        assert (st == 0xEE).all()


@pytest.mark.parametrize("name", CC.NAMES)
def test_the_table_at_the_wave_and_block_edges(name):
    for k, n in enumerate(SIZES):
        check(name, n, 64 * (k % 2), device=bool((k // 2) % 2))
    check(name, len(CC.rows(name)), 0, device=False)  # every row of the table, both entries
    check(name, len(CC.rows(name)), 64, device=True)


@pytest.mark.parametrize("m", CC.SIZES)
def test_each_side_of_the_width_rule(ed, m):
    edges = width_edges(ed, m)
    assert bool(edges) == (m > 4)
    for n in edges:
        assert ed.cosi_group_width(n, m) == (4 if n == edges[0] else 8)
        check(str(m), n, 0, device=False)
        check(str(m), n, 64, device=True)


@pytest.mark.parametrize("name", ["9", "64", "bad5"])
def test_count_and_status_may_be_null(name):
    for device in (False, True):
        check(name, 129, 64, device, want_count=False)
        check(name, 129, 0, device, want_status=False)
        check(name, 65, 0, device, want_count=False, want_status=False)


def test_the_wrapper_and_the_msm_with_0_1_scalars(ed):
    """batch_mask_aggregate on host and device buffers, and every row of three rosters against kyb_ed25519_msm"""
    import torch

    for name in ("9", "17", "65", "bad5"):
        rs, w_out, w_cnt, w_st = want_of(name, len(CC.rows(name)))
        m = len(CC.keys_of(name))
        roster = CC.pack_roster(name)
        out, cnt, st = ed.batch_mask_aggregate(roster, [r.mask for r in rs])
        assert (out == w_out).all() and (cnt == w_cnt).all() and (st == w_st).all(), name
        masks = torch.from_numpy(CC.pack_masks(rs, m, CO.mask_len(m) + 5)).cuda()
        out, cnt, st = ed.batch_mask_aggregate(torch.from_numpy(roster).cuda(), masks)
        assert (out.cpu().numpy() == w_out).all() and (cnt.cpu().numpy().view(np.uint32) == w_cnt).all(), name
        assert (st.cpu().numpy() == w_st).all(), name
        for r, want, s in zip(rs, w_out, w_st):
            scalars = np.zeros((m, 32), dtype=np.uint8)
            scalars[CO.enabled(r.mask, m), 0] = 1
            got, mst = ed.msm(scalars, roster)
            assert got.tobytes() == want.tobytes() and bool(mst.any()) == bool(s), (name, r.label)


def test_nothing_is_written_past_the_last_element():
    from kyber_amd import _lib

    lib = _lib.load()
    rs, w_out, w_cnt, w_st = want_of("17", 130)
    roster, masks = CC.pack_roster("17"), CC.pack_masks(rs, 17, 3)
    out, cnt, st = np.full((131, 32), 0xEE, np.uint8), np.full(131, 0xEEEEEEEE, np.uint32), np.full(131, 0xEE, np.uint8)
    assert lib.kyb_ed25519_mask_aggregate(130, 17, roster.ctypes.data, masks.ctypes.data, 3, out.ctypes.data, cnt.ctypes.data,
                                          st.ctypes.data, 0) == 0
    assert (out[:130] == w_out).all() and (out[130] == 0xEE).all() and cnt[130] == 0xEEEEEEEE and st[130] == 0xEE
    assert C.sizeof(C.c_uint32) == 4 and (cnt[:130] == w_cnt).all()
