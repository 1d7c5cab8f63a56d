"""kyb_ed25519_cosi_verify on the GPU: the labelled table of tests/_cosi_cases.py through the host and the device entry
against the oracle, with agg and count present and NULL, at both mask strides and on each side of the width rule; the
reference's sign.input as ONE roster of 1024 keys (row i under the one-bit mask i is accepted, under bit i + 1
rejected); the fused call against the composed path; and one batch of 2^18 + 5 elements across the piece edge."""
import numpy as np
import pytest

from tests import _cosi_cases as CC
from tests import _cosi_oracle as CO

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 127, 128, 129, 257)


@pytest.fixture(scope="module")
def ed():
    from kyber_amd.group import edwards25519

    return edwards25519


def pack_msgs(rs):
    off = np.zeros(len(rs) + 1, dtype=np.uint64)
    np.cumsum([len(r.msg) for r in rs], out=off[1:])
    blob = b"".join(r.msg for r in rs)
    return np.frombuffer(blob or b"\0", dtype=np.uint8).copy(), off


def want_of(name, n):
    rs, ex = CC.take(name, n)
    return (rs, np.array([e[0] for e in ex], dtype=np.uint8), np.frombuffer(b"".join(e[1] for e in ex), dtype=np.uint8).reshape(n, 32),
            np.array([e[2] for e in ex], dtype=np.uint32), np.array([e[3] for e in ex], dtype=np.uint8))


def raw_call(name, rs, stride, device, want_agg=True, want_count=True, want_status=True):
    """the C ABI itself: agg, count and status can be NULL, and the mask buffer ends with the last mask"""
    from kyber_amd import _lib

    lib = _lib.load()
    m, n = len(CC.keys_of(name)), len(rs)
    roster, sigs = CC.pack_roster(name), CC.pack_sigs(rs)
    masks = CC.pack_masks(rs, m, stride).reshape(-1)[:(n - 1) * stride + CO.mask_len(m)].copy()
    blob, off = pack_msgs(rs)
    if device:
        import torch

        d = [torch.from_numpy(x).cuda() for x in (roster, blob, off.view(np.int64), sigs, masks)]
        agg = torch.full((n, 32), 0xEE, dtype=torch.uint8, device="cuda")
        cnt = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        ok, st = (torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") for _ in range(2))
        rc = lib.kyb_ed25519_cosi_verify_dev(n, m, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(),
                                             stride, agg.data_ptr() if want_agg else None, cnt.data_ptr() if want_count else None,
                                             ok.data_ptr(), st.data_ptr() if want_status else None, 0,
                                             torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ok, agg, cnt, st = ok.cpu().numpy(), agg.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), st.cpu().numpy()
    else:
        agg, cnt = np.full((n, 32), 0xEE, np.uint8), np.full(n, 0xFFFFFFFF, np.uint32)
        ok, st = np.full(n, 0xEE, np.uint8), np.full(n, 0xEE, np.uint8)
        rc = lib.kyb_ed25519_cosi_verify(n, m, roster.ctypes.data, blob.ctypes.data, off.ctypes.data, sigs.ctypes.data, masks.ctypes.data,
                                         stride, agg.ctypes.data if want_agg else None, cnt.ctypes.data if want_count else None,
                                         ok.ctypes.data, st.ctypes.data if want_status else None, 0)
    assert rc == 0, lib.kyb_last_error()
    return ok, agg, cnt, st


def check(name, n, slack, device, want_agg=True, want_count=True, want_status=True):
    rs, w_ok, w_agg, w_cnt, w_st = want_of(name, n)
    m = len(CC.keys_of(name))
    ok, agg, cnt, st = raw_call(name, rs, CO.mask_len(m) + slack, device, want_agg, want_count, want_status)
    bad = np.nonzero(ok != w_ok)[0]
    assert not len(bad), (name, n, device, [rs[i].label for i in bad[:5]])
    for got, want, asked, untouched in ((agg, w_agg, want_agg, 0xEE), (cnt, w_cnt, want_count, 0xFFFFFFFF), (st, w_st, want_status, 0xEE)):
        assert (got == (want if asked else untouched)).all(), (name, n, device, asked)


@pytest.mark.parametrize("name", CC.NAMES)
def test_the_table_through_both_entries(name):
    rows = len(CC.rows(name))
    check(name, rows, 0, device=False)
    check(name, rows, 64, device=True)
    check(name, rows, 64, device=False, want_agg=False, want_count=False)
    check(name, rows, 0, device=True, want_agg=False, want_count=False, want_status=False)


@pytest.mark.parametrize("name", ["1", "5", "9", "17", "65"])
def test_the_wave_and_block_edges(name):
    for k, n in enumerate(SIZES):
        check(name, n, 64 * (k % 2), device=bool((k // 2) % 2), want_agg=bool(k % 3))


@pytest.mark.parametrize("m", [5, 8, 9, 16, 17, 64, 257])
def test_each_side_of_the_width_rule(ed, m):
    from tests.test_gpu_mask_aggregate import width_edges

    for n in width_edges(ed, m):
        check(str(m), n, 0, device=True)


def test_sign_input_as_one_roster_of_1024_keys(ed):
    """cosi_test.go:152-156: a cosignature without its mask is an EdDSA signature under the aggregate key"""
    pubs, msgs, sigs = CC.sign_input_roster()
    roster = b"".join(pubs)
    one = [CC.mask_of(1024, [i]) for i in range(1024)]
    other = [CC.mask_of(1024, [(i + 1) % 1024]) for i in range(1024)]
    ok, agg, cnt, st = ed.batch_cosi_verify(roster, msgs, sigs, one, want_agg=True)
    assert ok.all() and not st.any() and (cnt == 1).all() and agg.tobytes() == roster
    ok, agg, cnt, st = ed.batch_cosi_verify(roster, msgs, sigs, other, want_agg=True)
    assert not ok.any() and not st.any() and (cnt == 1).all() and agg.tobytes() == b"".join(pubs[1:] + pubs[:1])


def test_rfc8032_rows_with_a_roster_of_one(ed):
    from tests import _ed_verify_oracle as VO

    for pub, msg, sig in VO.rfc8032():
        ok, _, cnt, st = ed.batch_cosi_verify(pub, [msg, msg, msg + b"x"], [sig, sig, sig], [b"\x01", b"\x00", b"\x01"])
        assert list(ok) == [1, 0, 0] and list(cnt) == [1, 0, 1] and not st.any()


@pytest.mark.parametrize("name", ["9", "65", "bad5"])
def test_fused_against_composed(ed, name):
    from kyber_amd.sign import cosi

    rs, w_ok, w_agg, w_cnt, w_st = want_of(name, len(CC.rows(name)))
    roster = b"".join(CC.publics(CC.keys_of(name)))
    msgs, sigs, masks = [r.msg for r in rs], [r.sig for r in rs], [r.mask for r in rs]
    ok, agg, cnt, st = ed.batch_cosi_verify(roster, msgs, sigs, masks, want_agg=True)
    ok2, cnt2, st2 = cosi._verify_batch_composed(roster, msgs, sigs, masks)
    assert (ok == ok2).all() and (cnt == cnt2).all() and (st == st2).all()
    assert (ok == w_ok).all() and (agg == w_agg).all() and (cnt == w_cnt).all() and (st == w_st).all()


def test_one_batch_across_the_piece_edge():
    """2^18 + 5 elements over the roster of nine keys: the table's rows repeated in turn, so the oracle ran once per
    distinct row; five elements land in the second piece"""
    import torch
    from kyber_amd.group import edwards25519 as ed

    n = (1 << 18) + 5
    rs, ex = CC.rows("9"), CC.expected("9")
    t = len(rs)
    reps, rem = divmod(n, t)
    tile = lambda a: np.concatenate([np.tile(a, (reps,) + (1,) * (a.ndim - 1)), a[:rem]])
    sigs, masks = tile(CC.pack_sigs(rs)), tile(CC.pack_masks(rs, 9, 2))
    lens = tile(np.array([len(r.msg) for r in rs], dtype=np.int64))
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    block = b"".join(r.msg for r in rs)
    blob = np.frombuffer(block * reps + b"".join(r.msg for r in rs[:rem]), dtype=np.uint8).copy()
    assert blob.size == off[-1]
    d = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (blob, off, sigs, masks)]
    ok, agg, cnt, st = ed.batch_cosi_verify(torch.from_numpy(CC.pack_roster("9")).cuda(), (d[0], d[1]), d[2], d[3], want_agg=True)
    ok, agg, cnt, st = ok.cpu().numpy(), agg.cpu().numpy(), cnt.cpu().numpy().view(np.uint32), st.cpu().numpy()
    assert (ok == tile(np.array([e[0] for e in ex], dtype=np.uint8))).all()
    assert (agg == tile(np.frombuffer(b"".join(e[1] for e in ex), dtype=np.uint8).reshape(t, 32))).all()
    assert (cnt == tile(np.array([e[2] for e in ex], dtype=np.uint32))).all() and not st.any()
    assert ed.cosi_group_width(n, 9) == 8 and (n - (1 << 18)) == 5
