"""kyb_ed25519_lincomb on the GPU: the labelled table of tests/_proof_cases.py against the big-integer oracle through the
host and the device entry, at the wave and block edges and for every shape; large batches across the piece edges against
the composed device calls the kernel replaces (mul, mul_base, add), byte for byte; out and ok together and each alone."""
import numpy as np
import pytest

from tests import _proof_cases as PC

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 127, 128, 129, 257)  # the wave edge and the 128-lane block edge


@pytest.fixture(scope="module")
def ed():
    from kyber_amd.group import edwards25519

    return edwards25519


def _arr(rows_of_bytes, width):
    return np.frombuffer(b"".join(b"".join(r) for r in rows_of_bytes), dtype=np.uint8).reshape(len(rows_of_bytes), width, 32).copy()


def _table(ko, ks, nil_mask, vartime, n=None):
    """[(shared, scalars (n, k, 32), own (n, ko, 32) or None, expect (n, 32), want out, want ok, want status, labels)]: a
    batch per entry of the table, its rows repeated in turn up to n elements"""
    out = []
    for name, shared, rows in PC.batches(ko, ks, nil_mask):
        if n is not None:
            rows = [rows[i % len(rows)] for i in range(n)]
        vals = [PC.value(ko, ks, nil_mask, shared, r[1], r[2], vartime) for r in rows]
        expect = [PC.expect_bytes(r[3], v) for r, v in zip(rows, vals)]
        verdicts = [PC.verdict(v, e) for v, e in zip(vals, expect)]
        out.append(([None if nil_mask >> j & 1 else shared[j] for j in range(ks)], _arr([r[1] for r in rows], ko + ks),
                    _arr([r[2] for r in rows], ko) if ko else None,
                    np.frombuffer(b"".join(expect), dtype=np.uint8).reshape(len(rows), 32).copy(),
                    np.frombuffer(b"".join(v or bytes(32) for v in vals), dtype=np.uint8).reshape(len(rows), 32),
                    np.array([v[0] for v in verdicts], dtype=np.uint8), np.array([v[1] for v in verdicts], dtype=np.uint8),
                    [f"{name}: {r[0]} (expect: {PC.kind_checked(r[3], v)})" for r, v in zip(rows, vals)]))
    return out


def _check(ed, case, vartime, device):
    shared, s, own, expect, want_out, want_ok, want_st, labels = case
    if device:
        import torch

        s, own, expect = (None if x is None else torch.from_numpy(x).cuda() for x in (s, own, expect))
    res = [ed.batch_lincomb(s, own, shared, expect, vartime=vartime),  # out and ok together, and each alone
           ed.batch_lincomb(s, own, shared, None, vartime=vartime),
           ed.batch_lincomb(s, own, shared, expect, want_out=False, vartime=vartime)]
    res = [tuple(None if x is None else (x.cpu().numpy() if device else x) for x in r) for r in res]
    assert res[1][1] is None and res[2][0] is None
    for out, ok, st in res:
        for got, want, what in ((out, want_out, "out"), (ok, want_ok, "ok"), (st, want_st, "status")):
            if got is not None:
                bad = np.nonzero((got != want).reshape(len(labels), -1).any(axis=1))[0]
                assert not len(bad), (what, [labels[i] for i in bad[:5]], device)


@pytest.mark.parametrize("vartime", [False, True])
@pytest.mark.parametrize("ko,ks", [(a, b) for a in range(5) for b in range(5) if a + b])
def test_every_shape_matches_the_oracle_at_129_elements(ed, ko, ks, vartime):
    nil_mask = 5 & ((1 << ks) - 1)  # shared terms 0 and 2 on the standard base
    for case in _table(ko, ks, nil_mask, vartime, 129):
        _check(ed, case, vartime, device=False)
        _check(ed, case, vartime, device=True)


@pytest.mark.parametrize("ko,ks,nil_mask", [(1, 2, 1), (1, 2, 2), (3, 1, 0), (0, 2, 3)])
def test_the_wave_and_block_edges(ed, ko, ks, nil_mask):
    for n in SIZES:
        for vartime in (False, True):
            case = _table(ko, ks, nil_mask, vartime, n)[0]
            _check(ed, case, vartime, device=(n % 2 == 1))
            if n in (1, 129):
                _check(ed, case, vartime, device=(n % 2 == 0))


@pytest.mark.parametrize("ko,ks,nil_mask", sorted(PC.FULL_GRID))
def test_the_whole_table_with_every_special_scalar_in_every_slot(ed, ko, ks, nil_mask):
    for vartime in (False, True):
        for case in _table(ko, ks, nil_mask, vartime):
            _check(ed, case, vartime, device=True)


@pytest.mark.parametrize("ko,ks,n", [(1, 2, (1 << 18) + 5), (3, 1, (1 << 17) + 5)])
@pytest.mark.parametrize("vartime", [False, True])
def test_large_batches_equal_the_composed_calls_across_the_piece_edge(ed, ko, ks, n, vartime):
    """mul / mul_base / add composed on the device, byte for byte; rows of the table planted at both ends of the batch and
    on both sides of the piece edge are checked against the oracle as well"""
    import torch

    piece = n - 5
    shared_pt = PC.batches(ko, ks, 0)[0][1]
    shared = [None, shared_pt[1]] if ks == 2 else [shared_pt[0]]
    nil_mask = 1 if ks == 2 else 0
    g = torch.Generator().manual_seed(1000 * ko + ks)
    s = torch.randint(0, 256, (n, ko + ks, 32), dtype=torch.uint8, generator=g)  # unreduced scalars, half above 2^255
    own = ed.batch_mul_base(torch.randint(0, 256, (n * ko, 32), dtype=torch.uint8, generator=g).cuda()).cpu().view(n, ko, 32)
    rows = PC.batches(ko, ks, nil_mask)[0][2]
    # rows of the table: scalars at and above 2^255, exceptional own points, an undecodable one
    wanted = ("every scalar 2^256 - 1", f"= {2**255:#x}", "own 0 undecodable", "own 0 identity as y + p", "own 0 order 8", "zero scalars",
              f"= {PC.L:#x}", "own 0 order 4")
    picked = [next(r for r in rows if w in r[0]) for w in wanted]
    planted = dict(zip((0, 1, piece - 2, piece - 1, piece, piece + 1, n - 2, n - 1), picked))
    for at, r in planted.items():
        s[at] = torch.from_numpy(_arr([r[1]], ko + ks)[0])
        own[at] = torch.from_numpy(_arr([r[2]], ko)[0])
    s, own = s.cuda(), own.cuda().contiguous()
    out, _, st = ed.batch_lincomb(s, own, shared, vartime=vartime)
    # the composed path: one multiplication and one encoding per term, an addition per further term
    acc, bad = None, torch.zeros(n, dtype=torch.uint8, device="cuda")
    for j in range(ko + ks):
        sj = s[:, j].contiguous()
        if j < ko:
            t, tst = ed.batch_mul(sj, own[:, j].contiguous(), vartime=vartime)
            bad |= tst
        elif shared[j - ko] is None:
            t = ed.batch_mul_base(sj)
        else:
            t, tst = ed.batch_mul(sj, torch.from_numpy(np.frombuffer(shared[j - ko], dtype=np.uint8).copy()).cuda().repeat(n, 1),
                                  vartime=vartime)
            bad |= tst
        if acc is None:
            acc = t
        else:  # (an undecodable own point of a planted row: its term is zero bytes, the row is told by its status)
            good = (bad == 0).nonzero().view(-1)
            a2, ast = ed.batch_add(acc[good].contiguous(), t[good].contiguous())
            assert int(ast.max()) == 0
            acc = acc.clone()
            acc[good] = a2
    want = torch.where((bad == 0)[:, None], acc, torch.zeros_like(acc))
    assert torch.equal(st != 0, bad != 0)
    diff = (out != want).any(dim=1).nonzero().view(-1)
    assert diff.numel() == 0, diff[:8].tolist()
    out = out.cpu().numpy()
    oracle_shared = [bytes(32) if p is None else p for p in shared]
    for at, r in planted.items():
        v = PC.value(ko, ks, nil_mask, oracle_shared, r[1], r[2], vartime)
        assert out[at].tobytes() == (v or bytes(32)), (at, r[0])
        assert int(st[at]) == (v is None), (at, r[0])


def test_a_large_batch_takes_its_verdicts_across_the_piece_edge(ed):
    """expect = the batch's own output, with every 1000th element tampered: ok is 0 exactly there, on both sides of the edge"""
    import torch

    ko, ks, n = 1, 2, (1 << 18) + 5
    shared_pt = PC.batches(ko, ks, 0)[0][1]
    shared = [None, shared_pt[1]]
    g = torch.Generator().manual_seed(5)
    s = torch.randint(0, 256, (n, 3, 32), dtype=torch.uint8, generator=g).cuda()
    own = ed.batch_mul_base(torch.randint(0, 256, (n, 32), dtype=torch.uint8, generator=g).cuda()).view(n, 1, 32)
    out, _, st = ed.batch_lincomb(s, own, shared)
    assert int(st.max()) == 0
    expect = out.clone()
    tampered = torch.arange(0, n, 1000, device="cuda")
    tampered = torch.cat([tampered, torch.tensor([(1 << 18) - 1, 1 << 18, n - 1], device="cuda")]).unique()
    expect[tampered, 31] ^= 0x80
    _, ok, st = ed.batch_lincomb(s, own, shared, expect, want_out=False)
    want = torch.ones(n, dtype=torch.uint8, device="cuda")
    want[tampered] = 0
    assert torch.equal(ok, want) and int(st.max()) == 0
