"""Batched Point.Add on the device, every group (kyb_ed25519_add, kyb_{bls12381,bn256,bn254}_g{1,2}_add and their _dev
twins) against tests/_add_cases.py: the labelled table -- exceptional pairs, every kind of rejected operand in either
slot, torsion and non-canonical Ed25519 operands, BN G2 operands outside the subgroup -- through the host entry and the
device entry on a side stream; the table tiled and shuffled over many waves; batch sizes either side of the block size
with a guard element behind the outputs; status = NULL; argument errors; the Python wrappers; 2^20 + 5 (Ed25519) and
2^16 + 5 (pairing groups) elements, every output byte against the C oracle; two streams on two host threads; and
kyb_ed25519_mul2 against add(mul, mul) on the torsion and non-canonical operands.

Sizes: the table is 280-470 rows per group (tests/_add_cases.py FILLER = 192 generic rows), tiled 8 times; the batch
sizes share one oracle chain of 4096 + 77 rows."""
import os
import random
import threading

import numpy as np
import pytest

from tests import _add_cases as A

pytestmark = pytest.mark.gpu

KYB_E_ARG = -1
SENTINEL = 0xA5
THREADS = min(16, os.cpu_count() or 1)
SIZES = [1, 63, 64, 65, 127, 128, 129, 4096 + 77]


def _abi(name):
    """(host entry, device entry) of the C ABI"""
    from kyber_amd._lib import load

    stem = "kyb_ed25519_add" if name == "ed25519" else "kyb_%s_%s_add" % tuple(name.split("-"))
    return getattr(load(), stem), getattr(load(), stem + "_dev")


def _wrapper(name):
    """the Python batch entry: (a, b) -> (out, status), host buffers or CUDA tensors"""
    if name == "ed25519":
        from kyber_amd.group import edwards25519 as ed

        return ed.batch_add
    import importlib

    suite, g = name.split("-")
    return getattr(importlib.import_module("kyber_amd.pairing." + suite), g + "_batch_add")


def _mismatch(t, out, st):
    """the rows where (out, st) differ from the table's expectation, with their labels"""
    bad = np.nonzero((np.asarray(st) != t.status) | (np.asarray(out) != t.out).any(axis=1))[0]
    return [(int(i), t.labels[i], int(np.asarray(st)[i]), int(t.status[i])) for i in bad[:8]]


def _host_abi(name, a, b, n=None, status=True):
    """the host entry called directly: outputs one element longer than n and pre-filled, (rc, out, status)"""
    n = len(a) if n is None else n
    w = a.shape[1]
    out = np.full((n + 1, w), SENTINEL, dtype=np.uint8)
    st = np.full(n + 1, SENTINEL, dtype=np.uint8)
    rc = _abi(name)[0](n, a.ctypes.data, b.ctypes.data, out.ctypes.data, st.ctypes.data if status else None)
    return rc, out, st


def _dev_abi(name, a, b, n=None, status=True):
    """the device entry called directly on a stream of its own"""
    import torch

    n = len(a) if n is None else n
    w = a.shape[1]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        out = torch.full((n + 1, w), SENTINEL, dtype=torch.uint8, device="cuda")
        st = torch.full((n + 1,), SENTINEL, dtype=torch.uint8, device="cuda")
        rc = _abi(name)[1](n, da.data_ptr(), db.data_ptr(), out.data_ptr(), st.data_ptr() if status else None, s.cuda_stream)
        s.synchronize()
        return rc, out.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("name", A.GROUPS)
def test_case_table_host_and_device(name):
    """every labelled row, status and bytes, through the host entry and through the _dev entry on a non-default stream"""
    import torch

    t, add = A.table(name), _wrapper(name)
    out_h, st_h = add(t.a, t.b)
    assert not _mismatch(t, out_h, st_h), (name, "host", _mismatch(t, out_h, st_h))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_out, d_st = add(torch.from_numpy(t.a).cuda(), torch.from_numpy(t.b).cuda())
        s.synchronize()
        out_d, st_d = d_out.cpu().numpy(), d_st.cpu().numpy()
    assert not _mismatch(t, out_d, st_d), (name, "device", _mismatch(t, out_d, st_d))
    assert (out_h == out_d).all() and (st_h == st_d).all()


@pytest.mark.parametrize("name", A.GROUPS)
def test_case_table_tiled_and_shuffled(name):
    """the table eight times over in one shuffled batch (35 to 60 waves): rejected and infinite rows beside valid ones in
    every wave, every row compared"""
    import torch

    t = A.tiled(A.table(name), 8)
    assert len(t.labels) > 32 * 64
    add = _wrapper(name)
    out, st = add(t.a, t.b)
    assert not _mismatch(t, out, st), (name, "host", _mismatch(t, out, st))
    d_out, d_st = add(torch.from_numpy(t.a).cuda(), torch.from_numpy(t.b).cuda())
    assert not _mismatch(t, d_out.cpu().numpy(), d_st.cpu().numpy()), (name, "device")


@pytest.mark.parametrize("name", A.GROUPS)
def test_batch_sizes_and_nothing_written_past_n(name):
    """n either side of the block size (128 lanes on Ed25519, 64 on the pairing suites), n = 0: the whole batch against
    the oracle chain, the element behind the outputs untouched"""
    a, b, exp = A.chain(name, max(SIZES))
    for call in (_host_abi, _dev_abi):
        for n in [0] + SIZES:
            rc, out, st = call(name, a[:max(n, 1)].copy(), b[:max(n, 1)].copy(), n=n)
            assert rc == 0, (name, call.__name__, n)
            assert (out[:n] == exp[:n]).all() and not st[:n].any(), (name, call.__name__, n)
            assert (out[n:] == SENTINEL).all() and (st[n:] == SENTINEL).all(), (name, call.__name__, n, "written past n")


@pytest.mark.parametrize("name", A.GROUPS)
def test_null_status(name):
    """status = NULL (host: staged_call skips the buffer; device: the kernel skips the store): the same outputs, zero
    bytes on the rejected rows"""
    t = A.table(name)
    for call in (_host_abi, _dev_abi):
        rc, out, st = call(name, t.a, t.b, status=False)
        n = len(t.labels)
        assert rc == 0 and (out[:n] == t.out).all(), (name, call.__name__)
        assert (out[n:] == SENTINEL).all() and (st == SENTINEL).all(), (name, call.__name__)
        assert not out[:n][t.status != 0].any()


@pytest.mark.parametrize("name", A.GROUPS)
def test_argument_errors(name):
    import torch

    t = A.table(name)
    host, dev = _abi(name)
    a, b = t.a[:4].copy(), t.b[:4].copy()
    out, st = np.zeros_like(a), np.zeros(4, dtype=np.uint8)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dout, dst = torch.zeros_like(da), torch.zeros(4, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    for k in range(3):
        args = [a.ctypes.data, b.ctypes.data, out.ctypes.data]
        args[k] = None
        assert host(4, *args, st.ctypes.data) == KYB_E_ARG, (name, k)
        assert host(0, *args, st.ctypes.data) == 0, (name, k)
        dargs = [da.data_ptr(), db.data_ptr(), dout.data_ptr()]
        dargs[k] = None
        assert dev(4, *dargs, dst.data_ptr(), stream) == KYB_E_ARG, (name, k)
    torch.cuda.synchronize()
    assert not out.any() and not dout.any().item()


@pytest.mark.parametrize("name", A.GROUPS)
def test_python_wrappers(name):
    import torch

    t, add = A.table(name), _wrapper(name)
    with pytest.raises(ValueError):
        add(t.a[:5], t.b[:4])
    with pytest.raises(ValueError):
        add(torch.from_numpy(t.a[:5]).cuda(), torch.from_numpy(t.b[:4]).cuda())
    out, st = add(t.a[:70].tobytes(), t.b[:70].tobytes())  # plain bytes
    assert (out == t.out[:70]).all() and (st == t.status[:70]).all()
    if name != "ed25519":  # _engine.add: a on the device, b a host buffer
        n = len(t.labels)
        for hb in (t.b, t.b.tobytes(), torch.from_numpy(t.b)):
            out, st = add(torch.from_numpy(t.a).cuda(), hb)
            assert out.is_cuda and (out.cpu().numpy() == t.out).all() and (st.cpu().numpy() == t.status).all()
        with pytest.raises(ValueError):
            add(torch.from_numpy(t.a).cuda(), t.b[:n - 1])


def _scalar_rows(order, n, seed, byteorder):
    """(k, m, k + m mod order) as (n, 32) byte arrays: random below the order, with k + m = 0 and k = m rows sprinkled in"""
    rng = random.Random(seed)
    ks = [rng.randrange(order) for _ in range(n)]
    ms = [rng.randrange(order) for _ in range(n)]
    for i in range(0, n, 997):
        ms[i] = (order - ks[i]) % order
    for i in range(500, n, 997):
        ms[i] = ks[i]
    ks[n - 1], ms[n - 2] = 0, 0
    ms[n - 1] = 0  # 0 G + 0 G in the ragged tail
    arr = lambda v: np.frombuffer(b"".join(x.to_bytes(32, byteorder) for x in v), dtype=np.uint8).reshape(n, 32).copy()
    return ks, ms, arr(ks), arr(ms), arr([(k + m) % order for k, m in zip(ks, ms)])


@pytest.mark.parametrize("name", ["ed25519", "bls12381-g1", "bls12381-g2", "bn256-g1", "bn256-g2"])
def test_whole_batch_at_scale_against_the_c_oracle(name):
    """a = k G, b = m G and the expectation ((k + m) mod r) G all come from the C oracle; device-resident data, every
    output byte compared.  2^20 + 5 elements on Ed25519 (the size of README's Add figure), 2^16 + 5 on the pairing groups."""
    import torch

    from tests import _oracle_c as OC

    G = A.group(name)
    n = (1 << 20) + 5 if name == "ed25519" else (1 << 16) + 5
    _, _, k, m, km = _scalar_rows(G.order, n, "scale/" + name, "little" if name == "ed25519" else "big")
    if name == "ed25519":
        a, b, exp = (OC.ed_mul_base(s, threads=THREADS) for s in (k, m, km))
    else:
        fn = getattr(OC, name.replace("-", "_") + "_mul")
        base = np.tile(np.frombuffer(G.enc(G.gen), dtype=np.uint8), (n, 1))
        (a, sa), (b, sb), (exp, se) = (fn(s, base, threads=THREADS) for s in (k, m, km))
        assert not sa.any() and not sb.any() and not se.any()
    inf = np.frombuffer(G.enc(G.inf), dtype=np.uint8)
    assert (exp[0] == inf).all() and (exp[n - 1] == inf).all() and (a[500] == b[500]).all()
    out, st = _wrapper(name)(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    out, st = out.cpu().numpy(), st.cpu().numpy()
    assert not st.any()
    wrong = np.nonzero((out != exp).any(axis=1))[0]
    assert wrong.size == 0, (name, wrong[:8])


@pytest.mark.parametrize("name", ["bn254-g1", "bn254-g2"])
def test_whole_batch_at_scale_bn254(name):
    """bn254 has no C oracle: a = k G and b = m G are the engine's own multiples of the generator; 67 lanes at a stride
    (a, b and the sum: Python oracle, the sum both as a + b and as (k + m) G), and all 2^16 + 5 lanes against the engine's
    own multiplication by k + m -- that second comparison is NOT independent of the engine, it only ties every lane to the
    sampled ones."""
    import torch

    from kyber_amd.pairing import bn254 as m4
    from oracle import bn254 as O

    G = A.group(name)
    g = 1 if name.endswith("g1") else 2
    n = (1 << 16) + 5
    ks, ms, k, m, km = _scalar_rows(G.order, n, "scale/" + name, "big")
    commit = m4.ENGINE.g1_commit if g == 1 else m4.ENGINE.g2_commit
    (a, sa), (b, sb), (exp, se) = (commit(torch.from_numpy(s).cuda()) for s in (k, m, km))
    assert not sa.any().item() and not sb.any().item() and not se.any().item()
    out, st = _wrapper(name)(a, b)
    assert not st.any().item()
    wrong = torch.nonzero((out != exp).any(dim=1)).flatten()
    assert wrong.numel() == 0, (name, wrong[:8].tolist())
    ah, bh, oh = a.cpu().numpy(), b.cpu().numpy(), out.cpu().numpy()
    lanes = sorted(set(list(range(0, n, 997)) + [500, 1497, n - 2, n - 1]))
    assert len(lanes) >= 64
    for i in lanes:
        pa, pb = G.mul(ks[i], G.gen), G.mul(ms[i], G.gen)
        assert bytes(ah[i]) == G._enc(pa) and bytes(bh[i]) == G._enc(pb), (name, i)
        assert bytes(oh[i]) == G._enc(G.add(pa, pb)) == G._enc(G.mul((ks[i] + ms[i]) % O.ORDER, G.gen)), (name, i)


@pytest.mark.parametrize("name", A.GROUPS)
def test_two_streams_two_threads(name):
    """two host threads, a stream each, different batches at the same time, three calls each: what the serial run gives"""
    import torch

    add = _wrapper(name)
    batches = [A.tiled(A.table(name), 6, seed=11), A.tiled(A.table(name), 9, seed=12)]
    d_in = [(torch.from_numpy(t.a).cuda(), torch.from_numpy(t.b).cuda()) for t in batches]
    serial = [tuple(x.cpu().numpy() for x in add(*d)) for d in d_in]
    for t, (o, s) in zip(batches, serial):
        assert not _mismatch(t, o, s)
    streams = [torch.cuda.Stream() for _ in batches]
    torch.cuda.synchronize()
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def work(i):
        try:
            with torch.cuda.stream(streams[i]):
                gate.wait()
                outs = [add(*d_in[i]) for _ in range(3)]
                streams[i].synchronize()
                results[i] = [(o.cpu().numpy(), s.cpu().numpy()) for o, s in outs]
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    assert not errors, errors
    for i in range(2):
        for o, s in results[i]:
            assert (o == serial[i][0]).all() and (s == serial[i][1]).all(), (name, i)


@pytest.mark.parametrize("vartime", [False, True])
def test_mul2_is_add_of_muls_on_torsion_and_noncanonical_operands(vartime):
    """include/kyber_hip.h: kyb_ed25519_mul2(a, P, b, Q) is byte-identical to add(mul(a, P), mul(b, Q)) under the same
    flag -- here with P, Q among the eight torsion points, the non-canonical encodings and the non-points of the table"""
    from kyber_amd.group import edwards25519 as ed
    from oracle import ed25519 as O

    rng = random.Random(77)
    special = [O.encode(p) for p in A.torsion_points()] + A.ed_noncanonical() + A.ed_non_points()
    prime = [bytes(r) for r in A.chain("ed25519", 16)[0]]
    edge = [0, 1, 2, 4, 8, O.L - 1, O.L, O.L + 1, (1 << 255) - 1, 1 << 255, (1 << 256) - 1]
    rows = []
    for i, s in enumerate(special):
        for t in (special[(i + 1) % len(special)], special[(3 * i + 5) % len(special)], prime[i % 16], s):
            for _ in range(2):
                ka = rng.choice(edge) if rng.random() < 0.4 else rng.getrandbits(256)
                kb = rng.choice(edge) if rng.random() < 0.4 else rng.getrandbits(256)
                rows.append((ka, s, kb, t))
                rows.append((kb, t, ka, s))
    n = len(rows)
    arr = lambda col, enc: np.frombuffer(b"".join(enc(r[col]) for r in rows), dtype=np.uint8).reshape(n, 32).copy()
    le = lambda v: v.to_bytes(32, "little")
    a, P, b, Q = arr(0, le), arr(1, bytes), arr(2, le), arr(3, bytes)
    out2, st2 = ed.batch_mul2(a, P, b, Q, vartime=vartime)
    (aP, s1), (bQ, s2) = ed.batch_mul(a, P, vartime=vartime), ed.batch_mul(b, Q, vartime=vartime)
    out, st = ed.batch_add(aP, bQ)
    bad = (s1 != 0) | (s2 != 0)
    assert bad.any() and (st2[bad] == 1).all() and not out2[bad].any() and not st2[~bad].any()
    assert not st[~bad].any() and (out2[~bad] == out[~bad]).all()
    for i in range(0, n, 7):  # and a sample against the oracle, so that the two sides cannot be wrong together
        if not bad[i]:
            exp = O.add(O.decode(O.mul(le(rows[i][0]), rows[i][1], vartime)), O.decode(O.mul(le(rows[i][2]), rows[i][3], vartime)))
            assert bytes(out2[i]) == O.encode(exp), i
