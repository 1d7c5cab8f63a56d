"""The standard base's wide fixed-base comb (ed25519.hip EdWide): its rows against the oracle, and the fixed-base
batches that read it -- default and KYB_F_VARTIME, device and host buffers, edge scalars, concurrent streams, every
device -- against the C oracle."""
import ctypes
import os
import threading

import numpy as np
import pytest

from oracle import ed25519 as O
from tests import _oracle_c as OC

pytestmark = pytest.mark.gpu

THREADS = min(16, os.cpu_count() or 1)
B_ENC = np.frombuffer(O.encode(O.B), dtype=np.uint8)


@pytest.fixture(scope="module")
def ed():
    import torch

    assert torch.cuda.is_available()
    from kyber_amd.group import edwards25519 as ed

    return ed


@pytest.fixture(scope="module")
def info(ed):
    from kyber_amd import _lib

    a = (ctypes.c_int64 * 6)()
    _lib.check(_lib.load().kyb_ed25519_comb_info(a), "kyb_ed25519_comb_info")
    g, pos, ent, last, nbytes, _build_us = list(a)
    return {"G": g, "POS": pos, "ENT": ent, "LAST": last, "BYTES": nbytes}


def _val(l):
    x, off = 0, 0
    for i in range(10):
        x += int(l[i]) << off
        off += 25 if i & 1 else 26
    return x % O.P


def _rows(pos, row0, nrows):
    from kyber_amd import _lib

    out = np.zeros(nrows * 32, dtype=np.int32)
    _lib.check(_lib.load().kyb_ed25519_debug_comb_table(pos, row0, nrows, out.ctypes.data), "debug_comb_table")
    return out.reshape(nrows, 32)


def test_comb_shape(info):
    g = info["G"]
    assert g >= 3
    assert info["POS"] == -(-65 // g)
    assert info["ENT"] == 8 * (16 ** g - 1) // 15
    assert info["LAST"] == 8 * (16 ** (65 - g * (info["POS"] - 1)) - 1) // 15
    assert info["BYTES"] == ((info["POS"] - 1) * info["ENT"] + info["LAST"]) * 128


def test_comb_rows_match_oracle(info):
    g, npos, ent = info["G"], info["POS"], info["ENT"]
    for pos in sorted({0, 1, npos // 2, npos - 2, npos - 1}):
        nrows = info["LAST"] if pos == npos - 1 else ent
        for j in sorted({0, 1, 7, 8, 15, 16, 135, 136, 2183, nrows // 2, nrows - 2, nrows - 1}):
            if j >= nrows:
                continue
            r = _rows(pos, j, 1)[0]
            assert not r[30:].any()
            x, y = O.mul_int((j + 1) << (4 * g * pos), O.B)
            assert _val(r[0:10]) == (y + x) % O.P, (pos, j)
            assert _val(r[10:20]) == (y - x) % O.P, (pos, j)
            assert _val(r[20:30]) == 2 * O.D * x * y % O.P, (pos, j)
    # a run of consecutive rows across the middle of position 1 agrees row by row with single-row reads
    run = _rows(1, ent // 2 - 8, 16)
    for i in (0, 15):
        assert (run[i] == _rows(1, ent // 2 - 8 + i, 1)[0]).all()


def test_debug_comb_table_rejects_out_of_range(info):
    from kyber_amd import _lib

    buf = np.zeros(32, dtype=np.int32)
    lib = _lib.load()
    assert lib.kyb_ed25519_debug_comb_table(info["POS"], 0, 1, buf.ctypes.data) != 0
    assert lib.kyb_ed25519_debug_comb_table(info["POS"] - 1, info["LAST"], 1, buf.ctypes.data) != 0
    assert lib.kyb_ed25519_debug_comb_table(0, info["ENT"] - 1, 2, buf.ctypes.data) != 0
    assert lib.kyb_ed25519_debug_comb_table(-1, 0, 1, buf.ctypes.data) != 0


def _scalars(seed, n, top_mask=0xFF):
    s = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= top_mask
    return s


def test_fixed_base_2p20_vs_c_oracle(ed):
    import torch

    s = _scalars(21, 1 << 20)  # every bit random: half the scalars >= 2^255
    out = ed.batch_mul_base(torch.from_numpy(s).cuda()).cpu().numpy()
    assert (out == OC.ed_mul_base(s, threads=THREADS)).all()


def test_fixed_base_vartime_2p20(ed):
    import torch

    # below 2^252 the all-bits semantics and the constant-time recoding multiply by the same integer
    s = _scalars(22, 1 << 20, 0x0F)
    d_s = torch.from_numpy(s).cuda()
    out_vt = ed.batch_mul_base(d_s, vartime=True).cpu().numpy()
    assert (out_vt == ed.batch_mul_base(d_s).cpu().numpy()).all()
    assert (out_vt[::64] == OC.ed_mul_base(s[::64], threads=THREADS)).all()
    # every 256-bit value, against geScalarMultVartime's oracle on the base point
    f = _scalars(23, 8192)
    exp, st = OC.ed_mul(f, np.tile(B_ENC, (len(f), 1)), vartime=True, threads=THREADS)
    assert not st.any()
    assert (ed.batch_mul_base(torch.from_numpy(f).cuda(), vartime=True).cpu().numpy() == exp).all()


def _edge_scalars():
    vals = [0, 1, 2, 7, 8, 9, O.L - 1, O.L, O.L + 1, 2**252 - 1, 2**252, 2**253 - 1, 2**255 - 1, 2**255,
            2**255 + 1, 2**256 - 1, 2**256 - O.L]
    # nibbles 8, 7, 7, ...: every signed radix-16 digit -8, so every comb digit at its largest magnitude (the last row)
    vals.append(int("7" * 63 + "8", 16))
    vals.append(int("f" + "7" * 62 + "8", 16))
    # nibbles all 8 / all 7 / alternating 8 and 0: digits alternating in sign, the top digit at +8 and above
    vals += [int("8" * 64, 16), int("7" * 64, 16), int("80" * 32, 16), int("08" * 32, 16)]
    # one non-zero radix-16 digit at a time, each at +-1 and +-8, and one comb position at a time
    vals += [8 << (4 * i) for i in range(0, 64, 5)] + [(2**256 - (1 << (4 * i))) for i in range(0, 64, 7)]
    vals += [(2**16 - 1) << (16 * k) for k in range(16)] + [(2**12 - 1) << (12 * k) for k in range(21)]
    return np.array([list(v.to_bytes(32, "little")) for v in vals], dtype=np.uint8)


@pytest.mark.parametrize("n_pad", [0, 8192])  # encoded in the kernel / deferred to the encode kernel
def test_fixed_base_edge_scalars(ed, n_pad):
    import torch

    e = _edge_scalars()
    s = np.concatenate([e, _scalars(24, n_pad)]) if n_pad else e
    d_s = torch.from_numpy(s).cuda()
    out = ed.batch_mul_base(d_s).cpu().numpy()
    assert (out[: len(e)] == OC.ed_mul_base(e, threads=THREADS)).all()
    exp_vt, st = OC.ed_mul(e, np.tile(B_ENC, (len(e), 1)), vartime=True, threads=THREADS)
    assert not st.any()
    assert (ed.batch_mul_base(d_s, vartime=True).cpu().numpy()[: len(e)] == exp_vt).all()
    assert bytes(out[0]) == O.encode(O.IDENTITY)
    for i in (1, 6):
        assert bytes(out[i]) == O.mul_base(bytes(e[i]))


def test_fixed_base_comb_equals_uniform_scan(ed):
    import torch

    # KYB_F_UNIFORM keeps the radix-256 table and its scan: both paths give the same bytes
    d_s = torch.from_numpy(_scalars(25, 65536)).cuda()
    assert torch.equal(ed.batch_mul_base(d_s), ed.batch_mul_base(d_s, uniform=True))


def test_fixed_base_host_buffers_pipelined(ed):
    s = _scalars(26, 3 * (1 << 17) + 5)  # more than two pipeline chunks, a ragged tail
    assert (ed.batch_mul_base(s) == OC.ed_mul_base(s, threads=THREADS)).all()


def test_fixed_base_two_streams_two_threads(ed):
    import torch

    inputs = [_scalars(27 + i, (1 << 18) + 17 * i) for i in range(2)]
    expect = [OC.ed_mul_base(s, threads=THREADS) for s in inputs]
    d_in = [torch.from_numpy(s).cuda() for s in inputs]
    streams = [torch.cuda.Stream() for _ in inputs]
    results, errors = [None, None], []
    gate = threading.Barrier(2)

    def work(i):
        try:
            with torch.cuda.stream(streams[i]):
                gate.wait()
                outs = [ed.batch_mul_base(d_in[i]) for _ in range(3)]
                streams[i].synchronize()
                results[i] = [o.cpu().numpy() for o in outs]
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i in range(2):
        for o in results[i]:
            assert (o == expect[i]).all()


def test_fixed_base_every_device(ed):
    import torch

    s = _scalars(28, 4096 + 3)
    exp = OC.ed_mul_base(s, threads=THREADS)
    for dev in range(torch.cuda.device_count()):
        with torch.cuda.device(dev):
            out = ed.batch_mul_base(torch.from_numpy(s).to(f"cuda:{dev}")).cpu().numpy()
        assert (out == exp).all(), dev


@pytest.mark.parametrize("vartime", [False, True])
def test_var_base_edge_scalars_signed_loads(ed, vartime):
    import torch

    # the variable-base window takes the entry's sign and the zero digit by load address (ed25519.hip
    # TabGlobal::get_signed): a batch large enough for the global slab, edge scalars up front
    e = _edge_scalars()
    s = np.concatenate([e, _scalars(29, 8192)])
    pts = OC.ed_mul_base(_scalars(30, len(s), 0x0F), threads=THREADS)
    exp, est = OC.ed_mul(s, pts, vartime=vartime, threads=THREADS)
    out, st = ed.batch_mul(torch.from_numpy(s).cuda(), torch.from_numpy(pts).cuda(), vartime=vartime)
    assert (st.cpu().numpy() == est).all() and (out.cpu().numpy() == exp).all()
