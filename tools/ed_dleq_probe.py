#!/usr/bin/env python3
"""Times proof/dleq verification on Ed25519, the fused call (kyb_ed25519_dleq_verify) against the composed five-call
path (mul2, mul2, unmarshal, unmarshal, compare on the host), and the challenge kernel against the host's Python XOF,
in one process, alternating, medians of 20 after a warm-up, at 2^16 valid proofs.
  tools/ed_dleq_probe.py [out.json]      end to end from host buffers (PCIe and the host's share included; profiler off),
                                         plus the throughput of the two PVSS-shaped calls
  tools/ed_dleq_probe.py --once N        21 alternating passes of both paths at N proofs: the body of a
                                         `rocprofv3 --kernel-trace --stats -d DIR -- python tools/ed_dleq_probe.py --once N`
  tools/ed_dleq_probe.py --stats DIR     per-pass summed kernel time from that trace: medians over the 20 passes after the
                                         first, and their ratio (yardstick A)
"""
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FUSED = ("ed25519_dleq_kernel", "ed25519_dleq_encode_kernel")
COMPOSED = ("ed25519_mul2_kernel", "ed25519_mul2_encode_kernel", "ed25519_unmarshal_kernel", "ed25519_encode_kernel")


def make(n):
    """n valid proofs with Fiat-Shamir challenges, made by the engine; G shared or not is the caller's choice of rows"""
    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.proof import dleq

    rng = np.random.default_rng(n)
    rand = lambda k: rng.integers(0, 256, size=k, dtype=np.uint8).tobytes()
    sc = lambda: np.frombuffer(b"".join(ed.Scalar().Pick(rand).v for _ in range(n)), dtype=np.uint8).reshape(n, 32)
    G, H = ed.batch_mul_base(sc()), ed.batch_mul_base(sc())
    proofs, xG, xH = dleq.NewDLEQProofs(G, H, sc(), rand)
    col = lambda k: np.frombuffer(b"".join(getattr(p, k) for p in proofs), dtype=np.uint8).reshape(n, 32)
    return [G, H, np.asarray(xG), np.asarray(xH), col("C"), col("R"), col("VG"), col("VH")]


def paths(a):
    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.proof import dleq

    return {"fused": lambda: ed.batch_dleq_verify(*a)[0] != 0, "composed": lambda: dleq.batch_verify_composed(*a)}


def median_of(ts):
    v = sorted(ts)
    return {"median": 1e3 * v[len(v) // 2], "min": 1e3 * v[0], "max": 1e3 * v[-1]}


def timed(n, reps=20):
    import hashlib

    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.util import blake2xb

    a = make(n)
    p = paths(a)
    # the PVSS-shaped calls: VerifyDecShareBatch (G shared, challenges derived on the device) and VerifyEncShareBatch's
    # engine call (one base shared, one expected challenge: only proof 0 carries it, the others do the same work and
    # fail the byte comparison)
    p["verify_dec_share_batch"] = lambda: ed.batch_dleq_verify(a[0][:1], a[1], *a[2:], fiat_shamir=True)[0] != 0
    p["verify_enc_share_batch"] = lambda: ed.batch_dleq_verify(a[0][:1], a[1], *a[2:], expect_c=a[4][0])[0] != 0
    p["challenge_device"] = lambda: ed.batch_dleq_challenge(a[2], a[3], a[6], a[7])[0]
    outs = {k: f() for k, f in p.items()}  # warm-up, and the answers
    assert outs["fused"].all() and outs["composed"].all() and (np.asarray(outs["challenge_device"]) == a[4]).all()
    ts = {k: [] for k in p}
    for _ in range(reps):
        for k, f in p.items():  # alternating
            t0 = time.perf_counter()
            f()
            ts[k].append(time.perf_counter() - t0)
    res = {"n": n}
    for k, v in ts.items():
        res[k + "_ms_end_to_end"] = median_of(v)
    res["end_to_end_ratio_A"] = res["fused_ms_end_to_end"]["median"] / res["composed_ms_end_to_end"]["median"]
    for k in ("verify_dec_share_batch", "verify_enc_share_batch"):
        res[k + "_shares_per_s"] = n / (res[k + "_ms_end_to_end"]["median"] / 1e3)
    # yardstick B, reported only: the same challenges by the host's Python XOF, timed on the first m inputs
    m = min(n, 2048)
    t0 = time.perf_counter()
    for i in range(m):
        c = blake2xb.pick(blake2xb.New(hashlib.sha256(b"".join(a[k][i].tobytes() for k in (2, 3, 6, 7))).digest()).Read)
    host = (time.perf_counter() - t0) / m
    assert c == a[4][m - 1].tobytes()
    res["challenge_host_python_us_per_element"] = 1e6 * host
    res["challenge_host_python_sample"] = m
    res["challenge_device_us_per_element_end_to_end"] = 1e3 * res["challenge_device_ms_end_to_end"]["median"] / n
    res["challenge_ratio_B"] = res["challenge_device_us_per_element_end_to_end"] / res["challenge_host_python_us_per_element"]
    return res


def stats(d):
    """per-pass summed kernel time (ms) of each path from the kernel-trace CSVs under d: the trace alternates fused and
    composed passes, a pass being a run of consecutive kernels of one path"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    assert rows, "no kernel trace under " + d
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    kind = lambda r: "fused" if any(k in r["Kernel_Name"] for k in FUSED) else ("composed" if any(k in r["Kernel_Name"] for k in COMPOSED) else None)
    passes, prev = {"fused": [], "composed": []}, None
    for r in rows:
        k = kind(r)
        if k is None:
            continue
        if k != prev:
            passes[k].append([0.0, 0])
            prev = k
        passes[k][-1][0] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        passes[k][-1][1] += 1
    out = {}
    for k, v in passes.items():
        v = v[-20:]  # the passes after the warm-up (setup launches mul2 / encode kernels of its own before them)
        ms = sorted(x[0] for x in v)
        out[k + "_kernel_ms"] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "passes": len(ms)}
        out[k + "_kernels_per_pass"] = v[-1][1]
    out["kernel_time_ratio_A"] = out["fused_kernel_ms"]["median"] / out["composed_kernel_ms"]["median"]
    return out


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--once":
        import torch

        p = paths(make(int(sys.argv[2])))
        for _ in range(21):
            for k in ("fused", "composed"):
                assert p[k]().all()
                torch.cuda.synchronize()
    elif len(sys.argv) > 2 and sys.argv[1] == "--stats":
        print(json.dumps(stats(sys.argv[2])))
    else:
        line = json.dumps({"what": "proof/dleq verify on Ed25519, fused against composed; end to end from host buffers, "
                                   "median of 20, alternating", "sizes": [timed(1 << 16)]})
        print(line)
        if len(sys.argv) > 1:
            open(sys.argv[1], "w").write(line + "\n")
