#!/usr/bin/env python3
"""Times Ed25519 verification and a*P + b*Q, fused against composed, in one process, alternating, median of 20 after a
warm-up: end to end from host buffers (PCIe and the host's share included) at 2^16 and 2^18 valid signatures over
32-byte messages.  Signatures come from the oracle's C restatement (r*B, S = r + h a), checked by the composed path.
  tools/ed_verify_probe.py [out.json]          the end-to-end table (profiler off)
  tools/ed_verify_probe.py --once N            one pass of each path at N elements: the body of a
                                               `rocprofv3 --kernel-trace --stats -- python tools/ed_verify_probe.py --once N`
                                               run, whose per-kernel sums tools/ed_verify_probe.py --stats DIR adds up.
"""
import csv
import glob
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FUSED = ("ed25519_verify_kernel", "ed25519_verify_encode_kernel")
MUL2 = ("ed25519_mul2_kernel", "ed25519_mul2_encode_kernel")
COMPOSED = ("ed25519_mul_kernel", "ed25519_mul_base_kernel", "ed25519_add_kernel", "ed25519_encode_kernel")


def make(n):
    from kyber_amd.group import edwards25519 as ed

    rng = np.random.default_rng(n)
    L = ed.ORDER
    red = lambda a: np.frombuffer(b"".join((int.from_bytes(bytes(x), "little") % L).to_bytes(32, "little") for x in a), dtype=np.uint8).reshape(-1, 32)
    a, r = red(rng.integers(0, 256, size=(n, 32), dtype=np.uint8)), red(rng.integers(0, 256, size=(n, 32), dtype=np.uint8))
    A, R = ed.batch_mul_base(a), ed.batch_mul_base(r)
    msgs = [bytes(m) for m in rng.integers(0, 256, size=(n, 32), dtype=np.uint8)]
    sigs = []
    for i in range(n):
        h = int.from_bytes(hashlib.sha512(bytes(R[i]) + bytes(A[i]) + msgs[i]).digest(), "little") % L
        s = (int.from_bytes(bytes(r[i]), "little") + h * int.from_bytes(bytes(a[i]), "little")) % L
        sigs.append(bytes(R[i]) + s.to_bytes(32, "little"))
    return [bytes(x) for x in A], msgs, sigs, (a, A, r, R)


def paths(n):
    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.sign import eddsa

    pubs, msgs, sigs, (a, A, r, R) = make(n)

    def mul2_composed():
        x, _ = ed.batch_mul(a, A)
        y, _ = ed.batch_mul(r, R)
        return ed.batch_add(x, y)[0]

    return {"verify_fused": lambda: eddsa.batch_verify_with_checks(pubs, msgs, sigs),
            "verify_composed": lambda: eddsa._batch_verify_composed(pubs, msgs, sigs),
            "mul2_fused": lambda: ed.batch_mul2(a, A, r, R)[0], "mul2_composed": mul2_composed}


def timed(n, reps=20):
    p = paths(n)
    outs = {k: f() for k, f in p.items()}  # warm-up, and the answers
    assert outs["verify_fused"].all() and outs["verify_composed"].all()
    assert (np.asarray(outs["mul2_fused"]) == np.asarray(outs["mul2_composed"])).all()
    ts = {k: [] for k in p}
    for _ in range(reps):
        for k, f in p.items():  # alternating
            t0 = time.perf_counter()
            f()
            ts[k].append(time.perf_counter() - t0)
    res = {"n": n}
    for k, v in ts.items():
        v = sorted(v)
        res[k + "_ms_end_to_end"] = {"median": 1e3 * v[len(v) // 2], "min": 1e3 * v[0], "max": 1e3 * v[-1]}
    res["verify_signatures_per_s_end_to_end"] = n / (res["verify_fused_ms_end_to_end"]["median"] / 1e3)
    res["verify_end_to_end_ratio"] = res["verify_fused_ms_end_to_end"]["median"] / res["verify_composed_ms_end_to_end"]["median"]
    res["mul2_end_to_end_ratio"] = res["mul2_fused_ms_end_to_end"]["median"] / res["mul2_composed_ms_end_to_end"]["median"]
    return res


def stats(d):
    """summed kernel time (ms) per path from the kernel-trace CSVs under d; one pass of each path was traced"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    assert rows, "no kernel trace under " + d
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    name = lambda r: r["Kernel_Name"]
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    # the four passes run in the order of paths(): fused verify, composed verify, fused mul2, composed mul2; the trace is
    # cut at the first and last kernel of each fused pass
    iv = [i for i, r in enumerate(rows) if FUSED[0] in name(r)]
    im = [i for i, r in enumerate(rows) if MUL2[0] in name(r)]
    seg = {"verify_fused": [r for r in rows[iv[0]:] if any(k in name(r) for k in FUSED)],
           "verify_composed": [r for r in rows[iv[-1]:im[0]] if any(k in name(r) for k in COMPOSED)],
           "mul2_fused": [r for r in rows if any(k in name(r) for k in MUL2)],
           "mul2_composed": [r for r in rows[im[-1]:] if any(k in name(r) for k in COMPOSED)]}
    out = {k + "_kernel_ms": sum(dur(r) for r in v) for k, v in seg.items()}
    out.update({k + "_kernels": len(v) for k, v in seg.items()})
    out["verify_kernel_time_ratio"] = out["verify_fused_kernel_ms"] / out["verify_composed_kernel_ms"]
    out["mul2_kernel_time_ratio"] = out["mul2_fused_kernel_ms"] / out["mul2_composed_kernel_ms"]
    return out


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--once":
        import torch

        for k, f in paths(int(sys.argv[2])).items():
            f()
            torch.cuda.synchronize()
    elif len(sys.argv) > 2 and sys.argv[1] == "--stats":
        print(json.dumps(stats(sys.argv[2])))
    else:
        res = {"what": "Ed25519 verify / a*P + b*Q, fused against composed; end to end from host buffers, median of 20, alternating",
               "sizes": [timed(1 << 16), timed(1 << 18)]}
        line = json.dumps(res)
        print(line)
        if len(sys.argv) > 1:
            open(sys.argv[1], "w").write(line + "\n")
