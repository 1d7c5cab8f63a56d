#!/usr/bin/env python3
"""Times the two fused calls of sign/eddsa against the standing calls that reach the same bytes, at N = 2^16 elements, as
summed kernel time from a kernel trace (medians of 20 alternating passes after a warm-up; host buffers -- copies are no
kernels):
  * "sign32", "sign1024":  kyb_ed25519_eddsa_sign of 32-byte and of 1 024-byte messages under 2^16 keys against
                           kyb_ed25519_schnorr_sign with k = r, where r = SHA-512(prefix || msg) mod l comes from hashlib
                           on the host.  The kernel trace sets the fused call's kernels (both hashes on the device)
                           against schnorr_sign's alone (one hash; r's is no kernel); --e2e takes the wall time of both
                           paths from host buffers, the composed one with its host hashing.
  * "expand":              kyb_ed25519_eddsa_expand of 2^16 seeds against kyb_ed25519_mul_base of the 2^16 secrets (the
                           seeds' SHA-512 on the host is no kernel either).
  tools/ed_eddsa_probe.py --once WHAT N     21 alternating passes of the fused call and its composed counterpart: the body of
                                            `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ed_eddsa_probe.py --once WHAT N`
  tools/ed_eddsa_probe.py --stats DIR       per-pass summed kernel time from that trace (medians of the last 20)
  tools/ed_eddsa_probe.py --e2e WHAT N      wall time of both paths from host buffers (median of 5)
  tools/ed_eddsa_probe.py --merge OUT sign32=STATS sign1024=STATS expand=STATS [sign32_e2e=E2E ...]     profiles/ed_eddsa_probe.json
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

FUSED = ("ed25519_eddsa_expand_kernel", "ed25519_eddsa_encode_kernel", "ed25519_eddsa_nonce_kernel", "ed25519_eddsa_sign_kernel")
WHAT = ("summed kernel time from a kernel trace at 2^16 elements, medians of 20 alternating passes; *_e2e: wall time from host "
        "buffers, median of 5, the composed path with its hashlib hashing")
L = 2**252 + 27742317777372353535851937790883648493


def paths(what: str, n: int):
    from kyber_amd.group import edwards25519 as ed

    rng = np.random.default_rng(n + len(what))
    seeds = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    if what == "expand":
        def composed():
            d = [bytearray(hashlib.sha512(bytes(s)).digest()[:32]) for s in seeds]
            for x in d:
                x[0] &= 0xF8
                x[31] = (x[31] & 0x7F) | 0x40
            return ed.batch_mul_base(b"".join(d))

        return {"fused": lambda: ed.batch_eddsa_expand(seeds), "composed": composed}
    mlen = {"sign32": 32, "sign1024": 1024}[what]
    secrets, prefixes, pubs = (np.asarray(x) for x in ed.batch_eddsa_expand(seeds))
    msgs = [bytes(m) for m in rng.integers(0, 256, size=(n, mlen), dtype=np.uint8)]
    pre = [bytes(p) for p in prefixes]

    def composed():
        r = b"".join((int.from_bytes(hashlib.sha512(p + m).digest(), "little") % L).to_bytes(32, "little") for p, m in zip(pre, msgs))
        return ed.batch_schnorr_sign(r, secrets, msgs)

    return {"fused": lambda: ed.batch_eddsa_sign(secrets, prefixes, pubs, msgs), "composed": composed}


def stats(d):
    """per-pass summed kernel time (ms) from the kernel-trace CSVs under d: the trace alternates the fused call and its
    composed counterpart, a pass being a run of consecutive Ed25519 kernels of one of them"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    assert rows, "no kernel trace under " + d
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    name_of = lambda r: r["Kernel_Name"].split("(")[0].split("::")[-1].split("<")[0]
    kind = lambda r: "fused" if name_of(r) in FUSED else (None if r["Kernel_Name"].startswith("__amd_rocclr") else "composed")
    passes, prev = {"fused": [], "composed": []}, None
    for r in rows:
        k = kind(r)
        if k is None:
            continue
        if k != prev:
            passes[k].append([0.0, {}])
            prev = k
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        passes[k][-1][0] += ms
        passes[k][-1][1][name_of(r)] = passes[k][-1][1].get(name_of(r), 0.0) + ms
    out = {}
    for k, v in passes.items():
        v = v[-20:]  # the passes after the warm-up and the set-up's own expansion
        ms = sorted(x[0] for x in v)
        out[k + "_kernel_ms"] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "passes": len(ms)}
        out[k + "_kernels_of_the_last_pass_ms"] = v[-1][1]
    out["kernel_time_ratio"] = out["fused_kernel_ms"]["median"] / out["composed_kernel_ms"]["median"]
    return out


def e2e(what: str, n: int):
    import torch

    p = paths(what, n)
    out = {}
    for k in ("fused", "composed"):
        p[k]()  # warm-up
        torch.cuda.synchronize()
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            p[k]()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3)
        t.sort()
        out[k + "_wall_ms"] = {"median": t[2], "min": t[0], "max": t[-1]}
    out["wall_time_ratio"] = out["fused_wall_ms"]["median"] / out["composed_wall_ms"]["median"]
    return out


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--once":
        import torch

        p = paths(sys.argv[2], int(sys.argv[3]))
        for _ in range(21):
            for k in ("fused", "composed"):
                p[k]()
                torch.cuda.synchronize()
    elif len(sys.argv) > 2 and sys.argv[1] == "--stats":
        print(json.dumps(stats(sys.argv[2])))
    elif len(sys.argv) > 3 and sys.argv[1] == "--e2e":
        print(json.dumps(e2e(sys.argv[2], int(sys.argv[3]))))
    elif len(sys.argv) > 3 and sys.argv[1] == "--merge":
        out = {"what": WHAT}
        for arg in sys.argv[3:]:
            what, path = arg.split("=", 1)
            out[what] = json.load(open(path))
        open(sys.argv[2], "w").write(json.dumps(out) + "\n")
    else:
        print(__doc__)
