#!/usr/bin/env python3
"""Times sign/anon verification on Ed25519 at 2^16 signatures over one shared ring, ring 10 and ring 100, unlinkable and
linkable: the fused call (kyb_ed25519_ring_chain) against the path composed from the entry points that existed before
it -- per ring position a mul_base, a mul (three when linkable), an add (two) on the device and the challenge hash on
the host.  The chain's cost does not depend on whether a signature is valid, so the inputs are random scalars below l
over valid keys and a valid tag; the composed path is timed on the same shapes with the step's challenge taken from a
prepared array, and the host hash (the Python BLAKE2Xb) is timed separately on a sample and stated as host time.
  tools/ed_ring_probe.py [out.json]         end to end from host buffers, medians, alternating (profiler off)
  tools/ed_ring_probe.py --once RING LINK   7 alternating passes of both paths: the body of a
                                            `rocprofv3 --kernel-trace -d DIR -- python tools/ed_ring_probe.py --once RING LINK`
  tools/ed_ring_probe.py --stats DIR        per-pass summed kernel time from that trace and the ratio fused / composed
"""
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

N = 1 << 16
FUSED = ("ed25519_ring_chain_kernel", "ed25519_ring_tables_kernel")
COMPOSED = ("ed25519_mul_base_kernel", "ed25519_mul_kernel", "ed25519_encode_kernel", "ed25519_add_kernel")


def scalars(rng, n):
    a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] &= 0x0F  # below 2^252 < l
    return a


def make(ring, linkable, n=N):
    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.sign import anon

    rng = np.random.default_rng(ring)
    keys = ed.batch_mul_base(scalars(rng, ring))
    scope = b"probe scope" if linkable else None
    base = anon.link_base(scope) if linkable else None
    slots = ring + (2 if linkable else 1)
    sigs = scalars(rng, n * slots).reshape(n, slots, 32)
    if linkable:
        sigs[:, -1] = ed.commit(scalars(rng, n), base)
    msgs = [b"ballot %d" % i for i in range(n)]
    return dict(ring=ring, keys=keys, scope=scope, base=base, sigs=np.ascontiguousarray(sigs.reshape(n, 32 * slots)), msgs=msgs,
                c=scalars(rng, n), n=n)


def fused(a):
    from kyber_amd.group import edwards25519 as ed

    _, _, ok, st = ed.batch_ring_chain(a["keys"].reshape(1, -1), a["msgs"], a["scope"], a["base"], a["sigs"], a["ring"])
    assert not st.any()
    return ok


def composed_device(a):
    """the device share of the composed path: per position mul_base, mul and add (and mul, mul, add when linkable)"""
    from kyber_amd.group import edwards25519 as ed

    n, ring = a["n"], a["ring"]
    sig = a["sigs"].reshape(n, -1, 32)
    lb = np.ascontiguousarray(np.broadcast_to(np.frombuffer(a["base"], dtype=np.uint8), (n, 32))) if a["scope"] is not None else None
    for i in range(ring):
        s = np.ascontiguousarray(sig[:, 1 + i])
        key = np.ascontiguousarray(np.broadcast_to(a["keys"][i], (n, 32)))
        pg, _ = ed.batch_add(ed.batch_mul_base(s), ed.batch_mul(a["c"], key)[0])
        if a["scope"] is not None:
            tag = np.ascontiguousarray(sig[:, -1])
            ed.batch_add(ed.batch_mul(s, lb)[0], ed.batch_mul(a["c"], tag)[0])
    return pg


def host_hash_us(a, sample=512):
    """microseconds per challenge of the host's Python BLAKE2Xb + Pick, on `sample` elements"""
    from kyber_amd.util import blake2xb

    tag = a["sigs"][0, -32:].tobytes()
    t0 = time.perf_counter()
    for i in range(sample):
        x = blake2xb.New(a["msgs"][i])
        if a["scope"] is not None:
            x.Write(a["scope"])
            x.Write(tag)
        x.Write(tag)
        if a["scope"] is not None:
            x.Write(tag)
        blake2xb.pick(x.Read)
    return 1e6 * (time.perf_counter() - t0) / sample


def med(ts):
    v = sorted(ts)
    return {"median": 1e3 * v[len(v) // 2], "min": 1e3 * v[0], "max": 1e3 * v[-1]}


def timed(ring, linkable, reps):
    a = make(ring, linkable)
    p = {"fused": lambda: fused(a), "composed_device": lambda: composed_device(a)}
    for f in p.values():
        f()  # warm-up
    ts = {k: [] for k in p}
    for _ in range(reps):
        for k, f in p.items():  # alternating
            t0 = time.perf_counter()
            f()
            ts[k].append(time.perf_counter() - t0)
    res = {"n": a["n"], "ring": ring, "linkable": linkable, "reps": reps}
    for k, v in ts.items():
        res[k + "_ms_end_to_end"] = med(v)
    us = host_hash_us(a)
    res["host_hash_us_per_challenge"] = us
    res["composed_host_hash_ms_extrapolated"] = us * a["n"] * ring / 1e3
    res["fused_signatures_per_s"] = a["n"] / (res["fused_ms_end_to_end"]["median"] / 1e3)
    res["end_to_end_ratio_fused_over_composed_device_only"] = res["fused_ms_end_to_end"]["median"] / res["composed_device_ms_end_to_end"]["median"]
    return res


def stats(d):
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
        v = v[-6:]  # the passes after the warm-up (setup launches multiplication kernels of its own before them)
        ms = sorted(x[0] for x in v)
        out[k + "_kernel_ms"] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "passes": len(ms)}
        out[k + "_kernels_per_pass"] = v[-1][1]
    out["kernel_time_ratio_fused_over_composed"] = out["fused_kernel_ms"]["median"] / out["composed_kernel_ms"]["median"]
    return out


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--once":
        import torch

        a = make(int(sys.argv[2]), sys.argv[3] == "1")
        for _ in range(7):
            fused(a)
            torch.cuda.synchronize()
            composed_device(a)
            torch.cuda.synchronize()
    elif len(sys.argv) > 2 and sys.argv[1] == "--stats":
        print(json.dumps(stats(sys.argv[2])))
    else:
        line = json.dumps({"what": "sign/anon verify on Ed25519, 2^16 signatures, one shared ring: the fused chain against the "
                                   "composed per-position calls (device share) and the host hash; end to end from host buffers, "
                                   "medians, alternating",
                           "sizes": [timed(r, l, 5 if r == 10 else 3) for r in (10, 100) for l in (False, True)]})
        print(line)
        if len(sys.argv) > 1:
            open(sys.argv[1], "w").write(line + "\n")
