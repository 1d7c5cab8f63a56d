#!/usr/bin/env python3
"""Times the two fused calls of sign/dss against the standing calls they replace, at about N = 2^16 partial signatures, as
summed kernel time from a kernel trace (medians of 20 alternating passes after a warm-up; host buffers -- copies are no
kernels) and end to end from host buffers:
  * "check16":  kyb_ed25519_dss_check, np = 16 participants, tl = tr = 9, every participant's partial of every session
                but the receiver's own (15 a session), against the composed path on the same tree: kyb_ed25519_verify +
                mul_base (V) + poly_eval (the long-term polynomial once, each session's random polynomial) + mul (h, the
                long share) + add;
  * "check128": the same at np = 128, t = 65 (127 partials a session);
  * "partial":  kyb_ed25519_dss_partial of 2^16 sessions of one signer (tl = tr = 9) against kyb_ed25519_schnorr_sign of the
                same messages.
The composed path has no call that evaluates MANY polynomials at a few indices each and returns the points, so it asks
kyb_ed25519_poly_eval once per session for the random polynomial: about 4 370 small launches a pass at np = 16 and 516 at
np = 128.  Their launch overhead is real cost of composing the standing calls, but the count of field multiplications
behind PREDICTED does not see it: every result carries "composed_poly_eval_calls_a_pass", and the per-kernel times of the
last pass show how much of the composed time is poly_eval's.
Every partial signature is a VALID one (made by kyb_ed25519_dss_partial): a rejected signature would end its lane before
the share check.  The kernel-time passes hand the composed path its hashes ready made; the end-to-end passes (--e2e) let it
hash in Python, element by element, as a caller without the fused call has to.  Next to each measured ratio stands the
one predicted by counting field multiplications (PREDICTED below; DESIGN.md section 5 item 69 has the count).
  tools/ed_dss_probe.py --once WHAT N     21 alternating passes of the fused call and its composed counterpart: the body of
                                          `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ed_dss_probe.py --once WHAT N`
  tools/ed_dss_probe.py --stats DIR       per-pass summed kernel time from that trace (medians of the last 20)
  tools/ed_dss_probe.py --e2e WHAT N      wall time of both paths from host buffers (median of 5; the composed path hashes in Python)
  tools/ed_dss_probe.py --merge OUT check16=STATS check128=STATS partial=STATS     profiles/ed_dss_probe.json
"""
import csv
import glob
import hashlib
import json
import os
import struct
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

L = 2**252 + 27742317777372353535851937790883648493
FUSED_PREFIX = "ed25519_dss_"
# field multiplications a partial signature
PREDICTED = {"check16": (2910 + 190 + 560 + 1800) / 7825.0, "check128": (2910 + 190 + 6900 + 1535) / 20505.0, "partial": 0.55}
SHAPES = {"check16": (16, 9), "check128": (128, 65), "partial": (16, 9)}
WHAT = "summed kernel time from a kernel trace at about 2^16 partial signatures, medians of 20 alternating passes; predicted: by counting field multiplications"


def _eval(coeffs, i):
    x, v = i + 1, 0
    for c in reversed(coeffs):
        v = (v * x + c) % L
    return v


def _le(x):
    return x.to_bytes(32, "little")


def world(what: str, n: int):
    """a roster, a long-term key, ns sessions and every valid partial signature of them"""
    from kyber_amd.group import edwards25519 as ed

    np_, t = SHAPES[what]
    rng = np.random.default_rng(n + np_)
    rand = lambda k: [int.from_bytes(bytes(r), "little") % L for r in rng.integers(0, 256, size=(k, 32), dtype=np.uint8)]
    ns = n if what == "partial" else max(1, n // (np_ - 1))
    privs, long_c = rand(np_), rand(t)
    rand_c = [rand(t) for _ in range(ns)]
    pubs = np.asarray(ed.batch_mul_base(b"".join(_le(x) for x in privs)))
    lc = np.asarray(ed.batch_mul_base(b"".join(_le(c) for c in long_c)))
    rc = np.asarray(ed.batch_mul_base(b"".join(_le(c) for row in rand_c for c in row)))
    msgs = [bytes(m) for m in rng.integers(0, 256, size=(ns, 32), dtype=np.uint8)]
    signers = [0] if what == "partial" else range(1, np_)  # participant 0 receives
    parts = {}
    for i in signers:
        beta = b"".join(_le(_eval(row, i)) for row in rand_c)
        k = b"".join(_le(x) for x in rand(ns))
        parts[i] = (beta, k) + tuple(np.asarray(a) for a in ed.batch_dss_partial(_le(privs[i]), i, _le(_eval(long_c, i)), beta, k, lc, rc, msgs))
    return dict(np=np_, t=t, ns=ns, privs=privs, long=long_c, pubs=pubs, lc=lc, rc=rc, msgs=msgs, parts=parts)


def paths(what: str, n: int, hashed: bool):
    """{"fused": f, "composed": g}; hashed: the composed path gets its SHA-256 and SHA-512 outputs ready made"""
    from kyber_amd.group import edwards25519 as ed

    w = world(what, n)
    ns, np_, t, lc, rc, msgs = w["ns"], w["np"], w["t"], w["lc"], w["rc"], w["msgs"]
    if what == "partial":
        beta, k, V, sid, sigs = w["parts"][0]
        priv, alpha = _le(w["privs"][0]), _le(_eval(w["long"], 0))

        def composed():
            ms = [hashlib.sha256(hashlib.sha256(bytes(V[b]) + struct.pack("<I", 0)).digest() + bytes(sid[b])).digest() for b in range(ns)] if not hashed else pre
            return ed.batch_schnorr_sign(k, priv, ms)

        pre = [hashlib.sha256(hashlib.sha256(bytes(V[b]) + struct.pack("<I", 0)).digest() + bytes(sid[b])).digest() for b in range(ns)]
        return {"fused": lambda: ed.batch_dss_partial(priv, 0, alpha, beta, k, lc, rc, msgs), "composed": composed}
    signers = sorted(w["parts"])
    sess = np.repeat(np.arange(ns, dtype=np.uint32), len(signers))
    idx = np.tile(np.array(signers, dtype=np.uint32), ns)
    V = np.stack([w["parts"][i][2] for i in signers], axis=1).reshape(-1, 32)
    sid = np.stack([w["parts"][i][3] for i in signers], axis=1).reshape(-1, 32)
    sigs = np.stack([w["parts"][i][4] for i in signers], axis=1).reshape(-1, 64)
    keys = w["pubs"][idx]

    def hashes():
        ms = [hashlib.sha256(hashlib.sha256(bytes(V[j]) + struct.pack("<I", int(idx[j]))).digest() + bytes(sid[j])).digest() for j in range(len(idx))]
        hs = [_le(int.from_bytes(hashlib.sha512(bytes(rc[b * t]) + bytes(lc[0]) + msgs[b]).digest(), "little") % L) for b in range(ns)]
        return ms, np.frombuffer(b"".join(hs), dtype=np.uint8).reshape(ns, 32)

    pre = hashes()

    def composed():
        ms, hs = pre if hashed else hashes()
        ok, _ = ed.batch_verify(keys, ms, sigs)
        left = ed.batch_mul_base(V)
        long_sh, _ = ed.poly_eval(lc, signers)
        rnd = np.concatenate([np.asarray(ed.poly_eval(rc[b * t:(b + 1) * t], signers)[0]) for b in range(ns)])
        hl, _ = ed.batch_mul(hs[sess], np.tile(np.asarray(long_sh), (ns, 1)))
        right, _ = ed.batch_add(rnd, hl)
        return ok, (np.asarray(left) == np.asarray(right)).all(axis=1)

    return {"fused": lambda: ed.batch_dss_check(w["pubs"], lc, rc, msgs, sess, idx, V, sid, sigs), "composed": composed}


def stats(d):
    """per-pass summed kernel time (ms) from the kernel-trace CSVs under d: the trace alternates the fused call and its
    composed counterpart, a pass being a run of consecutive kernels of one of them"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    assert rows, "no kernel trace under " + d
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    name_of = lambda r: r["Kernel_Name"].split("(")[0].split("::")[-1].split("<")[0]
    kind = lambda r: "fused" if name_of(r).startswith(FUSED_PREFIX) else (None if r["Kernel_Name"].startswith("__amd_rocclr") else "composed")
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
        v = v[-20:]  # the passes after the warm-up and the set-up's own calls
        ms = sorted(x[0] for x in v)
        out[k + "_kernel_ms"] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "passes": len(ms)}
        out[k + "_kernels_of_the_last_pass_ms"] = v[-1][1]
    out["kernel_time_ratio"] = out["fused_kernel_ms"]["median"] / out["composed_kernel_ms"]["median"]
    return out


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--once":
        import torch

        p = paths(sys.argv[2], int(sys.argv[3]), hashed=True)
        for _ in range(21):
            for k in ("fused", "composed"):
                p[k]()
                torch.cuda.synchronize()
    elif len(sys.argv) > 3 and sys.argv[1] == "--e2e":
        p = paths(sys.argv[2], int(sys.argv[3]), hashed=False)
        out = {}
        for k in ("fused", "composed"):
            p[k]()
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                p[k]()
                ts.append((time.perf_counter() - t0) * 1e3)
            out[k + "_end_to_end_ms"] = sorted(ts)[2]
        np_, _ = SHAPES[sys.argv[2]]
        out["composed_poly_eval_calls_a_pass"] = 0 if sys.argv[2] == "partial" else 1 + max(1, int(sys.argv[3]) // (np_ - 1))
        print(json.dumps(out))
    elif len(sys.argv) > 2 and sys.argv[1] == "--stats":
        print(json.dumps(stats(sys.argv[2])))
    elif len(sys.argv) > 3 and sys.argv[1] == "--merge":
        out = {"what": WHAT}
        for arg in sys.argv[3:]:
            what, path = arg.split("=", 1)
            out[what] = dict(json.load(open(path)), predicted_ratio=PREDICTED[what])
        open(sys.argv[2], "w").write(json.dumps(out) + "\n")
    else:
        print(__doc__)
