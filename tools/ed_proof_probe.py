#!/usr/bin/env python3
"""Times kyb_ed25519_lincomb against the composed device calls it replaces, in one process, medians of 20 after a
warm-up, alternating, on device buffers:
  * "three": three terms an element, (ko, ks) = (1, 2) with both shared points given -- X = x1 B1 + x2 B2 next to c P --
    against mul + mul + mul + add + add;
  * "rep":   one check of the shape V == c P + r G, (ko, ks) = (1, 1) with expect, against mul2 + a comparison of the
    encodings;
  * "biffle": BiffleVerifyBatch over N pairs of ciphertexts (biffle.go:11-30: eight Reps of that shape, G = nil) from
    host buffers, against the same verification with each Rep checked by mul2 + compare.  Both paths run the same
    additions, unmarshal and challenge call; the kernel figures count the kernels that differ.  The N proofs are 256
    proofs made on the host, repeated.
  tools/ed_proof_probe.py [out.json]          time around each path at 2^16 elements (hipEvents on device buffers; the
                                              host clock for "biffle" and for fs_challenge alone; profiler off)
  tools/ed_proof_probe.py --once WHAT N       21 alternating passes of both paths of WHAT at N elements: the body of a
                                              `rocprofv3 --kernel-trace --stats -d DIR -- python tools/ed_proof_probe.py --once WHAT N`
  tools/ed_proof_probe.py --stats DIR [biffle]   per-pass summed kernel time from that trace: medians over the 20 passes after
                                              the first, and their ratio (fused over composed: below 1.0 is a gain)
  tools/ed_proof_probe.py --merge OUT EVENTS three=STATS rep=STATS biffle=STATS
                                              profiles/ed_proof_probe.json: the first mode's file and the --stats outputs in one
"""
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FUSED = ("ed25519_lincomb_tables_kernel", "ed25519_lincomb_kernel", "ed25519_lincomb_encode_kernel")
COMPOSED = ("ed25519_mul_kernel", "ed25519_add_kernel", "ed25519_encode_kernel", "ed25519_mul2_kernel", "ed25519_mul2_encode_kernel")
COMPOSED_BIFFLE = ("ed25519_mul2_kernel", "ed25519_mul2_encode_kernel")  # both paths of "biffle" launch add and unmarshal kernels


def paths(what: str, n: int):
    """{"fused": f, "composed": g} on device buffers; both return the n verdicts or encodings to compare"""
    if what == "biffle":
        return biffle_paths(n)
    import torch

    from kyber_amd.group import edwards25519 as ed

    g = torch.Generator().manual_seed(n)
    rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).cuda()

    def scalars(*shape):
        s = rnd(*shape)
        s[..., 31] &= 0x0F
        return s

    P = ed.batch_mul_base(scalars(n, 32))
    bases = ed.batch_mul_base(scalars(2, 32)).cpu().numpy()
    B1, B2 = bases[0].tobytes(), bases[1].tobytes()
    if what == "three":
        s = scalars(n, 3, 32)
        own = P.view(n, 1, 32)
        s0, s1, s2 = (s[:, j].contiguous() for j in range(3))
        B1n, B2n = (torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).cuda().repeat(n, 1) for b in (B1, B2))

        def fused():
            return ed.batch_lincomb(s, own, [B1, B2])[0]

        def composed():
            a = ed.batch_add(ed.batch_mul(s0, P)[0], ed.batch_mul(s1, B1n)[0])[0]
            return ed.batch_add(a, ed.batch_mul(s2, B2n)[0])[0]

        return {"fused": fused, "composed": composed}
    assert what == "rep"
    s = scalars(n, 2, 32)
    own = P.view(n, 1, 32)
    c, r = s[:, 0].contiguous(), s[:, 1].contiguous()
    Gn = torch.from_numpy(np.frombuffer(B1, dtype=np.uint8).copy()).cuda().repeat(n, 1)
    V = ed.batch_mul2(c, P, r, Gn)[0]
    V[::7, 0] ^= 1  # every seventh commitment is wrong

    def fused():
        return ed.batch_lincomb(s, own, [B1], V, want_out=False)[1]

    def composed():
        return (ed.batch_mul2(c, P, r, Gn)[0] == V).all(1).to(torch.uint8)

    return {"fused": fused, "composed": composed}


def biffle_paths(n: int, made: int = 256):
    """BiffleVerifyBatch as it is, and with every Rep checked by mul2 + compare; both return the number of accepted proofs"""
    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.proof import proof as PP
    from kyber_amd.shuffle import biffle as B
    from kyber_amd.util import blake2xb

    rng = np.random.default_rng(n)

    def points(k):
        s = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
        s[:, 31] &= 0x0F
        return np.asarray(ed.batch_mul_base(s))

    H = points(1)[0].tobytes()
    X, Y = points(2 * made).reshape(made, 2, 32), points(2 * made).reshape(made, 2, 32)
    Xbar, Ybar, proofs = B.BiffleBatch(None, H, X, Y, [blake2xb.New(b"ed_proof_probe %d" % i) for i in range(made)])
    X, Y, Xbar, Ybar = (np.ascontiguousarray(np.tile(a, (n // made, 1, 1))) for a in (X, Y, Xbar, Ybar))
    proofs = proofs * (n // made)
    base = np.frombuffer(ed._BASE_ENC, dtype=np.uint8)

    def mul2_compare(m, terms, expect=None):
        (c, P), (r, G) = terms  # every Rep of a biffle has one term
        G = np.tile(base if G is None else np.frombuffer(G, dtype=np.uint8), (m, 1))
        out, st = ed.batch_mul2(c, P, r, G)
        canon, st2 = ed.batch_unmarshal(expect)
        return None, ((np.asarray(out) == np.asarray(canon)).all(1) & (np.asarray(st2) == 0)).astype(np.uint8), np.asarray(st)

    def fused():
        return sum(e is None for e in B.BiffleVerifyBatch(None, H, X, Y, Xbar, Ybar, proofs))

    def composed():
        keep = PP.lincomb
        PP.lincomb = mul2_compare
        try:
            return fused()
        finally:
            PP.lincomb = keep

    return {"fused": fused, "composed": composed}


def time_host(p, n: int, reps: int = 20):
    import time

    assert p["fused"]() == p["composed"]() == n  # warm-up, and the answers
    ms = {k: [] for k in p}
    for _ in range(reps):
        for k, f in p.items():  # alternating
            t0 = time.perf_counter()
            f()
            ms[k].append(1e3 * (time.perf_counter() - t0))
    med = lambda v: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "reps": len(v)}
    res = {"n": n, "fused_ms_end_to_end": med(ms["fused"]), "composed_ms_end_to_end": med(ms["composed"])}
    res["end_to_end_ratio"] = res["fused_ms_end_to_end"]["median"] / res["composed_ms_end_to_end"]["median"]
    return res


def time_fs_challenge(n: int, data_len: int = 256, reps: int = 20):
    """kyb_ed25519_fs_challenge alone on device buffers: the eight commitments of a biffle under one name"""
    import torch

    from kyber_amd.group import edwards25519 as ed

    data = torch.randint(0, 256, (n, data_len), dtype=torch.uint8, generator=torch.Generator().manual_seed(n)).cuda()
    ed.batch_fs_challenge(b"Biffle", data)
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ed.batch_fs_challenge(b"Biffle", data)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"n": n, "data_len": data_len, "ms_events": {"median": sorted(ms)[len(ms) // 2], "min": min(ms), "max": max(ms), "reps": reps}}


def time_events(what: str, n: int, reps: int = 20):
    import torch

    p = paths(what, n)
    assert torch.equal(p["fused"](), p["composed"]())  # warm-up, and the answers
    ms = {k: [] for k in p}
    for _ in range(reps):
        for k, f in p.items():  # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    med = lambda v: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "reps": len(v)}
    res = {"n": n, "fused_ms_events": med(ms["fused"]), "composed_ms_events": med(ms["composed"])}
    res["event_time_ratio"] = res["fused_ms_events"]["median"] / res["composed_ms_events"]["median"]
    return res


def stats(d, composed=COMPOSED):
    """per-pass summed kernel time (ms) of each path from the kernel-trace CSVs under d: the trace alternates fused and
    composed passes, a pass being a run of consecutive kernels of one path (kernels of neither are skipped)"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    assert rows, "no kernel trace under " + d
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    name_of = lambda r: r["Kernel_Name"].split("(")[0].split("::")[-1].split("<")[0]
    kind = lambda r: "fused" if name_of(r) in FUSED else ("composed" if name_of(r) in composed else None)
    passes, prev = {"fused": [], "composed": []}, None
    for r in rows:
        k = kind(r)
        if k is None:
            continue
        if k != prev:
            passes[k].append([0.0, 0, {}])
            prev = k
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        passes[k][-1][0] += ms
        passes[k][-1][1] += 1
        passes[k][-1][2][name_of(r)] = passes[k][-1][2].get(name_of(r), 0.0) + ms
    out = {}
    for k, v in passes.items():
        v = v[-20:]  # the passes after the warm-up (setup launches kernels of the composed path before them)
        ms = sorted(x[0] for x in v)
        out[k + "_kernel_ms"] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "passes": len(ms)}
        out[k + "_kernels_per_pass"] = v[-1][1]
        out[k + "_kernels_of_the_last_pass_ms"] = v[-1][2]
    out["kernel_time_ratio"] = out["fused_kernel_ms"]["median"] / out["composed_kernel_ms"]["median"]
    return out


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--once":
        import torch

        p = paths(sys.argv[2], int(sys.argv[3]))
        torch.cuda.synchronize()
        for _ in range(21):
            for k in ("fused", "composed"):
                p[k]()
                torch.cuda.synchronize()
    elif len(sys.argv) > 2 and sys.argv[1] == "--stats":
        print(json.dumps(stats(sys.argv[2], COMPOSED_BIFFLE if sys.argv[3:] == ["biffle"] else COMPOSED)))
    elif len(sys.argv) > 3 and sys.argv[1] == "--merge":
        out = json.load(open(sys.argv[3]))
        for arg in sys.argv[4:]:
            what, path = arg.split("=", 1)
            out[what]["kernel_trace"] = json.load(open(path))
        open(sys.argv[2], "w").write(json.dumps(out) + "\n")
    else:
        n = 1 << 16
        line = json.dumps({"what": "kyb_ed25519_lincomb against the composed device calls at 2^16 elements, medians of 20, "
                                   "alternating: three terms an element against mul x 3 + add x 2 and one two-term check against "
                                   "mul2 + compare (hipEvent time on device buffers), BiffleVerifyBatch against the same "
                                   "verification over mul2 + compare (host clock, host buffers), fs_challenge alone; "
                                   "kernel_trace, where present: summed kernel time from a kernel trace in a run of its own",
                           "three": time_events("three", n), "rep": time_events("rep", n), "biffle": time_host(biffle_paths(n), n),
                           "fs_challenge": time_fs_challenge(n)})
        print(line)
        if len(sys.argv) > 1:
            open(sys.argv[1], "w").write(line + "\n")
