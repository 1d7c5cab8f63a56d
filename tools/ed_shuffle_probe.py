#!/usr/bin/env python3
"""Times the two engine calls behind shuffle/ on Ed25519 and the protocol layer over them, in one process, medians of 20
after a warm-up unless stated, at 2^16 elements:
  * kyb_ed25519_theta_check against the composed path it replaces (add, add, mul2, compare), alternating;
  * kyb_ed25519_xof_pick against the host's Python loop of Scalar.Pick over the Python XOF (timed on 300 picks);
  * proof.HashVerify and proof.HashProve of a pair shuffle, split into hashing (the root hashes of the reseeded pool),
    picks, engine calls and the rest (host glue; for the prover mostly scalar arithmetic in Python integers).
  tools/ed_shuffle_probe.py [out.json]     end to end from host buffers (PCIe and the host's share included; profiler off)
  tools/ed_shuffle_probe.py --once N       21 alternating passes of both theta paths on device buffers at N lanes: the
                                           body of a `rocprofv3 --kernel-trace --stats -d DIR -- python
                                           tools/ed_shuffle_probe.py --once N`
  tools/ed_shuffle_probe.py --stats DIR    per-pass summed kernel time from that trace: medians over the 20 passes after
                                           the first, and their ratio (the yardstick the fused call ships on: below 1.0)
"""
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FUSED = ("ed25519_theta_kernel", "ed25519_theta_encode_kernel")
COMPOSED = ("ed25519_add_kernel", "ed25519_mul2_kernel", "ed25519_mul2_encode_kernel", "ed25519_encode_kernel", "ed25519_unmarshal_kernel")
L = 2**252 + 27742317777372353535851937790883648493


def _scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x0F
    return s


def make_theta(n):
    """n valid rows (a, A, U, b, B, W, T) and Neg(b), made by the engine"""
    from kyber_amd.group import edwards25519 as ed

    rng = np.random.default_rng(n)
    a, b = _scalars(rng, n), _scalars(rng, n)
    A, B = ed.batch_mul_base(_scalars(rng, n)), ed.batch_mul_base(_scalars(rng, n))
    UW = ed.batch_mul_base(_scalars(rng, 2))
    U, W = UW[:1].copy(), UW[1:].copy()
    nb = np.frombuffer(b"".join((-int.from_bytes(x.tobytes(), "little") % L).to_bytes(32, "little") for x in b), dtype=np.uint8).reshape(n, 32).copy()
    T, st = ed.batch_mul2(a, ed.batch_add(A, np.repeat(U, n, 0))[0], nb, ed.batch_add(B, np.repeat(W, n, 0))[0])
    assert not np.asarray(st).any()
    return a, A, U, b, B, W, np.asarray(T), nb


def theta_paths(rows, device: bool):
    from kyber_amd.group import edwards25519 as ed

    a, A, U, b, B, W, T, nb = rows
    n = a.shape[0]
    Un, Wn = np.repeat(U, n, 0), np.repeat(W, n, 0)
    if device:
        import torch

        a, A, U, b, B, W, T, nb, Un, Wn = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (a, A, U, b, B, W, T, nb, Un, Wn))

    def fused():
        return ed.batch_theta_check(a, A, U, b, B, W, T)[0]

    def composed():
        out = ed.batch_mul2(a, ed.batch_add(A, Un)[0], nb, ed.batch_add(B, Wn)[0])[0]
        return (out == T).all(1) if device else (np.asarray(out) == T).all(1)

    return {"fused": fused, "composed": composed}


def median_of(ts):
    v = sorted(ts)
    return {"median": 1e3 * v[len(v) // 2], "min": 1e3 * v[0], "max": 1e3 * v[-1], "reps": len(v)}


def time_theta(n, reps=20):
    p = theta_paths(make_theta(n), device=False)
    assert p["fused"]().all() and p["composed"]().all()  # warm-up, and the answers
    ts = {k: [] for k in p}
    for _ in range(reps):
        for k, f in p.items():  # alternating
            t0 = time.perf_counter()
            f()
            ts[k].append(time.perf_counter() - t0)
    res = {"n": n, "fused_ms_end_to_end": median_of(ts["fused"]), "composed_ms_end_to_end": median_of(ts["composed"])}
    res["end_to_end_ratio"] = res["fused_ms_end_to_end"]["median"] / res["composed_ms_end_to_end"]["median"]
    return res


def time_picks(n, reps=20, sample=300):
    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.util import blake2xb

    xof = blake2xb.New(b"ed_shuffle_probe picks")
    xof.Read(8)
    root, pos = xof.Root(), xof.Tell()
    out, used = ed.batch_xof_pick(root, pos, n)  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ed.batch_xof_pick(root, pos, n)
        ts.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    host = b"".join(blake2xb.pick(xof.Read) for _ in range(sample))
    per_pick = (time.perf_counter() - t0) / sample
    assert host == np.asarray(out)[:sample].tobytes()
    res = {"n": n, "draws_used": used, "xof_pick_ms_end_to_end": median_of(ts), "host_python_us_per_pick": 1e6 * per_pick,
           "host_python_sample": sample, "host_python_ms_extrapolated": 1e3 * per_pick * n}
    res["ratio"] = res["xof_pick_ms_end_to_end"]["median"] / res["host_python_ms_extrapolated"]
    return res


class Split:
    """wall time of the wrapped functions by category, exclusive of the wrapped calls made inside them"""

    def __init__(self):
        self.t = {}
        self.stack = []
        self.undo = []

    def wrap(self, obj, name, cat):
        f = getattr(obj, name)

        def g(*a, **kw):
            t0 = time.perf_counter()
            self.stack.append(0.0)
            try:
                return f(*a, **kw)
            finally:
                dt = time.perf_counter() - t0
                self.t[cat] = self.t.get(cat, 0.0) + dt - self.stack.pop()
                if self.stack:
                    self.stack[-1] += dt

        setattr(obj, name, g)
        self.undo.append((obj, name, f))

    def restore(self):
        for obj, name, f in self.undo:
            setattr(obj, name, f)


def time_protocol(k, verify_reps=20, prove_reps=3):
    from kyber_amd import shuffle
    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.proof import hash as PH
    from kyber_amd.util import blake2xb

    rng = np.random.default_rng(k)
    H = ed.batch_mul_base(_scalars(rng, 1)).tobytes()
    Xs, Ys = ed.batch_mul_base(_scalars(rng, k)), ed.batch_mul_base(_scalars(rng, k))
    sp = Split()
    sp.wrap(blake2xb, "root_hash", "hashing")
    sp.wrap(PH, "picks", "picks")
    for name in ("batch_mul_base", "batch_mul", "commit", "msm", "batch_add", "batch_unmarshal", "batch_theta_check"):
        sp.wrap(ed, name, "engine_calls")
    sp.wrap(blake2xb, "output_node", "python_xof_nodes")  # Reseed's 128 bytes, single picks, Shuffle's 8-byte reads

    def run(f, reps):
        walls, parts = [], []
        for _ in range(reps + 1):  # the first pass warms up
            sp.t = {}
            t0 = time.perf_counter()
            out = f()
            walls.append(time.perf_counter() - t0)
            parts.append(dict(sp.t))
        walls, parts = walls[1:], parts[1:]
        order = sorted(range(len(walls)), key=walls.__getitem__)
        mid = order[len(order) // 2]
        split = {c: 1e3 * v for c, v in parts[mid].items()}
        split["rest_host"] = 1e3 * walls[mid] - sum(split.values())
        return out, {"wall_ms": median_of(walls), "split_of_the_median_pass_ms": split}

    def prove():
        rand = blake2xb.New(b"ed_shuffle_probe")
        suite = PH.NewBlakeSHA256Ed25519WithRand(rand)
        t0 = time.perf_counter()
        Xbar, Ybar, prover = shuffle.Shuffle(suite, None, H, Xs, Ys, rand)
        shuffle_s = time.perf_counter() - t0
        return Xbar, Ybar, PH.HashProve(suite, "PairShuffle", prover), shuffle_s

    try:
        (Xbar, Ybar, proof, shuffle_s), res_prove = run(prove, prove_reps)
        res_prove["of_which_Shuffle_ms_last_pass"] = 1e3 * shuffle_s
        suite = PH.NewBlakeSHA256Ed25519WithRand(blake2xb.New(b"verifier"))
        _, res_verify = run(lambda: PH.HashVerify(suite, "PairShuffle", shuffle.Verifier(suite, None, H, Xs, Ys, Xbar, Ybar), proof), verify_reps)
    finally:
        sp.restore()
    return {"k": k, "proof_bytes": len(proof), "Shuffle_plus_HashProve": res_prove, "HashVerify": res_verify}


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
            passes[k].append([0.0, 0, {}])
            prev = k
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        passes[k][-1][0] += ms
        passes[k][-1][1] += 1
        name = r["Kernel_Name"].split("(")[0].split("::")[-1]
        passes[k][-1][2][name] = passes[k][-1][2].get(name, 0.0) + ms
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
    if len(sys.argv) > 2 and sys.argv[1] == "--once":
        import torch

        p = theta_paths(make_theta(int(sys.argv[2])), device=True)
        torch.cuda.synchronize()
        for _ in range(21):
            for k in ("fused", "composed"):
                assert p[k]().all().item()
                torch.cuda.synchronize()
    elif len(sys.argv) > 2 and sys.argv[1] == "--stats":
        print(json.dumps(stats(sys.argv[2])))
    else:
        n = 1 << 16
        line = json.dumps({"what": "shuffle/ on Ed25519: theta_check fused against composed, xof_pick against the host's Python "
                                   "loop, HashVerify and HashProve of a pair shuffle split by where the time goes; end to end "
                                   "from host buffers, medians, alternating",
                           "theta_check": time_theta(n), "xof_pick": time_picks(n), "pair_shuffle": time_protocol(n)})
        print(line)
        if len(sys.argv) > 1:
            open(sys.argv[1], "w").write(line + "\n")
