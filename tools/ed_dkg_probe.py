#!/usr/bin/env python3
"""Times the three engine calls behind encrypt/ecies and the deal checks of share/dkg on Ed25519, in one process, hipEvent
medians of 20 after a warm-up on device buffers unless stated:
  * kyb_ed25519_ecies_seal at 2^16 x 32-byte messages against kyb_ed25519_mul_base + kyb_ed25519_mul on the same scalars
    (the two multiplications every seal contains: the floor the fused call shares), alternating; kyb_ed25519_ecies_open
    against kyb_ed25519_mul alone;
  * kyb_ed25519_deal_check at (m, t) = (256, 128) and (1024, 512), one check per polynomial, indices below 1024, against
    the composed way: one MSM pipeline per dealer (PubPoly.Eval as an MSM over the powers of x) and one batch_mul_base
    over all shares, from host buffers (wall clock; the fused call is timed the same way next to its event time).
  tools/ed_dkg_probe.py [out.json]      the figures above as one JSON line (profiler off)
  tools/ed_dkg_probe.py --once N        21 passes of seal, open and mul_base + mul on device buffers at N messages: the body
                                        of a `rocprofv3 --kernel-trace -d DIR -- python tools/ed_dkg_probe.py --once N`
  tools/ed_dkg_probe.py --stats DIR [out.json]
                                        per-kernel medians from that trace: the AEAD kernels' own time, the summed kernel
                                        time of a seal and of an open against that of the multiplications they contain
"""
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

L = 2**252 + 27742317777372353535851937790883648493
KERNELS = ("ed25519_ecies_seal_kernel", "ed25519_ecies_open_kernel", "ed25519_ecies_encode_kernel", "ed25519_ecies_seal_aead_kernel",
           "ed25519_ecies_open_aead_kernel")


def _scalars(rng, n):
    s = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    s[:, 31] &= 0x0F
    return s


def median_of(ts):
    v = sorted(ts)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "reps": len(v)}


def event_ms(paths, reps=20):
    """hipEvent time of every path, alternating, after one warm-up pass"""
    import torch

    for f in paths.values():
        f()
    torch.cuda.synchronize()
    ts = {k: [] for k in paths}
    for _ in range(reps):
        for k, f in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b))
    return {k: median_of(v) for k, v in ts.items()}


def ecies_paths(n, msg_len=32):
    import torch

    from kyber_amd.group import edwards25519 as ed

    rng = np.random.default_rng(n)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    r, x = dev(_scalars(rng, n)), dev(_scalars(rng, 1))
    pub = ed.batch_mul_base(x)
    pubs = pub.repeat(n, 1)
    msgs = dev(rng.integers(0, 256, size=n * msg_len, dtype=np.uint8))
    off = (torch.arange(n + 1, dtype=torch.int64) * msg_len).cuda()
    (ctx, coff), st = ed.batch_ecies_seal(r, pub, (msgs, off))
    (back, _), st2 = ed.batch_ecies_open(x, (ctx, coff))
    assert not st.any().item() and not st2.any().item()
    assert torch.equal(back.view(n, msg_len + 48)[:, :msg_len].reshape(-1), msgs)
    R = ctx.view(n, msg_len + 48)[:, :32].contiguous()
    xs = x.repeat(n, 1)
    return {
        "seal": lambda: ed.batch_ecies_seal(r, pub, (msgs, off)),
        "mul_base_plus_mul": lambda: (ed.batch_mul_base(r), ed.batch_mul(r, pubs)),
        "open": lambda: ed.batch_ecies_open(x, (ctx, coff)),
        "mul": lambda: ed.batch_mul(xs, R),
    }


def time_ecies(n):
    res = {"n": n, "message_bytes": 32, "event_ms": event_ms(ecies_paths(n))}
    e = res["event_ms"]
    res["seal_over_floor"] = e["seal"]["median"] / e["mul_base_plus_mul"]["median"]
    res["open_over_floor"] = e["open"]["median"] / e["mul"]["median"]
    return res


def time_deal_check(m, t, reps=20, composed_reps=3):
    import torch

    from kyber_amd.group import edwards25519 as ed

    rng = np.random.default_rng(m * t)
    coeffs = _scalars(rng, m * t)
    commits = np.asarray(ed.batch_mul_base(coeffs))
    idx = rng.integers(0, 1024, size=m).astype(np.uint32)
    ci = [int.from_bytes(c.tobytes(), "little") for c in coeffs]
    shares = []
    for k in range(m):
        x, v = int(idx[k]) + 1, 0
        for c in reversed(ci[k * t:(k + 1) * t]):
            v = (v * x + c) % L
        shares.append(v.to_bytes(32, "little"))
    shares = np.frombuffer(b"".join(shares), dtype=np.uint8).reshape(m, 32).copy()
    shares[m // 2, 0] ^= 1  # one wrong share
    poly = np.arange(m, dtype=np.uint32)
    want = np.ones(m, dtype=np.uint8)
    want[m // 2] = 0

    def fused_host():
        return ed.batch_deal_check(poly, idx, shares, commits, m, t)[0]

    def composed_host():
        left = np.asarray(ed.batch_mul_base(shares))
        ok = np.zeros(m, dtype=np.uint8)
        for k in range(m):
            x, pw, sc = int(idx[k]) + 1, 1, []
            for _ in range(t):
                sc.append(pw.to_bytes(32, "little"))
                pw = pw * x % L
            out, _ = ed.msm(b"".join(sc), commits[k * t:(k + 1) * t])
            ok[k] = bytes(np.asarray(out)) == bytes(left[k])
        return ok

    assert (np.asarray(fused_host()) == want).all() and (composed_host() == want).all()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = [dev(poly.view(np.int32)), dev(idx.view(np.int32)), dev(shares), dev(commits)]
    ev = event_ms({"deal_check": lambda: ed.batch_deal_check(d[0], d[1], d[2], d[3], m, t)}, reps)
    wall = {"fused": [], "composed": []}
    for _ in range(composed_reps):
        for k, f in (("fused", fused_host), ("composed", composed_host)):
            t0 = time.perf_counter()
            f()
            wall[k].append(1e3 * (time.perf_counter() - t0))
    res = {"m": m, "t": t, "checks": m, "fused_event_ms": ev["deal_check"], "fused_ms_end_to_end": median_of(wall["fused"]),
           "composed_ms_end_to_end": median_of(wall["composed"])}
    res["end_to_end_ratio"] = res["fused_ms_end_to_end"]["median"] / res["composed_ms_end_to_end"]["median"]
    return res


FLOOR = ("ed25519_mul_base_kernel", "ed25519_mul_kernel", "ed25519_encode_kernel")


def stats(d):
    """per-kernel milliseconds from a `--once` run under rocprofv3 --kernel-trace: the median over the last 20 launches of
    every kernel of a seal, of an open and of the multiplications they contain (the floor: mul_base + mul for a seal, mul
    for an open, each with its launch of the shared encoder), and the sums"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    assert rows, "no kernel trace under " + d
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].split("::")[-1]
        if any(k in name for k in KERNELS + FLOOR):
            per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    med = {}
    for name, v in per.items():
        v = sorted(v[-20:])
        med[name] = {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "launches": len(v)}
    pick = lambda part: sum(x["median_ms"] for name, x in med.items() if part in name)
    enc = pick("ed25519_encode_kernel")
    out = {"kernels": med,
           "seal_ms": pick("ecies_seal_kernel") + pick("ecies_encode_kernel<2>") + pick("ecies_seal_aead_kernel"),
           "open_ms": pick("ecies_open_kernel") + pick("ecies_encode_kernel<1>") + pick("ecies_open_aead_kernel"),
           "seal_aead_ms": pick("ecies_seal_aead_kernel"), "open_aead_ms": pick("ecies_open_aead_kernel"),
           "floor_seal_ms": pick("ed25519_mul_base_kernel") + pick("ed25519_mul_kernel") + 2 * enc,
           "floor_open_ms": pick("ed25519_mul_kernel") + enc}
    out["seal_over_floor"] = out["seal_ms"] / out["floor_seal_ms"]
    out["open_over_floor"] = out["open_ms"] / out["floor_open_ms"]
    return out


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--once":
        import torch

        p = ecies_paths(int(sys.argv[2]))
        torch.cuda.synchronize()
        for _ in range(21):
            for k in ("seal", "open", "mul_base_plus_mul"):
                p[k]()
                torch.cuda.synchronize()
    elif len(sys.argv) > 2 and sys.argv[1] == "--stats":
        line = json.dumps(stats(sys.argv[2]))
        print(line)
        if len(sys.argv) > 3:
            open(sys.argv[3], "w").write(line + "\n")
    else:
        line = json.dumps({"what": "encrypt/ecies seal and open against the multiplications they contain (hipEvent medians of 20 on "
                                   "device buffers, alternating); deal_check against one MSM per dealer + one mul_base (end to end "
                                   "from host buffers, wall clock)",
                           "ecies": time_ecies(1 << 16), "deal_check": [time_deal_check(256, 128), time_deal_check(1024, 512)]})
        print(line)
        if len(sys.argv) > 1:
            open(sys.argv[1], "w").write(line + "\n")
