#!/usr/bin/env python3
"""Times the three fused calls of share/vss against the standing calls they contain, at N = 2^16 elements, as summed
kernel time from a kernel trace (medians of 20 alternating passes after a warm-up; host buffers -- copies are no kernels):
  * "seal":   kyb_ed25519_vss_seal of 142-byte deals (t = 2) against mul_base (dh) + mul_base (k) + mul (dh, pubs);
  * "check2": kyb_ed25519_deal_check2 of ONE polynomial of t = 4 commitments at 2^16 indices against
              mul_base (f) + mul_same_base (g, H) + add + poly_eval;
  * "sign":   kyb_ed25519_schnorr_sign of 32-byte messages against mul_base (k) + mul_base (x).
Next to each measured ratio stands the one predicted by counting field multiplications (PREDICTED below; DESIGN.md
section 5 item 66 has the count).  Inputs are random: the lane programs do the same work whatever the verdict.
  tools/ed_vss_probe.py --once WHAT N     21 alternating passes of the fused call and its composed counterpart: the body of
                                          `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ed_vss_probe.py --once WHAT N`
  tools/ed_vss_probe.py --stats DIR       per-pass summed kernel time from that trace (medians of the last 20)
  tools/ed_vss_probe.py --merge OUT seal=STATS check2=STATS sign=STATS     profiles/ed_vss_probe.json
"""
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FUSED = ("ed25519_schnorr_points_kernel", "ed25519_schnorr_encode_kernel", "ed25519_schnorr_sign_kernel", "ed25519_vss_seal_kernel",
         "ed25519_vss_encode_kernel", "ed25519_vss_seal_aead_kernel", "ed25519_vss_open_kernel", "ed25519_vss_open_aead_kernel",
         "ed25519_vss_deal_decode_kernel", "ed25519_vss_deal_check2_kernel")
# field multiplications an element: a comb 190, a ladder 2 700 (85 of them its table), a decoding 265, a shared encoding
# 20, Horner at t = 4 and 16-bit indices 580, an addition 8; the hash and the AEAD have none
PREDICTED = {"seal": (190 + 190 + 2700 + 265 + 3 * 21) / (210 + 210 + 2985.0),
             "check2": (2615 + 190 + 580 + 4) / (210 + 2720 + 558 + 600.0),
             "sign": 1.0}
WHAT = "summed kernel time from a kernel trace at 2^16 elements, medians of 20 alternating passes; predicted: by counting field multiplications"


def paths(what: str, n: int):
    from kyber_amd.group import edwards25519 as ed

    rng = np.random.default_rng(n + len(what))

    def sc(k=n):
        s = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
        s[:, 31] &= 0x0F
        return s

    if what == "seal":
        dh, k, x = sc(), sc(), sc()
        pubs = np.asarray(ed.batch_mul_base(x))
        priv = sc(1)
        pub, ctx = np.asarray(ed.batch_mul_base(priv)), rng.integers(0, 256, size=(1, 32), dtype=np.uint8)
        msgs = [bytes(m) for m in rng.integers(0, 256, size=(n, 142), dtype=np.uint8)]
        return {"fused": lambda: ed.batch_vss_seal(dh, k, priv, pub, pubs, ctx, msgs),
                "composed": lambda: (ed.batch_mul_base(dh), ed.batch_mul_base(k), ed.batch_mul(dh, pubs))}
    if what == "sign":
        k, x = sc(), sc()
        msgs = [bytes(m) for m in rng.integers(0, 256, size=(n, 32), dtype=np.uint8)]
        return {"fused": lambda: ed.batch_schnorr_sign(k, x, msgs), "composed": lambda: (ed.batch_mul_base(k), ed.batch_mul_base(x))}
    f, g = sc(), sc()
    H = np.asarray(ed.batch_mul_base(sc(1)))
    commits = np.asarray(ed.batch_mul_base(sc(4)))
    idx = rng.integers(0, 1 << 16, size=n).astype(np.uint32)
    poly = np.zeros(n, dtype=np.uint32)

    def composed():
        fb, gh = ed.batch_mul_base(f), ed.commit(g, H.tobytes())
        return ed.batch_add(fb, gh), ed.poly_eval(commits, idx)

    return {"fused": lambda: ed.batch_deal_check2(poly, idx, f, g, commits, H, 1, 4), "composed": composed}


def stats(d):
    """per-pass summed kernel time (ms) from the kernel-trace CSVs under d: the trace alternates the fused call and its
    composed counterpart, a pass being a run of consecutive Ed25519 kernels of one of them"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    assert rows, "no kernel trace under " + d
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    name_of = lambda r: r["Kernel_Name"].split("(")[0].split("::")[-1].split("<")[0]
    # (host buffers: besides the runtime's own copy and fill kernels the process runs nothing else; poly_eval's kernel
    # is a template over the MSM's policy and carries no ed25519_ name)
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
        v = v[-20:]  # the passes after the warm-up and the set-up's own multiplications
        ms = sorted(x[0] for x in v)
        out[k + "_kernel_ms"] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "passes": len(ms)}
        out[k + "_kernels_of_the_last_pass_ms"] = v[-1][1]
    out["kernel_time_ratio"] = out["fused_kernel_ms"]["median"] / out["composed_kernel_ms"]["median"]
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
    elif len(sys.argv) > 3 and sys.argv[1] == "--merge":
        out = {"what": WHAT}
        for arg in sys.argv[3:]:
            what, path = arg.split("=", 1)
            out[what] = dict(json.load(open(path)), predicted_ratio=PREDICTED[what])
        open(sys.argv[2], "w").write(json.dumps(out) + "\n")
    else:
        print(__doc__)
