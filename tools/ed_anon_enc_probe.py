#!/usr/bin/env python3
"""Times the two fused calls of sign/anon's encryption against the standing calls they contain, at 2^16 product lanes --
ring 16 with 4 096 messages and ring 1 with 2^16 messages, of 32 bytes each, one set shared by the batch -- as summed
kernel time from a kernel trace (medians of 20 alternating passes after a warm-up; host buffers -- copies are no kernels):
  * "seal16", "seal1":  kyb_ed25519_anon_seal against kyb_ed25519_mul over the n ring (scalar, member) pairs plus
                        kyb_ed25519_mul_base over the n scalars;
  * "open16", "open1":  kyb_ed25519_anon_open of what the seal made against kyb_ed25519_mul over n (ring + 1) pairs -- the
                        ring's products and priv X -- plus kyb_ed25519_mul_base over n.
The composed side has no hash, no comparison and no stream cipher: it is the points alone.  Next to each measured ratio
stands the one predicted by counting field multiplications (PREDICTED below; DESIGN.md section 5 item 67 has the count).
  tools/ed_anon_enc_probe.py --once WHAT     21 alternating passes of the fused call and its composed counterpart: the body of
                                             `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ed_anon_enc_probe.py --once WHAT`
  tools/ed_anon_enc_probe.py --stats DIR     per-pass summed kernel time from that trace (medians of the last 20)
  tools/ed_anon_enc_probe.py --e2e WHAT      wall time from host buffers, no profiler: the fused call (median of 5) against
                                             the composed calls with their hashing in Python (util/blake2xb.py; one pass)
  tools/ed_anon_enc_probe.py --merge OUT seal16=STATS ... e2e_seal16=E2E ...     profiles/ed_anon_enc_probe.json
"""
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FUSED = ("ed25519_anon_tables_kernel", "ed25519_anon_seal_head_kernel", "ed25519_anon_open_head_kernel", "ed25519_anon_points_kernel",
         "ed25519_anon_encode_kernel", "ed25519_anon_slot_kernel", "ed25519_anon_body_kernel")
SHAPES = {"16": (4096, 16), "1": (1 << 16, 1)}
# Field multiplications, squarings counted as such: a constant-structure ladder of 63
# windows 2 276, a decoding 275 and the table behind it 57, a comb 112, a shared encoding 22, an encoding of one's own
# 265; a BLAKE2b compression is taken as 13 of them (about 3 400 32-bit operations against about 260 for a product).
LADDER, DECODE, TABLE, COMB, ENC, OWN_ENC, HASH = 2276, 275, 57, 112, 22, 265, 13
MUL, MUL_BASE = LADDER + DECODE + TABLE + ENC, COMB + ENC


def predicted(what: str) -> float:
    n, ring = SHAPES[what[4:]]
    tables = ring * (DECODE + TABLE) / n  # once per call
    if what.startswith("seal"):
        fused = ring * (LADDER + ENC + 2 * HASH) + COMB + ENC + 4 * HASH + tables
        return fused / (ring * MUL + MUL_BASE)
    fused = ring * (LADDER + ENC + 2 * HASH) + (DECODE + TABLE + LADDER + OWN_ENC + 2 * HASH + COMB + ENC) + 4 * HASH + tables
    return fused / ((ring + 1) * MUL + MUL_BASE)


WHAT = ("summed kernel time from a kernel trace at 2^16 product lanes (ring 16 x 4 096 messages, ring 1 x 2^16 messages, 32 bytes each, "
        "one shared set), medians of 20 alternating passes; predicted: by counting field multiplications; e2e: wall time from host buffers")


def inputs(what: str):
    from kyber_amd.group import edwards25519 as ed

    n, ring = SHAPES[what[4:]]
    rng = np.random.default_rng(n + ring)

    def sc(k):
        s = rng.integers(0, 256, size=(k, 32), dtype=np.uint8)
        s[:, 0] &= 0xF8
        s[:, 31] = (s[:, 31] & 0x3F) | 0x40  # clamped, as NewKey leaves them
        return s

    privs, x = sc(ring), sc(n)
    keys = np.asarray(ed.batch_mul_base(privs)).reshape(1, 32 * ring)
    msgs = [bytes(m) for m in rng.integers(0, 256, size=(n, 32), dtype=np.uint8)]
    return ed, n, ring, privs, x, keys, msgs


def paths(what: str):
    ed, n, ring, privs, x, keys, msgs = inputs(what)
    xr = np.repeat(x, ring, axis=0)                       # lane (i, k): scalar i
    kr = np.tile(keys.reshape(ring, 32), (n, 1))          # ... member k
    if what.startswith("seal"):
        return {"fused": lambda: ed.batch_anon_seal(keys, x, msgs, ring), "composed": lambda: (ed.batch_mul(xr, kr), ed.batch_mul_base(x))}
    cts, st = ed.batch_anon_seal(keys, x, msgs, ring)
    assert not np.asarray(st).any()
    mine = np.arange(n, dtype=np.uint32) % ring
    pv = privs[mine]
    X = np.frombuffer(b"".join(c[:32] for c in cts), dtype=np.uint8).reshape(n, 32)
    xo, ko = np.concatenate([xr, pv]), np.concatenate([kr, X])

    def fused():
        out, st = ed.batch_anon_open(keys, mine, pv, cts, ring)
        assert not np.asarray(st).any()

    return {"fused": fused, "composed": lambda: (ed.batch_mul(xo, ko), ed.batch_mul_base(x))}


def e2e(what: str):
    """wall seconds: the fused seal from host buffers, and the same ciphertexts from the composed calls with the hashes in
    Python"""
    import torch

    from kyber_amd.util import blake2xb

    assert what.startswith("seal")
    ed, n, ring, privs, x, keys, msgs = inputs(what)
    ed.batch_anon_seal(keys, x[:64], msgs[:64], ring)  # warm-up
    fused = []
    for _ in range(5):
        t = time.perf_counter()
        cts, _ = ed.batch_anon_seal(keys, x, msgs, ring)
        torch.cuda.synchronize()
        fused.append(time.perf_counter() - t)
    xr, kr = np.repeat(x, ring, axis=0), np.tile(keys.reshape(ring, 32), (n, 1))
    t = time.perf_counter()
    S, _ = ed.batch_mul(xr, kr)
    X = np.asarray(ed.batch_mul_base(x))
    S = np.asarray(S)
    points_s = time.perf_counter() - t
    order = ed.ORDER
    out = []
    for i in range(n):
        xb = (int.from_bytes(bytes(x[i]), "little") % order).to_bytes(32, "little")
        slots = b"".join(blake2xb.New(bytes(S[i * ring + k])).XORKeyStream(xb) for k in range(ring))
        ctx = blake2xb.New(xb).XORKeyStream(msgs[i])
        out.append(bytes(X[i]) + slots + ctx + blake2xb.New(ctx).Read(16))
    composed = time.perf_counter() - t
    assert out == cts, "the composed path and the fused call disagree"
    fused.sort()
    return {"fused_s": {"median": fused[2], "min": fused[0], "max": fused[-1], "passes": 5}, "composed_s": composed,
            "composed_points_s": points_s, "composed_python_hash_s": composed - points_s, "wall_ratio": fused[2] / composed,
            "wall_ratio_against_the_points_alone": fused[2] / points_s}


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
        v = v[-20:]  # the passes after the warm-up and the set-up's own calls
        ms = sorted(x[0] for x in v)
        out[k + "_kernel_ms"] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "passes": len(ms)}
        out[k + "_kernels_of_the_last_pass_ms"] = v[-1][1]
    out["kernel_time_ratio"] = out["fused_kernel_ms"]["median"] / out["composed_kernel_ms"]["median"]
    return out


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--once":
        import torch

        p = paths(sys.argv[2])
        for _ in range(21):
            for k in ("fused", "composed"):
                p[k]()
                torch.cuda.synchronize()
    elif len(sys.argv) > 2 and sys.argv[1] == "--stats":
        print(json.dumps(stats(sys.argv[2])))
    elif len(sys.argv) > 2 and sys.argv[1] == "--e2e":
        print(json.dumps(e2e(sys.argv[2])))
    elif len(sys.argv) > 3 and sys.argv[1] == "--merge":
        out = {"what": WHAT}
        for arg in sys.argv[3:]:
            what, path = arg.split("=", 1)
            d = json.load(open(path))
            out[what] = d if what.startswith("e2e") else dict(d, predicted_ratio=predicted(what))
        open(sys.argv[2], "w").write(json.dumps(out) + "\n")
    else:
        print(__doc__)
