#!/usr/bin/env python3
"""Times kyb_ed25519_cosi_verify against two baselines this unit does not change, in one process, medians of 20 after a
warm-up, alternating, at N = 2^16 signatures over ONE roster of m keys:
  * "verify":   kyb_ed25519_verify on the same (A_i, msg_i, V_i || r_i) on device buffers, the aggregate keys computed
                beforehand.  The excess of cosi over it is the whole price of aggregation, the extra encode pass and
                the tables.  Next to each measured ratio stands the one predicted by counting field multiplications:
                about 8 per table addition against about 2 900 per verification.
  * "composed": sign/cosi's _verify_batch_composed from host buffers (one mask_aggregate, SHA-512 on the host, one mul2,
                the comparison), against batch_cosi_verify from the same host buffers: the end-to-end figure.
for m in {16, 128, 1024} and masks full, half-dense random and one third absent.  The table width is the rule's
(kyb_ed25519_cosi_group_width: 8 at this N for every m > 4); width 4 cannot be asked for at this N and is not measured.
Signatures are random bytes: the lane programs do the same work whatever the verdict.
  tools/ed_cosi_probe.py [out.json]            hipEvent time around cosi and verify on device buffers, the host clock
                                               around the fused and the composed host paths (profiler off)
  tools/ed_cosi_probe.py --once M MASKS N      21 alternating passes of cosi and verify: the body of a
                                               `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/ed_cosi_probe.py --once M MASKS N`
  tools/ed_cosi_probe.py --stats DIR           per-pass summed kernel time from that trace (medians of the last 20)
  tools/ed_cosi_probe.py --merge OUT EVENTS m16/full=STATS ...   profiles/ed_cosi_probe.json
"""
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

COSI = ("ed25519_cosi_roster_kernel", "ed25519_cosi_tables_kernel", "ed25519_cosi_total_kernel", "ed25519_cosi_aggregate_kernel",
        "ed25519_cosi_encode_kernel", "ed25519_cosi_check_kernel", "ed25519_cosi_verdict_kernel")
VERIFY = ("ed25519_verify_kernel", "ed25519_verify_encode_kernel")
MASKS = ("full", "half", "third_absent")
MUL_PER_ADD, MUL_PER_VERIFY = 8, 2900
MSG_LEN = 32


def make(m: int, masks: str, n: int):
    """host arrays of the probe's inputs: roster, masks (n, L), sigs (n, 64), messages"""
    from kyber_amd.group import edwards25519 as ed

    rng = np.random.default_rng(1000 * m + n)
    s = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
    s[:, 31] &= 0x0F
    roster = np.asarray(ed.batch_mul_base(s))
    p = {"full": 1.0, "half": 0.5, "third_absent": 2.0 / 3.0}[masks]
    bits = rng.random((n, m)) < p
    mk = np.packbits(bits, axis=1, bitorder="little")
    sigs = rng.integers(0, 256, size=(n, 64), dtype=np.uint8)
    sigs[:, 63] &= 0x0F
    msgs = rng.integers(0, 256, size=(n, MSG_LEN), dtype=np.uint8)
    return roster, np.ascontiguousarray(mk), sigs, msgs, bits


def predicted(m: int, bits, g: int) -> float:
    """1 + 8 * (table additions per lane) / 2 900: a group adds where some lane of its wave has a non-zero digit in the
    polarity that lane walks; the complement's T_all - acc is one more"""
    n = bits.shape[0]
    flip = 2 * bits.sum(axis=1) > m
    walk = np.where(flip[:, None], ~bits, bits)
    pad = (-m) % g
    d = np.pad(walk, ((0, (-n) % 64), (0, pad))).reshape(-1, 64, (m + pad) // g, g).any(axis=3)
    adds = d.any(axis=1).sum(axis=1).mean() + flip.mean()
    return 1.0 + MUL_PER_ADD * float(adds) / MUL_PER_VERIFY


def paths(m: int, masks: str, n: int):
    import torch

    from kyber_amd import _lib
    from kyber_amd.group import edwards25519 as ed

    roster, mk, sigs, msgs, bits = make(m, masks, n)
    dev = lambda a: torch.from_numpy(a).cuda()
    d_roster, d_mk, d_sigs, d_blob = dev(roster), dev(mk), dev(sigs), dev(msgs.reshape(-1))
    d_off = dev(np.arange(n + 1, dtype=np.int64) * MSG_LEN)
    d_agg = ed.batch_mask_aggregate(d_roster, d_mk)[0]
    lib = _lib.load()
    ok2, st2 = torch.empty(n, dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")

    def cosi():
        return ed.batch_cosi_verify(d_roster, (d_blob, d_off), d_sigs, d_mk)[0]

    def verify():
        _lib.check(lib.kyb_ed25519_verify_dev(n, d_agg.data_ptr(), d_blob.data_ptr(), d_off.data_ptr(), d_sigs.data_ptr(), ok2.data_ptr(),
                                              st2.data_ptr(), 0, torch.cuda.current_stream().cuda_stream), "kyb_ed25519_verify_dev")
        return ok2

    return {"cosi": cosi, "verify": verify}, (roster, mk, sigs, msgs, bits)


def med(v):
    return {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "reps": len(v)}


def time_one(m: int, masks: str, n: int, reps: int = 20):
    import time

    import torch

    from kyber_amd.group import edwards25519 as ed
    from kyber_amd.sign import cosi as C

    p, (roster, mk, sigs, msgs, bits) = paths(m, masks, n)
    for f in p.values():
        f()
    ms = {k: [] for k in p}
    for _ in range(reps):
        for k, f in p.items():  # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    g = ed.cosi_group_width(n, m)
    res = {"n": n, "m": m, "masks": masks, "width": g, "cosi_ms_events": med(ms["cosi"]), "verify_ms_events": med(ms["verify"])}
    res["event_time_ratio"] = res["cosi_ms_events"]["median"] / res["verify_ms_events"]["median"]
    res["predicted_ratio"] = predicted(m, bits, g)
    rb, ml, sl, mm = roster.tobytes(), [x.tobytes() for x in mk], [x.tobytes() for x in sigs], [x.tobytes() for x in msgs]
    host = {"fused": lambda: ed.batch_cosi_verify(rb, mm, sl, ml)[0], "composed": lambda: C._verify_batch_composed(rb, mm, sl, ml)[0]}
    assert (np.asarray(host["fused"]()) == np.asarray(host["composed"]())).all()  # warm-up, and the answers
    hs = {k: [] for k in host}
    for _ in range(3):  # the composed path hashes 2^16 messages in Python: three passes
        for k, f in host.items():
            t0 = time.perf_counter()
            f()
            hs[k].append(1e3 * (time.perf_counter() - t0))
    res["fused_ms_end_to_end"], res["composed_ms_end_to_end"] = med(hs["fused"]), med(hs["composed"])
    res["end_to_end_ratio"] = res["fused_ms_end_to_end"]["median"] / res["composed_ms_end_to_end"]["median"]
    return res


def stats(d):
    """per-pass summed kernel time (ms) of cosi and verify from the kernel-trace CSVs under d: the trace alternates the
    two, a pass being a run of consecutive kernels of one of them (kernels of neither are skipped)"""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    assert rows, "no kernel trace under " + d
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    name_of = lambda r: r["Kernel_Name"].split("(")[0].split("::")[-1].split("<")[0]
    kind = lambda r: "cosi" if name_of(r) in COSI else ("verify" if name_of(r) in VERIFY else None)
    passes, prev = {"cosi": [], "verify": []}, None
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
        v = v[-20:]  # the passes after the warm-up (setup runs a mask_aggregate before them)
        ms = sorted(x[0] for x in v)
        out[k + "_kernel_ms"] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1], "passes": len(ms)}
        out[k + "_kernels_of_the_last_pass_ms"] = v[-1][1]
    out["kernel_time_ratio"] = out["cosi_kernel_ms"]["median"] / out["verify_kernel_ms"]["median"]
    return out


if __name__ == "__main__":
    if len(sys.argv) > 4 and sys.argv[1] == "--once":
        import torch

        p, _ = paths(int(sys.argv[2]), sys.argv[3], int(sys.argv[4]))
        torch.cuda.synchronize()
        for _ in range(21):
            for k in ("cosi", "verify"):
                p[k]()
                torch.cuda.synchronize()
    elif len(sys.argv) > 2 and sys.argv[1] == "--stats":
        print(json.dumps(stats(sys.argv[2])))
    elif len(sys.argv) > 3 and sys.argv[1] == "--merge":
        out = json.load(open(sys.argv[3]))
        for arg in sys.argv[4:]:
            what, path = arg.split("=", 1)
            out[what]["kernel_trace"] = json.load(open(path))
        open(sys.argv[2], "w").write(json.dumps(out) + "\n")
    else:
        n = 1 << 16
        res = {"what": "kyb_ed25519_cosi_verify at 2^16 signatures over one roster of m keys, medians of 20, alternating, against "
                       "kyb_ed25519_verify on the same (A, msg, V || r) (hipEvent time, device buffers; predicted_ratio counts 8 "
                       "field multiplications per table addition against 2 900 per verification) and against "
                       "_verify_batch_composed from host buffers (host clock, medians of 3); kernel_trace, where present: summed "
                       "kernel time from a kernel trace in a run of its own.  The width is the rule's; width 4 is not reachable at "
                       "this n and is not measured."}
        for m in (16, 128, 1024):
            for masks in MASKS:
                res["m%d/%s" % (m, masks)] = time_one(m, masks, n)
        line = json.dumps(res)
        print(line)
        if len(sys.argv) > 1:
            open(sys.argv[1], "w").write(line + "\n")
