#!/usr/bin/env python3
"""Times sign/bdn's fused calls on the pairing suites against the path they replace (the parent commit's
kyber_amd/sign/bdn.py: BLAKE2Xs in Python, then one mul and one add call, or an MSM of 129-bit scalars per mask), end to
end from host buffers with the host clock around calls that end in a synchronise, medians after a warm-up, profiler off:
  (a) NewMask: kyb_*_bdn_terms_* for 3 000 BLS12-381 G1 keys and 1 024 bn256 G2 keys, untrusted and vouched for, against
      hash_point_to_r + Engine.mul + Engine.add;
  (b) AggregatePublicKeys: one full and one half mask over 3 000 BLS12-381 G1 keys (the reference benchmark's shape),
      kyb_*_mask_aggregate_* at the planned S and at S = 1 (kyb_bdn_debug_set_slices), against Scheme.aggregate_public_keys as it
      stands (which hashes the roster again) and against its MSM alone;
  (c) VerifyBatch on bn256, 256 and 2^16 elements over 128 and 1 024 keys: one mask_aggregate + batch_verify with
      validated keys, against one MSM per element + an untrusted batch_verify (the MSMs of the 2^16 case are timed on 64
      elements and scaled: 65 536 calls are not worth the device time).
  tools/bdn_probe.py [out.json]      the timings above -> profiles/bdn_probe.json
  tools/bdn_probe.py --once          21 passes of NewMask and of the two aggregations: the body of a
                                     `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bdn_probe.py --once`
  tools/bdn_probe.py --stats DIR OUT merges the per-kernel times of that trace (the one-lane root among them) into OUT
"""
import csv
import glob
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

REPS = 20


def med(f, reps=REPS):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return {"median_ms": round(1e3 * statistics.median(ts), 4), "min_ms": round(1e3 * min(ts), 4), "reps": reps}


def keys(suite, group, m, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
    s[:, 0] &= 0x0F
    out, st = (suite.g1_commit if group == 1 else suite.g2_commit)(s)
    assert not np.asarray(st).any()
    return np.ascontiguousarray(out)


def new_mask_paths(suite, group, m):
    from kyber_amd.sign import bdn

    eng = suite.ENGINE
    roster = keys(suite, group, m, m)
    pubs = [bytes(r) for r in roster]

    def old():
        c = bdn.hash_point_to_r(pubs)
        sc = b"".join(x.to_bytes(32, "big") for x in c)
        t, st = eng.mul(group, sc, roster, False)
        return eng.add(group, t, roster)[0]

    def hash_only():
        return bdn.hash_point_to_r(pubs)

    return roster, old, hash_only, (lambda: eng.bdn_terms(group, roster, 0)), (lambda: eng.bdn_terms(group, roster, 0x100))


def aggregate_paths(suite, group, m):
    from kyber_amd.sign import bdn

    eng = suite.ENGINE
    roster = keys(suite, group, m, m)
    coefs, terms, st = eng.bdn_terms(group, roster, 0)
    assert not np.asarray(st).any()
    terms = np.ascontiguousarray(terms)
    L = (m + 7) >> 3
    full = np.full((1, L), 0xFF, np.uint8)
    half = np.zeros((1, L), np.uint8)
    half[0, :L // 2] = 0xFF
    pubs = [bytes(r) for r in roster]
    sch = bdn.Scheme(suite)
    cp1 = [(int.from_bytes(bytes(c), "little") + 1).to_bytes(32, "big") for c in np.asarray(coefs)]
    out = {}
    for label, mk in (("full", full), ("half", half)):
        bits = [bool(mk[0, j >> 3] >> (j & 7) & 1) for j in range(m)]
        on = [j for j in range(m) if bits[j]]
        sc, pts = b"".join(cp1[j] for j in on), np.ascontiguousarray(roster[on])
        # the parent's Scheme keeps keys on G2; its path for either group is the MSM below after the Python hash
        out[label] = {
            "fused": lambda mk=mk: eng.mask_aggregate(group, terms, mk, 0x100),
            "msm_only": lambda sc=sc, pts=pts: eng.msm(group, sc, pts, suite.F_SCALAR_BITS(129)),
            "parent": (lambda bits=bits: sch.aggregate_public_keys(pubs, bits)) if group == 2 else
                      (lambda sc=sc, pts=pts: (bdn.hash_point_to_r(pubs), eng.msm(group, sc, pts, suite.F_SCALAR_BITS(129)))),
        }
    return out


def run_all(path):
    import torch

    from kyber_amd.pairing import bls12381, bn256
    from kyber_amd import _lib
    from kyber_amd.sign import bdn, bls

    assert torch.cuda.is_available(), "the probe needs the GPU: it does not fall back"
    res = {"reps": REPS, "device": torch.cuda.get_device_name(0), "fill": 65536}
    # (a)
    for tag, suite, group, m in (("bls12381_g1_3000", bls12381, 1, 3000), ("bn256_g2_1024", bn256, 2, 1024)):
        roster, old, hash_only, new, new_trusted = new_mask_paths(suite, group, m)
        res["newmask_" + tag] = {"fused": med(new), "fused_trusted": med(new_trusted), "parent": med(old, 3), "parent_python_hash": med(hash_only, 3)}
    # (b)
    ap = aggregate_paths(bls12381, 1, 3000)
    res["plan_1_3000"] = bls12381.ENGINE.bdn_plan(1, 3000)
    for label, p in ap.items():
        row = {"fused_planned_S": med(p["fused"]), "msm_only": med(p["msm_only"]), "parent": med(p["parent"], 3)}
        for S in (1, 8, 64):
            _lib.load().kyb_bdn_debug_set_slices(S)
            row[f"fused_S{S}"] = med(p["fused"])
        _lib.load().kyb_bdn_debug_set_slices(0)
        res["aggregate_bls12381_g1_3000_" + label] = row
    # (c)
    sch_bls = bls.NewSchemeOnG1_bn256()
    for m in (128, 1024):
        roster = keys(bn256, 2, m, 7 * m)
        coefs, terms, st = bn256.ENGINE.bdn_terms(2, roster, 0)
        terms = np.ascontiguousarray(terms)
        cp1 = np.frombuffer(b"".join((int.from_bytes(bytes(c), "little") + 1).to_bytes(32, "big") for c in np.asarray(coefs)), np.uint8).reshape(m, 32)
        for n in (256, 1 << 16):
            rng = np.random.default_rng(n + m)
            masks = rng.integers(0, 256, size=(n, (m + 7) >> 3), dtype=np.uint8)
            msgs = [b"block %08d" % i for i in range(n)]
            sigs = keys(bn256, 1, 256, 3)[np.arange(n) % 256]  # valid points; the verdicts are False, the work is the same
            siglist = [bytes(s) for s in sigs]

            def fused():
                out, cnt, st = bn256.ENGINE.mask_aggregate(2, terms, masks, 0x100)
                return sch_bls.batch_verify([bytes(o) for o in out], msgs, siglist, keys_validated=True)

            def aggregate_only():
                return bn256.ENGINE.mask_aggregate(2, terms, masks, 0x100)

            sample = min(n, 64)

            def msms():
                outs = []
                for i in range(sample):
                    on = np.flatnonzero(np.unpackbits(masks[i], bitorder="little")[:m])
                    outs.append(bytes(bn256.ENGINE.msm(2, np.ascontiguousarray(cp1[on]), np.ascontiguousarray(roster[on]), bn256.F_SCALAR_BITS(129))[0]))
                return outs

            agg_keys = [bytes(o) for o in aggregate_only()[0]]

            def untrusted_verify():
                return sch_bls.batch_verify(agg_keys, msgs, siglist, keys_validated=False)

            reps = REPS if n == 256 else 3
            res[f"verifybatch_bn256_m{m}_n{n}"] = {"fused": med(fused, reps), "fused_aggregate_only": med(aggregate_only, reps),
                                                   "parent_msm_per_element_sampled": dict(med(msms, 3), elements=sample),
                                                   "parent_untrusted_batch_verify": med(untrusted_verify, reps)}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    json.dump(res, open(path, "w"), indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


def run_once():
    from kyber_amd.pairing import bls12381, bn256

    for suite, group, m in ((bls12381, 1, 3000), (bn256, 2, 1024)):
        _, _, _, new, _ = new_mask_paths(suite, group, m)
        for _ in range(21):
            new()
    ap = aggregate_paths(bls12381, 1, 3000)
    for _ in range(21):
        ap["full"]["fused"]()
        ap["half"]["fused"]()


def merge_stats(directory, out):
    """per kernel of the trace: calls and the median and the largest time of a call, in microseconds"""
    times = {}
    for f in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            if "bdn_" in name:
                short = name[name.index("bdn_"):].split("(")[0][:60]
                times.setdefault(short, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    rows = {k: {"calls": len(v), "median_us": round(statistics.median(v), 2), "max_us": round(max(v), 2)} for k, v in times.items()}
    res = json.load(open(out)) if os.path.exists(out) else {}
    res["kernel_trace"] = rows
    json.dump(res, open(out, "w"), indent=1, sort_keys=True)
    print(json.dumps(rows, sort_keys=True))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--once":
        run_once()
    elif len(sys.argv) > 1 and sys.argv[1] == "--stats":
        merge_stats(sys.argv[2], sys.argv[3])
    else:
        run_all(sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "bdn_probe.json"))
