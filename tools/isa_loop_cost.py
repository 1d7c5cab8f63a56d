"""Issue cost of the loops of one kernel in a gfx950 assembly listing (hipcc --cuda-device-only -S): the opcode histogram
of tools/isa_loop_hist.py, each VALU instruction weighted with the measured cycles per wave64 instruction of
tools/valu_rates.hip (profiles/r02_valu_rates.jsonl):
python tools/isa_loop_cost.py file.s <kernel-name-substring> [min_valu] [rates.jsonl].
A VALU-bound kernel (the Ed25519 window loop: 97.6 % busy) takes the sum of these costs; instructions the table does not
name cost what their class costs there: 2.85 cycles with two 32-bit operands, 4.7 with three, 4.85 on 64-bit values."""
import collections
import json
import os
import re
import sys

RATE_OF = {"v_mad_i64_i32": "mad_i64_i32", "v_mad_u64_u32": "mad_u64_u32", "v_ashrrev_i64": "ashr_i64",
           "v_lshl_add_u64": "lshl_add_u64", "v_mul_lo_u32": "mul_lo_u32", "v_mul_hi_u32": "mul_hi_u32",
           "v_add_u32": "add_u32", "v_sub_u32": "sub_u32", "v_subrev_u32": "sub_u32", "v_and_b32": "and_b32",
           "v_ashrrev_i32": "ashr_i32", "v_alignbit_b32": "alignbit", "v_add3_u32": "add3_u32", "v_and_or_b32": "and_or",
           "v_lshl_add_u32": "lshl_add_u32", "v_bfe_i32": "bfe_i32", "v_cndmask_b32": "cndmask",
           "v_mad_i32_i24": "mad_u32_u24", "v_mad_u32_u24": "mad_u32_u24", "v_mul_i32_i24": "mul_i32_i24",
           "v_add_co_u32": "add_co_pair", "v_addc_co_u32": "add_co_pair", "v_sub_co_u32": "add_co_pair", "v_subb_co_u32": "add_co_pair"}
TWO_OP, THREE_OP, WIDE = 2.85, 4.7, 4.85


def cost_of(op, nsrc, rates):
    if op in RATE_OF:
        return rates[RATE_OF[op]]
    if op.endswith(("_b64", "_u64", "_i64")):
        return WIDE
    return THREE_OP if nsrc >= 3 else TWO_OP


def main():
    lines = open(sys.argv[1]).read().split("\n")
    name = sys.argv[2]
    min_valu = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    rates_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "r02_valu_rates.jsonl")
    rates = {r["instr"]: r["cycles_per_wave_instr"] for r in map(json.loads, open(rates_path)) if "instr" in r}
    start = next(i for i, l in enumerate(lines) if l.startswith("_") and name in l and l.split(";")[0].rstrip().endswith(":"))
    end = next(i for i in range(start + 1, len(lines)) if lines[i].startswith(".Lfunc_end"))
    body = lines[start:end]
    labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    for i, l in enumerate(body):
        t = l.strip().split()
        if not t or not (t[0].startswith("s_cbranch") or t[0] == "s_branch"):
            continue
        tgt = t[-1]
        if tgt not in labels or labels[tgt] >= i:
            continue
        ops, cycles = collections.Counter(), collections.Counter()
        for x in body[labels[tgt]:i]:
            code = x.split(";")[0].strip()
            tt = code.split()
            if not tt or tt[0].startswith(".") or tt[0].endswith(":"):
                continue
            op = re.sub(r"_e32|_e64", "", tt[0])
            ops[op] += 1
            if op.startswith("v_"):
                cycles[op] += cost_of(op, len(code[len(tt[0]):].split(",")) - 1, rates)
        valu = sum(v for k, v in ops.items() if k.startswith("v_"))
        if valu < min_valu:
            continue
        print(f"loop {tgt}: {valu} VALU, {sum(v for k, v in ops.items() if k.startswith('v_mad_'))} MAD, {sum(cycles.values()):.0f} cycles")
        print("   " + ", ".join(f"{k} {v}" for k, v in ops.most_common(16)))
        print("   cycles: " + ", ".join(f"{k} {v:.0f}" for k, v in cycles.most_common(10)))


if __name__ == "__main__":
    main()
