#!/bin/bash
# A/B: library builds kyber_amd/lib/libkyberhip_<v>.so against each other on one box: per-suite probes + the bench
# usage: r03_ab.sh OUTPUT_DIR   (results go to OUTPUT_DIR/r03_ab)
O=${1:?usage: r03_ab.sh OUTPUT_DIR}/r03_ab
mkdir -p $O; rocm-smi --showclocks --showperflevel --showpower --showmemuse > $O/smi_$(date +%s).txt 2>&1
for v in ${VARIANTS:-a b c d}; do
  L=$PWD/kyber_amd/lib/libkyberhip_$v.so
  for s in bls12381 bn256 bn254; do
    KYBER_HIP_LIB=$L timeout 300 python tools/ab_probe.py $s 65536 5 > $O/probe_${s}_$v.json 2> $O/probe_${s}_$v.err
  done
  [ -n "$SKIP_BENCH" ] || KYBER_HIP_LIB=$L timeout 400 python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-host-path > $O/bench_$v.json 2> $O/bench_$v.err
done
cat $O/probe_*.json; tail -n 2 $O/*.err | grep -v amdgpu.ids | head -30
