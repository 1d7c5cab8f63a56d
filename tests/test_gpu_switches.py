"""Every environment switch the shipped library reads selects a code path that must give the reference's bytes: one
subprocess per value (the switches are function-local statics, read once), tests/_switch_probe.py holds each workload
against the oracles.  VERDICT r3 item 2: "test what ships"."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [
    ("fb", {}), ("fb", {"KYB_FB_MIN": "0"}), ("fb", {"KYB_FB_MIN": "1000"}),
    ("msm", {"KYB_MSM_TAIL": "coop"}), ("msm", {"KYB_MSM_TAIL": "lane"}), ("msm", {"KYB_MSM_SUB": "64"}),
    ("msm", {"KYB_MSM_CHUNK": "16"}), ("msm", {"KYB_MSM_CHUNK": "4"}),
    # round 6: the three-lane final kernel instead of the limb-per-lane one; the four-lane fixed-base chain; one staging pool
    ("msm", {"KYB_MSM_FINAL": "lanes"}), ("fb", {"KYB_FB_CHAIN": "lanes"}), ("pipe", {"KYB_STAGE_POOLS": "1"}), ("msm", {"KYB_STAGE_POOLS": "1"}),
    # round 6, the MSM: one-pass sort, the tail that multiplies every chunk's lo * run / the tree all in the fold launches, the
    # one-lane bucket join, one decode kernel for every convention
    ("msmbig", {}), ("msmbig", {"KYB_MSM_SORT": "single"}), ("msmbig", {"KYB_MSM_REDUCE": "mul"}), ("msmbig", {"KYB_MSM_REDUCE": "nofuse"}),
    ("msmbig", {"KYB_MSM_JOIN": "lane"}), ("msmbig", {"KYB_MSM_DECODE": "full"}), ("msmbig", {"KYB_MSM_FINAL": "lanes"}),
    ("msm", {"KYB_MSM_REDUCE": "mul"}), ("msm", {"KYB_MSM_REDUCE": "nofuse"}), ("msm", {"KYB_MSM_JOIN": "lane"}),
    ("msmgiant", {}), ("msmgiant", {"KYB_MSM_JOIN": "lane"}), ("msmgiant", {"KYB_MSM_SORT": "single"}),  # giant buckets
    ("msm", {"KYB_BN_MSM_GLV": "0"}),  # the BN G1 MSM on plain windows instead of balanced GLV halves
    ("msm", {"KYB_BLS_G2_MSM_GLS": "0"}),  # the BLS12-381 G2 MSM on plain windows instead of balanced GLS quarters
    ("msmg2short", {}), ("msmg2short", {"KYB_BLS_G2_MSM_GLS": "0"}), ("msmg2short", {"KYB_BLS_G2_MSM_GLS": "1"}),
    ("msmg2short", {"KYB_BLS_G2_MSM_GLS": "2"}),  # short scalars (KYB_F_SCALAR_BITS) on either G2 adapter
    ("bnhash", {}), ("bnhash", {"KYB_BN_HASH_QUEUE": "0"}), ("bnhash", {"KYB_BN_HASH_HQ": "512"}),
    ("pipe", {}), ("pipe", {"KYB_PIPE_CHUNK": "4096", "KYB_PIPE_STREAMS": "1"}), ("pipe", {"KYB_PIPE_CHUNK": "4096", "KYB_PIPE_STREAMS": "3"}),
    ("unmw2", {}), ("unmw2", {"KYB_UNM_W2": "0"}), ("hashw2", {}), ("hashw2", {"KYB_UNM_W2": "0"}),
    ("g1split", {}), ("g1split", {"KYB_G1_SPLIT": "0"}),
    ("bncheck", {}), ("bncheck", {"KYB_BN_CHECK": "two"}),
    ("lvm", {"KYB_LVM_MIN": "0"}), ("lvm", {"KYB_LVM_MIN": "1000000000"}),
    ("lvm", {"KYB_G2_COOP_MAX": "0"}), ("lvm", {"KYB_G2_COOP_MAX": "0", "KYB_LVM_MIN": "1000000000"}),
    ("lvm", {"KYB_G1_COOP_MAX": "0"}), ("lvm", {"KYB_G1_COOP_MAX": "0", "KYB_LVM_MIN": "0"}), ("lvm", {"KYB_G1_COOP_MAX": "1000000"}),
    # equal, opposite and cancelling operands (tests/_msm_exceptional.py) through every stage variant
    ("msmexc", {}), ("msmexc", {"KYB_MSM_TAIL": "lane"}), ("msmexc", {"KYB_MSM_JOIN": "lane"}), ("msmexc", {"KYB_MSM_REDUCE": "mul"}),
    ("msmexc", {"KYB_MSM_REDUCE": "nofuse"}), ("msmexc", {"KYB_MSM_FINAL": "lanes"}), ("msmexc", {"KYB_MSM_SORT": "single"}),
    ("msmexc", {"KYB_BN_MSM_GLV": "0"}), ("msmexc", {"KYB_BLS_G2_MSM_GLS": "0"}), ("msmexc", {"KYB_BLS_G2_MSM_GLS": "1"}),
    ("msmexc", {"KYB_BLS_G2_MSM_GLS": "2"}),
    # encrypt/ibe: the generator's table through either chain kernel, host staging on one pool
    ("ibe", {}), ("ibe", {"KYB_FB_CHAIN": "lanes"}), ("ibe", {"KYB_STAGE_POOLS": "1"}),
    # the per-lane Mul kernel in pieces of three waves (pairing_abi.cuh mul_dev): the bn256 G2 slab; the BLS12-381 G1 slab
    # without a mask; the lane machine's redo launch with the mask offset per piece
    ("mulpiece", {"KYB_MUL_PIECE": "192"}),
    ("mulpiece-bls12381-g1", {"KYB_MUL_PIECE": "192", "KYB_LVM_MIN": "1000000000", "KYB_G1_COOP_MAX": "0", "KYB_G1_SPLIT": "0"}),
    ("mulpiece-bls12381-g1", {"KYB_MUL_PIECE": "192", "KYB_LVM_MIN": "0", "KYB_G1_COOP_MAX": "0"}),
]


@pytest.mark.parametrize("what,env", CASES, ids=[f"{w}-{'-'.join(f'{k}={v}' for k, v in e.items()) or 'default'}" for w, e in CASES])
def test_switch(what, env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_switch_probe.py"), what], env=e, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0 and f"switch-probe ok {what}" in r.stdout, r.stdout[-3000:]
