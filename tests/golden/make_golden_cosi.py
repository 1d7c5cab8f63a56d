#!/usr/bin/env python3
"""Extract the messages of lines 384..1023 of the reference's SUPERCOP file into tests/golden/ (data only).  Run where
the reference is checked out at /root/reference; the fixture it writes is committed.

Source: sign/eddsa/testdata/sign.input.gz (TestGolden, eddsa_test.go:285).  tests/golden/ed25519_sign_input_msgs.npz
holds lines 0..383 whole and tests/golden/ed25519_sign_input.npy the keys and signatures of all 1024 lines; with these
messages the 1024 lines make ONE roster of 1024 keys for sign/cosi (cosi_test.go:152-156: a cosignature without its
mask is an EdDSA signature under the aggregate key), tests/_cosi_cases.py sign_input_roster().

Arrays: msgs (sum of lengths,), off (641,) uint64 -- the message of line 384 + i is msgs[off[i]:off[i+1]].
"""
import gzip
import os

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
FIRST, ROWS = 384, 1024


def main():
    kat = np.load(os.path.join(OUT, "ed25519_sign_input.npy"))
    msgs = []
    with gzip.open(f"{REF}/sign/eddsa/testdata/sign.input.gz", "rt") as f:
        for i, line in enumerate(f):
            if i < FIRST:
                continue
            sk, pub, msg, sigmsg = (bytes.fromhex(x) for x in line.strip().split(":")[:4])
            assert sk[32:] == pub == kat[i, 1].tobytes() and len(msg) == i and sigmsg[64:] == msg
            assert sigmsg[:32] == kat[i, 3].tobytes() and sigmsg[32:64] == kat[i, 5].tobytes()
            msgs.append(msg)
    assert len(msgs) == ROWS - FIRST
    off = np.cumsum([0] + [len(m) for m in msgs]).astype(np.uint64)
    np.savez_compressed(os.path.join(OUT, "ed25519_sign_input_msgs_tail.npz"),
                        msgs=np.frombuffer(b"".join(msgs), dtype=np.uint8), off=off)


if __name__ == "__main__":
    main()
