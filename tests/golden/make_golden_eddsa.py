#!/usr/bin/env python3
"""Extract the seeds of the reference's SUPERCOP file into tests/golden/ (data only).  Run where the reference is
checked out at /root/reference; the fixture it writes is committed.

Source: sign/eddsa/testdata/sign.input.gz (TestGolden, eddsa_test.go:285).  Field 1 of a line is seed || public key;
tests/golden/ed25519_sign_input.npy holds, for all 1024 lines, the columns a, A, r, R, h, S that eddsa.go computes from
that seed and the line's message.  Before anything is written every line is held to them: SHA-512(seed)[0:32] clamped
(curve.go:51-60) is column 0, and bytes 32..64 of field 1 are column 1.

Array: eddsa_sign_input_seeds.npy (1024, 32) uint8 -- the seed of line i.
"""
import gzip
import hashlib
import os

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROWS = 1024


def main():
    kat = np.load(os.path.join(OUT, "ed25519_sign_input.npy"))
    seeds = []
    with gzip.open(f"{REF}/sign/eddsa/testdata/sign.input.gz", "rt") as f:
        for i, line in enumerate(f):
            sk = bytes.fromhex(line.strip().split(":")[0])
            assert len(sk) == 64
            d = bytearray(hashlib.sha512(sk[:32]).digest())
            d[0] &= 0xF8
            d[31] &= 0x7F
            d[31] |= 0x40
            assert bytes(d[:32]) == kat[i, 0].tobytes() and sk[32:] == kat[i, 1].tobytes(), i
            seeds.append(sk[:32])
    assert len(seeds) == ROWS
    np.save(os.path.join(OUT, "eddsa_sign_input_seeds.npy"), np.frombuffer(b"".join(seeds), dtype=np.uint8).reshape(ROWS, 32))


if __name__ == "__main__":
    main()
