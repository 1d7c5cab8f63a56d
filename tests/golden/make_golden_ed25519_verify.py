#!/usr/bin/env python3
"""Extract the first 384 signed messages of the reference's SUPERCOP file into tests/golden/ (data only).  Run where
the reference is checked out at /root/reference; the fixture it writes is committed.

Source: sign/eddsa/testdata/sign.input.gz (TestGolden, eddsa_test.go:285), lines 0..383: line i signs a message of
i bytes, so with the 64 hashed bytes R || A in front these cross every SHA-512 block boundary up to four blocks
(message lengths 47/48, 175/176, 303/304).  tests/golden/ed25519_sign_input.npy holds the same rows' derived scalars
for all 1024 lines but not the messages.

Arrays: pub (384, 32), sig (384, 64), msgs (sum of lengths,), off (385,) uint64 -- message i is msgs[off[i]:off[i+1]].
"""
import gzip
import os

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROWS = 384


def main():
    pubs, sigs, msgs = [], [], []
    with gzip.open(f"{REF}/sign/eddsa/testdata/sign.input.gz", "rt") as f:
        for i, line in enumerate(f):
            if i == ROWS:
                break
            sk, pub, msg, sigmsg = (bytes.fromhex(x) for x in line.strip().split(":")[:4])
            assert sk[32:] == pub and len(msg) == i and sigmsg[64:] == msg
            pubs.append(pub)
            sigs.append(sigmsg[:64])
            msgs.append(msg)
    off = np.cumsum([0] + [len(m) for m in msgs]).astype(np.uint64)
    np.savez_compressed(os.path.join(OUT, "ed25519_sign_input_msgs.npz"),
                        pub=np.frombuffer(b"".join(pubs), dtype=np.uint8).reshape(ROWS, 32),
                        sig=np.frombuffer(b"".join(sigs), dtype=np.uint8).reshape(ROWS, 64),
                        msgs=np.frombuffer(b"".join(msgs), dtype=np.uint8), off=off)


if __name__ == "__main__":
    main()
