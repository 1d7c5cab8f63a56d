#!/usr/bin/env python3
"""Extract the method sets of the reference's interfaces that go/kyberhip/suite implements into
tests/golden/kyber_interfaces.json (tests/test_cabi.py compares against it).

usage: make_golden_interfaces.py KYBER_SOURCE_TREE   (a checkout of dedis/kyber v4)

Sources, relative to the tree: group.go:23-131 (Point), :175-183 (Group), encoding.go:15-32 (Marshaling),
pairing/pairing.go:8-20 (Suite).  Methods are listed in declaration order; embedded interfaces are not expanded.
"""
import json
import os
import re
import sys

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kyber_interfaces.json")
SOURCES = (("Point", "group.go"), ("Group", "group.go"), ("Marshaling", "encoding.go"), ("Suite", "pairing/pairing.go"))


def iface(src: str, name: str):
    body = src[src.index("type %s interface {" % name):]
    body = body[:body.index("\n}")]
    return re.findall(r"^\t(\w+)\(", body, re.M)


def main(ref: str):
    out = {"source": "dedis/kyber v4: " + ", ".join("%s (%s)" % (f, n) for n, f in SOURCES)}
    for name, f in SOURCES:
        out[name] = iface(open(os.path.join(ref, f)).read(), name)
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
