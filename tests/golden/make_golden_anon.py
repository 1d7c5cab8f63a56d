"""Extracts the three printed examples of the reference's sign/anon tests (sig_test.go: ExampleSign_one,
ExampleSign_anonSet, ExampleSign_linkable) into tests/golden/anon.json: the hex dumps of the six signatures and the
four printed tags.  Data only; run with the path of sig_test.go."""
import json
import os
import re
import sys


def main(path: str) -> None:
    src = open(path).read()
    examples = {}
    for name, body in re.findall(r"func (ExampleSign_\w+)\(\) \{(.*?)\n\}\n", src, re.S):
        out = body.split("// Output:")[1]
        sigs, cur = [], None
        for line in out.splitlines():
            line = line.strip()
            if re.fullmatch(r"// Signature( \d)?:", line):
                cur = []
                sigs.append(cur)
                continue
            m = re.match(r"// [0-9a-f]{8}  ((?:[0-9a-f]{2} +)+)\|", line)
            if m and cur is not None:
                cur.append(m.group(1).replace(" ", ""))
        examples[name] = {"signatures": ["".join(s) for s in sigs],
                          "tags": re.findall(r"// Sig\d tag: ([0-9a-f]{64})", out)}
    assert [len(examples[k]["signatures"]) for k in ("ExampleSign_one", "ExampleSign_anonSet", "ExampleSign_linkable")] == [1, 1, 4]
    doc = {"source": "sign/anon/sig_test.go, the // Output: blocks of the three examples",
           "message": "Hello World!", "bad_message": "Goodbye world!", "scope": "My Linkage Scope",
           "stream": "blake2xb.New(nil)", "examples": examples}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "anon.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
