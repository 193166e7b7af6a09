#!/usr/bin/env python3
"""Writes tests/golden/reference_test_methods.json: the names of every test method of the
reference's TestCompactionQueue.java and TestTsdbQueryRollup.java (names only, no program text),
so the "every test method is transcribed" tests need no reference tree.

  python tests/golden/make_method_lists_golden.py REFERENCE_TREE
"""
import json
import os
import re
import sys

FILES = {
    "TestCompactionQueue": ("test/core/TestCompactionQueue.java", {"before"}),
    "TestTsdbQueryRollup": ("test/core/TestTsdbQueryRollup.java", {"beforeLocal"}),
}


def main():
    ref = sys.argv[1]
    out = {}
    for cls, (rel, setup) in FILES.items():
        with open(os.path.join(ref, rel)) as f:
            out[cls] = sorted(set(re.findall(r"public void (\w+)\(\) throws", f.read())) - setup)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_test_methods.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print({k: len(v) for k, v in out.items()})


if __name__ == "__main__":
    main()
