#!/usr/bin/env python3
"""Record the line count of every Rust source of a checkout of the reference
(NealRame/nr-ray-tracer) in tests/golden/reference_rs_lines.json, the fixture
tests/test_citations.py checks the repository's `<file>.rs:N-M` citations against.

    python scripts/make_reference_lines.py <reference checkout>
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ref = os.path.abspath(sys.argv[1])
    lines = {}
    for dp, _, fs in os.walk(ref):
        for f in fs:
            if f.endswith(".rs"):
                p = os.path.join(dp, f)
                with open(p, errors="replace") as fh:
                    lines[os.path.relpath(p, ref)] = sum(1 for _ in fh)
    out = os.path.join(ROOT, "tests", "golden", "reference_rs_lines.json")
    with open(out, "w") as fh:
        json.dump({"source": "line counts of the reference's *.rs files (path relative to its root)",
                   "lines": dict(sorted(lines.items()))}, fh, indent=1)
        fh.write("\n")
    print(f"{len(lines)} files -> {out}")


if __name__ == "__main__":
    main()
