#!/usr/bin/env python3
"""The accuracy of every kernel family against the extended-precision DFT, as a
record: runs the cases of tests/test_accuracy_gpu.py through that file's own
functions (one pytest session in this process) and writes what exact_dft.check
measured: family, n, variant, err_u, e_ref (both in u = 2**-53), their ratio
and the margin asserted. --out (default profiles/accuracy.json) takes the JSON
list; the worst ratio per family is printed, the table of DESIGN.md
"Accuracy". No test reads a bound from the file."""
import argparse
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))

import exact_dft  # noqa: E402  (the module object the tests import too)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "accuracy.json"))
    args = ap.parse_args()
    rc = pytest.main([os.path.join(REPO, "tests", "test_accuracy_gpu.py"), "-q",
                      "-p", "no:cacheprovider", "--durations=15"])
    recs = exact_dft.RECORDS
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(recs, f, indent=1)
        f.write("\n")
    worst = {}
    for r in recs:
        if r["family"] not in worst or r["ratio"] > worst[r["family"]]["ratio"]:
            worst[r["family"]] = r
    print("%-22s %8s %-40s %9s %9s %7s" % ("family", "n", "variant", "err_u", "e_ref", "ratio"))
    for fam, r in worst.items():
        print("%-22s %8s %-40s %9.3g %9.3g %7.3g" % (fam, r["n"], r["variant"], r["err_u"],
                                                     r["e_ref"], r["ratio"]))
    return int(rc)


if __name__ == "__main__":
    sys.exit(main())
