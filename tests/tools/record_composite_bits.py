"""Writes tests/golden/composite_bits.json: the sha256 of every output of the compositing kernels and the ray generators on the
cases of tests/composite_bits.py, from the library that is built in the tree.  Needs the MI355X.

Run it on a commit whose ray_ops.hip is the one to be held; a commit that changes ray_ops.hip never re-records.

    python tests/tools/record_composite_bits.py [--out tests/golden/composite_bits.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from nerfmeshes_amd import hip_ops, train_ops  # noqa: E402
from tests import composite_bits as CB  # noqa: E402
from tests import composite_cases as CC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=CB.PATH)
    opt = ap.parse_args()
    out = {"composite": {CC.case_id(c): CB.composite_entry(hip_ops, train_ops, c) for c in CC.CASES}, "rays": CB.ray_entries(hip_ops)}
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as fh:
        fh.write(json.dumps(out, indent=1, sort_keys=True) + "\n")
    print(f"{len(out['composite'])} compositing cases and {len(out['rays'])} ray generators -> {opt.out}")


if __name__ == "__main__":
    main()
