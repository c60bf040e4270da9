#!/usr/bin/env python
"""Writes tests/golden/deriv_bits.json: the SHA-256 digests of the outputs of every case of tests/test_gpu_deriv_bits.py -- the three
level-derivative entries and the three fused ones (gradient, sensor Jacobian, its sun-angle series).

Run it on the GPU from a built checkout of the commit whose bits are to be pinned, with this file and tests/test_gpu_deriv_bits.py copied
into that checkout (the package and the library next to this file are the ones used), never from the tree under test:
    python tools/gen_deriv_bits.py [output.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_gpu_deriv_bits as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "deriv_bits.json")
    bits = {T.case_id(*c): T.digests(*c) for c in T.cases()}
    with open(out, "w") as f:
        json.dump(bits, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(bits)} cases -> {out}")


if __name__ == "__main__":
    main()
