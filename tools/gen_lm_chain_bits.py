#!/usr/bin/env python
"""Writes tests/golden/lm_chain_bits.npz: every state array and the covariance that crt_hip_lm_step_chain_f64 /
crt_hip_lm_chain_covariance_f64 leave after each of the three steps of the 16 (nd, npar) cases of
tests/test_gpu_lm_shared.py::test_nothing_shared_is_the_chain_bitwise (npix = 3).  Only outputs are stored; the inputs come from the seeds
of the test, whose helpers are imported, not restated.

The bits to pin are those of the commit BEFORE the chain kernels and the shared-parameter kernels became one pair, so --lib names a
library built from that commit (a copy of its tree kept out of git, `make -C <copy>/crt1d_amd/csrc`), never the library of the tree
under test.  It is the only build of the library in the process (crt1d_amd._lib loads it in place of the tree's own: CRT1D_HIP_LIB);
the package and the test helpers are this tree's.  Run it on the GPU:
    python tools/gen_lm_chain_bits.py --lib <copy>/crt1d_amd/libcrt1d_hip.so [--out tests/golden/lm_chain_bits.npz]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="libcrt1d_hip.so built from the commit whose chain kernels are to be pinned")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    own = os.path.join(ROOT, "crt1d_amd", "libcrt1d_hip.so")
    assert os.path.realpath(args.lib) != os.path.realpath(own), "--lib must not be the library of the tree under test"
    os.environ["CRT1D_HIP_LIB"] = os.path.abspath(args.lib)  # (read when crt1d_amd._lib is imported: below)

    import numpy as np

    import test_gpu_lm_shared as T
    from crt1d_amd import _lib

    assert _lib.LIB_PATH == os.environ["CRT1D_HIP_LIB"], _lib.LIB_PATH
    bits = {}
    for nd, npar in T.BITS_CASES:
        got = T.chain_bits(nd, npar, T.Chain)
        assert got["2/naccept"].min() >= 2, (nd, npar)
        bits.update({f"nd{nd}_npar{npar}/{k}": v for k, v in got.items()})
    out = args.out or T.BITS
    np.savez_compressed(out, **bits)
    print(f"{len(T.BITS_CASES)} cases, {len(bits)} arrays, {sum(v.nbytes for v in bits.values())} bytes, {_lib.LIB_PATH} -> {out}")


if __name__ == "__main__":
    main()
