"""Prints the digests tests/test_gpu_learn_digests.py pins: runs that file's CASES (dictionary-learning calls on fixtures
of tests/golden) on the library in place, or on the one EVC_LIB names, and prints `"case": "sha256",` lines ready for its
PARENT_DIGESTS.  Run it on the commit whose results are to be pinned; needs a HIP device.

The pymf case stops on tol = PYMF_TOL (2.58e-3) of that file: |err - err_prev| / T of the fixture's recorded errors
passes 2.61e-3 -> 2.54e-3 between its 6th and 7th iteration, so the run stops at 7 of 40.

    python tools/make_learn_digests.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import test_gpu_learn_digests as t  # noqa: E402

if __name__ == "__main__":
    for case in sorted(t.CASES):
        print(f'    "{case}": "{t.CASES[case]()}",', flush=True)
