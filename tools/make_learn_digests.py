"""Prints the digests a digest test pins: runs the CASES of tests/test_gpu_learn_digests.py (dictionary-learning calls on
fixtures of tests/golden) or of the test module named on the command line (tests/test_gpu_solve_digests.py: the
fixed-dictionary solves; tests/test_gpu_prox_digests.py: the sparse family and the semi-NMF solve) on the library in place, or on the one EVC_LIB names, and prints `"case": "sha256",` lines ready
for that module's PARENT_DIGESTS.  Every case runs twice; one whose two runs differ is named in a comment line instead
and must not be pinned.  Run it on the commit whose results are to be pinned; needs a HIP device.

The pymf case stops on tol = PYMF_TOL (2.58e-3) of the learn file: |err - err_prev| / T of the fixture's recorded errors
passes 2.61e-3 -> 2.54e-3 between its 6th and 7th iteration, so the run stops at 7 of 40.

    python tools/make_learn_digests.py [test_gpu_solve_digests]
"""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

if __name__ == "__main__":
    t = importlib.import_module(sys.argv[1] if len(sys.argv) > 1 else "test_gpu_learn_digests")
    for case in sorted(t.CASES):
        first, second = t.CASES[case](), t.CASES[case]()
        if first == second:
            print(f'    "{case}": "{first}",', flush=True)
        else:
            print(f"    # {case}: two runs differ ({first[:16]} / {second[:16]}): not reproducible, do not pin", flush=True)
