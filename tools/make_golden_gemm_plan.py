"""Records which block shape and split count the generic path's contractions run with: tests/golden/gemm_plan.json.

tests/gemm_plan_host_main.hip prints the plans of gemm_nt, gemm_nt_mu, gemm2 and gemm2_mu over a fixed grid (no device, no
library, no arguments).  This script builds it with the host half of hipcc, runs it and stores the lines.  Run on the commit
whose answers are to be pinned: a change to csrc/evc_gemm_plan.h records its parent; the first recording, of the commit
before the header existed, is built with --parent (the program then holds a literal copy of the conditions that stood in
csrc/evc_gemm.hip and csrc/evc_gemm2.hip).  tests/test_gemm_plan_host.py builds the program on the current tree and
compares line by line.

    python tools/make_golden_gemm_plan.py [--parent] [--check]
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "gemm_plan.json")
SRC = os.path.join(ROOT, "tests", "gemm_plan_host_main.hip")


def build(exe, parent=False, sanitize=False):
    """Compiles the program to `exe` (host code only) and returns the compiler's CompletedProcess."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "--offload-host-only", "-O1", "-std=c++17", SRC, "-o", exe]
    if parent:
        cmd.insert(1, "-DGEMM_PLAN_PARENT")
    if sanitize:
        cmd[1:1] = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-g"]
    return subprocess.run(cmd, capture_output=True, text=True)


def lines(parent=False, sanitize=False):
    """Builds and runs the program; its output as a list of lines.  Anything on its standard error is an error."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "gemm_plan_host_main")
        p = build(exe, parent, sanitize)
        if p.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + p.stderr)
        p = subprocess.run([exe], capture_output=True, text=True)
        if p.returncode != 0 or p.stderr:
            raise RuntimeError("gemm_plan_host_main: exit %d\n%s" % (p.returncode, p.stderr))
        return p.stdout.split("\n")[:-1]


if __name__ == "__main__":
    got = {"lines": lines(parent="--parent" in sys.argv, sanitize="--sanitize" in sys.argv)}
    if "--check" in sys.argv:
        with open(OUT) as f:
            sys.exit(0 if json.load(f) == got else "the program's lines differ from " + OUT)
    with open(OUT, "w") as f:
        json.dump(got, f, indent=0)
        f.write("\n")
    print("%d lines, %d bytes -> %s" % (len(got["lines"]), os.path.getsize(OUT), OUT))
