"""Records what the main solve decides and carves before it launches anything: tests/golden/solve_plan.json.

tests/solve_plan_host_main.hip prints every field of plan_route, every field of plan_fused_tail and the byte offsets of
every sub-array of carve<T>, carve_wide<T> and dict_image<T> over a fixed grid (no device, no arguments).  This script builds
it with the host half of hipcc against the library next to the package, runs it and stores the lines.  Run on the commit whose
answers are to be pinned: a refactor of that host code records its parent, where csrc/evc_solve_plan.h did not exist yet and
the program is built with --parent (it then includes csrc/evc_api.hip whole and restates the tail's conditions).
tests/test_solve_plan_host.py builds the program on the current tree and compares line by line.

    python tools/make_golden_solve_plan.py [--parent] [--check]
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "solve_plan.json")
SRC = os.path.join(ROOT, "tests", "solve_plan_host_main.hip")
PKG = os.path.join(ROOT, "exemplars_vc_amd")


def build(exe, parent=False, sanitize=False):
    """Compiles the program to `exe` (host code only) and returns the compiler's CompletedProcess."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "--offload-host-only", "-O1", "-std=c++17", SRC, "-o", exe, "-L" + PKG, "-levc_hip", "-Wl,-rpath," + PKG]
    if parent:
        cmd.insert(1, "-DSOLVE_PLAN_PARENT")
    if sanitize:
        cmd[1:1] = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-g"]
    return subprocess.run(cmd, capture_output=True, text=True)


def lines(parent=False, sanitize=False):
    """Builds and runs the program; its output as a list of lines.  Anything on its standard error is an error."""
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "solve_plan_host_main")
        p = build(exe, parent, sanitize)
        if p.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + p.stderr)
        p = subprocess.run([exe], capture_output=True, text=True)
        if p.returncode != 0 or p.stderr:
            raise RuntimeError("solve_plan_host_main: exit %d\n%s" % (p.returncode, p.stderr))
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
