"""The int8 shared-prefix launch plans (csrc/kernels/host_plan.h) in a stand-alone host program, plain and under
AddressSanitizer + UndefinedBehaviorSanitizer (CPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")
@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_q8_plans(tmp_path, sanitize):
    exe = tmp_path / "shared_prefix_q8_plan_test"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", *sanitize, "-I", os.path.join(ROOT, "csrc", "kernels"),
           os.path.join(ROOT, "tests", "native", "shared_prefix_q8_plan_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "shared_prefix_q8_plan_test: ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
