"""The logit-bias launch plan under AddressSanitizer + UndefinedBehaviorSanitizer (CPU).

``plan_logit_bias`` (csrc/kernels/host_plan.h) is plain C++: tests/native/logit_bias_plan_test.cpp is
built here with ``-fsanitize=address,undefined -fno-sanitize-recover=all`` and run on the production
shapes, the mask-word and span edges and the refused inputs (any sanitizer report fails)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs a host C++ compiler")
def test_logit_bias_plan_under_asan_ubsan(tmp_path):
    exe = tmp_path / "logit_bias_plan_test"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "csrc", "kernels"),
           os.path.join(ROOT, "tests", "native", "logit_bias_plan_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "logit_bias_plan_test: ok" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
