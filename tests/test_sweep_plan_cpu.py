"""AddressSanitizer + UBSan run of the sweep's host-only planning
(csrc/ace_sweep_plan.cpp) through tests/sweep_plan_check.cpp: the event names,
both schedules' tile lists walked launch by launch (single GPU, and sharded
over 1 .. 4 and 8 ranks), the work counts, the lists and counters pinned to
the commits before each part of the plan moved into the unit, and the small-n
layout rules.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_sweep_plan_is_consistent_and_sanitizer_clean(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no host compiler")
    csrc = os.path.join(ROOT, "additivecausalexpansion_amd", "csrc")
    flags = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    exe = str(tmp_path / "sweep_plan_check")
    subprocess.run([gxx, *flags, "-std=c++17", "-I", csrc,
                    os.path.join(ROOT, "tests", "sweep_plan_check.cpp"),
                    os.path.join(csrc, "ace_sweep_plan.cpp"), "-o", exe], check=True)
    # verify_asan_link_order=0: the process environment may preload other
    # libraries ahead of the ASan runtime; that is not a finding
    env = dict(os.environ,
               ASAN_OPTIONS="halt_on_error=1:detect_leaks=1:verify_asan_link_order=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sweep_plan_check: OK" in out.stdout
